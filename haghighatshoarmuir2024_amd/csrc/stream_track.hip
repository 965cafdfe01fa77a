// The tracking rule of include/micloc_hip.h ("moving-target tracking") cut at launch borders: the streams of streaming.py emit the DoA index
// and the peak envelope of every frame that became final in a tile (include/micloc_hip.h "streaming, tracking").
//
// track.hip's workgroup -- 64 DoA columns of ONE trial, chunks of 64 frames, stages 1 to 4 of its header: the same text, track_ws_walk /
// track_wsc_walk of track_rows.h -- walks the frames a tile made final instead of a recording from frame 0 to T.  What stands here is what
// differs: whose words give the range, the state load and store (the range, the ring store and the pair store: stream_track_rows.h):
//   track_ws_stream_kernel    the SNN stream: the window-relative chunks ctl[4] .. ctl[5] of CH frames that rz_stream_horizon_kernel left,
//                             cut at ctl[10], the frames of the raster window that exist; window row 0 is frame ctl[STREAM_CLK_BASE];
//   track_wsc_stream_kernel   the complex stream: the staging columns [fill, fill + n), fill = ctl[2] (the carry), n = ctl[SC_N]; column
//                             fill is frame ctl[STREAM_CLK_T].
// No launch argument depends on time: the range and the clock are device words written by EARLIER launches of the tile (the launch sits in
// front of the commit / the slide, which write the words the next tile reads), so a tile stays one replayable graph.
// The envelope state e[t-1][g] of the frame in front of the range lives in `state` [B][ceil(G / 64) 64] doubles: the chain wave loads its
// lane's value at the start and stores it at the end; state_0 = |y_0| is taken when the ABSOLUTE frame is 0.  A workgroup reads and writes
// only its own 64 columns of its own trial, waits on nobody, and a launch with an empty range returns before its first barrier with
// nothing written.
// Results: frame t goes to row t % R of index [B][R] / peak [B][R], the newest one also to latest_index [B] / latest_peak [B].  With one
// column group the kernel writes them itself; otherwise the pairs go to pval / pidx [B][cap][ncg], addressed by the frame's position in the
// window / the staging array, and track_stream_combine_kernel finishes them by track_combine_kernel's rule.
#include "bandpass_rows.h"
#include "stream_track.h"
#include "stream_track_rows.h"
#include "track_rows.h"

namespace micloc {

namespace {

// SNN: the raster window [B][cap][C] int8, C <= 16; CH: frames per chunk of the stream (a multiple of TRK_CH, 4 NK - 16 <= CH)
__global__ __launch_bounds__(TRK_THREADS) void track_ws_stream_kernel(const int8_t *__restrict__ win, const int *__restrict__ ctl, int CH, int cap,
                                                                      const double *__restrict__ ntab_g, int NK, const double *__restrict__ Wp,
                                                                      int GT, int C, int G, double a_rise, double i_rise, double a_fall,
                                                                      double *__restrict__ state_g, const TrackSink out,
                                                                      double *__restrict__ pval, int32_t *__restrict__ pidx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const TrackSpan sp = track_span<false>(ctl, CH, cap);
    if (sp.f1 <= sp.f0) return;  // nothing became final (or a lag failure): no barrier yet, nothing written
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
    const int cg = blockIdx.x, ncg = gridDim.x, b = blockIdx.y;
    double *sg = state_g + ((size_t)b * ncg + cg) * TRK_COLS + l;
    double state = 0.0;
    if (wv == 0) state = *sg;
    // (rows at or behind sp.f1 are zero, as the one-shot kernel's rows at or behind T; rows in front of the window exist only with base 0)
    track_ws_walk(smem, win + (size_t)b * cap * C, C, sp.f0, sp.f1, sp.abs0, ntab_g, NK, Wp, GT, G, cg, a_rise, i_rise, a_fall, state,
                  [&](int cs, int row, double best, int bi) { TrackEmit{out, sp, b, cg, ncg, cap, cs, pval, pidx}(row, best, bi); });
    if (wv == 0) *sg = state;
}

// complex Beamformer: the staging array [B][C = 2M][cap] of band-passed rows, C <= 16; G = complex DoAs.  fill is any value, so a 16-frame
// tile starts at any column: the operands are single doubles, which need no more than their own alignment.
template <int KM, int KV>
__global__ __launch_bounds__(TRK_THREADS) void track_wsc_stream_kernel(const double *__restrict__ stg, const int *__restrict__ ctl, int cap,
                                                                       const double *__restrict__ Wp, int GT, int C, int G, double a_rise,
                                                                       double i_rise, double a_fall, double *__restrict__ state_g,
                                                                       const TrackSink out, double *__restrict__ pval,
                                                                       int32_t *__restrict__ pidx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const TrackSpan sp = track_span<true>(ctl, 0, cap);
    if (sp.f1 <= sp.f0) return;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
    const int cg = blockIdx.x, ncg = gridDim.x, b = blockIdx.y;
    double *sg = state_g + ((size_t)b * ncg + cg) * TRK_COLS + l;
    double state = 0.0;
    if (wv == 0) state = *sg;
    track_wsc_walk<KM, KV>(smem, stg + (size_t)b * C * cap, C, cap, sp.f0, sp.f1, sp.abs0, Wp, GT, G, cg, a_rise, i_rise, a_fall, state,
                           [&](int cs, int row, double best, int bi) { TrackEmit{out, sp, b, cg, ncg, cap, cs, pval, pidx}(row, best, bi); });
    if (wv == 0) *sg = state;
}

// the combine of a tile (track_stream_combine of stream_track_rows.h) on the range of the stream's own words
template <bool COMPLEX>
__global__ __launch_bounds__(256) void track_stream_combine_kernel(const double *__restrict__ pval, const int32_t *__restrict__ pidx,
                                                                   const int *__restrict__ ctl, int CH, int cap, int ncg, const TrackSink out)
{
    track_stream_combine(track_span<COMPLEX>(ctl, CH, cap), pval, pidx, cap, ncg, out);
}

}  // namespace

size_t stream_track_state_bytes(int B, int G) { return track_al256((size_t)B * track_col_groups(G) * TRK_COLS * sizeof(double)); }

size_t stream_track_pairs_bytes(int B, int cap, int G)
{
    const int ncg = track_col_groups(G);
    if (ncg == 1) return 256;  // (the kernel writes the ring itself; a workspace is never empty)
    return track_pairs_size((size_t)B * cap * ncg);
}

int stream_track_halo(const NeuronTab &nt) { return 4 * nt.NK - 16; }

hipError_t launch_stream_track(const BeamformW &W, const NeuronTab &nt, int is_complex, const void *src, const int *ctl, int B, int cap, int CH,
                               int G, double a_rise, double i_rise, double a_fall, double *state, int R, int32_t *index, double *peak,
                               int32_t *latest_index, double *latest_peak, void *pairs, hipStream_t stream)
{
    const int ncg = track_col_groups(G);
    double *pval;
    int32_t *pidx;
    track_pairs_split(pairs, (size_t)B * cap * ncg, pval, pidx);
    const TrackSink out{R, index, peak, latest_index, latest_peak};
    const size_t lds = track_lds_bytes(is_complex != 0, nt.NK);
    dim3 grid(ncg, B), block(TRK_THREADS);
    if (!is_complex) {
        if (CH < TRK_CH || CH % TRK_CH != 0 || stream_track_halo(nt) > CH || cap % CH != 0) return hipErrorInvalidValue;
        auto k = &track_ws_stream_kernel;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k, grid, block, lds, stream, static_cast<const int8_t *>(src), ctl, CH, cap, nt.tab, nt.NK, W.Wp, W.GT, W.C, G, a_rise,
                           i_rise, a_fall, state, out, pval, pidx);
    } else {
        const double *stg = static_cast<const double *>(src);
        const bool served = track_wsc_dispatch(W.C, [&](auto k) {
            hipLaunchKernelGGL((track_wsc_stream_kernel<decltype(k)::km, decltype(k)::kv>), grid, block, lds, stream, stg, ctl, cap, W.Wp, W.GT, W.C, G,
                               a_rise, i_rise, a_fall, state, out, pval, pidx);
        });
        if (!served) return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || ncg == 1) return e;
    dim3 cgrid((unsigned)((cap + 255) / 256), B);
    if (is_complex)
        hipLaunchKernelGGL(track_stream_combine_kernel<true>, cgrid, dim3(256), 0, stream, pval, pidx, ctl, CH, cap, ncg, out);
    else
        hipLaunchKernelGGL(track_stream_combine_kernel<false>, cgrid, dim3(256), 0, stream, pval, pidx, ctl, CH, cap, ncg, out);
    return hipGetLastError();
}

}  // namespace micloc
