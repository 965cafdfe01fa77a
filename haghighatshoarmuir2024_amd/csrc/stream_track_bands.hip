// The wideband tracking rule of include/micloc_hip.h ("wideband moving-target tracking") cut at launch borders: the wideband streams of
// streaming.py emit the DoA index and the peak envelope of every frame that became final in EVERY band (include/micloc_hip.h "wideband
// streaming, tracking").
//
// track.hip's band workgroup -- 64 DoA columns of ONE trial, chunks of 64 frames, per chunk the bands in ascending order into one magnitude
// tile: the same text, track_bands_ws_walk / track_bands_wsc_walk of track_bands_rows.h -- walks the frames a tile made final.  The range,
// the ring store and the pair store are the single-plan stream's (stream_track_rows.h).  What stands here is whose words give the range:
//   track_bands_ws_stream_kernel    SNN bands, each with its own horizon: the range is [previous frontier, new frontier) of the joint
//                                   frontier min(min_f done_f CH, t_end), which track_bands_frontier_kernel -- one thread, in front of this
//                                   launch -- leaves in the head of the tracked state as rows of the bands' raster windows (they share
//                                   cap and CH and therefore the base: rz_stream_clock_begin_kernel's schedule depends on the tile sizes only);
//   track_bands_wsc_stream_kernel   complex bands, in lock step as ONE complex stream of F B rows: the range of that stream's words
//                                   (track_span<true>); band f's rows are rows [f B, (f + 1) B) of the one staging array.
// Why the rows of the SNN range are still there: a band without a lag failure keeps chunk done_f - 1 in its window (rz_window_slide_kernel's
// check), the frontier is at most done_f CH for every f, and the windows share their base, so the chunk in front of the frontier is in every
// band's window, and with it the LIF history 4 NK_f - 16 <= CH of every band.  A band's lag failure stops its done_f and with it the
// frontier; the frontier kernel also refuses a range whose history chunk has left the window, so no wrong row is ever emitted.
// No launch argument depends on time; a workgroup reads and writes only its own 64 columns of its own trial, waits on nobody, and a launch
// with an empty range returns before its first barrier with nothing written.
#include "stream_track.h"
#include "stream_track_bands.h"
#include "stream_track_rows.h"
#include "track_bands_rows.h"
#include "track_rows.h"

namespace micloc {

namespace {

// the range the frontier kernel left (SNN bands)
__device__ __forceinline__ TrackSpan track_bands_span(const int *__restrict__ head, int cap)
{
    TrackSpan s;
    s.f0 = head[STB_F0];
    s.f1 = head[STB_F1];
    s.abs0 = head[STB_ABS0];
    if (s.f0 < 0) s.f0 = 0;  // (never: the words are the frontier kernel's)
    if (s.f1 > cap) s.f1 = cap;
    return s;
}

// one thread, plain loads and stores: the joint frontier of the bands behind their commits and ticks of this tile
__global__ void track_bands_frontier_kernel(const TrackBandsCtl c, int F, int CH, int cap, int *__restrict__ head)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int t_end = c.ctl[0][STREAM_CLK_T], base = c.ctl[0][STREAM_CLK_BASE];
    int done = c.ctl[0][0];
    for (int f = 1; f < F; ++f) {
        const int d = c.ctl[f][0];
        done = d < done ? d : done;
    }
    const int prev = head[STB_FRONT];
    int front = (long long)done * CH < (long long)t_end ? done * CH : t_end;
    if (front < prev) front = prev;
    int f0 = prev - base, f1 = front - base;
    // the chunk in front of the range holds the LIF history of its first chunk: a range without it (only behind a band's lag failure)
    // or outside the window is not tracked, and the frontier stays
    if (f1 > f0 && (f0 < 0 || f1 > cap || (base > 0 && f0 < CH))) {
        front = prev;
        f1 = f0;
    }
    head[STB_FRONT] = front;
    head[STB_F0] = f0;
    head[STB_F1] = f1;
    head[STB_ABS0] = base;
}

// SNN bands: every band's raster window [B][cap][C] int8, C <= 16
__global__ __launch_bounds__(TRK_THREADS) void track_bands_ws_stream_kernel(const TrackBandsArgs a, int F, int NKmax, const int *__restrict__ head,
                                                                            int cap, int C, int G, double a_rise, double i_rise, double a_fall,
                                                                            double *__restrict__ state_g, const TrackSink out,
                                                                            double *__restrict__ pval, int32_t *__restrict__ pidx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const TrackSpan sp = track_bands_span(head, cap);
    if (sp.f1 <= sp.f0) return;  // nothing became final in every band: no barrier yet, nothing written
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
    const int cg = blockIdx.x, ncg = gridDim.x, b = blockIdx.y;
    double *sg = state_g + ((size_t)b * ncg + cg) * TRK_COLS + l;
    double state = 0.0;
    if (wv == 0) state = *sg;
    track_bands_ws_walk(smem, a, F, NKmax, b, C, cap, sp.f0, sp.f1, sp.abs0, G, cg, a_rise, i_rise, a_fall, state,
                        [&](int cs, int row, double best, int bi) { TrackEmit{out, sp, b, cg, ncg, cap, cs, pval, pidx}(row, best, bi); });
    if (wv == 0) *sg = state;
}

// complex bands: band f's rows [B][C = 2M][cap] of the staging array, C <= 16; G = complex DoAs.  Two workgroups per CU are asked for: left
// to itself the compiler gives <3, 2> (seven microphones) 248 VGPRs + 12 AGPRs, four past the 256 that two waves per SIMD may hold
template <int KM, int KV>
__global__ __launch_bounds__(TRK_THREADS, 2) void track_bands_wsc_stream_kernel(const TrackBandsArgs a, int F, const int *__restrict__ ctl, int cap,
                                                                             int C, int G, double a_rise, double i_rise, double a_fall,
                                                                             double *__restrict__ state_g, const TrackSink out,
                                                                             double *__restrict__ pval, int32_t *__restrict__ pidx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const TrackSpan sp = track_span<true>(ctl, 0, cap);
    if (sp.f1 <= sp.f0) return;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
    const int cg = blockIdx.x, ncg = gridDim.x, b = blockIdx.y;
    double *sg = state_g + ((size_t)b * ncg + cg) * TRK_COLS + l;
    double state = 0.0;
    if (wv == 0) state = *sg;
    track_bands_wsc_walk<KM, KV>(smem, a, F, b, C, cap, sp.f0, sp.f1, sp.abs0, G, cg, a_rise, i_rise, a_fall, state,
                                 [&](int cs, int row, double best, int bi) { TrackEmit{out, sp, b, cg, ncg, cap, cs, pval, pidx}(row, best, bi); });
    if (wv == 0) *sg = state;
}

// the combine of a tile (track_stream_combine of stream_track_rows.h) on the bands' range
template <bool COMPLEX>
__global__ __launch_bounds__(256) void track_bands_stream_combine_kernel(const double *__restrict__ pval, const int32_t *__restrict__ pidx,
                                                                         const int *__restrict__ words, int cap, int ncg, const TrackSink out)
{
    track_stream_combine(COMPLEX ? track_span<true>(words, 0, cap) : track_bands_span(words, cap), pval, pidx, cap, ncg, out);
}

template <bool COMPLEX>
hipError_t combine_launch(const double *pval, const int32_t *pidx, const int *words, int B, int cap, int ncg, const TrackSink &out, hipStream_t stream)
{
    hipLaunchKernelGGL(track_bands_stream_combine_kernel<COMPLEX>, dim3((unsigned)((cap + 255) / 256), B), dim3(256), 0, stream, pval, pidx, words, cap,
                       ncg, out);
    return hipGetLastError();
}

}  // namespace

size_t stream_track_bands_state_bytes(int B, int G) { return STB_HEAD_BYTES + stream_track_state_bytes(B, G); }

hipError_t launch_stream_track_bands(const TrackBandsArgs &a, const TrackBandsCtl &c, int F, int NKmax, int C, int B, int cap, int CH, int G,
                                     double a_rise, double i_rise, double a_fall, void *track_state, int R, int32_t *index, double *peak,
                                     int32_t *latest_index, double *latest_peak, void *pairs, hipStream_t stream)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || CH < TRK_CH || CH % TRK_CH != 0 || 4 * NKmax - 16 > CH || cap % CH != 0) return hipErrorInvalidValue;
    const int ncg = track_col_groups(G);
    double *pval;
    int32_t *pidx;
    track_pairs_split(pairs, (size_t)B * cap * ncg, pval, pidx);
    const TrackSink out{R, index, peak, latest_index, latest_peak};
    int *head = reinterpret_cast<int *>(track_state);
    double *state = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(track_state) + STB_HEAD_BYTES);
    hipLaunchKernelGGL(track_bands_frontier_kernel, dim3(1), dim3(1), 0, stream, c, F, CH, cap, head);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    auto k = &track_bands_ws_stream_kernel;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(ncg, B), dim3(TRK_THREADS), track_lds_bytes(false, NKmax), stream, a, F, NKmax, head, cap, C, G, a_rise, i_rise, a_fall,
                       state, out, pval, pidx);
    e = hipGetLastError();
    if (e != hipSuccess || ncg == 1) return e;
    return combine_launch<false>(pval, pidx, head, B, cap, ncg, out, stream);
}

hipError_t launch_stream_track_bands_complex(const TrackBandsArgs &a, int F, const int *ctl, int C, int B, int cap, int G, double a_rise,
                                             double i_rise, double a_fall, void *track_state, int R, int32_t *index, double *peak,
                                             int32_t *latest_index, double *latest_peak, void *pairs, hipStream_t stream)
{
    if (F < 1 || F > MICLOC_MAX_BANDS) return hipErrorInvalidValue;
    const int ncg = track_col_groups(G);
    double *pval;
    int32_t *pidx;
    track_pairs_split(pairs, (size_t)B * cap * ncg, pval, pidx);
    const TrackSink out{R, index, peak, latest_index, latest_peak};
    double *state = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(track_state) + STB_HEAD_BYTES);
    const bool served = track_wsc_dispatch(C, [&](auto k) {
        hipLaunchKernelGGL((track_bands_wsc_stream_kernel<decltype(k)::km, decltype(k)::kv>), dim3(ncg, B), dim3(TRK_THREADS), track_lds_bytes(true, 0),
                           stream, a, F, ctl, cap, C, G, a_rise, i_rise, a_fall, state, out, pval, pidx);
    });
    if (!served) return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || ncg == 1) return e;
    return combine_launch<true>(pval, pidx, ctl, B, cap, ncg, out, stream);
}

}  // namespace micloc
