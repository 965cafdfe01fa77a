// The tracking rule of include/micloc_hip.h ("moving-target tracking") cut at launch borders: the streams of streaming.py emit the DoA index
// and the peak envelope of every frame that became final in a tile (include/micloc_hip.h "streaming, tracking").
//
// track.hip's workgroup -- 64 DoA columns of ONE trial, chunks of 64 frames, stages 1 to 4 of its header with the same instruction
// sequences (track_rows.h) -- walks the frames a tile made final instead of a recording from frame 0 to T:
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
#include "track_rows.h"

namespace micloc {

namespace {

// the frames [f0, f1) of the window (SNN) or of the staging array (complex) that this tile made final; position p is frame abs0 + p
struct TrackSpan {
    int f0, f1, abs0;
};

template <bool COMPLEX>
__device__ __forceinline__ TrackSpan track_span(const int *__restrict__ ctl, int CH, int cap)
{
    TrackSpan s;
    if (COMPLEX) {
        const int fill = ctl[2], n = ctl[SC_N];
        s.f0 = fill;
        s.f1 = fill + n;
        s.abs0 = ctl[STREAM_CLK_T] - fill;
    } else {
        const int exist = ctl[10];
        s.f0 = ctl[4] * CH;
        s.f1 = ctl[5] * CH < exist ? ctl[5] * CH : exist;
        s.abs0 = ctl[STREAM_CLK_BASE];
    }
    if (s.f0 < 0) s.f0 = 0;  // (never: the words are the stream's own)
    if (s.f1 > cap) s.f1 = cap;
    return s;
}

struct TrackSink {
    int R;  // ring depth
    int32_t *index;
    double *peak;
    int32_t *latest_index;
    double *latest_peak;
};

// a finished row of trial b: frame `abs` into its ring row, the newest frame of the launch also into the latest words
__device__ __forceinline__ void track_ring_store(const TrackSink &o, int b, int abs, bool newest, double best, int bi)
{
    const size_t r = (size_t)b * o.R + (size_t)((unsigned)abs % (unsigned)o.R);  // (abs >= 0: the clock's)
    const int idx = track_row_index(bi);
    const double pk = track_row_peak(best, bi);
    o.index[r] = idx;
    o.peak[r] = pk;
    if (newest) {
        o.latest_index[b] = idx;
        o.latest_peak[b] = pk;
    }
}

// the emit of both kernels for the chunk at position cs
struct TrackEmit {
    const TrackSink &o;
    const TrackSpan &sp;
    int b, cg, ncg, cap, cs;
    double *__restrict__ pval;
    int32_t *__restrict__ pidx;
    __device__ __forceinline__ void operator()(int row, double best, int bi) const
    {
        const int f = cs + row;
        if (ncg == 1) {
            track_ring_store(o, b, sp.abs0 + f, f == sp.f1 - 1, best, bi);
        } else {
            const size_t e = ((size_t)b * cap + f) * ncg + cg;
            pidx[e] = bi;
            pval[e] = best;
        }
    }
};

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
    const int T = sp.f1;         // rows at or behind it are zero, as the one-shot kernel's rows at or behind T
    const int Gp = 16 * GT;
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    const int lc = l & 15;
    const int q = l >> 4;
    const int cg = blockIdx.x, ncg = gridDim.x, b = blockIdx.y;
    const int R = TRK_CH + 4 * NK - 16;
    const int ntab_len = 4 * NK + 16;
    double *Y = reinterpret_cast<double *>(smem);  // [TRK_CH][TRK_LD]
    double *ntab = Y + TRK_CH * TRK_LD;
    double *S = ntab + ntab_len;  // spike tile as fp64 [R][16]

    for (int e = tid; e < ntab_len; e += TRK_THREADS) ntab[e] = ntab_g[e];
    double Wf[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gt = 4 * cg + j;
        const double *wp = Wp + 16 * (gt < GT ? gt : GT - 1) + lc;
#pragma unroll
        for (int k = 0; k < 4; ++k) Wf[j][k] = wp[(size_t)(4 * k + q) * Gp];
    }
    const int8_t *sb = win + (size_t)b * cap * C;
    double *sg = state_g + ((size_t)b * ncg + cg) * TRK_COLS + l;
    double state = 0.0;
    if (wv == 0) state = *sg;
    for (int cs = sp.f0; cs < T; cs += TRK_CH) {
        {  // window rows tau0 .. tau0 + R - 1; rows in front of the window (only with base 0: frames before 0), rows at or behind T and the channel padding are zero
            const int tau0 = cs + 16 - 4 * NK;
            const int c = tid & 15;
            for (int rho = tid >> 4; rho < R; rho += TRK_THREADS / 16) {
                const int tau = tau0 + rho;
                const bool ok = c < C && tau >= 0 && tau < T;
                S[rho * 16 + c] = ok ? (double)sb[(size_t)tau * C + c] : 0.0;
            }
        }
        __syncthreads();
        // ---- membrane fragments of this wave's tile (track_ws_kernel, stage 1) ----
        const int tb0 = cs + wv * 16;
        double4_t vacc = double4_t{0.0, 0.0, 0.0, 0.0};
        if (tb0 < T) {  // (wave-uniform)
            const double *sp_ = S + (size_t)(wv * 16 + q) * 16 + lc;
            const double *np_ = ntab + (lc - q + 4 * NK - 1);
            for (int ks = 0; ks < NK; ++ks) vacc = __builtin_amdgcn_mfma_f64_16x16x4f64(sp_[ks * 64], np_[-4 * ks], vacc, 0, 0, 0);
            if (tb0 + 16 > T) {
                const bool tvalid = (tb0 + lc) < T;
#pragma unroll
                for (int r = 0; r < 4; ++r) vacc[r] = tvalid ? vacc[r] : 0.0;
            }
        }
        // ---- y of the tile against the four DoA tiles, |y| into the LDS tile (stage 2) ----
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vacc[k], Wf[j][k], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) Y[(wv * 16 + q + 4 * r) * TRK_LD + 16 * j + lc] = fabs(acc[r]);
        }
        __syncthreads();
        const int nrow = T - cs < TRK_CH ? T - cs : TRK_CH;
        track_chain_reduce(Y, wv, l, tid, sp.abs0 + cs == 0, nrow, G, cg, a_rise, i_rise, a_fall, state,
                           TrackEmit{out, sp, b, cg, ncg, cap, cs, pval, pidx});
    }
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
    constexpr int KF = KM + (KV > 0 ? 1 : 0);
    constexpr int KVD = KV > 0 ? KV : 1;
    const TrackSpan sp = track_span<true>(ctl, 0, cap);
    if (sp.f1 <= sp.f0) return;
    const int T = sp.f1;
    const int Gp = 16 * GT, GTc = GT >> 1;
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    const int lc = l & 15;
    const int q = l >> 4;
    const int cg = blockIdx.x, ncg = gridDim.x, b = blockIdx.y;
    double *Y = reinterpret_cast<double *>(smem);
    double *tail = Y + TRK_CH * TRK_LD + wv * 64;  // this wave's fragment of the KV tail channels

    double Wf[4][2][KM], Wv[4][2][KVD];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ct = 4 * cg + j;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const double *wp = Wp + 16 * ((ct < GTc ? ct : GTc - 1) + part * GTc) + lc;
#pragma unroll
            for (int k = 0; k < KM; ++k) Wf[j][part][k] = wp[(size_t)(4 * k + q) * Gp];
#pragma unroll
            for (int i = 0; i < KV; ++i) Wv[j][part][i] = wp[(size_t)(4 * KM + i) * Gp];
        }
    }
    const double *pb = stg + (size_t)b * C * cap;
    double *sg = state_g + ((size_t)b * ncg + cg) * TRK_COLS + l;
    double state = 0.0;
    if (wv == 0) state = *sg;
    for (int cs = sp.f0; cs < T; cs += TRK_CH) {
        // ---- this wave's tile as A-fragments (track_wsc_kernel, stage 1): lane l of k-step k = channel 4k + (l >> 4), frame l & 15 ----
        double V[KF];
        {
            const int t = cs + wv * 16 + lc;
#pragma unroll
            for (int k = 0; k < KF; ++k) {
                const int c = 4 * k + q;
                const double v = pb[(size_t)(c < C ? c : C - 1) * cap + (t < T ? t : T - 1)];  // (clamped: unconditional loads)
                V[k] = (t < T && c < C) ? v : 0.0;
            }
        }
        if (KV > 0) tail[l] = V[KF - 1];
        __syncthreads();  // (also: the previous chunk's row reduction is done with Y)
        double Vv[KVD][4];
#pragma unroll
        for (int i = 0; i < KV; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) Vv[i][r] = tail[16 * i + q + 4 * r];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double4_t acc[2];
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                acc[part] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < KM; ++k) acc[part] = __builtin_amdgcn_mfma_f64_16x16x4f64(V[k], Wf[j][part][k], acc[part], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < KV; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[part][r] = __builtin_fma(Vv[i][r], Wv[j][part][i], acc[part][r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Y[(wv * 16 + q + 4 * r) * TRK_LD + 16 * j + lc] = hypot(acc[0][r], acc[1][r]);
        }
        __syncthreads();
        const int nrow = T - cs < TRK_CH ? T - cs : TRK_CH;
        track_chain_reduce(Y, wv, l, tid, sp.abs0 + cs == 0, nrow, G, cg, a_rise, i_rise, a_fall, state,
                           TrackEmit{out, sp, b, cg, ncg, cap, cs, pval, pidx});
    }
    if (wv == 0) *sg = state;
}

// one thread per position of the window / the staging array; positions outside the tile's range return
template <bool COMPLEX>
__global__ __launch_bounds__(256) void track_stream_combine_kernel(const double *__restrict__ pval, const int32_t *__restrict__ pidx,
                                                                   const int *__restrict__ ctl, int CH, int cap, int ncg, const TrackSink out)
{
    const TrackSpan sp = track_span<COMPLEX>(ctl, CH, cap);
    const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (f < sp.f0 || f >= sp.f1) return;
    const size_t e = ((size_t)b * cap + f) * ncg;
    double best;
    int bi;
    track_combine_row(pval + e, pidx + e, ncg, best, bi);
    track_ring_store(out, b, sp.abs0 + f, f == sp.f1 - 1, best, bi);
}

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

size_t stream_track_state_bytes(int B, int G) { return al256((size_t)B * track_col_groups(G) * TRK_COLS * sizeof(double)); }

size_t stream_track_pairs_bytes(int B, int cap, int G)
{
    const int ncg = track_col_groups(G);
    if (ncg == 1) return 256;  // (the kernel writes the ring itself; a workspace is never empty)
    const size_t n = (size_t)B * cap * ncg;
    return al256(n * sizeof(double)) + al256(n * sizeof(int32_t));
}

int stream_track_halo(const NeuronTab &nt) { return 4 * nt.NK - 16; }

hipError_t launch_stream_track(const BeamformW &W, const NeuronTab &nt, int is_complex, const void *src, const int *ctl, int B, int cap, int CH,
                               int G, double a_rise, double i_rise, double a_fall, double *state, int R, int32_t *index, double *peak,
                               int32_t *latest_index, double *latest_peak, void *pairs, hipStream_t stream)
{
    const int ncg = track_col_groups(G);
    const size_t n = (size_t)B * cap * ncg;
    double *pval = reinterpret_cast<double *>(pairs);
    int32_t *pidx = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(pairs) + al256(n * sizeof(double)));
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
#define TRK_K(KM_, KV_)                                                                                                                       \
    hipLaunchKernelGGL((track_wsc_stream_kernel<KM_, KV_>), grid, block, lds, stream, stg, ctl, cap, W.Wp, W.GT, W.C, G, a_rise, i_rise, a_fall, \
                       state, out, pval, pidx);                                                                                               \
    break
        switch (W.C) {  // (2 x microphones: even; track_wsc_kernel's table)
            case 2: case 4: TRK_K(1, 0);
            case 6: TRK_K(1, 2);
            case 8: TRK_K(2, 0);
            case 10: TRK_K(2, 2);
            case 12: TRK_K(3, 0);
            case 14: TRK_K(3, 2);
            case 16: TRK_K(4, 0);
            default: return hipErrorInvalidValue;
        }
#undef TRK_K
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
