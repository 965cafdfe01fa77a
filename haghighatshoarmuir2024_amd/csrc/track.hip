// Fused moving-target tracking: beamforming + Envelope.evolve + arg-max over the DoA grid per time step, without the T x G arrays.
// Reference: paper_plots/target_snn_localization.py:595-622 (`np.argmax(Envelope.evolve(sig_bf), axis=1)`), micloc/utils.py:36-81.
//
// The two-step route (apply_to_signal(to_host=False) -> envelope_kernel -> rows_argmax_kernel, sweep.hip) writes y [T][G], reads it,
// writes an envelope of the same size and reads that: 2 x 8 T G bytes of device memory per trial, every value four times through
// HBM.  Here a workgroup owns 64 DoA columns of ONE trial and walks the recording in chunks of 64 frames:
//   1. (SNN) the int8 spike rows of the chunk and of its LIF halo are staged in LDS as fp64; every wave forms the membrane fragments of
//      its 16-frame tile on the matrix cores -- beamform_ws_kernel's stage 1: the same operands in the same k-step order -- and keeps
//      them in registers: lane l of accumulator register r holds V[t = l & 15][c = (l >> 4) + 4 r], the A-operand of k-step r.
//      (complex) the planar band-passed rows are read as A-fragments straight from memory (beamform_wsc_kernel's stage 1).
//   2. y = V W for the wave's tile and the workgroup's four DoA tiles: v_mfma_f64_16x16x4_f64 over k = 0 .. 3 in that order from a
//      zero accumulator (complex: the k-steps that hold channels, then the tail channels as plain FMAs) -- the instruction sequence
//      of the WANT_Y paths of beamform.hip, so every y[t][g] has the bits apply_to_signal(to_host=False) gives it.  |y| (fabs, or
//      the device hypot of (re, im) as EnvIn<MICLOC_ENV_C128>) goes to an LDS tile [64 frames][64 columns].
//   3. wave 0 walks the 64 envelope chains (one lane per column) over the tile in place: envelope_kernel's recurrence, __dmul_rn /
//      __dadd_rn, nothing fused, state_0 = |y_0|, rise when |y_t| >= state.  The chain state stays in a register across chunks.
//   4. every frame of the tile is reduced to (max envelope, first index) over the workgroup's columns by the first-maximum rule of
//      readout_rows.h (a NaN never wins).  With one column group (G <= 64) that is the result; otherwise the pairs go to
//      pval / pidx [B][T][ceil(G / 64)] and track_combine_kernel finishes in ascending column order.
// No buffer grows with T G.  The chain is latency (one wave, ~8 dependent instructions per step); the matrix work of a chunk is a few
// hundred cycles per wave, and several workgroups share a compute unit (46 KB of LDS), so one workgroup's chain runs beside the
// others' staging and matrix phases.
// The four stages are written once, in track_rows.h (track_ws_walk / track_wsc_walk over track_chain_reduce), for these kernels and for
// the streaming ones of stream_track.hip, with the channel-count table and the pairs layout of the launchers.  Here: the kernels as a walk
// from frame 0 with a zero chain state, the store of a pair, the last envelope row; the combine; the kernels over F bands (wideband
// tracking: one magnitude tile summed over the bands, the walk of track_bands_rows.h); the read-out of the two-step route.
#include "track_rows.h"
#include "track_bands.h"
#include "track_bands_rows.h"

namespace micloc {

int track_col_groups(int G) { return (G + TRK_COLS - 1) / TRK_COLS; }

// The shapes the fused kernels serve: those whose y the bf_mat-stationary kernels of beamform.hip produce (their eligibility rules,
// restated), as long as this kernel's own LDS tile fits as well.
bool track_fused_eligible(const BeamformW &W, const NeuronTab &nt, int is_complex)
{
    if (W.CT != 1) return false;
    if (is_complex) return W.complex_pairs && (W.GT & 1) == 0;
    if (W.GT > 4 * BF_WAVES) return false;
    const size_t tile = (size_t)(BF_WAVES * 2 * 16 + 4 * nt.NK - 16) * 16, vfrag = (size_t)BF_WAVES * 2 * 256;
    const size_t tab = (size_t)(4 * nt.NK + 16);
    const size_t ws_y = ((tile > vfrag ? tile : vfrag) + ((tab + 1) & ~(size_t)1) + (size_t)16 * W.G) * sizeof(double);
    return ws_y <= 160 * 1024 && track_lds_bytes(false, nt.NK) <= 160 * 1024;
}

// where the one-shot kernels leave the pair of frame cs + row: with one column group the result itself, else pval / pidx for the combine
__device__ __forceinline__ void track_store_pair(size_t o, int ncg, double best, int bi, double *__restrict__ pval, int32_t *__restrict__ pidx)
{
    if (ncg == 1) {
        pidx[o] = track_row_index(bi);
        if (pval) pval[o] = track_row_peak(best, bi);
    } else {
        pidx[o] = bi;
        pval[o] = best;
    }
}

// a one-shot kernel around its walk: workgroup (cg, b) of a (column groups, trials) grid walks trial b from frame 0 with a zero chain
// state -- walk(state, emit) -- leaves every pair by track_store_pair and, asked for it, the last envelope row of its columns
template <class Walk>
__device__ __forceinline__ void track_one_shot(int T, int G, double *__restrict__ pval, int32_t *__restrict__ pidx, double *__restrict__ env_last,
                                               const Walk &walk)
{
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
    const int cg = blockIdx.x, ncg = gridDim.x, b = blockIdx.y;
    const size_t row0 = (size_t)b * T;
    double state = 0.0;
    walk(state, [&](int cs, int row, double best, int bi) { track_store_pair((row0 + (size_t)(cs + row)) * ncg + cg, ncg, best, bi, pval, pidx); });
    if (env_last && wv == 0 && cg * TRK_COLS + l < G) env_last[(size_t)b * G + cg * TRK_COLS + l] = state;
}

// SNN: int8 spike raster [B][T][C], C <= 16 (the beamform_ws_kernel family)
__global__ __launch_bounds__(TRK_THREADS) void track_ws_kernel(const int8_t *__restrict__ spikes, const double *__restrict__ ntab_g, int NK,
                                                               const double *__restrict__ Wp, int GT, int C, int T, int G, double a_rise,
                                                               double i_rise, double a_fall, double *__restrict__ pval,
                                                               int32_t *__restrict__ pidx, double *__restrict__ env_last)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    track_one_shot(T, G, pval, pidx, env_last, [&](double &state, const auto &emit) {
        track_ws_walk(smem, spikes + (size_t)blockIdx.y * T * C, C, 0, T, 0, ntab_g, NK, Wp, GT, G, blockIdx.x, a_rise, i_rise, a_fall, state, emit);
    });
}

// complex Beamformer: planar band-passed analytic signal [B][C = 2M][Ts], C <= 16 (the beamform_wsc_kernel family); G = complex DoAs
template <int KM, int KV>
__global__ __launch_bounds__(TRK_THREADS) void track_wsc_kernel(const double *__restrict__ pre, const double *__restrict__ Wp, int GT, int C,
                                                                int T, int Ts, int G, double a_rise, double i_rise, double a_fall,
                                                                double *__restrict__ pval, int32_t *__restrict__ pidx,
                                                                double *__restrict__ env_last)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    track_one_shot(T, G, pval, pidx, env_last, [&](double &state, const auto &emit) {
        track_wsc_walk<KM, KV>(smem, pre + (size_t)blockIdx.y * C * Ts, C, Ts, 0, T, 0, Wp, GT, G, blockIdx.x, a_rise, i_rise, a_fall, state, emit);
    });
}

// pairs [rows][ncg] in ascending column order -> the first maximum of every row (a strictly larger value takes over)
__global__ __launch_bounds__(256) void track_combine_kernel(const double *__restrict__ pval, const int32_t *__restrict__ pidx, size_t rows,
                                                            int ncg, int32_t *__restrict__ index, double *__restrict__ peak)
{
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    double best;
    int bi;
    track_combine_row(pval + row * ncg, pidx + row * ncg, ncg, best, bi);
    index[row] = track_row_index(bi);
    if (peak) peak[row] = track_row_peak(best, bi);
}

size_t track_pairs_bytes(int B, int T, int G) { return track_pairs_size((size_t)B * T * track_col_groups(G)); }

// the launches of a fused call: launch(grid, pval, pidx) starts the one-shot kernel on a (column groups, trials) grid -- with one column
// group it writes the result itself, else the pairs of `pairs` (track_pairs_bytes), which track_combine_kernel then finishes
template <class Launch>
static hipError_t track_launch_fused(int B, int T, int G, int32_t *index, double *peak, void *pairs, hipStream_t stream, const Launch &launch)
{
    const int ncg = track_col_groups(G);
    double *pval = peak;
    int32_t *pidx = index;
    if (ncg > 1) track_pairs_split(pairs, (size_t)B * T * ncg, pval, pidx);
    hipError_t e = launch(dim3(ncg, B), pval, pidx);
    if (e != hipSuccess || ncg == 1) return e;
    const size_t rows = (size_t)B * T;
    hipLaunchKernelGGL(track_combine_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, pval, pidx, rows, ncg, index, peak);
    return hipGetLastError();
}

// src: the spike raster (real bf_mat) or the planar band-passed rows (complex); G: the DoA grid the caller sees; pairs: track_pairs_bytes
hipError_t launch_track_fused(const BeamformW &W, const NeuronTab &nt, int is_complex, const void *src, int B, int T, int Ts, int G,
                              double a_rise, double i_rise, double a_fall, int32_t *index, double *peak, double *env_last, void *pairs,
                              hipStream_t stream)
{
    const size_t lds = track_lds_bytes(is_complex != 0, nt.NK);
    return track_launch_fused(B, T, G, index, peak, pairs, stream, [&](dim3 grid, double *pval, int32_t *pidx) {
        const dim3 block(TRK_THREADS);
        if (!is_complex) {
            auto k = &track_ws_kernel;
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k, grid, block, lds, stream, static_cast<const int8_t *>(src), nt.tab, nt.NK, W.Wp, W.GT, W.C, T, G, a_rise, i_rise,
                               a_fall, pval, pidx, env_last);
        } else {
            const double *pre = static_cast<const double *>(src);
            const bool served = track_wsc_dispatch(W.C, [&](auto k) {
                hipLaunchKernelGGL((track_wsc_kernel<decltype(k)::km, decltype(k)::kv>), grid, block, lds, stream, pre, W.Wp, W.GT, W.C, T, Ts, G,
                                   a_rise, i_rise, a_fall, pval, pidx, env_last);
            });
            if (!served) return hipErrorInvalidValue;
        }
        return hipGetLastError();
    });
}

// ---- wideband: F bands, one magnitude tile (the rule: include/micloc_hip.h, "wideband moving-target tracking") ----
// The walks over the bands of a chunk are track_bands_ws_walk / track_bands_wsc_walk of track_bands_rows.h, which the streaming band
// kernels of stream_track_bands.hip run as well; here they walk a whole recording: the range (0, T, 0), the rows' stride the recording's.
__global__ __launch_bounds__(TRK_THREADS) void track_bands_ws_kernel(TrackBandsArgs a, int F, int NKmax, int C, int T, int G, double a_rise,
                                                                     double i_rise, double a_fall, double *__restrict__ pval,
                                                                     int32_t *__restrict__ pidx, double *__restrict__ env_last)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    track_one_shot(T, G, pval, pidx, env_last, [&](double &state, const auto &emit) {
        track_bands_ws_walk(smem, a, F, NKmax, blockIdx.y, C, T, 0, T, 0, G, blockIdx.x, a_rise, i_rise, a_fall, state, emit);
    });
}

template <int KM, int KV>
__global__ __launch_bounds__(TRK_THREADS) void track_bands_wsc_kernel(TrackBandsArgs a, int F, int C, int T, int Ts, int G, double a_rise,
                                                                      double i_rise, double a_fall, double *__restrict__ pval,
                                                                      int32_t *__restrict__ pidx, double *__restrict__ env_last)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    track_one_shot(T, G, pval, pidx, env_last, [&](double &state, const auto &emit) {
        track_bands_wsc_walk<KM, KV>(smem, a, F, blockIdx.y, C, Ts, 0, T, 0, G, blockIdx.x, a_rise, i_rise, a_fall, state, emit);
    });
}

bool track_bands_fused_eligible(const BeamformW *const *W, const NeuronTab *const *nt, int F, int is_complex)
{
    int NKmax = 0;
    for (int f = 0; f < F; ++f) {
        if (!track_fused_eligible(*W[f], *nt[f], is_complex)) return false;
        if (W[f]->GT != W[0]->GT || W[f]->C != W[0]->C) return false;  // (one grid and one channel count: one launch shape)
        if (!is_complex && nt[f]->NK > NKmax) NKmax = nt[f]->NK;
    }
    return track_lds_bytes(is_complex != 0, NKmax) <= 160 * 1024;
}

hipError_t launch_track_bands_fused(const TrackBandsArgs &a, int F, int NKmax, int is_complex, int C, int B, int T, int Ts, int G, double a_rise,
                                    double i_rise, double a_fall, int32_t *index, double *peak, double *env_last, void *pairs,
                                    hipStream_t stream)
{
    const size_t lds = track_lds_bytes(is_complex != 0, NKmax);
    return track_launch_fused(B, T, G, index, peak, pairs, stream, [&](dim3 grid, double *pval, int32_t *pidx) {
        const dim3 block(TRK_THREADS);
        if (!is_complex) {
            auto k = &track_bands_ws_kernel;
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k, grid, block, lds, stream, a, F, NKmax, C, T, G, a_rise, i_rise, a_fall, pval, pidx, env_last);
        } else {
            const bool served = track_wsc_dispatch(C, [&](auto k) {
                hipLaunchKernelGGL((track_bands_wsc_kernel<decltype(k)::km, decltype(k)::kv>), grid, block, lds, stream, a, F, C, T, Ts, G, a_rise,
                                   i_rise, a_fall, pval, pidx, env_last);
            });
            if (!served) return hipErrorInvalidValue;
        }
        return hipGetLastError();
    });
}

// the band sum of the two-step route, element by element: the magnitude expressions of the tiles above and their one rounded add
template <bool CPX>
__global__ __launch_bounds__(256) void track_bands_magnitude_kernel(const double *__restrict__ y, size_t n, int first, double *__restrict__ m)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = CPX ? track_magnitude(y[2 * i], y[2 * i + 1]) : fabs(y[i]);
    m[i] = first ? v : __dadd_rn(m[i], v);
}

hipError_t launch_track_bands_magnitude(const double *y, int is_complex, size_t n, int first, double *m, hipStream_t stream)
{
    const size_t nblk = (n + 255) / 256;
    if (nblk > 0x7fffffffull) return hipErrorInvalidValue;
    if (is_complex)
        hipLaunchKernelGGL(track_bands_magnitude_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, stream, y, n, first, m);
    else
        hipLaunchKernelGGL(track_bands_magnitude_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, stream, y, n, first, m);
    return hipGetLastError();
}

// ---- the read-out of the two-step route (the shapes the general beamforming kernel serves): rows of a stored envelope ----
// index[row] = first maximum of env[row, :], peak[row] = its value (row_first_max of readout_rows.h, as rows_argmax_kernel; one wave per row)
__global__ __launch_bounds__(256) void track_rows_kernel(const double *__restrict__ env, size_t rows, int G, int32_t *__restrict__ index,
                                                         double *__restrict__ peak)
{
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int l = threadIdx.x & 63;
    double best;
    int bi;
    row_first_max(env + row * G, G, l, best, bi);
    if (l == 0) {
        index[row] = track_row_index(bi);
        if (peak) peak[row] = track_row_peak(best, bi);
    }
}

__global__ __launch_bounds__(256) void track_last_row_kernel(const double *__restrict__ env, int B, int T, int G, double *__restrict__ env_last)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * G) return;
    const int b = i / G, g = i - b * G;
    env_last[i] = env[((size_t)b * T + (T - 1)) * G + g];
}

hipError_t launch_track_rows(const double *env, int B, int T, int G, int32_t *index, double *peak, double *env_last, hipStream_t stream)
{
    const size_t rows = (size_t)B * T;
    hipLaunchKernelGGL(track_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, env, rows, G, index, peak);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !env_last) return e;
    hipLaunchKernelGGL(track_last_row_kernel, dim3((B * G + 255) / 256), dim3(256), 0, stream, env, B, T, G, env_last);
    return hipGetLastError();
}

}  // namespace micloc
