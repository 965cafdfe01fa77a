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
//      hypot(re, im) as EnvIn<MICLOC_ENV_C128>) goes to an LDS tile [64 frames][64 columns].
//   3. wave 0 walks the 64 envelope chains (one lane per column) over the tile in place: envelope_kernel's recurrence, __dmul_rn /
//      __dadd_rn, nothing fused, state_0 = |y_0|, rise when |y_t| >= state.  The chain state stays in a register across chunks.
//   4. every frame of the tile is reduced to (max envelope, first index) over the workgroup's columns by rows_argmax_kernel's rule
//      (first maximum; a NaN never wins).  With one column group (G <= 64) that is the result; otherwise the pairs go to
//      pval / pidx [B][T][ceil(G / 64)] and track_combine_kernel finishes in ascending column order.
// No buffer grows with T G.  The chain is latency (one wave, ~8 dependent instructions per step); the matrix work of a chunk is a few
// hundred cycles per wave, and several workgroups share a compute unit (46 KB of LDS), so one workgroup's chain runs beside the
// others' staging and matrix phases.
#include "track_rows.h"

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

// SNN: int8 spike raster [B][T][C], C <= 16 (the beamform_ws_kernel family)
__global__ __launch_bounds__(TRK_THREADS) void track_ws_kernel(const int8_t *__restrict__ spikes, const double *__restrict__ ntab_g, int NK,
                                                               const double *__restrict__ Wp, int GT, int C, int T, int G, double a_rise,
                                                               double i_rise, double a_fall, double *__restrict__ pval,
                                                               int32_t *__restrict__ pidx, double *__restrict__ env_last)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
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
    // bf_mat fragments of the workgroup's four DoA tiles, once (a tile beyond the grid multiplies a clamped one; its columns are never read)
    double Wf[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gt = 4 * cg + j;
        const double *wp = Wp + 16 * (gt < GT ? gt : GT - 1) + lc;
#pragma unroll
        for (int k = 0; k < 4; ++k) Wf[j][k] = wp[(size_t)(4 * k + q) * Gp];
    }
    const int8_t *sb = spikes + (size_t)b * T * C;
    const size_t row0 = (size_t)b * T;
    double state = 0.0;
    for (int cs = 0; cs < T; cs += TRK_CH) {
        {  // rows tau0 .. tau0 + R - 1 of the raster; rows outside [0, T) and the channel padding are zero
            const int tau0 = cs + 16 - 4 * NK;
            const int c = tid & 15;
            for (int rho = tid >> 4; rho < R; rho += TRK_THREADS / 16) {
                const int tau = tau0 + rho;
                const bool ok = c < C && tau >= 0 && tau < T;
                S[rho * 16 + c] = ok ? (double)sb[(size_t)tau * C + c] : 0.0;
            }
        }
        __syncthreads();
        // ---- membrane fragments of this wave's tile (beamform_ws_kernel, stage 1) ----
        const int tb0 = cs + wv * 16;
        double4_t vacc = double4_t{0.0, 0.0, 0.0, 0.0};
        if (tb0 < T) {  // (wave-uniform)
            const double *sp = S + (size_t)(wv * 16 + q) * 16 + lc;
            const double *np_ = ntab + (lc - q + 4 * NK - 1);
            for (int ks = 0; ks < NK; ++ks) vacc = __builtin_amdgcn_mfma_f64_16x16x4f64(sp[ks * 64], np_[-4 * ks], vacc, 0, 0, 0);
            if (tb0 + 16 > T) {
                const bool tvalid = (tb0 + lc) < T;
#pragma unroll
                for (int r = 0; r < 4; ++r) vacc[r] = tvalid ? vacc[r] : 0.0;
            }
        }
        // ---- y of the tile against the four DoA tiles, |y| into the LDS tile ----
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
        track_chain_reduce(Y, wv, l, tid, cs == 0, nrow, G, cg, a_rise, i_rise, a_fall, state, [&](int row, double best, int bi) {
            track_store_pair((row0 + (size_t)(cs + row)) * ncg + cg, ncg, best, bi, pval, pidx);
        });
        // (the next chunk's staging touches S only; its writes to Y come after the barrier behind the staging)
    }
    if (env_last && wv == 0 && cg * TRK_COLS + l < G) env_last[(size_t)b * G + cg * TRK_COLS + l] = state;
}

// complex Beamformer: planar band-passed analytic signal [B][C = 2M][Ts], C <= 16 (the beamform_wsc_kernel family); G = complex DoAs
template <int KM, int KV>
__global__ __launch_bounds__(TRK_THREADS) void track_wsc_kernel(const double *__restrict__ pre, const double *__restrict__ Wp, int GT, int C,
                                                                int T, int Ts, int G, double a_rise, double i_rise, double a_fall,
                                                                double *__restrict__ pval, int32_t *__restrict__ pidx,
                                                                double *__restrict__ env_last)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int KF = KM + (KV > 0 ? 1 : 0);
    constexpr int KVD = KV > 0 ? KV : 1;
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
    const double *pb = pre + (size_t)b * C * Ts;
    const size_t row0 = (size_t)b * T;
    double state = 0.0;
    for (int cs = 0; cs < T; cs += TRK_CH) {
        // ---- this wave's tile as A-fragments (beamform_wsc_kernel, stage 1): lane l of k-step k = channel 4k + (l >> 4), frame l & 15 ----
        double V[KF];
        {
            const int t = cs + wv * 16 + lc;
#pragma unroll
            for (int k = 0; k < KF; ++k) {
                const int c = 4 * k + q;
                const double v = pb[(size_t)(c < C ? c : C - 1) * Ts + (t < T ? t : T - 1)];  // (clamped: unconditional loads)
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
        track_chain_reduce(Y, wv, l, tid, cs == 0, nrow, G, cg, a_rise, i_rise, a_fall, state, [&](int row, double best, int bi) {
            track_store_pair((row0 + (size_t)(cs + row)) * ncg + cg, ncg, best, bi, pval, pidx);
        });
    }
    if (env_last && wv == 0 && cg * TRK_COLS + l < G) env_last[(size_t)b * G + cg * TRK_COLS + l] = state;
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

size_t track_pairs_bytes(int B, int T, int G)
{
    const size_t n = (size_t)B * T * track_col_groups(G);
    return ((n * sizeof(double) + 255) & ~(size_t)255) + ((n * sizeof(int32_t) + 255) & ~(size_t)255);
}

// src: the spike raster (real bf_mat) or the planar band-passed rows (complex); G: the DoA grid the caller sees; pairs: track_pairs_bytes
hipError_t launch_track_fused(const BeamformW &W, const NeuronTab &nt, int is_complex, const void *src, int B, int T, int Ts, int G,
                              double a_rise, double i_rise, double a_fall, int32_t *index, double *peak, double *env_last, void *pairs,
                              hipStream_t stream)
{
    const int ncg = track_col_groups(G);
    const size_t n = (size_t)B * T * ncg;
    double *pval = ncg == 1 ? peak : reinterpret_cast<double *>(pairs);
    int32_t *pidx = ncg == 1 ? index : reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(pairs) + ((n * sizeof(double) + 255) & ~(size_t)255));
    const size_t lds = track_lds_bytes(is_complex != 0, nt.NK);
    dim3 grid(ncg, B), block(TRK_THREADS);
    if (!is_complex) {
        auto k = &track_ws_kernel;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k, grid, block, lds, stream, static_cast<const int8_t *>(src), nt.tab, nt.NK, W.Wp, W.GT, W.C, T, G, a_rise, i_rise,
                           a_fall, pval, pidx, env_last);
    } else {
        const double *pre = static_cast<const double *>(src);
#define TRK_K(KM_, KV_)                                                                                                                   \
    hipLaunchKernelGGL((track_wsc_kernel<KM_, KV_>), grid, block, lds, stream, pre, W.Wp, W.GT, W.C, T, Ts, G, a_rise, i_rise, a_fall, pval, \
                       pidx, env_last);                                                                                                   \
    break
        switch (W.C) {  // (2 x microphones: even; beamform_wsc_kernel's table)
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
    const size_t rows = (size_t)B * T;
    hipLaunchKernelGGL(track_combine_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, pval, pidx, rows, ncg, index, peak);
    return hipGetLastError();
}

// ---- the read-out of the two-step route (the shapes the general beamforming kernel serves): rows of a stored envelope ----
// index[row] = first maximum of env[row, :], peak[row] = its value (rows_argmax_kernel's rule; one wave per row)
__global__ __launch_bounds__(256) void track_rows_kernel(const double *__restrict__ env, size_t rows, int G, int32_t *__restrict__ index,
                                                         double *__restrict__ peak)
{
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int l = threadIdx.x & 63;
    const double *r = env + row * G;
    double best = -1.0;
    int bi = TRK_NONE;
    for (int g = l; g < G; g += 64) {
        const double v = r[g];
        if (v > best) {
            best = v;
            bi = g;
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double ov = __shfl_xor(best, s, 64);
        const int oi = __shfl_xor(bi, s, 64);
        if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
    if (l == 0) {
        index[row] = bi == TRK_NONE ? 0 : bi;
        if (peak) peak[row] = bi == TRK_NONE ? (double)NAN : best;
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
