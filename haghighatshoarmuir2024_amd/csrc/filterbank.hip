// Wideband front and back end for gfx950: the filterbank of the live demo (micloc/localization_demo_snn.py:160-164,
// micloc/filterbank.py:25-46: scipy.signal.lfilter per band) as ONE launch for all bands of a batch, and the sum of the per-band
// angular power patterns with its arg-max (:166-190).
//
// filterbank_kernel: x [B][T][M] -> xf [F][B][T][M].  The arithmetic is the project's DF2T contract from zero state, Df2tChain<N>
// (bandpass_rows.h) -- every term, no zero-coefficient skipping, so the results are those of micloc_lfilter_f64 band by band.  Time is
// serial per (band, trial, microphone) chain: one lane owns one chain.
//   * A workgroup owns one trial (and a group of `mg` microphones: all of them unless (1 + F) * M > FB_MAX_ROWS) with ALL its
//     bands: an input tile of FB_TT frames comes from HBM once and every band reads it from LDS (lanes of different bands read the
//     same address: a broadcast).
//   * Global traffic goes through LDS time tiles: a tile of a trial is one contiguous run of FB_TT * M doubles in x and in every
//     band's slice of xf, read and written by all 256 threads 8 bytes per lane in address order (a frame row is M doubles -- 56 B at
//     M = 7 -- so nothing wider is aligned).  Only the chain lanes (F * mg <= 64: one wave) run the serial recurrence.
//   * Both LDS tiles are double buffered and there is ONE barrier per tile: while tile k is filtered, the loads of tile k + 1 are in
//     flight into registers (issued before the recurrence, written to LDS after it) and tile k - 1 is on its way out.
//   * The chain lanes take the tile in groups of 8 steps: 8 LDS reads, 8 steps in registers, 8 LDS writes -- the reads of a group do
//     not wait behind the writes of the one before.
// No time chunking: a lone, very long recording runs at the pace of one chain (the live demo's packs are 12 000 frames).
//
// filterbank_tile_kernel: the same tile loop for ONE TILE of a stream, x_tile [B][n][M] -> xf_tile [F][B][n][M], with the DF2T state of
// every chain loaded from and stored to a device block (micloc_filterbank_tile_f64; the band chains and the band sum of a streamed
// tile are in stream_bands.hip).
//
// band_sum_kernel: band_power [F][R][G] -> power [R][G] = ((p_0 + p_1) + p_2) + ... in ascending band order (__dadd_rn, starting
// from p_0: the additions of Demo.power_grid) and argmax [R] with power_argmax_kernel's rule (first maximum, a NaN never wins, a
// row of NaN only gives 0).  One workgroup per row, no atomics.
#include "bandpass_rows.h"
#include "readout_rows.h"

namespace micloc {

constexpr int FB_TT = 64;         // frames per time tile
constexpr int FB_THREADS = 256;
constexpr int FB_MAX_ROWS = 64;   // (1 + F) * mg <= FB_MAX_ROWS: LDS = 2 buffers x (1 + F) mg rows of (FB_TT + 1) doubles <= 65 KB
constexpr int FB_MAX_MG = 16;     // microphones per workgroup (FB_XREG registers hold a thread's share of an input tile)
constexpr int FB_XREG = FB_TT * FB_MAX_MG / FB_THREADS;
constexpr int FB_GROUP = 8;       // steps per register group of the recurrence

// LDS: [2][xin: mg rows... ] as time-major tiles.  xin[buf][t * mg + j]; yout[buf][f][t * mg + j] with a band stride of
// (FB_TT + 1) * mg doubles: lanes (f, j) of one step then write F * mg different banks (up to 16 doubles) instead of F-way conflicts.
//
// fb_tiles<N, Resume> is the tile loop of both kernels.  Resume = false: the one-shot filterbank_kernel, zero state, exactly the code it
// always was (`state` is not touched and every `if (Resume)` below is a compile-time false).  Resume = true: filterbank_tile_kernel,
// one tile of a stream -- each chain lane loads its n - 1 DF2T states from `state` before the first LDS tile and stores them after the
// last; the steps are the same Df2tChain<N>::step calls in the same order, so a stream cut into tiles at any frames gives the bits of one
// call on the whole recording.  The only difference in the loop: the one-shot kernel may run the recurrence over the zero frames that
// pad its last group of 8 (nothing of them is stored); the stream's state must not see them, so its ragged last group is stepped
// frame by frame.  state layout: [B][n - 1][F][M] doubles -- element i of chain (f, b, m) at ((b (n - 1) + i) F + f) M + m -- so the
// F * mw chain lanes c = f * mw + j of a workgroup read and write consecutive addresses per i when the workgroup owns all M microphones.
template <int N, bool Resume>
__device__ __forceinline__ void fb_tiles(double *fb_lds, const FilterbankCoef &co, const double *__restrict__ x, int F, int B, int T, int M,
                                         int mg, int ngroups, double *__restrict__ xf, double *__restrict__ state)
{
    const int tid = threadIdx.x;
    const int b = blockIdx.x / ngroups;
    const int m0 = (blockIdx.x - b * ngroups) * mg;
    const int mw = M - m0 < mg ? M - m0 : mg;  // microphones of this workgroup (the last group may be narrower)
    const bool full = mw == M;                 // the tile is one contiguous run
    const int xin_sz = FB_TT * mg, bstride = (FB_TT + 1) * mg, yout_sz = F * bstride;
    double *xin = fb_lds;                      // [2][xin_sz]
    double *yout = fb_lds + 2 * xin_sz;        // [2][yout_sz]
    const size_t trial = (size_t)T * M;        // doubles per trial
    const double *xb = x + (size_t)b * trial + m0;
    const int ntiles = (T + FB_TT - 1) / FB_TT;

    // chain lanes: lane c = f * mw + j
    const bool chain = tid < F * mw;
    const int cf = chain ? tid / mw : 0, cj = chain ? tid - (tid / mw) * mw : 0;
    Df2tChain<N> ch;
    ch.init(co, cf);
    // the chain's state word i (Resume only); all indices size_t
    auto sidx = [&](int i) -> size_t { return (((size_t)b * (N - 1) + i) * F + cf) * M + m0 + cj; };
    if (Resume && N > 1 && chain) {
#pragma unroll
        for (int i = 0; i < N - 1; ++i) ch.z[i] = state[sidx(i)];
    }

    // element e of a tile (e < frames * mw) -> offset from the tile's first frame row
    auto goff = [&](int e) -> size_t { return full ? (size_t)e : (size_t)(e / mw) * M + (e - (e / mw) * mw); };

    double xr[FB_XREG];
    auto load_tile = [&](int k) {
        const int nt = T - k * FB_TT < FB_TT ? T - k * FB_TT : FB_TT;
        const double *src = xb + (size_t)k * FB_TT * M;
#pragma unroll
        for (int r = 0; r < FB_XREG; ++r) {
            const int e = tid + r * FB_THREADS;
            xr[r] = e < nt * mw ? src[goff(e)] : 0.0;
        }
    };
    auto stash_tile = [&](int k) {
        double *dst = xin + (k & 1) * xin_sz;
#pragma unroll
        for (int r = 0; r < FB_XREG; ++r) {
            const int e = tid + r * FB_THREADS;
            if (e < FB_TT * mw) dst[e] = xr[r];  // (frames past T hold zeros: the recurrence may run over them, nothing is stored)
        }
    };
    auto store_tile = [&](int k) {
        const int nt = T - k * FB_TT < FB_TT ? T - k * FB_TT : FB_TT;
        const double *src = yout + (k & 1) * yout_sz;
        for (int f = 0; f < F; ++f) {
            double *dst = xf + ((size_t)f * B + b) * trial + (size_t)k * FB_TT * M + m0;
            for (int e = tid; e < nt * mw; e += FB_THREADS) dst[goff(e)] = src[f * bstride + e];
        }
    };

    load_tile(0);
    stash_tile(0);
    __syncthreads();
    for (int k = 0; k < ntiles; ++k) {
        if (k + 1 < ntiles) load_tile(k + 1);  // in flight during the recurrence below
        if (k > 0) store_tile(k - 1);
        if (chain) {
            const int nt = T - k * FB_TT < FB_TT ? T - k * FB_TT : FB_TT;
            const double *xi = xin + (k & 1) * xin_sz + cj;
            double *yo = yout + (k & 1) * yout_sz + cf * bstride + cj;
            const int ngrp = Resume ? nt - nt % FB_GROUP : nt;  // (one-shot: the last group may run over the padding zeros)
            for (int t0 = 0; t0 < ngrp; t0 += FB_GROUP) {
                double v[FB_GROUP];
#pragma unroll
                for (int u = 0; u < FB_GROUP; ++u) v[u] = xi[(t0 + u) * mw];
#pragma unroll
                for (int u = 0; u < FB_GROUP; ++u) v[u] = ch.step(v[u]);
#pragma unroll
                for (int u = 0; u < FB_GROUP; ++u) yo[(t0 + u) * mw] = v[u];
            }
            if (Resume) {
                for (int t = ngrp; t < nt; ++t) yo[t * mw] = ch.step(xi[t * mw]);  // the ragged end of the stream's tile: no step past it
            }
        }
        if (k + 1 < ntiles) stash_tile(k + 1);
        __syncthreads();
    }
    store_tile(ntiles - 1);
    if (Resume && N > 1 && chain) {
#pragma unroll
        for (int i = 0; i < N - 1; ++i) state[sidx(i)] = ch.z[i];
    }
}

template <int N>
__global__ __launch_bounds__(FB_THREADS) void filterbank_kernel(const FilterbankCoef co, const double *__restrict__ x, int F, int B, int T,
                                                                  int M, int mg, int ngroups, double *__restrict__ xf)
{
    extern __shared__ __attribute__((aligned(16))) double fb_lds[];
    fb_tiles<N, false>(fb_lds, co, x, F, B, T, M, mg, ngroups, xf, nullptr);
}

// one tile of a stream: x_tile [B][T][M] -> xf_tile [F][B][T][M] with the chains' states carried in `state` (layout above)
template <int N>
__global__ __launch_bounds__(FB_THREADS) void filterbank_tile_kernel(const FilterbankCoef co, const double *__restrict__ x, int F, int B, int T,
                                                                       int M, int mg, int ngroups, double *__restrict__ xf,
                                                                       double *__restrict__ state)
{
    extern __shared__ __attribute__((aligned(16))) double fb_lds[];
    fb_tiles<N, true>(fb_lds, co, x, F, B, T, M, mg, ngroups, xf, state);
}

// microphones per workgroup: all of them when the trial's tiles fit the LDS budget
static int fb_mic_group(int F, int M)
{
    int mg = FB_MAX_ROWS / (1 + F);
    if (mg > FB_MAX_MG) mg = FB_MAX_MG;
    if (mg > M) mg = M;
    return mg < 1 ? 1 : mg;
}

template <int N>
static hipError_t fb_launch(const FilterbankCoef &co, const double *x, int F, int B, int T, int M, double *xf, hipStream_t stream)
{
    const int mg = fb_mic_group(F, M);
    const int ngroups = (M + mg - 1) / mg;
    const size_t lds = (size_t)2 * (FB_TT * mg + (size_t)F * (FB_TT + 1) * mg) * sizeof(double);
    const long long blocks = (long long)B * ngroups;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filterbank_kernel<N>, dim3((unsigned)blocks), dim3(FB_THREADS), lds, stream, co, x, F, B, T, M, mg, ngroups, xf);
    return hipGetLastError();
}

hipError_t launch_filterbank(const FilterbankCoef &co, const double *x, int F, int B, int T, int M, double *xf, hipStream_t stream)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || B < 1 || T < 1 || M < 1) return hipErrorInvalidValue;
    return dispatch_iir_order(co.n, [&](auto N) { return fb_launch<decltype(N)::value>(co, x, F, B, T, M, xf, stream); });
}

// ---- the resumable form ----------------------------------------------------------------------------------------------------------
size_t filterbank_stream_state_bytes(int F, int n, int B, int M)
{
    const size_t words = (size_t)F * B * M * (n - 1);
    const size_t bytes = (words * sizeof(double) + 255) & ~(size_t)255;
    return bytes < 256 ? 256 : bytes;  // (n = 1 has no state: one unused block, so that 0 can mean "bad arguments")
}

template <int N>
static hipError_t fb_tile_launch(const FilterbankCoef &co, const double *x, int F, int B, int T, int M, double *xf, double *state, hipStream_t stream)
{
    const int mg = fb_mic_group(F, M);
    const int ngroups = (M + mg - 1) / mg;
    const size_t lds = (size_t)2 * (FB_TT * mg + (size_t)F * (FB_TT + 1) * mg) * sizeof(double);
    const long long blocks = (long long)B * ngroups;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filterbank_tile_kernel<N>, dim3((unsigned)blocks), dim3(FB_THREADS), lds, stream, co, x, F, B, T, M, mg, ngroups, xf, state);
    return hipGetLastError();
}

hipError_t launch_filterbank_tile(const FilterbankCoef &co, const double *x, int F, int B, int T, int M, double *xf, double *state,
                                  hipStream_t stream)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || B < 1 || T < 1 || M < 1 || !state) return hipErrorInvalidValue;
    return dispatch_iir_order(co.n, [&](auto N) { return fb_tile_launch<decltype(N)::value>(co, x, F, B, T, M, xf, state, stream); });
}

// (the arg-max: this kernel's scan -- band sums may be negative -- then block_first_max of readout_rows.h)
// ---- band sum + arg-max ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void band_sum_kernel(const double *__restrict__ band_power, int F, size_t R, int G,
                                                        double *__restrict__ power, int32_t *__restrict__ argmax)
{
    __shared__ double sv[256];
    __shared__ int si[256];
    const size_t r = blockIdx.x;
    const size_t band = R * (size_t)G;  // doubles per band
    const double *p0 = band_power + r * G;
    double best = 0.0;
    int bi = RO_NONE;
    for (int g = threadIdx.x; g < G; g += 256) {
        double s = p0[g];
        for (int f = 1; f < F; ++f) s = __dadd_rn(s, p0[(size_t)f * band + g]);
        if (power) power[r * G + g] = s;
        if (s == s && (bi == RO_NONE || s > best)) {  // ascending g per thread: the first maximum; a NaN never wins
            best = s;
            bi = g;
        }
    }
    const int a = block_first_max<256>(best, bi, sv, si, (int)threadIdx.x);
    if (threadIdx.x == 0 && argmax) argmax[r] = a;
}

hipError_t launch_band_sum(const double *band_power, int F, long long R, int G, double *power, int32_t *argmax, hipStream_t stream)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || R < 1 || R > 0x7fffffffll || G < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(band_sum_kernel, dim3((unsigned)R), dim3(256), 0, stream, band_power, F, (size_t)R, G, power, argmax);
    return hipGetLastError();
}

}  // namespace micloc
