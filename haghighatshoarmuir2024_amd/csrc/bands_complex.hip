// Wideband form of the complex Beamformer's front end (micloc_beamformer_pipeline_bands_f64): the band-pass of the analytic signal for
// ALL bands of a batch in ONE launch.  The rule is stated in include/micloc_hip.h ("wideband localisation, complex Beamformer"); DESIGN
// 4.17 has the footprint and the measurement.
//
// bands_bandpass_kernel<N, CH>: chain g of the F * B * 2M chains is (band f, trial b, channel c) = (g / (B 2M), (g / 2M) % B, g % 2M).
//   * in-phase channels c < M read the filterbank's output xf [F][B][T][M] through the roll's index map, x[(t - L/2) mod T][c] (the
//     map of rzcc.hip's loaders, which the one-shot complex front end reads `x` with); quadrature channels read the planar STHT rows
//     h [F B][2M][Ts] (rows c >= M; the in-phase rows of h are never written and never read);
//   * band f filters with row f of the coefficient table, which travels by value as FilterbankCoef does (the plans' own band-pass
//     coefficients, already divided by a[0]);
//   * the arithmetic is the project's DF2T contract from zero state, rzcc.hip's Iir<N>::step restated as filterbank.hip and
//     stream_complex.hip restate it (rzcc.hip is pinned by the profile manifest): the same fmas in the same order, every term computed;
//   * output: the planar rows pre [F B][2M][Ts] launch_planar_beamform reads, frames [T, Ts) zero.
// One lane per chain.  The frames go through LDS time tiles of BC_TT frames, double buffered, filtered in place, ONE barrier per tile
// (the loop of stream_bandpass_tile_kernel): while tile k is filtered the loads of tile k + 1 are in flight into registers and tile
// k - 1 is on its way out; every thread stores and stashes the SAME elements of a tile, so the buffer tile k - 1 leaves from can take
// tile k + 1 without a second barrier.  The step is latency bound whatever the number of live lanes, so CH -- chains per workgroup, the
// lanes of wave 0 that run a recurrence -- is a template parameter: the launcher takes the smallest of {16, 32, 64} that keeps the
// launch at one resident round, so that as many SIMDs as possible carry a recurrence and the movers' share of a tile stays small.
#include "micloc_internal.h"

namespace micloc {

namespace {

constexpr int BC_TT = 32;           // frames per LDS time tile
constexpr int BC_ROW = BC_TT + 1;   // padded row (doubles): the chain lanes of one step fall into different banks
constexpr int BC_THREADS = 256;
constexpr int BC_GROUP = 8;         // steps per register group of the recurrence

template <int N>
struct BcChain {
    double b[N], a[N];
    double z[N > 1 ? N - 1 : 1];

    __device__ __forceinline__ void init(const FilterbankCoef &co, int f)
    {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            b[i] = co.b[f][i];
            a[i] = co.a[f][i];
        }
#pragma unroll
        for (int i = 0; i < (N > 1 ? N - 1 : 1); ++i) z[i] = 0.0;
    }

    // the DF2T step of the contract, operation for operation rzcc.hip's Iir<N>::step
    __device__ __forceinline__ double step(double xin)
    {
        double y;
        if (N == 1) {
            y = __builtin_fma(b[0], xin, 0.0);
        } else {
            y = __builtin_fma(b[0], xin, z[0]);
#pragma unroll
            for (int i = 0; i < N - 2; ++i) z[i] = __builtin_fma(-a[i + 1], y, __builtin_fma(b[i + 1], xin, z[i + 1]));
            z[N - 2] = __builtin_fma(-a[N - 1], y, b[N - 1] * xin);
        }
        return y;
    }
};

// nl = F * band_chains chains, band_chains = B * C, C = 2M; sh = (L / 2) % T, the roll.  All indices into xf, h and pre are size_t.
template <int N, int CH>
__global__ __launch_bounds__(BC_THREADS) void bands_bandpass_kernel(const FilterbankCoef co, const double *__restrict__ xf,
                                                                     const double *__restrict__ h, int nl, int band_chains, int C, int M, int T,
                                                                     int Ts, int sh, double *__restrict__ pre)
{
    constexpr int SHARE = CH * BC_TT / BC_THREADS;  // elements of a tile per thread
    static_assert(SHARE >= 1 && CH <= 64, "a tile is shared by all threads and one wave carries the chains");
    __shared__ double tile[2][CH * BC_ROW];
    const int tid = threadIdx.x;
    const int g0 = blockIdx.x * CH;
    const int rows = nl - g0 < CH ? nl - g0 : CH;  // chains of this workgroup
    const int ntiles = (T + BC_TT - 1) / BC_TT;    // (Ts <= ntiles * BC_TT: Ts is T rounded up to 8)

    const bool chain = tid < rows;
    BcChain<N> chn;
    chn.init(co, chain ? (g0 + tid) / band_chains : 0);

    // element e of a tile: row e / BC_TT, frame e % BC_TT (consecutive threads: consecutive frames of one row).  The row of an element does
    // not depend on the tile, so its source is resolved once.
    const double *src[SHARE];
    bool rolled[SHARE], live[SHARE];
    double *dst[SHARE];
#pragma unroll
    for (int r = 0; r < SHARE; ++r) {
        const int e = tid + r * BC_THREADS;
        const int row = e / BC_TT;
        live[r] = row < rows;
        const int g = live[r] ? g0 + row : g0;
        const int trial = g / C, c = g - trial * C;  // trial counts over bands: f * B + b
        rolled[r] = c < M;
        src[r] = rolled[r] ? xf + (size_t)trial * T * M + c : h + (size_t)g * Ts;
        dst[r] = pre + (size_t)g * Ts;
    }

    double xr[SHARE];
    auto load_tile = [&](int k) {
        const int nt = T - k * BC_TT < BC_TT ? T - k * BC_TT : BC_TT;
#pragma unroll
        for (int r = 0; r < SHARE; ++r) {
            const int tl = (tid + r * BC_THREADS) % BC_TT;
            const int t = k * BC_TT + tl;
            int tr = t - sh;
            tr = tr < 0 ? tr + T : tr;
            xr[r] = (live[r] && tl < nt) ? (rolled[r] ? src[r][(size_t)tr * M] : src[r][t]) : 0.0;  // frames past T: the zeros of pre's padding
        }
    };
    auto stash_tile = [&](int k) {
        double *d = tile[k & 1];
#pragma unroll
        for (int r = 0; r < SHARE; ++r) {
            const int e = tid + r * BC_THREADS;
            const int row = e / BC_TT, tl = e - row * BC_TT;
            d[row * BC_ROW + tl] = xr[r];
        }
    };
    auto store_tile = [&](int k) {
        const int ns = Ts - k * BC_TT < BC_TT ? Ts - k * BC_TT : BC_TT;  // (stores reach the padded end of the row: frames [T, Ts) are zero)
        const double *s = tile[k & 1];
#pragma unroll
        for (int r = 0; r < SHARE; ++r) {
            const int e = tid + r * BC_THREADS;
            const int row = e / BC_TT, tl = e - row * BC_TT;
            if (live[r] && tl < ns) dst[r][(size_t)k * BC_TT + tl] = s[row * BC_ROW + tl];
        }
    };

    load_tile(0);
    stash_tile(0);
    __syncthreads();
    for (int k = 0; k < ntiles; ++k) {
        if (k + 1 < ntiles) load_tile(k + 1);  // in flight during the recurrence below
        if (k > 0) store_tile(k - 1);
        if (chain) {
            const int nt = T - k * BC_TT < BC_TT ? T - k * BC_TT : BC_TT;
            double *xi = tile[k & 1] + tid * BC_ROW;
            const int ngrp = nt - nt % BC_GROUP;
            for (int t0 = 0; t0 < ngrp; t0 += BC_GROUP) {
                double v[BC_GROUP];
#pragma unroll
                for (int u = 0; u < BC_GROUP; ++u) v[u] = xi[t0 + u];
#pragma unroll
                for (int u = 0; u < BC_GROUP; ++u) v[u] = chn.step(v[u]);
#pragma unroll
                for (int u = 0; u < BC_GROUP; ++u) xi[t0 + u] = v[u];
            }
            for (int t = ngrp; t < nt; ++t) xi[t] = chn.step(xi[t]);  // the ragged end frame by frame: the padding stays zero
        }
        if (k + 1 < ntiles) stash_tile(k + 1);
        __syncthreads();
    }
    store_tile(ntiles - 1);
}

template <int N, int CH>
hipError_t bc_launch_ch(const FilterbankCoef &co, const double *xf, const double *h, int nl, int band_chains, int C, int M, int T, int Ts, int sh,
                        double *pre, hipStream_t stream)
{
    hipLaunchKernelGGL((bands_bandpass_kernel<N, CH>), dim3((nl + CH - 1) / CH), dim3(BC_THREADS), 0, stream, co, xf, h, nl, band_chains, C, M,
                       T, Ts, sh, pre);
    return hipGetLastError();
}

template <int N>
hipError_t bc_launch(const FilterbankCoef &co, const double *xf, const double *h, int nl, int band_chains, int C, int M, int T, int Ts, int sh,
                     double *pre, hipStream_t stream)
{
    switch (bands_bandpass_chains(nl)) {
        case 16: return bc_launch_ch<N, 16>(co, xf, h, nl, band_chains, C, M, T, Ts, sh, pre, stream);
        case 32: return bc_launch_ch<N, 32>(co, xf, h, nl, band_chains, C, M, T, Ts, sh, pre, stream);
        default: return bc_launch_ch<N, 64>(co, xf, h, nl, band_chains, C, M, T, Ts, sh, pre, stream);
    }
}

}  // namespace

// Chains per workgroup.  256 CUs; a workgroup is four waves, one per SIMD, and 8.4 KB (CH = 16) or 16.9 KB (CH = 32) of LDS; every
// instantiation with CH <= 32 runs at least four waves per SIMD (DESIGN 4.17 has the registers), so four workgroups are resident per CU: up
// to 1024 workgroups run as one round.  Past that the 64-chain form (33.8 KB) keeps the number of rounds down.
int bands_bandpass_chains(int nl)
{
    constexpr int ROUND = 1024;
    if (nl <= 16 * ROUND) return 16;
    if (nl <= 32 * ROUND) return 32;
    return 64;
}

hipError_t launch_bands_bandpass(const FilterbankCoef &co, const double *xf, const double *h, int F, int B, int T, int M, int Ts, int shift,
                                 double *pre, hipStream_t stream)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || B < 1 || T < 1 || M < 1 || Ts < T || Ts > ((T + BC_TT - 1) / BC_TT) * BC_TT || shift < 0)
        return hipErrorInvalidValue;
    const long long nl = (long long)F * B * 2 * M;
    if (nl > 0x7fffffffll) return hipErrorInvalidValue;
    const int C = 2 * M;
#define BC_CASE(NN) \
    case NN: return bc_launch<NN>(co, xf, h, (int)nl, B * C, C, M, T, Ts, shift % T, pre, stream);
    switch (co.n) {
        BC_CASE(1)
        BC_CASE(2)
        BC_CASE(3)
        BC_CASE(4)
        BC_CASE(5)
        BC_CASE(6)
        BC_CASE(7)
        BC_CASE(8)
        BC_CASE(9)
        default: return hipErrorInvalidValue;
    }
#undef BC_CASE
}

}  // namespace micloc
