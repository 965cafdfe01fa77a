// The band-pass of planar rows, one DF2T chain per row, shared by the complex Beamformer's band-pass kernels (stream_complex.hip,
// stream_bands_complex.hip, bands_complex.hip) and, for the chain and the order dispatch, by filterbank.hip:
//   Df2tChain<N>            the DF2T step of the contract, stated ONCE outside the encoder
//   dispatch_iir_order      the filter order 1..9 -> a template argument (dispatch_bandpass_chains: the chains per workgroup)
//   bandpass_rows_tiles     the one-barrier, double-buffered LDS tile pipeline of CH chains per workgroup
//   stream_bandpass_tile    the pipeline as one tile of a stream: carry, state, chunk padding, pending control words
// rzcc.hip and rzcc_sweep.hip keep their own Iir<N>::step: both files are pinned by the profile manifest (their text cannot change
// without a new profile round), which is why the step is restated here -- once -- and not included from them.
#pragma once
#include <type_traits>

#include "micloc_internal.h"

namespace micloc {

// The DF2T step of the contract, operation for operation rzcc.hip's Iir<N>::step:
//   y = fma(b0, x, z0); z_i = fma(-a_{i+1}, y, fma(b_{i+1}, x, z_{i+1})); z_{n-2} = fma(-a_{n-1}, y, b_{n-1} * x)
// -- the same fmas in the same order, every term computed (no zero-coefficient skipping), coefficients already divided by a[0].  init
// leaves the state zero; a resumed chain overwrites z afterwards.
template <int N>
struct Df2tChain {
    double b[N], a[N];
    double z[N > 1 ? N - 1 : 1];

    // uniform coefficients: every chain of the launch filters with `co`
    __device__ __forceinline__ void init(const IirCoef &co)
    {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            b[i] = co.b[i];
            a[i] = co.a[i];
        }
#pragma unroll
        for (int i = 0; i < (N > 1 ? N - 1 : 1); ++i) z[i] = 0.0;
    }

    // band f of a filterbank
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

// f(std::integral_constant<int, n>) for a filter order n in 1..MICLOC_MAX_IIR, hipErrorInvalidValue otherwise
template <class F>
hipError_t dispatch_iir_order(int n, F &&f)
{
    static_assert(MICLOC_MAX_IIR == 9, "one case per order");
    switch (n) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 9: return f(std::integral_constant<int, 9>{});
        default: return hipErrorInvalidValue;
    }
}

// f(std::integral_constant<int, chains>) for the chains per workgroup the band-pass kernels are instantiated for
template <class F>
hipError_t dispatch_bandpass_chains(int chains, F &&f)
{
    switch (chains) {
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        default: return hipErrorInvalidValue;
    }
}

constexpr int BR_TT = 32;           // frames per LDS time tile
constexpr int BR_ROW = BR_TT + 1;   // padded row (doubles): the chain lanes of one step fall into different banks pairwise
constexpr int BR_THREADS = 256;
constexpr int BR_GROUP = 8;         // steps per register group of the recurrence

// n frames of the `rows` (<= CH) chains of this workgroup, chain r by lane r of wave 0, all BR_THREADS threads moving the tiles.  The
// frames go through LDS time tiles of BR_TT frames, double buffered, filtered IN PLACE (a chain lane reads x[t] and writes y[t] to the
// same slot), ONE barrier per tile: while tile k is filtered the loads of tile k + 1 are in flight into registers and tile k - 1 is on
// its way out.  Tile k + 1 is stashed into the buffer tile k - 1 is stored from; every thread stores and stashes the SAME elements of a
// tile (e = tid + r * 256: row e / BR_TT, frame e % BR_TT -- consecutive threads, consecutive frames of one row), and reads its share of
// k - 1 before it overwrites it, so no second barrier is needed.  Steps come in groups of BR_GROUP (reads, steps in registers, writes:
// the reads of a group do not wait behind the writes of the one before), the ragged end of a tile frame by frame: a carried state never
// advances over padding, and padding stays zero.  What differs between the kernels is the caller's, as four functors:
//   init(chn, chain)         once, before the first load: the coefficients and the starting state of the lane's chain (chain: the lane
//                            has one), and whatever else the caller resolves once per thread
//   load(k, r, row, t)       the thread's r-th element of tile k -- frame k BR_TT + t of chain `row` -- or 0.0 where there is none
//   store(k, r, row, t, y)   the filtered element to its place, or nothing; y is a reference into LDS, read only by a store that happens
//   done(chn, chain)         once, after the last store: the chain's final state
// The chain is a local of this function and reaches the caller through init and done only: handed in by reference it costs every
// instantiation a register move per group of steps and two to four VGPRs.
template <int N, int CH, class Init, class Load, class Store, class Done>
__device__ __forceinline__ void bandpass_rows_tiles(int rows, int n, Init init, Load load, Store store, Done done)
{
    constexpr int SHARE = CH * BR_TT / BR_THREADS;  // elements of a tile per thread
    static_assert(SHARE >= 1 && CH <= 64 && BR_THREADS % 64 == 0, "a tile is shared by all threads and one wave carries the chains");
    __shared__ double tile[2][CH * BR_ROW];
    const int tid = threadIdx.x;
    const bool chain = tid < rows;
    const int ntiles = (n + BR_TT - 1) / BR_TT;
    Df2tChain<N> chn;
    init(chn, chain);

    double xr[SHARE];
    auto load_tile = [&](int k) {
#pragma unroll
        for (int r = 0; r < SHARE; ++r) {
            const int e = tid + r * BR_THREADS;
            const int row = e / BR_TT, t = e - row * BR_TT;
            xr[r] = load(k, r, row, t);
        }
    };
    auto stash_tile = [&](int k) {
        double *dst = tile[k & 1];
#pragma unroll
        for (int r = 0; r < SHARE; ++r) {
            const int e = tid + r * BR_THREADS;
            const int row = e / BR_TT, t = e - row * BR_TT;
            dst[row * BR_ROW + t] = xr[r];
        }
    };
    auto store_tile = [&](int k) {
        const double *src = tile[k & 1];
#pragma unroll
        for (int r = 0; r < SHARE; ++r) {
            const int e = tid + r * BR_THREADS;
            const int row = e / BR_TT, t = e - row * BR_TT;
            store(k, r, row, t, src[row * BR_ROW + t]);
        }
    };

    load_tile(0);
    stash_tile(0);
    __syncthreads();
    for (int k = 0; k < ntiles; ++k) {
        if (k + 1 < ntiles) load_tile(k + 1);  // in flight during the recurrence below
        if (k > 0) store_tile(k - 1);
        if (chain) {
            const int nt = n - k * BR_TT < BR_TT ? n - k * BR_TT : BR_TT;
            double *xi = tile[k & 1] + tid * BR_ROW;
            const int ngrp = nt - nt % BR_GROUP;
            for (int t0 = 0; t0 < ngrp; t0 += BR_GROUP) {
                double v[BR_GROUP];
#pragma unroll
                for (int u = 0; u < BR_GROUP; ++u) v[u] = xi[t0 + u];
#pragma unroll
                for (int u = 0; u < BR_GROUP; ++u) v[u] = chn.step(v[u]);
#pragma unroll
                for (int u = 0; u < BR_GROUP; ++u) xi[t0 + u] = v[u];
            }
            for (int t = ngrp; t < nt; ++t) xi[t] = chn.step(xi[t]);
        }
        if (k + 1 < ntiles) stash_tile(k + 1);
        __syncthreads();
    }
    store_tile(ntiles - 1);
    done(chn, chain);
}

constexpr int SC_N = 20;  // pending control word of a complex stream: the tile's length (stream_complex.hip "CONTROL WORDS")

// One tile of a complex stream: n frames of chains [blockIdx.x CH, +CH) of nl.  h: planar rows, chain g's tile at h + g * row_stride
// (the caller has added first_col); stg [nl][S]; carry [nl][chunk]; zst [N - 1][nl]: state word i of chain g at i * nl + g, so the chain
// lanes of a wave read and write consecutive doubles per word; chunk: frames per chunk of the contraction kernels (S is a multiple of
// it).  carry -> staging [0, fill); the DF2T steps of the tile -> staging [fill, fill + n); zeros up to the next chunk border; the
// pending control words {frames pushed after this tile, the tile's length} for the kernels behind -- no thread of this launch reads a word
// that one of its threads writes.  coef(chn, chain, g): Df2tChain::init with the coefficients of chain g (chain: the lane has one).  All
// indices into h, the staging array, the carry and the state are size_t.
template <int N, int CH, class Coef>
__device__ __forceinline__ void stream_bandpass_tile(Coef coef, const double *__restrict__ h, int nl, int n, size_t row_stride,
                                                     double *__restrict__ stg, int S, int chunk, const double *__restrict__ carry,
                                                     double *__restrict__ zst, int *__restrict__ ctl)
{
    const int tid = threadIdx.x;
    const int g0 = blockIdx.x * CH;
    const int rows = nl - g0 < CH ? nl - g0 : CH;  // chains of this workgroup
    const int fill = ctl[2];
    if (fill < 0 || fill >= chunk || (long long)fill + n > S) return;  // (never: the API sizes S for max_tile + chunk - 1 frames)

    // the frames behind the last whole chunk of the previous tiles, back in front of this tile's
    for (int r = tid >> 6; r < rows; r += BR_THREADS / 64) {
        const double *src = carry + (size_t)(g0 + r) * chunk;
        double *dst = stg + (size_t)(g0 + r) * S;
        for (int i = tid & 63; i < fill; i += 64) dst[i] = src[i];
    }

    bandpass_rows_tiles<N, CH>(
        rows, n,
        [&](Df2tChain<N> &chn, bool chain) {
            coef(chn, chain, g0 + tid);
            if (N > 1 && chain) {
#pragma unroll
                for (int i = 0; i < N - 1; ++i) chn.z[i] = zst[(size_t)i * nl + g0 + tid];
            }
        },
        [&](int k, int, int row, int t) {
            const int nt = n - k * BR_TT < BR_TT ? n - k * BR_TT : BR_TT;
            return (row < rows && t < nt) ? h[(size_t)(g0 + row) * row_stride + (size_t)k * BR_TT + t] : 0.0;
        },
        [&](int k, int, int row, int t, const double &y) {
            const int nt = n - k * BR_TT < BR_TT ? n - k * BR_TT : BR_TT;
            if (row < rows && t < nt) stg[(size_t)(g0 + row) * S + fill + (size_t)k * BR_TT + t] = y;
        },
        [&](const Df2tChain<N> &chn, bool chain) {
            if (N > 1 && chain) {
#pragma unroll
                for (int i = 0; i < N - 1; ++i) zst[(size_t)i * nl + g0 + tid] = chn.z[i];
            }
        });

    // zeros from the last frame to the next chunk border: a ragged last chunk of the recording is then contracted with exactly the
    // values the one-shot kernels give it (they put zeros behind frame T - 1); before the final tile nobody reads that chunk row
    const int end = fill + n;
    const int pad_end = (end + chunk - 1) / chunk * chunk;  // (<= S: S is a multiple of chunk and end <= S)
    for (int r = tid >> 6; r < rows; r += BR_THREADS / 64) {
        double *dst = stg + (size_t)(g0 + r) * S;
        for (int i = end + (tid & 63); i < pad_end; i += 64) dst[i] = 0.0;
    }
    if (blockIdx.x == 0 && tid == 0) {  // pending words: no thread of this launch reads them
        ctl[STREAM_CLK_TEND] = ctl[STREAM_CLK_T] + n;
        ctl[SC_N] = n;
    }
}

}  // namespace micloc
