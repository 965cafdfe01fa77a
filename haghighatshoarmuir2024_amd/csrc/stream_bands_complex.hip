// Wideband streaming form of the complex Beamformer's chain (micloc_stream_complex_bands_*): the band-pass tile of ALL bands' chains in
// ONE launch.  The rule is stated in include/micloc_hip.h ("wideband streaming, complex Beamformer"); DESIGN 4.18 has the footprint and
// the measurement.
//
// The complex chain has no encoder state and no horizon, so a stream of F bands x B recordings is one complex stream (stream_complex.hip)
// of F * B rows: its state layout, its staging array, its control words and every kernel behind the band-pass are that file's, unchanged.
// What differs is the band-pass tile:
//
// stream_bands_bandpass_tile_kernel<N, CH>: stream_bandpass_tile_kernel<N> (stream_complex.hip) with the two changes of
// bands_bandpass_kernel<N, CH> (bands_complex.hip) --
//   * chain g of the F * B * 2M chains belongs to band g / (B 2M) and filters with that row of the coefficient table, which travels by
//     value as FilterbankCoef does (the plans' own band-pass coefficients, already divided by a[0]);
//   * CH, the chains per workgroup -- the lanes of wave 0 that run a recurrence --, is a template parameter: the step is latency bound
//     whatever the number of live lanes, so at large F * B more SIMDs carry a recurrence and the movers' share of a tile shrinks.
// Everything else is stream_bandpass_tile_kernel's: one lane per chain; LDS time tiles of 32 frames (rows of 33 doubles), double
// buffered, filtered in place, ONE barrier per tile; steps in groups of 8, the ragged end frame by frame, so a carried state never
// advances over padding; state word i of chain g at i * nl + g; [carry | tile] into the chunk-aligned staging rows, zeros up to the next
// chunk border; the pending control words {frames pushed after this tile, the tile's length} left for the kernels behind it -- no thread
// of this launch reads a word that one of its threads writes.  All indices into h, the staging array, the carry and the state are size_t.
// The arithmetic is rzcc.hip's Iir<N>::step restated as the sibling kernels restate it (rzcc.hip is pinned by the profile manifest): the
// same fmas in the same order, every term computed.
#include "micloc_internal.h"

namespace micloc {

namespace {

constexpr int SBC_N = 20;            // pending control word: the tile's length (stream_complex.hip's SC_N, which its accumulate kernel reads)
constexpr int SBC_TT = 32;           // frames per LDS time tile
constexpr int SBC_ROW = SBC_TT + 1;  // padded row (doubles): the chain lanes of one step fall into different banks pairwise
constexpr int SBC_THREADS = 256;
constexpr int SBC_GROUP = 8;         // steps per register group of the recurrence

template <int N>
struct SbcChain {
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

// h: planar rows, chain g's tile at h + g * row_stride (the caller has added first_col); nl = F * band_chains chains, band_chains = B * 2M;
// stg [nl][S]; carry [nl][chunk]; zst [N - 1][nl]; chunk: frames per chunk of the contraction kernels (S is a multiple of it).
template <int N, int CH>
__global__ __launch_bounds__(SBC_THREADS) void stream_bands_bandpass_tile_kernel(const FilterbankCoef co, const double *__restrict__ h, int nl,
                                                                                  int band_chains, int n, size_t row_stride,
                                                                                  double *__restrict__ stg, int S, int chunk,
                                                                                  const double *__restrict__ carry, double *__restrict__ zst,
                                                                                  int *__restrict__ ctl)
{
    constexpr int SHARE = CH * SBC_TT / SBC_THREADS;  // elements of a tile per thread
    static_assert(SHARE >= 1 && CH <= 64 && SBC_THREADS % 64 == 0, "a tile is shared by all threads and one wave carries the chains");
    __shared__ double tile[2][CH * SBC_ROW];
    const int tid = threadIdx.x;
    const int g0 = blockIdx.x * CH;
    const int rows = nl - g0 < CH ? nl - g0 : CH;  // chains of this workgroup
    const int fill = ctl[2];
    if (fill < 0 || fill >= chunk || (long long)fill + n > S) return;  // (never: the API sizes S for max_tile + chunk - 1 frames)
    const int ntiles = (n + SBC_TT - 1) / SBC_TT;

    // the frames behind the last whole chunk of the previous tiles, back in front of this tile's
    for (int r = tid >> 6; r < rows; r += SBC_THREADS / 64) {
        const double *src = carry + (size_t)(g0 + r) * chunk;
        double *dst = stg + (size_t)(g0 + r) * S;
        for (int i = tid & 63; i < fill; i += 64) dst[i] = src[i];
    }

    const bool chain = tid < rows;
    SbcChain<N> chn;
    chn.init(co, chain ? (g0 + tid) / band_chains : 0);
    if (N > 1 && chain) {
#pragma unroll
        for (int i = 0; i < N - 1; ++i) chn.z[i] = zst[(size_t)i * nl + g0 + tid];
    }

    // element e of a tile: row e / SBC_TT, frame e % SBC_TT (consecutive threads: consecutive frames of one row)
    double xr[SHARE];
    auto load_tile = [&](int k) {
        const int nt = n - k * SBC_TT < SBC_TT ? n - k * SBC_TT : SBC_TT;
#pragma unroll
        for (int r = 0; r < SHARE; ++r) {
            const int e = tid + r * SBC_THREADS;
            const int row = e / SBC_TT, t = e - row * SBC_TT;
            xr[r] = (row < rows && t < nt) ? h[(size_t)(g0 + row) * row_stride + (size_t)k * SBC_TT + t] : 0.0;
        }
    };
    auto stash_tile = [&](int k) {
        double *dst = tile[k & 1];
#pragma unroll
        for (int r = 0; r < SHARE; ++r) {
            const int e = tid + r * SBC_THREADS;
            const int row = e / SBC_TT, t = e - row * SBC_TT;
            dst[row * SBC_ROW + t] = xr[r];
        }
    };
    auto store_tile = [&](int k) {
        const int nt = n - k * SBC_TT < SBC_TT ? n - k * SBC_TT : SBC_TT;
        const double *src = tile[k & 1];
#pragma unroll
        for (int r = 0; r < SHARE; ++r) {
            const int e = tid + r * SBC_THREADS;
            const int row = e / SBC_TT, t = e - row * SBC_TT;
            if (row < rows && t < nt) stg[(size_t)(g0 + row) * S + fill + (size_t)k * SBC_TT + t] = src[row * SBC_ROW + t];
        }
    };

    load_tile(0);
    stash_tile(0);
    __syncthreads();
    for (int k = 0; k < ntiles; ++k) {
        if (k + 1 < ntiles) load_tile(k + 1);  // in flight during the recurrence below
        if (k > 0) store_tile(k - 1);
        if (chain) {
            const int nt = n - k * SBC_TT < SBC_TT ? n - k * SBC_TT : SBC_TT;
            double *xi = tile[k & 1] + tid * SBC_ROW;
            const int ngrp = nt - nt % SBC_GROUP;
            for (int t0 = 0; t0 < ngrp; t0 += SBC_GROUP) {
                double v[SBC_GROUP];
#pragma unroll
                for (int u = 0; u < SBC_GROUP; ++u) v[u] = xi[t0 + u];
#pragma unroll
                for (int u = 0; u < SBC_GROUP; ++u) v[u] = chn.step(v[u]);
#pragma unroll
                for (int u = 0; u < SBC_GROUP; ++u) xi[t0 + u] = v[u];
            }
            for (int t = ngrp; t < nt; ++t) xi[t] = chn.step(xi[t]);  // the ragged end frame by frame: a carried state never advances over padding
        }
        if (k + 1 < ntiles) stash_tile(k + 1);
        __syncthreads();
    }
    store_tile(ntiles - 1);
    if (N > 1 && chain) {
#pragma unroll
        for (int i = 0; i < N - 1; ++i) zst[(size_t)i * nl + g0 + tid] = chn.z[i];
    }

    // zeros from the last frame to the next chunk border: a ragged last chunk of the recording is then contracted with exactly the
    // values the one-shot kernels give it; before the final tile nobody reads that chunk row
    const int end = fill + n;
    const int pad_end = (end + chunk - 1) / chunk * chunk;  // (<= S: S is a multiple of chunk and end <= S)
    for (int r = tid >> 6; r < rows; r += SBC_THREADS / 64) {
        double *dst = stg + (size_t)(g0 + r) * S;
        for (int i = end + (tid & 63); i < pad_end; i += 64) dst[i] = 0.0;
    }
    if (blockIdx.x == 0 && tid == 0) {  // pending words: no thread of this launch reads them
        ctl[STREAM_CLK_TEND] = ctl[STREAM_CLK_T] + n;
        ctl[SBC_N] = n;
    }
}

template <int N, int CH>
hipError_t sbc_launch_ch(const FilterbankCoef &co, const double *h, int nl, int band_chains, int n, size_t row_stride, double *stg, int S,
                         int chunk, const double *carry, double *zst, int *ctl, hipStream_t stream)
{
    hipLaunchKernelGGL((stream_bands_bandpass_tile_kernel<N, CH>), dim3((nl + CH - 1) / CH), dim3(SBC_THREADS), 0, stream, co, h, nl,
                       band_chains, n, row_stride, stg, S, chunk, carry, zst, ctl);
    return hipGetLastError();
}

template <int N>
hipError_t sbc_launch(int chains, const FilterbankCoef &co, const double *h, int nl, int band_chains, int n, size_t row_stride, double *stg,
                      int S, int chunk, const double *carry, double *zst, int *ctl, hipStream_t stream)
{
    switch (chains) {
        case 16: return sbc_launch_ch<N, 16>(co, h, nl, band_chains, n, row_stride, stg, S, chunk, carry, zst, ctl, stream);
        case 32: return sbc_launch_ch<N, 32>(co, h, nl, band_chains, n, row_stride, stg, S, chunk, carry, zst, ctl, stream);
        case 64: return sbc_launch_ch<N, 64>(co, h, nl, band_chains, n, row_stride, stg, S, chunk, carry, zst, ctl, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

// Chains per workgroup the launcher takes for nl chains: bands_bandpass_chains' rule (bands_complex.hip) -- the LDS of a workgroup (8.4,
// 16.9, 33.8 KB) and the registers are those of the batch kernel, so up to 1024 workgroups of the 16- and 32-chain forms
// run as one resident round on the 256 CUs; past that the 64-chain form keeps the number of rounds down.
int stream_bands_bandpass_chains(int nl)
{
    constexpr int ROUND = 1024;
    if (nl <= 16 * ROUND) return 16;
    if (nl <= 32 * ROUND) return 32;
    return 64;
}

// Ring depth of the bands' windows: how many windows ONE tile can complete, plus the one cut at the end of the recording.  A tile
// contracts at most Ks chunk rows (stream_complex_chunks: its own max_tile frames and a carry of fewer than `chunk`).  With `done` chunks
// contracted before the tile and `ready` = done + r after it, stream_window_kernel has emitted e(c) = c < w ? 0 : (c - w) / h + 1 windows
// (w, h: window and hop in chunks) at c = done and at c = ready: e(ready) - e(done) <= ceil(r / h) <= ceil(Ks / h).  On the final tile the
// windows of micloc_window_count(T) are emitted, of which at most ONE is not complete by chunks: a window that starts at n h frames is cut
// only if T - window < n hop < T - window + hop, an open interval of one hop.  All bands emit the same windows in the same tile, so the
// band sum finds count - emitted <= this depth and never gives a window up.
int stream_bands_ring_depth(int Ks, int hop_chunks) { return (Ks + hop_chunks - 1) / hop_chunks + 1; }

hipError_t launch_stream_bands_bandpass(const FilterbankCoef &co, const double *h, int F, int band_chains, int n, size_t row_stride,
                                        double *staging, int S, int chunk, void *state, const StreamComplexLayout &L, int chains,
                                        hipStream_t stream)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || band_chains < 1 || n < 1 || chunk < 1 || S < chunk || S % chunk != 0 || n > S - (chunk - 1))
        return hipErrorInvalidValue;
    const long long nll = (long long)F * band_chains;
    if (nll > 0x7fffffffll) return hipErrorInvalidValue;
    const int nl = (int)nll;
    if (chains == 0) chains = stream_bands_bandpass_chains(nl);
    unsigned char *base = reinterpret_cast<unsigned char *>(state);
    int *ctl = reinterpret_cast<int *>(base);
    double *zst = reinterpret_cast<double *>(base + L.z);
    const double *carry = reinterpret_cast<const double *>(base + L.carry);
#define SBC_CASE(NN) \
    case NN: return sbc_launch<NN>(chains, co, h, nl, band_chains, n, row_stride, staging, S, chunk, carry, zst, ctl, stream);
    switch (co.n) {
        SBC_CASE(1)
        SBC_CASE(2)
        SBC_CASE(3)
        SBC_CASE(4)
        SBC_CASE(5)
        SBC_CASE(6)
        SBC_CASE(7)
        SBC_CASE(8)
        SBC_CASE(9)
        default: return hipErrorInvalidValue;
    }
#undef SBC_CASE
}

}  // namespace micloc
