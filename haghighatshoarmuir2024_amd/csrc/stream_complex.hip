// Streaming form of the complex Beamformer's chain (micloc_stream_complex_*): band-pass with state carry, the one-shot time reduction
// cut at the stream's chunk borders, the running and the windowed read-out.  The rule is stated in full in include/micloc_hip.h
// ("streaming, complex Beamformer"); DESIGN 4.16 has the state layout and the footprint.
//
// No spikes, no open clusters, no horizon: a frame is final once its tile has been band-passed.  A tile of n frames is
//   stream_bandpass_tile_kernel<N>      carry -> staging [0, fill); DF2T steps of the tile -> staging [fill, fill + n); zeros up to the
//                                       next chunk border (what the one-shot kernels put behind a ragged last chunk)
//   launch_planar_beamform              (beamform.hip, unchanged) on staging [B][2M][Ks CH] as a recording of Ks whole chunks: the launch
//                                       shape depends on max_tile only; rows past the valid ones are computed and never read
//   stream_complex_accumulate_kernel    the new chunk rows onto {total, open-block sum} in the one-shot order, Re | Im folded
//   stream_window_kernel<1>             (windowed; stream_windows.hip) the streaming read-out's one kernel, instantiated for folded rows
//   stream_complex_slide_kernel         frames behind the last whole chunk -> carry; the one-thread clock commit
// all on one stream, one after the other.
//
// CONTROL WORDS (the first 64 ints of the state).  A launch with more than one workgroup must never read a word that one of its own
// threads writes, so the words come in two sets: the COMMITTED ones {[0] chunks contracted, [2] carry fill, [8] frames contracted,
// [STREAM_CLK_T] frames pushed} are written by the slide kernel's commit only, and the PENDING ones are written by one thread of the
// kernel in front of their readers: the band-pass kernel leaves {[STREAM_CLK_TEND] frames pushed after this tile, [SC_N] the tile's
// length}, the accumulate kernel {[4] = 0, [5] new chunk rows, [6] chunks contracted after this tile -- the words stream_window_kernel
// reads --, [SC_SRC] first staging column behind the rows, [SC_REM] frames that stay, [SC_FRAMES] frames contracted after this tile}.
#include "micloc_internal.h"

namespace micloc {

namespace {

constexpr int SC_N = 20, SC_SRC = 21, SC_REM = 22, SC_FRAMES = 23;

constexpr int SB_CHAINS = 64;   // chains per workgroup: wave 0 runs the recurrences, all four waves move the tiles
constexpr int SB_TT = 32;       // frames per LDS time tile
constexpr int SB_ROW = SB_TT + 1;  // padded row (doubles): the 64 chain lanes of one step fall into different banks pairwise
constexpr int SB_THREADS = 256;
constexpr int SB_SHARE = SB_CHAINS * SB_TT / SB_THREADS;  // elements of a tile per thread
constexpr int SB_GROUP = 8;     // steps per register group of the recurrence

// the DF2T step of the contract, operation for operation rzcc.hip's Iir<N>::step (that file is pinned by the profile
// manifest, so the step is restated here as filterbank.hip restates it)
template <int N>
struct ScChain {
    double z[N > 1 ? N - 1 : 1];

    __device__ __forceinline__ double step(const IirCoef &co, double xin)
    {
        double y;
        if (N == 1) {
            y = __builtin_fma(co.b[0], xin, 0.0);
        } else {
            y = __builtin_fma(co.b[0], xin, z[0]);
#pragma unroll
            for (int i = 0; i < N - 2; ++i) z[i] = __builtin_fma(-co.a[i + 1], y, __builtin_fma(co.b[i + 1], xin, z[i + 1]));
            z[N - 2] = __builtin_fma(-co.a[N - 1], y, co.b[N - 1] * xin);
        }
        return y;
    }
};

// h: planar rows, chain g's tile at h + g * row_stride (the caller has added first_col); stg [nl][S]; carry [nl][CH]; zst [N - 1][nl]: state
// word i of chain g at i * nl + g, so the chain lanes of a wave read and write consecutive doubles per word.
//
// The tile goes through LDS time tiles of SB_TT frames, double buffered, filtered IN PLACE (a chain lane reads x[t] and writes y[t] to the
// same slot), ONE barrier per tile: while tile k is filtered the loads of tile k + 1 are in flight into registers and tile k - 1 is on its
// way out.  Tile k + 1 is stashed into the buffer tile k - 1 is stored from; every thread stores and stashes the SAME elements of a tile
// (e = tid + r * 256), and reads its share of k - 1 before it overwrites it, so no second barrier is needed.
template <int N>
__global__ __launch_bounds__(SB_THREADS) void stream_bandpass_tile_kernel(const IirCoef co, const double *__restrict__ h, int nl, int n,
                                                                          size_t row_stride, double *__restrict__ stg, int S, int CH,
                                                                          const double *__restrict__ carry, double *__restrict__ zst,
                                                                          int *__restrict__ ctl)
{
    __shared__ double tile[2][SB_CHAINS * SB_ROW];
    const int tid = threadIdx.x;
    const int g0 = blockIdx.x * SB_CHAINS;
    const int rows = nl - g0 < SB_CHAINS ? nl - g0 : SB_CHAINS;  // chains of this workgroup
    const int fill = ctl[2];
    if (fill < 0 || fill >= CH || (long long)fill + n > S) return;  // (never: the API sizes S for max_tile + CH - 1 frames)
    const int ntiles = (n + SB_TT - 1) / SB_TT;

    // the frames behind the last whole chunk of the previous tiles, back in front of this tile's
    for (int r = tid >> 6; r < rows; r += SB_THREADS / 64) {
        const double *src = carry + (size_t)(g0 + r) * CH;
        double *dst = stg + (size_t)(g0 + r) * S;
        for (int i = tid & 63; i < fill; i += 64) dst[i] = src[i];
    }

    const bool chain = tid < rows;
    ScChain<N> chn;
#pragma unroll
    for (int i = 0; i < (N > 1 ? N - 1 : 1); ++i) chn.z[i] = 0.0;
    if (N > 1 && chain) {
#pragma unroll
        for (int i = 0; i < N - 1; ++i) chn.z[i] = zst[(size_t)i * nl + g0 + tid];
    }

    // element e of a tile: row e / SB_TT, frame e % SB_TT (consecutive threads: consecutive frames of one row)
    double xr[SB_SHARE];
    auto load_tile = [&](int k) {
        const int nt = n - k * SB_TT < SB_TT ? n - k * SB_TT : SB_TT;
#pragma unroll
        for (int r = 0; r < SB_SHARE; ++r) {
            const int e = tid + r * SB_THREADS;
            const int row = e / SB_TT, t = e - row * SB_TT;
            xr[r] = (row < rows && t < nt) ? h[(size_t)(g0 + row) * row_stride + (size_t)k * SB_TT + t] : 0.0;
        }
    };
    auto stash_tile = [&](int k) {
        double *dst = tile[k & 1];
#pragma unroll
        for (int r = 0; r < SB_SHARE; ++r) {
            const int e = tid + r * SB_THREADS;
            const int row = e / SB_TT, t = e - row * SB_TT;
            dst[row * SB_ROW + t] = xr[r];
        }
    };
    auto store_tile = [&](int k) {
        const int nt = n - k * SB_TT < SB_TT ? n - k * SB_TT : SB_TT;
        const double *src = tile[k & 1];
#pragma unroll
        for (int r = 0; r < SB_SHARE; ++r) {
            const int e = tid + r * SB_THREADS;
            const int row = e / SB_TT, t = e - row * SB_TT;
            if (row < rows && t < nt) stg[(size_t)(g0 + row) * S + fill + (size_t)k * SB_TT + t] = src[row * SB_ROW + t];
        }
    };

    load_tile(0);
    stash_tile(0);
    __syncthreads();
    for (int k = 0; k < ntiles; ++k) {
        if (k + 1 < ntiles) load_tile(k + 1);  // in flight during the recurrence below
        if (k > 0) store_tile(k - 1);
        if (chain) {
            const int nt = n - k * SB_TT < SB_TT ? n - k * SB_TT : SB_TT;
            double *xi = tile[k & 1] + tid * SB_ROW;
            const int ngrp = nt - nt % SB_GROUP;
            for (int t0 = 0; t0 < ngrp; t0 += SB_GROUP) {
                double v[SB_GROUP];
#pragma unroll
                for (int u = 0; u < SB_GROUP; ++u) v[u] = xi[t0 + u];
#pragma unroll
                for (int u = 0; u < SB_GROUP; ++u) v[u] = chn.step(co, v[u]);
#pragma unroll
                for (int u = 0; u < SB_GROUP; ++u) xi[t0 + u] = v[u];
            }
            for (int t = ngrp; t < nt; ++t) xi[t] = chn.step(co, xi[t]);  // the ragged end frame by frame: a carried state never advances over padding
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
    // values the one-shot kernels give it (they put zeros behind frame T - 1); before the final tile nobody reads that chunk row
    const int end = fill + n;
    const int pad_end = (end + CH - 1) / CH * CH;  // (<= S: S is a multiple of CH and end <= S)
    for (int r = tid >> 6; r < rows; r += SB_THREADS / 64) {
        double *dst = stg + (size_t)(g0 + r) * S;
        for (int i = end + (tid & 63); i < pad_end; i += 64) dst[i] = 0.0;
    }
    if (blockIdx.x == 0 && tid == 0) {  // pending words: no thread of this launch reads them
        ctl[STREAM_CLK_TEND] = ctl[STREAM_CLK_T] + n;
        ctl[SC_N] = n;
    }
}

constexpr int SA_COLS = 256;

// first maximum of (best, bi) over the workgroup -> thread 0's return value (0 for a row without a winner)
__device__ __forceinline__ int sc_argmax(double best, int bi, double *sv, int *si)
{
    const int col = threadIdx.x;
    sv[col] = best;
    si[col] = bi;
    __syncthreads();
    for (int s = SA_COLS / 2; s > 0; s >>= 1) {
        if (col < s) {
            const double ov = sv[col + s];
            const int oi = si[col + s];
            if (ov > sv[col] || (ov == sv[col] && oi < si[col])) {
                sv[col] = ov;
                si[col] = oi;
            }
        }
        __syncthreads();
    }
    return si[0] == 0x7fffffff ? 0 : si[0];
}

// partial [B][Ks][Gp]: rows 0 .. nrows - 1 are the chunks [done, done + nrows) of the stream, columns [0, Ghp) Re and [Ghp, Gp) Im.  The
// additions are power_argmax_kernel's with complex_pairs = 1 (beamform.hip): s += Re; s += Im per chunk in ascending order inside blocks of
// STREAM_BLOCK_CHUNKS chunks counted from chunk 0, block sums in ascending order onto the total; the open block is added last.
__global__ __launch_bounds__(SA_COLS) void stream_complex_accumulate_kernel(const double *__restrict__ partial, int Ks, int Gp, int G, int Ghp,
                                                                             int CH, int final_tile, int *__restrict__ ctl,
                                                                             double *__restrict__ acc, double *__restrict__ power,
                                                                             int32_t *__restrict__ argmax)
{
    __shared__ double sv[SA_COLS];
    __shared__ int si[SA_COLS];
    const int b = blockIdx.x, col = threadIdx.x;
    const int done = ctl[0], fill = ctl[2], frames0 = ctl[8], n = ctl[SC_N];
    const int avail = fill + n;
    const int whole = avail / CH;
    int nrows = final_tile ? (avail + CH - 1) / CH : whole;
    if (nrows > Ks) nrows = Ks;  // (never: Ks covers max_tile + CH - 1 frames)
    const int taken = final_tile ? avail : whole * CH;
    const double frames = (double)(frames0 + taken);
    const double *pb = partial + (size_t)b * Ks * Gp;
    double *tot = acc + (size_t)b * 2 * G, *blk = tot + G;
    double best = -1.0;
    int bi = 0x7fffffff;
    for (int g = col; g < G; g += SA_COLS) {
        double total = tot[g], s = blk[g];
        int open = done % STREAM_BLOCK_CHUNKS;
        for (int ch = 0; ch < nrows; ++ch) {
            s += pb[(size_t)ch * Gp + g];
            s += pb[(size_t)ch * Gp + Ghp + g];
            if (++open == STREAM_BLOCK_CHUNKS) {
                total += s;
                s = 0.0;
                open = 0;
            }
        }
        tot[g] = total;
        blk[g] = s;
        const double now = open > 0 ? total + s : total;
        const double p = frames > 0.0 ? now / frames : 0.0;
        if (power) power[(size_t)b * G + g] = p;
        if (p > best) {  // ascending g per thread: its first maximum; a NaN never wins
            best = p;
            bi = g;
        }
    }
    const int a = sc_argmax(best, bi, sv, si);
    if (col == 0 && argmax) argmax[b] = a;
    if (b == 0 && col == 0) {  // pending words: no thread of this launch reads them
        ctl[4] = 0;
        ctl[5] = nrows;
        ctl[6] = done + nrows;
        ctl[SC_SRC] = whole * CH;
        ctl[SC_REM] = final_tile ? 0 : avail - whole * CH;
        ctl[SC_FRAMES] = frames0 + taken;
    }
}

// One workgroup per (trial, channel) row: the frames behind the last contracted chunk go to the row's carry.  Source (staging, the
// workspace) and destination (carry, the state) are different arrays: they never overlap, so there is no scratch pass.  Thread 0 of
// workgroup 0 commits the clock; the words it writes are read by no thread of this launch.
__global__ __launch_bounds__(256) void stream_complex_slide_kernel(const double *__restrict__ stg, int S, int CH, double *__restrict__ carry,
                                                                    int *__restrict__ ctl)
{
    const int row = blockIdx.x;
    const int src0 = ctl[SC_SRC], rem = ctl[SC_REM];
    if (rem > 0 && rem < CH && src0 >= 0 && (long long)src0 + rem <= S) {
        const double *src = stg + (size_t)row * S + src0;
        double *dst = carry + (size_t)row * CH;
        for (int i = threadIdx.x; i < rem; i += 256) dst[i] = src[i];
    }
    if (row == 0 && threadIdx.x == 0) {
        ctl[0] = ctl[6];
        ctl[2] = rem;
        ctl[8] = ctl[SC_FRAMES];
        ctl[STREAM_CLK_T] = ctl[STREAM_CLK_TEND];
    }
}

template <int N>
hipError_t sc_bandpass_launch(const IirCoef &co, const double *h, int nl, int n, size_t row_stride, double *stg, int S, int CH,
                              const double *carry, double *zst, int *ctl, hipStream_t stream)
{
    hipLaunchKernelGGL(stream_bandpass_tile_kernel<N>, dim3((nl + SB_CHAINS - 1) / SB_CHAINS), dim3(SB_THREADS), 0, stream, co, h, nl, n,
                       row_stride, stg, S, CH, carry, zst, ctl);
    return hipGetLastError();
}

}  // namespace

int stream_complex_chunks(int max_tile, int CH) { return (int)(((long long)max_tile + 2 * (long long)CH - 2) / CH); }

StreamComplexLayout stream_complex_layout(int B, int C, int G, int iir_n, int CH)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    StreamComplexLayout L{};
    size_t off = 256;  // control words
    L.z = off;
    off += al((size_t)(iir_n > 1 ? iir_n - 1 : 1) * B * C * sizeof(double));
    L.carry = off;
    off += al((size_t)B * C * CH * sizeof(double));
    L.acc = off;
    off += al((size_t)B * 2 * G * sizeof(double));
    L.total = off;
    return L;
}

hipError_t launch_stream_complex_bandpass(const IirCoef &co, const double *h, int nl, int n, size_t row_stride, double *staging, int S,
                                          int CH, void *state, const StreamComplexLayout &L, hipStream_t stream)
{
    if (nl < 1 || n < 1 || CH < 1 || S < CH || S % CH != 0 || n > S - (CH - 1)) return hipErrorInvalidValue;
    unsigned char *base = reinterpret_cast<unsigned char *>(state);
    int *ctl = reinterpret_cast<int *>(base);
    double *zst = reinterpret_cast<double *>(base + L.z);
    const double *carry = reinterpret_cast<const double *>(base + L.carry);
    switch (co.n) {
        case 1: return sc_bandpass_launch<1>(co, h, nl, n, row_stride, staging, S, CH, carry, zst, ctl, stream);
        case 2: return sc_bandpass_launch<2>(co, h, nl, n, row_stride, staging, S, CH, carry, zst, ctl, stream);
        case 3: return sc_bandpass_launch<3>(co, h, nl, n, row_stride, staging, S, CH, carry, zst, ctl, stream);
        case 4: return sc_bandpass_launch<4>(co, h, nl, n, row_stride, staging, S, CH, carry, zst, ctl, stream);
        case 5: return sc_bandpass_launch<5>(co, h, nl, n, row_stride, staging, S, CH, carry, zst, ctl, stream);
        case 6: return sc_bandpass_launch<6>(co, h, nl, n, row_stride, staging, S, CH, carry, zst, ctl, stream);
        case 7: return sc_bandpass_launch<7>(co, h, nl, n, row_stride, staging, S, CH, carry, zst, ctl, stream);
        case 8: return sc_bandpass_launch<8>(co, h, nl, n, row_stride, staging, S, CH, carry, zst, ctl, stream);
        case 9: return sc_bandpass_launch<9>(co, h, nl, n, row_stride, staging, S, CH, carry, zst, ctl, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_stream_complex_accumulate(const double *partial, int B, int Ks, int Gp, int G, int CH, int final_tile, void *state,
                                            const StreamComplexLayout &L, double *power, int32_t *argmax, hipStream_t stream)
{
    unsigned char *base = reinterpret_cast<unsigned char *>(state);
    hipLaunchKernelGGL(stream_complex_accumulate_kernel, dim3(B), dim3(SA_COLS), 0, stream, partial, Ks, Gp, G, Gp / 2, CH, final_tile ? 1 : 0,
                       reinterpret_cast<int *>(base), reinterpret_cast<double *>(base + L.acc), power, argmax);
    return hipGetLastError();
}

hipError_t launch_stream_complex_slide(const double *staging, int nl, int S, int CH, void *state, const StreamComplexLayout &L,
                                       hipStream_t stream)
{
    unsigned char *base = reinterpret_cast<unsigned char *>(state);
    hipLaunchKernelGGL(stream_complex_slide_kernel, dim3(nl), dim3(256), 0, stream, staging, S, CH, reinterpret_cast<double *>(base + L.carry),
                       reinterpret_cast<int *>(base));
    return hipGetLastError();
}

}  // namespace micloc
