// What the tracking kernels share -- the one-shot ones of track.hip and the streaming ones of stream_track.hip: the shape of a
// workgroup (four waves, 64 frames x 64 DoA columns per chunk), stages 1 and 2 of track.hip's header, which decide the bits of every y[t][g], as pieces, the
// walk of one plan's frames chunk by chunk built from them (track_ws_walk, track_wsc_walk), the envelope recurrence over a chunk, the
// reduction of every frame to (max envelope, first index) over the workgroup's columns (track_chain_reduce: stages 3 and 4), and the rule
// of a row without a winner; on the host the complex channel-count table and the layout of the pairs workspace.  Stated once, so that a
// frame has the same bits whether its recording was walked in one launch or cut at launch borders.  The kernels keep what differs: where
// the walk starts, which position is frame 0, where a finished pair goes, and where the chain state comes from and goes to.
#pragma once
#include <math.h>

#include "readout_rows.h"

namespace micloc {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int TRK_WAVES = 4;
constexpr int TRK_THREADS = TRK_WAVES * 64;
constexpr int TRK_CH = TRK_WAVES * 16;  // frames per chunk: one 16-frame tile per wave
constexpr int TRK_COLS = 64;            // DoA columns per workgroup = lanes of the chain wave
constexpr int TRK_LD = TRK_COLS + 1;    // row stride of the magnitude tile (odd: the row reduction reads down columns)
constexpr int TRK_NONE = RO_NONE;

// LDS of a tracking workgroup: the magnitude tile, then the tail fragments (complex) or the Toeplitz table and the spike tile (SNN)
inline size_t track_lds_bytes(bool complex_src, int NK)
{
    size_t d = (size_t)TRK_CH * TRK_LD;
    if (complex_src)
        d += (size_t)TRK_WAVES * 64;
    else
        d += (size_t)(4 * NK + 16) + (size_t)(TRK_CH + 4 * NK - 16) * 16;
    return d * sizeof(double);
}

// the (value, index) pairs of n rows x column groups in one workspace: pval [n] doubles, then pidx [n] int32, each rounded to 256 bytes
inline size_t track_al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t track_pairs_size(size_t n) { return track_al256(n * sizeof(double)) + track_al256(n * sizeof(int32_t)); }
inline void track_pairs_split(void *pairs, size_t n, double *&pval, int32_t *&pidx)
{
    pval = reinterpret_cast<double *>(pairs);
    pidx = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(pairs) + track_al256(n * sizeof(double)));
}

// the complex kernels' <KM, KV> of a channel count C (2 x microphones: even; beamform_wsc_kernel's table): KM k-steps of four channels
// on the matrix cores, then KV tail channels as plain FMAs.  f gets a TrackK<KM, KV>; false: a C nobody serves, f was not called.
template <int KM, int KV>
struct TrackK {
    static constexpr int km = KM, kv = KV;
};

template <class F>
inline bool track_wsc_dispatch(int C, F f)
{
    switch (C) {
        case 2: case 4: f(TrackK<1, 0>{}); return true;
        case 6: f(TrackK<1, 2>{}); return true;
        case 8: f(TrackK<2, 0>{}); return true;
        case 10: f(TrackK<2, 2>{}); return true;
        case 12: f(TrackK<3, 0>{}); return true;
        case 14: f(TrackK<3, 2>{}); return true;
        case 16: f(TrackK<4, 0>{}); return true;
        default: return false;
    }
}

// a finished row: an all-NaN row (no column ever won) gives index 0 and peak NaN
__device__ __forceinline__ int track_row_index(int bi) { return bi == TRK_NONE ? 0 : bi; }
__device__ __forceinline__ double track_row_peak(double best, int bi) { return bi == TRK_NONE ? (double)NAN : best; }

// steps 3 and 4 of track.hip's header for the chunk at position cs, nrow frames whose magnitudes lie in Y.  first: the chunk begins at
// frame 0 of the recording (state_0 = |y_0|).  emit(cs, row, best, bi): the pair of frame `row` of the chunk over this workgroup's
// columns, bi == TRK_NONE when no column won; called by one thread per frame.
template <class Emit>
__device__ __forceinline__ void track_chain_reduce(double *Y, int wv, int l, int tid, int cs, bool first, int nrow, int G, int cg,
                                                   double a_rise, double i_rise, double a_fall, double &state, const Emit &emit)
{
    if (wv == 0) {
        double *y = Y + l;
        auto step = [&](int j) {
            const double m = y[j * TRK_LD];
            const double up = __dadd_rn(__dmul_rn(a_rise, state), __dmul_rn(i_rise, m));
            const double down = __dmul_rn(a_fall, state);
            state = (m >= state) ? up : down;
            y[j * TRK_LD] = state;
        };
        int j0 = 0;
        if (first) {  // state_0 = |y_0|: the tile already holds it
            state = y[0];
            j0 = 1;
        }
        if (nrow == TRK_CH && j0 == 0) {
#pragma unroll 16
            for (int j = 0; j < TRK_CH; ++j) step(j);
        } else {
            for (int j = j0; j < nrow; ++j) step(j);
        }
    }
    __syncthreads();
    {
        const int row = tid >> 2, part = tid & 3;
        double best = -1.0;
        int bi = TRK_NONE;
        if (row < nrow) {
            const double *r = Y + row * TRK_LD + part * 16;
            const int g0 = cg * TRK_COLS + part * 16;
#pragma unroll
            for (int i = 0; i < 16; ++i) {  // ascending: this thread's first maximum
                const double v = r[i];
                if (g0 + i < G && v > best) {
                    best = v;
                    bi = g0 + i;
                }
            }
        }
        wave_first_max<4>(best, bi);  // the four parts of a row are adjacent lanes
        if (part == 0 && row < nrow) emit(cs, row, best, bi);
    }
}

// ---- the per-chunk step "stage -> membrane -> |y| fragments", in the pieces the walks are made of: cut where a band walk of track.hip
// gets in -- between the bands' staging, and where the magnitude is put -- with the magnitude handed to `put` ----
// |y| of a complex value: the expression of the tiles, for the band sum of the two-step route as well
__device__ __forceinline__ double track_magnitude(double re, double im) { return hypot(re, im); }

// the neuron table of a plan into LDS
__device__ __forceinline__ void track_ws_table(double *ntab, const double *__restrict__ ntab_g, int NK, int tid)
{
    const int ntab_len = 4 * NK + 16;
    for (int e = tid; e < ntab_len; e += TRK_THREADS) ntab[e] = ntab_g[e];
}

// bf_mat fragments of the workgroup's four DoA tiles (a tile beyond the grid multiplies a clamped one; its columns are never read)
__device__ __forceinline__ void track_ws_weights(double (&Wf)[4][4], const double *__restrict__ Wp, int GT, int cg, int lc, int q)
{
    const int Gp = 16 * GT;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gt = 4 * cg + j;
        const double *wp = Wp + 16 * (gt < GT ? gt : GT - 1) + lc;
#pragma unroll
        for (int k = 0; k < 4; ++k) Wf[j][k] = wp[(size_t)(4 * k + q) * Gp];
    }
}

// rows tau0 .. tau0 + R - 1 of the raster, tau0 = cs + 16 - 4 NK, as fp64 [R][16]; rows outside [0, T) and the channel padding are zero
__device__ __forceinline__ void track_ws_stage(double *S, const int8_t *__restrict__ sb, int C, int cs, int T, int NK, int tid)
{
    const int R = TRK_CH + 4 * NK - 16;
    const int tau0 = cs + 16 - 4 * NK;
    const int c = tid & 15;
    for (int rho = tid >> 4; rho < R; rho += TRK_THREADS / 16) {
        const int tau = tau0 + rho;
        const bool ok = c < C && tau >= 0 && tau < T;
        S[rho * 16 + c] = ok ? (double)sb[(size_t)tau * C + c] : 0.0;
    }
}

// stages 1 and 2 of this wave's 16-frame tile of the chunk at cs: put(row of the chunk, column of the workgroup, |y|)
template <class Put>
__device__ __forceinline__ void track_ws_tile(const double *S, const double *ntab, int NK, int cs, int T, int wv, int lc, int q,
                                              const double (&Wf)[4][4], const Put &put)
{
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
    // ---- y of the tile against the four DoA tiles, |y| to the caller ----
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vacc[k], Wf[j][k], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) put(wv * 16 + q + 4 * r, 16 * j + lc, fabs(acc[r]));
    }
}

// the same step, complex
template <int KM, int KV>
struct TrackCW {
    static constexpr int KVD = KV > 0 ? KV : 1;
    double Wf[4][2][KM], Wv[4][2][KVD];
};

template <int KM, int KV>
__device__ __forceinline__ void track_wsc_weights(TrackCW<KM, KV> &w, const double *__restrict__ Wp, int GT, int cg, int lc, int q)
{
    const int Gp = 16 * GT, GTc = GT >> 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ct = 4 * cg + j;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const double *wp = Wp + 16 * ((ct < GTc ? ct : GTc - 1) + part * GTc) + lc;
#pragma unroll
            for (int k = 0; k < KM; ++k) w.Wf[j][part][k] = wp[(size_t)(4 * k + q) * Gp];
#pragma unroll
            for (int i = 0; i < KV; ++i) w.Wv[j][part][i] = wp[(size_t)(4 * KM + i) * Gp];
        }
    }
}

// this wave's tile as A-fragments (beamform_wsc_kernel, stage 1): lane l of k-step k = channel 4k + (l >> 4), frame l & 15; the fragment
// of the KV tail channels goes to the wave's `tail`, which track_wsc_tile reads behind a barrier
template <int KM, int KV>
__device__ __forceinline__ void track_wsc_frags(double (&V)[KM + (KV > 0 ? 1 : 0)], double *tail, const double *__restrict__ pb, int C, int stride,
                                                int cs, int T, int wv, int l)
{
    constexpr int KF = KM + (KV > 0 ? 1 : 0);
    const int lc = l & 15, q = l >> 4;
    const int t = cs + wv * 16 + lc;
#pragma unroll
    for (int k = 0; k < KF; ++k) {
        const int c = 4 * k + q;
        const double v = pb[(size_t)(c < C ? c : C - 1) * stride + (t < T ? t : T - 1)];  // (clamped: unconditional loads)
        V[k] = (t < T && c < C) ? v : 0.0;
    }
    if (KV > 0) tail[l] = V[KF - 1];
}

// stage 2 of the tile: put(row of the chunk, column of the workgroup, |y| = hypot(re, im))
template <int KM, int KV, class Put>
__device__ __forceinline__ void track_wsc_tile(const double (&V)[KM + (KV > 0 ? 1 : 0)], const double *tail, const TrackCW<KM, KV> &w, int wv, int lc,
                                               int q, const Put &put)
{
    constexpr int KVD = KV > 0 ? KV : 1;
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
            for (int k = 0; k < KM; ++k) acc[part] = __builtin_amdgcn_mfma_f64_16x16x4f64(V[k], w.Wf[j][part][k], acc[part], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < KV; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[part][r] = __builtin_fma(Vv[i][r], w.Wv[j][part][i], acc[part][r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) put(wv * 16 + q + 4 * r, 16 * j + lc, track_magnitude(acc[0][r], acc[1][r]));
    }
}

// where a tile's magnitude goes: stored (the single-plan walks, and the first band of a band walk) or added with one rounded add (every
// later band).  A thread meets the same elements of Y in every band: the bands need no barrier for Y among themselves.
struct TrackBandPut {
    double *Y;
    bool first;
    __device__ __forceinline__ void operator()(int row, int col, double a) const
    {
        double *y = Y + row * TRK_LD + col;
        *y = first ? a : __dadd_rn(*y, a);
    }
};

// SNN: the frames [f0, T) of one trial's int8 raster sb [..][C], C <= 16, in chunks of TRK_CH from f0; position p is frame abs0 + p.
// Rows outside [0, T) and the channel padding are zero.  Per chunk: staging, stages 1 and 2, then track_chain_reduce with
// emit(cs, row, best, bi) for the pair of position cs + row.  state: the chain wave's e[t-1] of its column, carried across the chunks.
// One plan: the neuron table and the bf_mat fragments are fetched once, in front of the chunks.
template <class Emit>
__device__ __forceinline__ void track_ws_walk(unsigned char *smem, const int8_t *__restrict__ sb, int C, int f0, int T, int abs0,
                                              const double *__restrict__ ntab_g, int NK, const double *__restrict__ Wp, int GT, int G, int cg,
                                              double a_rise, double i_rise, double a_fall, double &state, const Emit &emit)
{
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    const int lc = l & 15;
    const int q = l >> 4;
    double *Y = reinterpret_cast<double *>(smem);  // [TRK_CH][TRK_LD]
    double *ntab = Y + TRK_CH * TRK_LD;
    double *S = ntab + 4 * NK + 16;  // spike tile as fp64 [R][16]

    track_ws_table(ntab, ntab_g, NK, tid);
    double Wf[4][4];
    track_ws_weights(Wf, Wp, GT, cg, lc, q);
    for (int cs = f0; cs < T; cs += TRK_CH) {
        track_ws_stage(S, sb, C, cs, T, NK, tid);
        __syncthreads();
        track_ws_tile(S, ntab, NK, cs, T, wv, lc, q, Wf, TrackBandPut{Y, true});
        __syncthreads();
        const int nrow = T - cs < TRK_CH ? T - cs : TRK_CH;
        track_chain_reduce(Y, wv, l, tid, cs, abs0 + cs == 0, nrow, G, cg, a_rise, i_rise, a_fall, state, emit);
        // (the next chunk's staging touches S only; its writes to Y come after the barrier behind the staging)
    }
}

// complex: the frames [f0, T) of one trial's planar band-passed rows pb [C = 2M][stride], C <= 16; the rest as track_ws_walk.  A
// 16-frame tile starts at any column: the operands are single doubles, which need no more than their own alignment.
template <int KM, int KV, class Emit>
__device__ __forceinline__ void track_wsc_walk(unsigned char *smem, const double *__restrict__ pb, int C, int stride, int f0, int T, int abs0,
                                               const double *__restrict__ Wp, int GT, int G, int cg, double a_rise, double i_rise,
                                               double a_fall, double &state, const Emit &emit)
{
    constexpr int KF = KM + (KV > 0 ? 1 : 0);
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    const int lc = l & 15;
    const int q = l >> 4;
    double *Y = reinterpret_cast<double *>(smem);
    double *tail = Y + TRK_CH * TRK_LD + wv * 64;  // this wave's fragment of the KV tail channels

    TrackCW<KM, KV> w;
    track_wsc_weights<KM, KV>(w, Wp, GT, cg, lc, q);
    for (int cs = f0; cs < T; cs += TRK_CH) {
        double V[KF];
        track_wsc_frags<KM, KV>(V, tail, pb, C, stride, cs, T, wv, l);
        __syncthreads();  // (also: the previous chunk's row reduction is done with Y)
        track_wsc_tile<KM, KV>(V, tail, w, wv, lc, q, TrackBandPut{Y, true});
        __syncthreads();
        const int nrow = T - cs < TRK_CH ? T - cs : TRK_CH;
        track_chain_reduce(Y, wv, l, tid, cs, abs0 + cs == 0, nrow, G, cg, a_rise, i_rise, a_fall, state, emit);
    }
}

// pairs of one row in ascending column order -> the first maximum (a strictly larger value takes over)
__device__ __forceinline__ void track_combine_row(const double *__restrict__ pval, const int32_t *__restrict__ pidx, int ncg, double &best, int &bi)
{
    best = -1.0;
    bi = TRK_NONE;
    for (int c = 0; c < ncg; ++c) {
        const double v = pval[c];
        const int i = pidx[c];
        if (i != TRK_NONE && v > best) {
            best = v;
            bi = i;
        }
    }
}

}  // namespace micloc
