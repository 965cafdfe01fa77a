// What the tracking kernels share -- the one-shot ones of track.hip and the streaming ones of stream_track.hip: the shape of a
// workgroup (four waves, 64 frames x 64 DoA columns per chunk), the envelope recurrence over a chunk, the reduction of every frame to
// (max envelope, first index) over the workgroup's columns, and the rule of a row without a winner.  Stated once, so that a frame has the
// same bits whether its recording was walked in one launch or cut at launch borders.
#pragma once
#include <math.h>

#include "micloc_internal.h"

namespace micloc {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int TRK_WAVES = 4;
constexpr int TRK_THREADS = TRK_WAVES * 64;
constexpr int TRK_CH = TRK_WAVES * 16;  // frames per chunk: one 16-frame tile per wave
constexpr int TRK_COLS = 64;            // DoA columns per workgroup = lanes of the chain wave
constexpr int TRK_LD = TRK_COLS + 1;    // row stride of the magnitude tile (odd: the row reduction reads down columns)
constexpr int TRK_NONE = 0x7fffffff;

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

// a finished row: an all-NaN row (no column ever won) gives index 0 and peak NaN
__device__ __forceinline__ int track_row_index(int bi) { return bi == TRK_NONE ? 0 : bi; }
__device__ __forceinline__ double track_row_peak(double best, int bi) { return bi == TRK_NONE ? (double)NAN : best; }

// steps 3 and 4 of track.hip's header for a chunk of nrow frames whose magnitudes lie in Y.  first: the chunk begins at frame 0 of the
// recording (state_0 = |y_0|).  emit(row, best, bi): the pair of frame `row` of the chunk over this workgroup's columns, bi == TRK_NONE
// when no column won; called by one thread per frame.
template <class Emit>
__device__ __forceinline__ void track_chain_reduce(double *Y, int wv, int l, int tid, bool first, int nrow, int G, int cg, double a_rise,
                                                   double i_rise, double a_fall, double &state, Emit emit)
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
#pragma unroll
        for (int s = 1; s <= 2; s <<= 1) {
            const double ov = __shfl_xor(best, s, 64);
            const int oi = __shfl_xor(bi, s, 64);
            if (ov > best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
        if (part == 0 && row < nrow) emit(row, best, bi);
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
