// The multi-source row rule as a device function: the K strongest local maxima of ONE stored row of a DoA power profile, by one wave.
// The rule is stated in full in include/micloc_hip.h ("Multi-source read-out"); tests/multisource_ref.py restates it in NumPy.
//
// New code that applies the rule to a row includes this header (stream_peaks.hip: the running row and the window rows of a stream).
// THE ONE EXCEPTION, after the precedent of readout_rows.h rule 1: csrc/peaks.hip (doa_peaks_kernel, micloc_doa_peaks_f64) keeps its own
// text.  Its hash is pinned by profiles/multisource/RECORD.json, which tests/test_multitarget_golden_cpu.py checks against the tree; the copy
// folds in here with the next profile round.  Until then tests/test_hip_stream_peaks.py holds the two spellings to each other bit for bit.
//
// One wave (64 lanes, a workgroup of its own) per row.  The row's ring values and their reported indices are staged in LDS (12 bytes per
// ring point, G <= 4096: at most 48 KiB); a first pass marks the candidates (local maxima above the threshold), then K rounds each take
// the best remaining candidate by a cross-lane first maximum (value descending, reported index ascending: __shfl_xor, no LDS) and strike
// every candidate closer to it than min_separation.  The comparison and the butterfly are readout_rows.h's (rule 1: `better`,
// wave_first_max).  Greedy suppression in candidate order is the selection of the rule: a point struck by an accepted peak would have
// been rejected when visited, and the best unstruck candidate is the next one the rule accepts.  Unfilled slots get -1 and NaN.  No atomics.
#pragma once
#include "readout_rows.h"

namespace micloc {

constexpr int PKR_WAVE = 64;
constexpr int PKR_NONE = RO_NONE;  // no candidate

// ring points of a row of G grid points
__host__ __device__ inline int peaks_ring_points(int G, int kind) { return (kind == MICLOC_GRID_CIRCULAR_CLOSED && G >= 2) ? G - 1 : G; }
// dynamic LDS of a workgroup that calls peaks_row
__host__ __device__ inline size_t peaks_row_lds_bytes(int G, int kind) { return (size_t)peaks_ring_points(G, kind) * (sizeof(double) + sizeof(int)); }

__device__ __forceinline__ double peaks_dist(double a, double b, int circular)
{
    const double r = fabs(a - b);
    if (!circular) return r;
    const double w = 6.283185307179586 - r;  // 2 pi (the double np.pi * 2)
    return w < r ? w : r;
}

// p [G]: the row; doa [G]; lds: peaks_row_lds_bytes(G, kind) bytes of the workgroup's LDS, 8-byte aligned.  index [K] and value [K] (value
// may be NULL) take the accepted peaks in selection order; index2 / value2 (each may be NULL) take the same K entries a second time (the
// newest window of a stream).  EVERY lane of the workgroup (one wave) calls it with the same arguments; it ends behind a barrier, so the
// caller may call it again on the same LDS.
__device__ __forceinline__ void peaks_row(const double *__restrict__ p, int G, const double *__restrict__ doa, int kind, int K, double min_sep,
                                          double rel, int32_t *__restrict__ index, double *__restrict__ value, int32_t *__restrict__ index2,
                                          double *__restrict__ value2, double *lds)
{
    const int lane = threadIdx.x;
    const bool closed = kind == MICLOC_GRID_CIRCULAR_CLOSED && G >= 2;
    const int circular = kind != MICLOC_GRID_LINEAR;
    const int R = closed ? G - 1 : G;             // ring points
    double *sv = lds;                             // [R] ring values
    int *si = reinterpret_cast<int *>(lds + R);   // [R] reported index while a candidate, PKR_NONE otherwise

    // stage the ring; row maximum over the non-NaN values
    double mx = -__builtin_inf();
    for (int r = lane; r < R; r += PKR_WAVE) {
        double v = p[r];
        if (closed && r == 0) {
            // the seam: points 0 and G-1 are one direction; a NaN counts as lower
            const double q = p[G - 1];
            if (!(isnan(q) || v >= q)) v = q;
        }
        sv[r] = v;
        if (v > mx) mx = v;
    }
    for (int off = PKR_WAVE / 2; off > 0; off >>= 1) {
        const double o = __shfl_xor(mx, off, PKR_WAVE);
        mx = o > mx ? o : mx;
    }
    const double thr = rel * mx;
    __syncthreads();

    // candidates: non-NaN, >= each neighbour (a NaN neighbour counts as lower), above the threshold when rel > 0
    for (int r = lane; r < R; r += PKR_WAVE) {
        const double v = sv[r];
        bool c = !isnan(v);
        if (r > 0 || circular) {
            const double l = sv[r > 0 ? r - 1 : R - 1];
            c = c && (isnan(l) || v >= l);
        }
        if (r < R - 1 || circular) {
            const double h = sv[r < R - 1 ? r + 1 : 0];
            c = c && (isnan(h) || v >= h);
        }
        if (rel > 0.0) c = c && v >= thr;
        int id = r;
        if (closed && r == 0 && !(isnan(p[G - 1]) || p[0] >= p[G - 1])) id = G - 1;
        si[r] = c ? id : PKR_NONE;
    }
    __syncthreads();

    int found = 0;
    for (int k = 0; k < K; ++k) {
        double bv = 0.0;
        int bi = PKR_NONE;
        for (int r = lane; r < R; r += PKR_WAVE) {
            const int i = si[r];
            const double v = sv[r];
            if (better(v, i, bv, bi)) {  // value descending, reported index ascending; PKR_NONE is no candidate
                bv = v;
                bi = i;
            }
        }
        wave_first_max<PKR_WAVE>(bv, bi);
        if (bi == PKR_NONE) break;  // (wave-uniform after the butterfly)
        if (lane == 0) {
            index[k] = bi;
            if (value) value[k] = bv;
            if (index2) index2[k] = bi;
            if (value2) value2[k] = bv;
        }
        ++found;
        // strike the accepted point and every candidate closer to it than min_sep
        const double da = doa[bi];
        for (int r = lane; r < R; r += PKR_WAVE) {
            const int i = si[r];
            if (i == PKR_NONE) continue;
            if (i == bi || !(peaks_dist(doa[i], da, circular) >= min_sep)) si[r] = PKR_NONE;
        }
        __syncthreads();
    }
    for (int k = found + lane; k < K; k += PKR_WAVE) {
        index[k] = -1;
        if (value) value[k] = __builtin_nan("");
        if (index2) index2[k] = -1;
        if (value2) value2[k] = __builtin_nan("");
    }
    __syncthreads();  // the next row of this workgroup restages the LDS
}

}  // namespace micloc
