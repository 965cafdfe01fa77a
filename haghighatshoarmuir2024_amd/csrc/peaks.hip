// Multi-source read-out: the K strongest local maxima of every row of a DoA power profile (micloc_doa_peaks_f64).
// The rule is stated in full in include/micloc_hip.h; tests/multisource_ref.py restates it in NumPy and the two agree bit for bit.
//
// One wave (64 lanes) per row.  The row's ring values and their reported indices are staged in LDS (12 bytes per grid point);
// a first pass marks the candidates (local maxima above the threshold), then K rounds each take the best remaining candidate
// by a cross-lane arg-max (value descending, index ascending: __shfl_xor, no LDS) and strike every candidate closer to it than
// min_separation.  Greedy suppression in candidate order is the selection of the rule: a point struck by an accepted peak
// would have been rejected when visited, and the best unstruck candidate is the next one the rule accepts.
// No atomics, no host synchronisation: graph-capturable.
#include "micloc_internal.h"

namespace micloc {

namespace {

constexpr int PK_WAVE = 64;
constexpr int PK_NONE = 0x7fffffff;

// (va, ia) beats (vb, ib): value descending, reported index ascending; PK_NONE is no candidate
__device__ __forceinline__ bool pk_better(double va, int ia, double vb, int ib)
{
    if (ia == PK_NONE) return false;
    if (ib == PK_NONE) return true;
    return va > vb || (va == vb && ia < ib);
}

__device__ __forceinline__ double pk_dist(double a, double b, int circular)
{
    const double r = fabs(a - b);
    if (!circular) return r;
    const double w = 6.283185307179586 - r;  // 2 pi (the double np.pi * 2)
    return w < r ? w : r;
}

}  // namespace

__global__ __launch_bounds__(PK_WAVE) void doa_peaks_kernel(const double *__restrict__ power, int G, const double *__restrict__ doa,
                                                             int kind, int K, double min_sep, double rel, int32_t *__restrict__ index,
                                                             double *__restrict__ value)
{
    extern __shared__ double pk_lds[];
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const bool closed = kind == MICLOC_GRID_CIRCULAR_CLOSED && G >= 2;
    const int circular = kind != MICLOC_GRID_LINEAR;
    const int R = closed ? G - 1 : G;  // ring points
    double *sv = pk_lds;                                   // [R] ring values
    int *si = reinterpret_cast<int *>(pk_lds + R);         // [R] reported index while a candidate, PK_NONE otherwise
    const double *p = power + (size_t)b * G;

    // stage the ring; row maximum over the non-NaN values
    double mx = -__builtin_inf();
    for (int r = lane; r < R; r += PK_WAVE) {
        double v = p[r];
        if (closed && r == 0) {
            // the seam: points 0 and G-1 are one direction; a NaN counts as lower
            const double q = p[G - 1];
            if (!(isnan(q) || v >= q)) v = q;
        }
        sv[r] = v;
        if (v > mx) mx = v;
    }
    for (int off = PK_WAVE / 2; off > 0; off >>= 1) {
        const double o = __shfl_xor(mx, off, PK_WAVE);
        mx = o > mx ? o : mx;
    }
    const double thr = rel * mx;
    __syncthreads();

    // candidates: non-NaN, >= each neighbour (a NaN neighbour counts as lower), above the threshold when rel > 0
    for (int r = lane; r < R; r += PK_WAVE) {
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
        si[r] = c ? id : PK_NONE;
    }
    __syncthreads();

    int found = 0;
    for (int k = 0; k < K; ++k) {
        double bv = 0.0;
        int bi = PK_NONE;
        for (int r = lane; r < R; r += PK_WAVE) {
            const int i = si[r];
            const double v = sv[r];
            if (pk_better(v, i, bv, bi)) {
                bv = v;
                bi = i;
            }
        }
        for (int off = PK_WAVE / 2; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, PK_WAVE);
            const int oi = __shfl_xor(bi, off, PK_WAVE);
            if (pk_better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (bi == PK_NONE) break;  // (wave-uniform after the butterfly)
        if (lane == 0) {
            index[(size_t)b * K + k] = bi;
            if (value) value[(size_t)b * K + k] = bv;
        }
        ++found;
        // strike the accepted point and every candidate closer to it than min_sep
        const double da = doa[bi];
        for (int r = lane; r < R; r += PK_WAVE) {
            const int i = si[r];
            if (i == PK_NONE) continue;
            if (i == bi || !(pk_dist(doa[i], da, circular) >= min_sep)) si[r] = PK_NONE;
        }
        __syncthreads();
    }
    for (int k = found + lane; k < K; k += PK_WAVE) {
        index[(size_t)b * K + k] = -1;
        if (value) value[(size_t)b * K + k] = __builtin_nan("");
    }
}

hipError_t launch_doa_peaks(const double *power, int B, int G, const double *doa, int kind, int K, double min_sep, double rel, int32_t *index,
                            double *value, hipStream_t stream)
{
    const int R = (kind == MICLOC_GRID_CIRCULAR_CLOSED && G >= 2) ? G - 1 : G;
    // G <= 4096 (checked by the API): at most 48 KiB, within the default dynamic-LDS limit.  A larger G limit would need
    // hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize) here.
    const size_t dyn = (size_t)R * (sizeof(double) + sizeof(int));
    hipLaunchKernelGGL(doa_peaks_kernel, dim3(B), dim3(PK_WAVE), dyn, stream, power, G, doa, kind, K, min_sep, rel, index, value);
    return hipGetLastError();
}

}  // namespace micloc
