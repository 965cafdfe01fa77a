// The arithmetic of MUSIC, stated ONCE for the one-shot kernels (music.hip) and the stream (stream_music.hip): the bits of a slice depend
// on these statements only, never on the buffers they run on, which is what makes a stream end on micloc_music_f64's bits.
//   music_df2t_step     one sample of the band-pass (music.hip's own statement: the last state is fma(b, x, 0.0), NC == 1 is b0 * x --
//                       not Df2tChain's of bandpass_rows.h)
//   music_dft_rows      the k-loop of the band-limited DFT of 64 frame rows on the fp64 matrix cores
//   music_bin_power, music_bin_rank      mean |X|^2 of a bin over (mic, frame); its place in the stable ascending sort.  THE RANK RULE:
//                       a total order -- ascending power, a NaN behind every number, equal powers and NaNs by bin index (the later bin
//                       sorts later).  Every position of sel is written exactly once, by one thread, with a bin in [0, nbin), whatever
//                       the samples hold (a NaN or Inf sample makes every bin power of its slice NaN)
//   music_steer_sum     P[g] over the selected bins, in their order
//   music_power_add, music_first_max, music_first_argmax      the read-out  sum_s P^2  and the first maximum
// The frame rows of a slice are rows (base M + m) Fs + f of xf / X: base = trial x slice (one-shot) or trial x slot (stream), Fs the
// frames a slice has room for.
#pragma once
#include <type_traits>

#include "readout_rows.h"

namespace micloc {

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double double2_t __attribute__((ext_vector_type(2)));

constexpr int MU_KC = 32;  // k rows of W staged in LDS per step of the DFT

// DF2T: y = fma(b0, x, z0); z_i = fma(-a_{i+1}, y, fma(b_{i+1}, x, z_{i+1})); z has max(NC - 1, 1) words
template <int NC>
__device__ __forceinline__ double music_df2t_step(const IirCoef &co, double xv, double *z)
{
    const double y = NC > 1 ? __builtin_fma(co.b[0], xv, z[0]) : co.b[0] * xv;
#pragma unroll
    for (int k = 0; k < NC - 1; ++k) z[k] = __builtin_fma(-co.a[k + 1], y, __builtin_fma(co.b[k + 1], xv, k + 1 < NC - 1 ? z[k + 1] : 0.0));
    return y;
}

// f(std::integral_constant<int, n>) for a filter of n coefficients (any n past 8 runs the MICLOC_MAX_IIR form)
template <class Fn>
hipError_t music_dispatch_order(int n, Fn &&f)
{
    switch (n) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, MICLOC_MAX_IIR>{});
    }
}

// f(std::integral_constant<int, CT>) for the column tiles of 16 a DFT workgroup takes: all Cp / 16 of them up to 8
template <class Fn>
hipError_t music_dispatch_tiles(int Cp, Fn &&f)
{
    const int tiles = Cp / 16;
    switch (tiles < 8 ? tiles : 8) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
    }
}

// One workgroup of 256: 4 waves x 16 frame rows, CT column tiles of 16 (one 16 x 16 accumulator each).  Per step of 32 k: the W rows
// [k0, k0 + 32) x the workgroup's columns go to LDS; every lane holds 8 consecutive samples of its row (k = k0 + 8 (lane >> 4) + j in
// k-step j), so the A operand is read as 64 contiguous bytes per lane and the B operand of k-step j is W row k0 + 8 (lane >> 4) + j.
// arow: the lane's row at column 8 (lane >> 4); Ws: MU_KC * 16 CT doubles of LDS; acc: the f64 C/D map -- acc[t][r] is row
// (lane >> 4) + 4 r of the wave's 16, column 16 t + (lane & 15).  Every thread of the workgroup calls it (barriers inside).
template <int CT>
__device__ __forceinline__ void music_dft_rows(const double *__restrict__ arow, const double *__restrict__ W, int Np, int Cp, int col0, int ncol,
                                               double *Ws, double4_t (&acc)[CT])
{
    constexpr int WC = 16 * CT;
    const int lane = threadIdx.x & 63;
    const int q = lane >> 4, c = lane & 15;
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
    double2_t a[4], an[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const double2_t *>(arow + 2 * i);
    for (int k0 = 0; k0 < Np; k0 += MU_KC) {
        __syncthreads();
        for (int e = threadIdx.x; e < MU_KC * WC; e += 256) {
            const int r = e / WC, cc = e - r * WC;
            Ws[e] = cc < ncol ? W[(size_t)(k0 + r) * Cp + col0 + cc] : 0.0;
        }
        __syncthreads();
        const bool more = k0 + MU_KC < Np;
#pragma unroll
        for (int i = 0; i < 4; ++i) an[i] = more ? *reinterpret_cast<const double2_t *>(arow + k0 + MU_KC + 2 * i) : a[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double av = a[j >> 1][j & 1];
            const double *wr = Ws + (8 * q + j) * WC + c;
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, wr[16 * t], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = an[i];
    }
}

// mean over (mic, frame) of |X|^2 at in-band bin j of the slice whose rows are (base M + m) Fs + f, f < F
__device__ __forceinline__ double music_bin_power(const double *__restrict__ X, size_t base, int M, int Fs, int F, int Cp, int j)
{
    const double inv = (double)(M * F);
    double sum = 0.0;
    for (int m = 0; m < M; ++m) {
        const double *xr = X + ((base * M + m) * Fs) * Cp + 2 * j;
        for (int f = 0; f < F; ++f) {
            const double re = xr[(size_t)f * Cp], im = xr[(size_t)f * Cp + 1];
            sum = sum + (re * re + im * im);
        }
    }
    return sum / inv;
}

// position of bin j in a stable ascending sort of pw[0 .. nbin): the last ksel positions are the selection, in that order.  The order
// is total (np.argsort(kind="stable")'s): a NaN sorts behind every number, and among NaNs as among equal numbers the later bin sorts
// later -- so the ranks of the nbin bins are a permutation of 0 .. nbin - 1, whatever pw holds
__device__ __forceinline__ int music_bin_rank(const double *pw, int nbin, int j)
{
    const double p = pw[j];
    const bool pnan = p != p;
    int rank = 0;
    for (int i = 0; i < nbin; ++i) {
        const double pi = pw[i];
        rank += pnan ? (pi == pi || i < j) : ((pi < p) || (pi == p && i < j));
    }
    return rank;
}

// P[g] = sum over the selected bins, in that order, of mean_f |a(bin, g)^H X[:, f, bin]|^2
__device__ __forceinline__ double music_steer_sum(const double *__restrict__ X, size_t base, int M, int Fs, int F, int Cp,
                                                  const int32_t *sel, int ksel, const double *__restrict__ sre, const double *__restrict__ sim,
                                                  int G, int g)
{
    double P = 0.0;
    for (int i = 0; i < ksel; ++i) {
        const int j = sel[i];
        double acc = 0.0;
        for (int f = 0; f < F; ++f) {
            double zr = 0.0, zi = 0.0;
            for (int m = 0; m < M; ++m) {
                const size_t ai = ((size_t)j * M + m) * G + g;
                const double ar = sre[ai], aim = sim[ai];
                const double *xr = X + ((base * M + m) * Fs + f) * Cp + 2 * j;
                const double re = xr[0], im = xr[1];
                // conj(a) x = (ar re + ai im) + 1j (ar im - ai re)
                zr = zr + (ar * re + aim * im);
                zi = zi + (ar * im - aim * re);
            }
            acc = acc + (zr * zr + zi * zi);
        }
        P = P + acc / (double)F;
    }
    return P;
}

// the read-out's sum over slices, left to right: p_s = p_{s-1} + v_s v_s from p = 0; power = p / S
__device__ __forceinline__ double music_power_add(double p, double v) { return p + v * v; }

// a thread's running first maximum over ascending g (besti < 0: none yet)
__device__ __forceinline__ void music_first_max(double p, int g, double &best, int &besti)
{
    if (besti < 0 || p > best) {
        best = p;
        besti = g;
    }
}

// first maximum (np.argmax) over a workgroup of 256: the larger value, on equal values the smaller index -> bi[0] (valid after the call)
__device__ __forceinline__ int music_first_argmax(double best, int besti, double *bv, int *bi)
{
    bv[threadIdx.x] = best;
    bi[threadIdx.x] = besti;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const double ov = bv[threadIdx.x + h];
            const int oi = bi[threadIdx.x + h];
            if (better<-1>(ov, oi, bv[threadIdx.x], bi[threadIdx.x])) {  // readout_rows.h's rule; "none" is any index < 0 here, and only -1 occurs
                bv[threadIdx.x] = ov;
                bi[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    return bi[0];
}

}  // namespace micloc
