// The MUSIC baseline beamformer for gfx950.
// Reference: micloc/music_beamformer.py MUSIC.beamforming (:92-176) per slice of MUSIC.apply_to_signal (:178-247), and the scripts'
// read-out power = np.mean(np.abs(P)**2, axis=0), argmax (paper_plots/target_localization_MUSIC.py).
//
// Per (trial b, slice s) of L samples advancing by `hop` (the last one may be shorter: the reference's leftover slice), with
// F_s = len_s // N FFT frames:
//   1. music_filter_kernel   the band-pass lfilter(b, a) of the slice from zero state (DF2T), only the first F_s N
//                            samples (the filter is causal), written as frame rows  xf[(bs M + m) Fmax + f][0 .. Np)  (zero padded
//                            to Np = N rounded up to 64; frames f >= F_s of a short slice are zero rows).  One lane per (slice, mic)
//                            stream, its samples loaded one chunk of 32 ahead; 32 samples of 64 streams go through an LDS tile so
//                            that the rows leave as contiguous stores.
//   2. music_dft_kernel      the band-limited DFT  X = xf . W  on the fp64 matrix cores (v_mfma_f64_16x16x4_f64): W [Np][Cp] holds
//                            cos / -sin of 2 pi ((k n) mod N) / N for the in-band bins only (column 2j: Re, 2j + 1: Im of bin j),
//                            built on the host once per plan.  Only the in-band bins are ever used (34 of 2048 at the scripts' shape),
//                            so this is a skinny GEMM rather than an FFT; any N works, odd sizes included.
//   3. music_select_kernel   bin power = mean over (mic, frame) of |X|^2, and the k strongest bins in np.argsort order (ascending
//                            power; exact ties: the later bin sorts later -- the stable "later index wins" contract of DESIGN section 2;
//                            a NaN power sorts behind every number: music_rows.h's rank rule, which fills every position of sel).
//   4. music_steer_kernel    P[g] = sum over the selected bins, in that order, of mean_f |a(bin, g)^H X[:, f, bin]|^2, with the
//                            steering table a = exp(-1j 2 pi freq_vec[bin] delays) computed by NumPy (the reference's own expression).
//   5. music_readout_kernel  optional: power[b][g] = mean_s P[b][s][g]^2 and its first arg-max.
// The arithmetic of every stage is music_rows.h's, which the stream (stream_music.hip) runs as well.
#include "music_rows.h"

namespace micloc {

namespace {

constexpr int MU_FILT_STREAMS = 64;  // streams per filter tile
constexpr int MU_FILT_CHUNK = 32;    // samples per stream and tile (Np is a multiple of it)

__device__ __forceinline__ int slice_frames(const MusicDims &d, int s)
{
    const int start = s * d.hop;
    return min(d.L, d.T - start) / d.N;
}

template <int NC>
__global__ __launch_bounds__(64) void music_filter_kernel(const double *__restrict__ x, double *__restrict__ xf, MusicDims d, IirCoef co)
{
    __shared__ double tile[MU_FILT_STREAMS][MU_FILT_CHUNK + 1];
    const int lane = threadIdx.x;
    const long long nstreams = (long long)d.B * d.S * d.M;
    const long long q = (long long)blockIdx.x * MU_FILT_STREAMS + lane;
    const bool valid = q < nstreams;
    const int m = valid ? (int)(q % d.M) : 0;
    const long long bs = valid ? q / d.M : 0;
    const int s = (int)(bs % d.S);
    const long long b = bs / d.S;
    const int F = valid ? slice_frames(d, s) : 0;
    const double *xs = x + ((size_t)b * d.T + (size_t)s * d.hop) * d.M + m;
    double z[NC > 1 ? NC - 1 : 1];
#pragma unroll
    for (int i = 0; i < NC - 1; ++i) z[i] = 0.0;
    // the samples of chunk (f, c0) are loaded one chunk ahead: the recurrence never waits for memory
    double cur[MU_FILT_CHUNK], nxt[MU_FILT_CHUNK];
#pragma unroll
    for (int i = 0; i < MU_FILT_CHUNK; ++i) cur[i] = (0 < F && i < d.N) ? xs[(size_t)i * d.M] : 0.0;
    const int chunks = d.Np / MU_FILT_CHUNK;
    for (int f = 0; f < d.Fmax; ++f) {
        for (int c = 0; c < chunks; ++c) {
            const int c0 = c * MU_FILT_CHUNK;
            const int fn = c + 1 < chunks ? f : f + 1, cn = c + 1 < chunks ? c0 + MU_FILT_CHUNK : 0;
#pragma unroll
            for (int i = 0; i < MU_FILT_CHUNK; ++i) nxt[i] = (fn < F && cn + i < d.N) ? xs[((size_t)fn * d.N + cn + i) * d.M] : 0.0;
#pragma unroll
            for (int i = 0; i < MU_FILT_CHUNK; ++i) {
                double v = 0.0;
                if (f < F && c0 + i < d.N) {
                    v = music_df2t_step<NC>(co, cur[i], z);
                }
                tile[lane][i] = v;
            }
            __syncthreads();
            // two rows per store instruction: lane -> row r + (lane >> 5), sample lane & 31
            for (int r = 0; r < MU_FILT_STREAMS; r += 2) {
                const int rr = r + (lane >> 5);
                const long long qr = (long long)blockIdx.x * MU_FILT_STREAMS + rr;
                if (qr < nstreams) xf[((size_t)qr * d.Fmax + f) * d.Np + c0 + (lane & 31)] = tile[rr][lane & 31];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < MU_FILT_CHUNK; ++i) cur[i] = nxt[i];
        }
    }
}

// One workgroup: 64 frame rows x CT column tiles of 16 (music_dft_rows).  Rows beyond R are padding of the frame buffer: computed, never
// stored (rows are independent in the product).
template <int CT>
__global__ __launch_bounds__(256) void music_dft_kernel(const double *__restrict__ xf, const double *__restrict__ W, double *__restrict__ X,
                                                        int Np, int Cp, long long R)
{
    constexpr int WC = 16 * CT;
    __shared__ double Ws[MU_KC * WC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = lane >> 4, c = lane & 15;
    const int col0 = blockIdx.y * WC;
    const int ncol = min(WC, Cp - col0);
    const size_t row0 = (size_t)blockIdx.x * 64 + (size_t)w * 16;
    double4_t acc[CT];
    music_dft_rows<CT>(xf + (row0 + c) * (size_t)Np + 8 * q, W, Np, Cp, col0, ncol, Ws, acc);
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        if (16 * t >= ncol) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t row = row0 + q + 4 * r;  // f64 C/D map: row (lane >> 4) + 4 r, column lane & 15
            if ((long long)row < R) X[row * Cp + col0 + 16 * t + c] = acc[t][r];
        }
    }
}

// One workgroup per (trial, slice).  pw in LDS (nbin doubles).
__global__ __launch_bounds__(256) void music_select_kernel(const double *__restrict__ X, int32_t *__restrict__ sel, MusicDims d)
{
    extern __shared__ double pw[];
    const int bs = blockIdx.x;
    const int F = slice_frames(d, bs % d.S);
    for (int j = threadIdx.x; j < d.nbin; j += blockDim.x) pw[j] = music_bin_power(X, (size_t)bs, d.M, d.Fmax, F, d.Cp, j);
    __syncthreads();
    // the last ksel positions of the stable ascending sort are the selection, in that order
    for (int j = threadIdx.x; j < d.nbin; j += blockDim.x) {
        const int pos = music_bin_rank(pw, d.nbin, j) - (d.nbin - d.ksel);
        if (pos >= 0) sel[(size_t)bs * d.ksel + pos] = j;
    }
}

__global__ __launch_bounds__(128) void music_steer_kernel(const double *__restrict__ X, const int32_t *__restrict__ sel,
                                                          const double *__restrict__ sre, const double *__restrict__ sim,
                                                          double *__restrict__ spec, MusicDims d)
{
    const int bs = blockIdx.x;
    const int g = blockIdx.y * blockDim.x + threadIdx.x;
    if (g >= d.G) return;
    const int F = slice_frames(d, bs % d.S);
    const double P = music_steer_sum(X, (size_t)bs, d.M, d.Fmax, F, d.Cp, sel + (size_t)bs * d.ksel, d.ksel, sre, sim, d.G, g);
    spec[(size_t)bs * d.G + g] = P;
}

__global__ __launch_bounds__(256) void music_readout_kernel(const double *__restrict__ spec, double *__restrict__ power,
                                                            int32_t *__restrict__ argmax, int S, int G)
{
    __shared__ double bv[256];
    __shared__ int bi[256];
    const int b = blockIdx.x;
    double best = 0.0;
    int besti = -1;
    for (int g = threadIdx.x; g < G; g += 256) {
        double p = 0.0;
        for (int s = 0; s < S; ++s) {
            p = music_power_add(p, spec[((size_t)b * S + s) * G + g]);
        }
        p = p / (double)S;
        if (power) power[(size_t)b * G + g] = p;
        music_first_max(p, g, best, besti);
    }
    const int first = music_first_argmax(best, besti, bv, bi);  // np.argmax: the larger value, on equal values the smaller index
    if (threadIdx.x == 0 && argmax) argmax[b] = first;
}

template <int CT>
hipError_t launch_dft(const double *xf, const double *W, double *X, int Np, int Cp, long long R, long long Rp, hipStream_t st)
{
    dim3 grid((unsigned)(Rp / 64), (unsigned)((Cp + 16 * CT - 1) / (16 * CT)));
    hipLaunchKernelGGL(music_dft_kernel<CT>, grid, dim3(256), 0, st, xf, W, X, Np, Cp, R);
    return hipGetLastError();
}

template <int NC>
hipError_t launch_filter(const double *x, double *xf, const MusicDims &d, const IirCoef &co, hipStream_t st)
{
    const long long nstreams = (long long)d.B * d.S * d.M;
    hipLaunchKernelGGL(music_filter_kernel<NC>, dim3((unsigned)((nstreams + MU_FILT_STREAMS - 1) / MU_FILT_STREAMS)), dim3(MU_FILT_STREAMS), 0, st,
                       x, xf, d, co);
    return hipGetLastError();
}

}  // namespace

MusicBuffers music_layout(const MusicDims &d)
{
    MusicBuffers L{};
    const long long R = (long long)d.B * d.S * d.M * d.Fmax;
    L.R = R;
    L.Rp = (R + 63) / 64 * 64;
    L.xf_bytes = (size_t)L.Rp * d.Np * sizeof(double);
    L.X_bytes = (size_t)L.Rp * d.Cp * sizeof(double);
    L.sel_bytes = (size_t)d.B * d.S * d.ksel * sizeof(int32_t);
    L.spec_bytes = (size_t)d.B * d.S * d.G * sizeof(double);
    return L;
}

hipError_t launch_music(const MusicDims &d, const IirCoef &co, const double *x, const double *W, const double *sre, const double *sim,
                        double *xf, double *X, int32_t *sel, double *spec, double *power, int32_t *argmax, hipStream_t st)
{
    const MusicBuffers L = music_layout(d);
    hipError_t e = hipSuccess;
    e = music_dispatch_order(co.n, [&](auto NC) { return launch_filter<decltype(NC)::value>(x, xf, d, co, st); });
    if (e != hipSuccess) return e;
    e = music_dispatch_tiles(d.Cp, [&](auto CT) { return launch_dft<decltype(CT)::value>(xf, W, X, d.Np, d.Cp, L.R, L.Rp, st); });
    if (e != hipSuccess) return e;
    const unsigned BS = (unsigned)(d.B * d.S);
    hipLaunchKernelGGL(music_select_kernel, dim3(BS), dim3(256), (size_t)d.nbin * sizeof(double), st, X, sel, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(music_steer_kernel, dim3(BS, (unsigned)((d.G + 127) / 128)), dim3(128), 0, st, X, sel, sre, sim, spec, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (power || argmax) {
        hipLaunchKernelGGL(music_readout_kernel, dim3((unsigned)d.B), dim3(256), 0, st, spec, power, argmax, d.S, d.G);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace micloc
