// MUSIC as a stream (micloc_stream_music_*): a recording that arrives in tiles, ending on micloc_music_f64's bits for any tiling.  The rule
// is stated in include/micloc_hip.h ("streaming, MUSIC"); DESIGN 4.19 has the state and the footprint.  The arithmetic is music_rows.h's,
// the statements the one-shot kernels of music.hip run.
//
// Slice s covers samples [s hop, s hop + L) and lives in slot s % K of the state, K = ceil(L / hop) + 1: the slot's next slice starts at
// least hop samples after this one's last sample.  A lane, a frame row and a slot find their place in time from the clock alone:
// with P = K hop the slot's slices start at  slot hop + j P.
//
// A tile is cut into pieces of at most hop samples (a cut that depends on the tile's length only), and a piece of n samples is
//   music_stream_filter_tile_kernel<NC>   one lane per (trial, slot, mic): the DF2T chain of the slot's slice over the piece's samples
//                                         that fall into the slice's first F N samples, from zero state at the slice's first sample;
//                                         appended to the slot's frame rows.  Samples are loaded one chunk of 32 ahead
//   music_stream_dft_kernel<CT>           music_dft_rows on the 64-row blocks that hold a frame whose last sample arrived in this piece
//                                         (a block without one leaves at once); only those rows are stored
//   music_stream_slice_kernel             one workgroup per (trial, slot): for the slot whose slice ends in this piece (and, on the final
//                                         piece, the leftover slice) bin power, stable rank, steering sum, first arg-max -> the slot's
//                                         spectrum row, the result ring and latest_*
//   music_stream_readout_kernel           one workgroup per trial: the slices closed by this piece in ascending order onto sum_s P^2,
//                                         power = sum / count, first arg-max; then the trial's clock
// on one stream, one after the other.  Why a piece is at most hop samples and a slot rests for hop samples: the filter kernel runs over the
// whole piece before the DFT and the slice kernel see it, so nothing it writes in a piece may land on a frame row or a DFT row that the
// later kernels of the same piece still read.  Frame f of a slice is complete P - N + 1 >= hop + 1 samples before the slot's next slice
// reaches the row, and a slice's DFT rows are read (at its last sample) P - L + N >= hop + N samples before the next slice's frame 0 is
// transformed.  A piece also closes at most one full slice.
//
// THE CLOCK is one record of four ints per trial {samples pushed, slices emitted, short-leftover flag, open slices}: workgroup b of the
// read-out kernel is the only writer of record b and the only reader of it in that launch (behind a barrier), every other kernel only
// reads it.  All records hold the same clock.
#include "music_rows.h"
#include "stream_music.h"

namespace micloc {

namespace {

constexpr int MS_LANES = 64;  // chains per workgroup of the filter kernel
constexpr int MS_CHUNK = 32;  // samples loaded ahead per chain

// does an event that happens at samples e + j P (j >= 0) happen in [t0, t1)?  *j: which one (the last, should there be several)
__device__ __forceinline__ bool ms_event(long long e, int P, long long t0, long long t1, long long *j)
{
    if (t1 - 1 < e) return false;
    *j = (t1 - 1 - e) / P;
    return e + *j * P >= t0;
}

// the reference's leftover slice of a recording of T samples: *s (or -1: none) and its frames (0: shorter than N)
__device__ __forceinline__ void ms_leftover(const MusicStreamDims &d, long long T, long long *s, int *F)
{
    const long long full = T >= d.L ? (T - d.L) / d.hop + 1 : 0;
    const long long rest = T - full * d.hop;
    *s = 2 * rest > d.L ? full : -1;  // (T - start) > 0.5 L
    *F = (int)(rest / d.N);
}

template <int NC>
__global__ __launch_bounds__(MS_LANES) void music_stream_filter_tile_kernel(const double *__restrict__ x, size_t trial_stride, int n,
                                                                            MusicStreamDims d, IirCoef co, const int *__restrict__ clk,
                                                                            double *__restrict__ zst, double *__restrict__ xf)
{
    const long long nl = (long long)d.B * d.slots * d.M;
    const long long q = (long long)blockIdx.x * MS_LANES + threadIdx.x;
    if (q >= nl) return;  // (no barrier in this kernel)
    const int m = (int)(q % d.M);
    const long long bk = q / d.M;
    const int slot = (int)(bk % d.slots);
    const long long b = bk / d.slots;
    const int P = d.slots * d.hop, FN = d.F * d.N;
    // o: the sample's place in the slot's current slice (< 0: the slot's first slice has not begun); (f, p): its frame and column
    long long o0 = (long long)clk[4 * b] - (long long)slot * d.hop;
    if (o0 >= 0) o0 %= P;
    int o = (int)o0;
    int f = o > 0 ? o / d.N : 0, p = o > 0 ? o % d.N : 0;
    double z[NC > 1 ? NC - 1 : 1];
#pragma unroll
    for (int i = 0; i < NC - 1; ++i) z[i] = zst[(size_t)i * nl + q];
    const double *xs = x + (size_t)b * trial_stride + m;
    double *rows = xf + (size_t)q * d.F * d.Np;
    double cur[MS_CHUNK], nxt[MS_CHUNK];
#pragma unroll
    for (int i = 0; i < MS_CHUNK; ++i) cur[i] = i < n ? xs[(size_t)i * d.M] : 0.0;
    for (int c0 = 0; c0 < n; c0 += MS_CHUNK) {
#pragma unroll
        for (int i = 0; i < MS_CHUNK; ++i) nxt[i] = c0 + MS_CHUNK + i < n ? xs[(size_t)(c0 + MS_CHUNK + i) * d.M] : 0.0;
        // a whole chunk that every lane of the wave spends inside one frame of its slice (act) or outside the filtered part of it (idle):
        // no per-sample bookkeeping -- the steady state of a tile that is cut like the frames
        const bool act = o >= 0 && o + MS_CHUNK <= FN && p + MS_CHUNK <= d.N;
        const bool idle = o < 0 ? o + MS_CHUNK <= 0 : (o >= FN && o + MS_CHUNK <= P);
        if (c0 + MS_CHUNK <= n && __all(act || idle)) {
            if (act) {
                if (o == 0) {
#pragma unroll
                    for (int k = 0; k < NC - 1; ++k) z[k] = 0.0;
                    f = 0, p = 0;
                }
                double *dst = rows + (size_t)f * d.Np + p;
#pragma unroll
                for (int i = 0; i < MS_CHUNK; ++i) dst[i] = music_df2t_step<NC>(co, cur[i], z);
                if ((p += MS_CHUNK) == d.N) p = 0, ++f;
            }
            if ((o += MS_CHUNK) == P) o = 0;
        } else {
#pragma unroll
            for (int i = 0; i < MS_CHUNK; ++i) {
                if (c0 + i < n) {
                    if (o == 0) {  // the slot's next slice begins: lfilter's zero state
#pragma unroll
                        for (int k = 0; k < NC - 1; ++k) z[k] = 0.0;
                        f = 0, p = 0;
                    }
                    if (o >= 0 && o < FN) {
                        rows[(size_t)f * d.Np + p] = music_df2t_step<NC>(co, cur[i], z);
                        if (++p == d.N) p = 0, ++f;
                    }
                    if (++o == P) o = 0;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < MS_CHUNK; ++i) cur[i] = nxt[i];
    }
#pragma unroll
    for (int i = 0; i < NC - 1; ++i) zst[(size_t)i * nl + q] = z[i];
}

// frame row r = ((b K + slot) M + m) F + f: does its last sample arrive in this piece?
__device__ __forceinline__ bool ms_row_completes(const MusicStreamDims &d, const int *__restrict__ clk, long long r, int n)
{
    const int f = (int)(r % d.F);
    const long long bk = r / d.F / d.M;
    const int slot = (int)(bk % d.slots);
    const long long t0 = clk[4 * (bk / d.slots)];
    long long j;
    return ms_event((long long)slot * d.hop + (long long)(f + 1) * d.N - 1, d.slots * d.hop, t0, t0 + n, &j);
}

template <int CT>
__global__ __launch_bounds__(256) void music_stream_dft_kernel(const double *__restrict__ xf, const double *__restrict__ W, double *__restrict__ X,
                                                               MusicStreamDims d, int n, const int *__restrict__ clk, long long R)
{
    constexpr int WC = 16 * CT;
    __shared__ double Ws[MU_KC * WC];
    __shared__ int done[64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = lane >> 4, c = lane & 15;
    const int col0 = blockIdx.y * WC;
    const int ncol = min(WC, d.Cp - col0);
    int mine = 0;
    if (threadIdx.x < 64) {
        const long long r = (long long)blockIdx.x * 64 + threadIdx.x;
        mine = r < R && ms_row_completes(d, clk, r, n);
        done[threadIdx.x] = mine;
    }
    if (!__syncthreads_or(mine)) return;
    const size_t row0 = (size_t)blockIdx.x * 64 + (size_t)w * 16;
    double4_t acc[CT];
    music_dft_rows<CT>(xf + (row0 + c) * (size_t)d.Np + 8 * q, W, d.Np, d.Cp, col0, ncol, Ws, acc);
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        if (16 * t >= ncol) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lr = w * 16 + q + 4 * r;  // f64 C/D map: row (lane >> 4) + 4 r, column lane & 15
            if (done[lr]) X[((size_t)blockIdx.x * 64 + lr) * d.Cp + col0 + 16 * t + c] = acc[t][r];
        }
    }
}

// dynamic LDS: pw [nbin] doubles, then sel [ksel] ints
__global__ __launch_bounds__(256) void music_stream_slice_kernel(const double *__restrict__ X, MusicStreamDims d, int n, int final_tile,
                                                                 const int *__restrict__ clk, const double *__restrict__ sre,
                                                                 const double *__restrict__ sim, double *__restrict__ slot_spec,
                                                                 double *__restrict__ slice_spec, int32_t *__restrict__ slice_sel,
                                                                 int32_t *__restrict__ slice_argmax, double *__restrict__ latest_spec,
                                                                 int32_t *__restrict__ latest_argmax)
{
    extern __shared__ double pw[];
    __shared__ double bv[256];
    __shared__ int bi[256];
    int32_t *sel = reinterpret_cast<int32_t *>(pw + d.nbin);
    const int bk = blockIdx.x;
    const int slot = bk % d.slots, b = bk / d.slots;
    const long long t0 = clk[4 * b], t1 = t0 + n;
    long long lo_s = -1, s, j;
    int lo_F = 0, F;
    if (final_tile) ms_leftover(d, t1, &lo_s, &lo_F);
    const bool leftover = lo_s >= 0 && lo_F > 0;
    bool newest = true;
    if (ms_event((long long)slot * d.hop + d.L - 1, d.slots * d.hop, t0, t1, &j)) {
        s = slot + j * d.slots;
        F = d.F;
        newest = !leftover;
    } else if (leftover && lo_s % d.slots == slot) {
        s = lo_s;
        F = lo_F;
    } else {
        return;  // (the whole workgroup)
    }
    for (int i = threadIdx.x; i < d.nbin; i += 256) pw[i] = music_bin_power(X, (size_t)bk, d.M, d.F, F, d.Cp, i);
    __syncthreads();
    for (int i = threadIdx.x; i < d.nbin; i += 256) {
        const int pos = music_bin_rank(pw, d.nbin, i) - (d.nbin - d.ksel);
        if (pos >= 0) sel[pos] = i;
    }
    __syncthreads();
    const size_t row = (size_t)b * d.max_slices + (size_t)(s % d.max_slices);
    if (slice_sel)
        for (int i = threadIdx.x; i < d.ksel; i += 256) slice_sel[row * d.ksel + i] = sel[i];
    double best = 0.0;
    int besti = -1;
    for (int g = threadIdx.x; g < d.G; g += 256) {
        const double P = music_steer_sum(X, (size_t)bk, d.M, d.F, F, d.Cp, sel, d.ksel, sre, sim, d.G, g);
        slot_spec[(size_t)bk * d.G + g] = P;
        if (slice_spec) slice_spec[row * d.G + g] = P;
        if (newest && latest_spec) latest_spec[(size_t)b * d.G + g] = P;
        music_first_max(P, g, best, besti);
    }
    const int first = music_first_argmax(best, besti, bv, bi);
    if (threadIdx.x == 0) {
        if (slice_argmax) slice_argmax[row] = first;
        if (newest && latest_argmax) latest_argmax[b] = first;
    }
}

__global__ __launch_bounds__(256) void music_stream_readout_kernel(MusicStreamDims d, int n, int final_tile, int *__restrict__ clk,
                                                                   const double *__restrict__ slot_spec, double *__restrict__ sum,
                                                                   double *__restrict__ power, int32_t *__restrict__ argmax)
{
    __shared__ double bv[256];
    __shared__ int bi[256];
    const int b = blockIdx.x;
    const long long t0 = clk[4 * b], t1 = t0 + n;
    const long long count0 = clk[4 * b + 1];  // every full slice that ended before this piece has been emitted
    int flag = clk[4 * b + 2];
    const long long full = t1 >= d.L ? (t1 - d.L) / d.hop + 1 : 0;
    long long lo_s = -1;
    int lo_F = 0;
    if (final_tile) ms_leftover(d, t1, &lo_s, &lo_F);
    const bool leftover = lo_s >= 0 && lo_F > 0;
    if (lo_s >= 0 && lo_F == 0) flag = 1;  // a leftover slice shorter than N: not emitted (the one-shot call refuses the recording)
    const long long count = full + (leftover ? 1 : 0);
    double best = 0.0;
    int besti = -1;
    for (int g = threadIdx.x; g < d.G; g += 256) {
        double p = sum[(size_t)b * d.G + g];
        for (long long s = count0; s < count; ++s) p = music_power_add(p, slot_spec[((size_t)b * d.slots + (size_t)(s % d.slots)) * d.G + g]);
        sum[(size_t)b * d.G + g] = p;
        if (count > 0) {
            p = p / (double)count;
            if (power) power[(size_t)b * d.G + g] = p;
            music_first_max(p, g, best, besti);
        }
    }
    const int first = music_first_argmax(best, besti, bv, bi);  // (its barriers: every thread has read the clock by now)
    if (threadIdx.x == 0) {
        if (count > 0 && argmax) argmax[b] = first;
        const long long begun = t1 > 0 ? (t1 - 1) / d.hop + 1 : 0;
        clk[4 * b] = (int)t1;
        clk[4 * b + 1] = (int)count;
        clk[4 * b + 2] = flag;
        clk[4 * b + 3] = final_tile ? 0 : (int)(begun - full);
    }
}

}  // namespace

bool music_stream_dims(int B, int M, int L, int hop, int N, int nbin, int G, int k, int max_slices, MusicStreamDims *d)
{
    if (B < 1 || B > 65535 || M < 1 || L < 1 || L > (1 << 28) || hop < 1 || hop > L || N < 2 || N > L || nbin < 1 || nbin > N || nbin > 4096 ||
        G < 1 || k < 0 || k > nbin || max_slices < 1)
        return false;
    d->B = B, d->M = M, d->L = L, d->hop = hop, d->N = N;
    d->Np = (N + 63) / 64 * 64;
    d->F = L / N;
    d->nbin = nbin;
    d->Cp = (2 * nbin + 15) / 16 * 16;
    d->G = G;
    d->ksel = k == 0 ? nbin : k;
    d->slots = (L + hop - 1) / hop + 1;
    d->max_slices = max_slices;
    return (long long)B * d->slots <= 0x7fffffffll / ((long long)M * d->F);
}

MusicStreamLayout music_stream_layout(const MusicStreamDims &d)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    MusicStreamLayout S{};
    const size_t nl = (size_t)d.B * d.slots * d.M;
    S.R = (long long)nl * d.F;
    S.Rp = (S.R + 63) / 64 * 64;
    size_t off = 0;
    S.clk = off;
    off += al((size_t)d.B * 4 * sizeof(int));
    S.z = off;
    off += al((size_t)(MICLOC_MAX_IIR - 1) * nl * sizeof(double));
    S.sum = off;
    off += al((size_t)d.B * d.G * sizeof(double));
    S.spec = off;
    off += al((size_t)d.B * d.slots * d.G * sizeof(double));
    S.xf = off;
    off += al((size_t)S.Rp * d.Np * sizeof(double));
    S.X = off;
    off += al((size_t)S.Rp * d.Cp * sizeof(double));
    S.total = off;
    return S;
}

hipError_t launch_music_stream_tile(const MusicStreamDims &d, const IirCoef &co, const double *x, int n, int final_tile, void *state,
                                    const double *W, const double *sre, const double *sim, double *power, int32_t *argmax,
                                    double *latest_spec, int32_t *latest_argmax, double *slice_spec, int32_t *slice_sel, int32_t *slice_argmax,
                                    hipStream_t st)
{
    const MusicStreamLayout S = music_stream_layout(d);
    unsigned char *base = reinterpret_cast<unsigned char *>(state);
    int *clk = reinterpret_cast<int *>(base + S.clk);
    double *zst = reinterpret_cast<double *>(base + S.z), *sum = reinterpret_cast<double *>(base + S.sum);
    double *slot_spec = reinterpret_cast<double *>(base + S.spec), *xf = reinterpret_cast<double *>(base + S.xf);
    double *X = reinterpret_cast<double *>(base + S.X);
    const long long nl = (long long)d.B * d.slots * d.M;
    const size_t lds = (size_t)d.nbin * sizeof(double) + (size_t)d.ksel * sizeof(int32_t);
    for (int i0 = 0; i0 < n; i0 += d.hop) {  // pieces of at most hop samples: the cut depends on n only
        const int np = n - i0 < d.hop ? n - i0 : d.hop;
        const int fin = final_tile && i0 + np == n;
        const double *xp = x + (size_t)i0 * d.M;
        hipError_t e = music_dispatch_order(co.n, [&](auto NC) {
            hipLaunchKernelGGL(music_stream_filter_tile_kernel<decltype(NC)::value>, dim3((unsigned)((nl + MS_LANES - 1) / MS_LANES)), dim3(MS_LANES), 0,
                               st, xp, (size_t)n * d.M, np, d, co, clk, zst, xf);
            return hipGetLastError();
        });
        if (e != hipSuccess) return e;
        e = music_dispatch_tiles(d.Cp, [&](auto CT) {
            constexpr int WC = 16 * decltype(CT)::value;
            hipLaunchKernelGGL(music_stream_dft_kernel<decltype(CT)::value>, dim3((unsigned)(S.Rp / 64), (unsigned)((d.Cp + WC - 1) / WC)), dim3(256), 0,
                               st, xf, W, X, d, np, clk, S.R);
            return hipGetLastError();
        });
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(music_stream_slice_kernel, dim3((unsigned)(d.B * d.slots)), dim3(256), lds, st, X, d, np, fin, clk, sre, sim, slot_spec,
                           slice_spec, slice_sel, slice_argmax, latest_spec, latest_argmax);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(music_stream_readout_kernel, dim3((unsigned)d.B), dim3(256), 0, st, d, np, fin, clk, slot_spec, sum, power, argmax);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace micloc
