// Time-resolved read-out of the beamforming partial sums: power and arg-max per window (micloc_*_windows_f64).
// The window rule is stated in full in include/micloc_hip.h; utils.window_bounds restates it for Python.
//
// Input is the buffer the beamforming kernels already write for the one-shot reduction: partial [B][nchunks][Gp], one row of
// sum_t y^2 per time chunk of CH frames (the ragged last chunk holds the frames that exist).  Windows start and end on chunk
// boundaries (window and hop are multiples of CH), so window n of a trial is the rows [n hop / CH, n hop / CH + window / CH)
// cut at nchunks.  One workgroup per (window, trial): grid (nW, B), so the launch scales with B nW; overlapping windows re-read
// their rows (window / hop times the buffer, from L2 / MALL for the shapes of the sweeps).
//
// The order of the additions is the one-shot reduction's (power_argmax_kernel, beamform.hip) re-based at the window's first
// chunk: chunk sums ascending inside blocks of STREAM_BLOCK_CHUNKS chunks counted from that chunk, block sums ascending onto
// the total.  A single window with window >= T therefore returns the bits of the unwindowed power and arg-max.  Long windows
// (>= 128 chunks) sum four blocks side by side like the one-shot kernel does -- the same additions, four of them in flight.
// The arg-max is the first maximum of readout_rows.h (block_first_max); window_count is its window_count64.
// No atomics, no host synchronisation, no state: safe on any stream and graph-capturable.
#include "readout_rows.h"

namespace micloc {

namespace {

constexpr int WN_BLOCK = STREAM_BLOCK_CHUNKS;
constexpr int WN_COLS = 256;  // DoA columns per pass

template <int S>
__global__ __launch_bounds__(WN_COLS * S) void window_power_kernel(const double *__restrict__ partial, int nchunks, int Gp, int G,
                                                                    int complex_pairs, int Ghp, int CH, int T, int wchunks, int hchunks,
                                                                    int nW, double *__restrict__ power_w, int32_t *__restrict__ argmax_w)
{
    constexpr int U = S > 1 ? 4 : 1;  // blocks per slice and round
    __shared__ double sv[WN_COLS];
    __shared__ int si[WN_COLS];
    __shared__ double ps[U][S][WN_COLS];
    const int n = blockIdx.x, b = blockIdx.y;
    const int col = threadIdx.x & (WN_COLS - 1);
    const int slice = threadIdx.x / WN_COLS;
    // chunks [c0, c1) and frames [c0 CH, min(c0 CH + window, T)) of this window; 64-bit: n * hchunks * CH may pass 2^31
    const long long c0l = (long long)n * hchunks;
    const int c0 = c0l < nchunks ? (int)c0l : nchunks;
    const int nc = nchunks - c0 < wchunks ? nchunks - c0 : wchunks;  // chunks of the window (0: it starts past the recording)
    long long frames = (long long)T - c0l * CH;
    if (frames > (long long)wchunks * CH) frames = (long long)wchunks * CH;
    const double *pb = partial + ((size_t)b * nchunks + c0) * Gp;
    const int nblocks = (nc + WN_BLOCK - 1) / WN_BLOCK;
    const size_t row = (size_t)b * nW + n;
    double best = -1.0;
    int bi = RO_NONE;
    for (int g0 = 0; g0 < G; g0 += WN_COLS) {
        const int g = g0 + col;
        double total = 0.0;
        for (int blk0 = 0; blk0 < nblocks; blk0 += S * U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int blk = blk0 + S * u + slice;
                double s = 0.0;
                if (g < G && blk < nblocks) {
                    const int c_hi = (blk + 1) * WN_BLOCK < nc ? (blk + 1) * WN_BLOCK : nc;
                    for (int ch = blk * WN_BLOCK; ch < c_hi; ++ch) {
                        s += pb[(size_t)ch * Gp + g];
                        if (complex_pairs) s += pb[(size_t)ch * Gp + Ghp + g];
                    }
                }
                if (S > 1)
                    ps[u][slice][col] = s;
                else
                    total += s;
            }
            if (S > 1) {
                __syncthreads();
                if (slice == 0) {
                    // the block sums onto the total in ascending block order: blk0 + S u + v
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int v = 0; v < S; ++v)
                            if (blk0 + S * u + v < nblocks) total += ps[u][v][col];
                }
                __syncthreads();
            }
        }
        if (slice == 0 && g < G) {
            // (a window without a frame -- possible only with hop > window -- has no mean: NaN, which never wins the arg-max)
            const double p = frames > 0 ? total / (double)frames : __builtin_nan("");
            if (power_w) power_w[row * G + g] = p;
            if (p > best) {
                best = p;
                bi = g;
            }
        }
    }
    if (!argmax_w) return;  // (uniform over the workgroup)
    // (S = 4: slice 0 holds the pairs; every thread passes the barriers)
    const int a = block_first_max<WN_COLS>(best, bi, sv, si, col, slice == 0);
    if (threadIdx.x == 0) argmax_w[row] = a;
}

}  // namespace

long long window_count(int T, int window, int hop) { return window_count64(T, window, hop); }

hipError_t launch_window_power(const double *partial, int B, int T, int nchunks, int Gp, int G, int complex_pairs, int Ghalf_pad,
                               int chunk_frames, int window, int hop, double *power_w, int32_t *argmax_w, hipStream_t stream)
{
    const long long nW = window_count(T, window, hop);
    if (chunk_frames < 1 || window % chunk_frames != 0 || hop % chunk_frames != 0 || hop < 1 || window < 1 || nW > 0x7fffffffll || B > 65535)
        return hipErrorInvalidValue;
    const int wchunks = window / chunk_frames, hchunks = hop / chunk_frames;
    const dim3 grid((unsigned)nW, B);
    if ((wchunks < nchunks ? wchunks : nchunks) >= 128)
        hipLaunchKernelGGL(window_power_kernel<4>, grid, dim3(WN_COLS * 4), 0, stream, partial, nchunks, Gp, G, complex_pairs, Ghalf_pad,
                           chunk_frames, T, wchunks, hchunks, (int)nW, power_w, argmax_w);
    else
        hipLaunchKernelGGL(window_power_kernel<1>, grid, dim3(WN_COLS), 0, stream, partial, nchunks, Gp, G, complex_pairs, Ghalf_pad,
                           chunk_frames, T, wchunks, hchunks, (int)nW, power_w, argmax_w);
    return hipGetLastError();
}

}  // namespace micloc
