// Streaming form of the time-resolved read-out: power and arg-max per window WHILE the recording arrives
// (micloc_stream_localize_tile_windows_f64).  The rule -- window bounds, when a window is emitted, its value -- is stated in
// full in include/micloc_hip.h ("streaming windows"); utils.windows_complete restates the emission count for Python.
//
// The kernel runs between the accumulate and the commit of a tile.  It sees what stream_accumulate_kernel (beamform.hip) sees:
// partial [B][nwin][Gp], the rows of sum_t y^2 of the chunks that became final in this call at the window-relative rows
// [lo, hi) (ctl[4], ctl[5]); ctl[0] = chunks done before this call (absolute), ctl[6] = chunks done after it.  A window is
// hop / CH chunks apart from the next and window / CH chunks long, so with `done` chunks beamformed
//     emitted(done) = done < wchunks ? 0 : (done - wchunks) / hchunks + 1
// windows are complete, and the windows that have started but are not complete are n = emitted(done) .. (done - 1) / hchunks:
// at most K = ceil(window / hop) of them.  Window n keeps {total, open-block sum} (two rows of G doubles) in slot n % K of
// state [B][K][2][G]; the fill of its open block is (chunks of the window so far) % STREAM_BLOCK_CHUNKS and needs no word of
// its own.  Every open window takes the new rows it covers in ascending order -- the additions of window_power_kernel<1>
// (windows.hip) on the whole recording, to the bit, in O(K G) memory per trial.  A window whose last chunk arrived is divided by
// its frame count, written to row n % max_windows of the outputs and, if it is the newest of this call, to latest_*.  On
// the final tile (ctl[6] chunks cover STREAM_CLK_TEND = T frames) every window of window_count(T, window, hop) not emitted yet
// is emitted over the frames it has; windows past that count started but do not exist in the rule and are dropped.
//
// One workgroup per trial, the windows of a call in a loop inside the kernel: the grid depends on B only, no launch argument
// on time, so the launch is part of the tile's graph.  No atomics, no host synchronisation.
//
// The complex Beamformer's stream (stream_complex.hip) emits its windows through the same kernel: its rows are folded, columns
// [0, Ghp) Re and [Ghp, Gp) Im, and its control words carry the same meaning.  PAIRS = 1 adds both halves per chunk, s += Re; s += Im,
// the additions of window_power_kernel with complex_pairs = 1 (windows.hip); PAIRS = 0 is the real read-out, which never reads Ghp.
#include "micloc_internal.h"

namespace micloc {

namespace {

constexpr int SW_COLS = 256;

template <int PAIRS>
__global__ __launch_bounds__(SW_COLS) void stream_window_kernel(const double *__restrict__ partial, int nwin, int Gp, int G, int CH,
                                                                 const int *__restrict__ ctl, int final_tile, int wchunks, int hchunks,
                                                                 int K, int max_windows, double *__restrict__ state,
                                                                 int *__restrict__ head, double *__restrict__ power_w,
                                                                 int32_t *__restrict__ argmax_w, double *__restrict__ latest_power,
                                                                 int32_t *__restrict__ latest_argmax, int Ghp)
{
    __shared__ double sv[SW_COLS];
    __shared__ int si[SW_COLS];
    const int b = blockIdx.x;
    const int col = threadIdx.x;
    const int done = ctl[0], lo = ctl[4], hi = ctl[5], ready = ctl[6];
    const int T = ctl[STREAM_CLK_TEND];
    // the recording is complete once the final tile's chunks cover its T frames (a lag failure leaves them short: no read-out)
    const bool ended = final_tile && (long long)ready * CH >= T;
    if (ready - done != hi - lo || hi < lo || lo < 0 || hi > nwin) return;  // (never: the kernel in front writes both)
    const int n0 = done < wchunks ? 0 : (done - wchunks) / hchunks + 1;      // first window not emitted before this call
    const int n_started = ready > 0 ? (ready - 1) / hchunks : -1;            // last window that holds a chunk
    long long n_emit;                                                        // windows emitted after this call
    if (ended)
        n_emit = T <= (long long)wchunks * CH ? 1 : 1 + ((long long)T - (long long)wchunks * CH + (long long)hchunks * CH - 1) / ((long long)hchunks * CH);
    else
        n_emit = ready < wchunks ? 0 : (ready - wchunks) / hchunks + 1;
    const double *pb = partial + (size_t)b * nwin * Gp;
    for (int n = n0; n <= n_started; ++n) {
        const int c0 = n * hchunks;  // (n <= (ready - 1) / hchunks: no overflow)
        const int ca = done > c0 ? done : c0;
        const int cb = ready - c0 < wchunks ? ready : c0 + wchunks;
        const bool emit = n < n_emit;  // complete, or cut at the end of the recording
        double *tot = state + (((size_t)b * K + n % K) * 2) * G, *blk = tot + G;
        long long frames = (long long)T - (long long)c0 * CH;
        if (!ended || frames > (long long)wchunks * CH) frames = (long long)wchunks * CH;
        const size_t row = (size_t)b * max_windows + n % max_windows;
        const bool newest = n == n_emit - 1;
        double best = -1.0;
        int bi = 0x7fffffff;
        for (int g = col; g < G; g += SW_COLS) {
            double total = 0.0, s = 0.0;
            if (ca > c0) {  // the window opened in an earlier call
                total = tot[g];
                s = blk[g];
            }
            int open = (ca - c0) % STREAM_BLOCK_CHUNKS;
            for (int ch = ca; ch < cb; ++ch) {
                s += pb[(size_t)(lo + ch - done) * Gp + g];
                if (PAIRS) s += pb[(size_t)(lo + ch - done) * Gp + Ghp + g];
                if (++open == STREAM_BLOCK_CHUNKS) {
                    total += s;
                    s = 0.0;
                    open = 0;
                }
            }
            if (!emit) {
                tot[g] = total;
                blk[g] = s;
                continue;
            }
            if (open > 0) total += s;  // the last block of the window, if it holds any chunk
            const double p = total / (double)frames;
            if (power_w) power_w[row * G + g] = p;
            if (newest && latest_power) latest_power[(size_t)b * G + g] = p;
            if (p > best) {
                best = p;
                bi = g;
            }
            tot[g] = 0.0;
            blk[g] = 0.0;
        }
        if (!emit) continue;  // (uniform over the workgroup)
        sv[col] = best;
        si[col] = bi;
        __syncthreads();
        for (int s = SW_COLS / 2; s > 0; s >>= 1) {
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
        if (col == 0) {
            const int32_t a = si[0] == 0x7fffffff ? 0 : si[0];
            if (argmax_w) argmax_w[row] = a;
            if (newest && latest_argmax) latest_argmax[b] = a;
        }
        __syncthreads();  // sv / si are rewritten by the next window
    }
    if (b == 0 && col == 0) head[0] = (int)(n_emit > 0x7fffffffll ? 0x7fffffffll : n_emit);
}

}  // namespace

int stream_window_slots(int window, int hop) { return (window + hop - 1) / hop; }

size_t stream_window_state_bytes(int B, int G, int window, int hop)
{
    return 256 + (((size_t)B * stream_window_slots(window, hop) * 2 * G * sizeof(double) + 255) & ~(size_t)255);
}

hipError_t launch_stream_windows(const double *partial, int B, int nwin, int Gp, int G, int complex_pairs, int Ghp, int chunk_frames,
                                 const int *ctl, int final_tile, int window, int hop, int max_windows, void *win_state, double *power_w,
                                 int32_t *argmax_w, double *latest_power, int32_t *latest_argmax, hipStream_t stream)
{
    if (chunk_frames < 1 || window < 1 || hop < 1 || hop > window || window % chunk_frames != 0 || hop % chunk_frames != 0 || max_windows < 1)
        return hipErrorInvalidValue;
    int *head = reinterpret_cast<int *>(win_state);
    double *state = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(win_state) + 256);
    hipLaunchKernelGGL(complex_pairs ? stream_window_kernel<1> : stream_window_kernel<0>, dim3(B), dim3(SW_COLS), 0, stream, partial, nwin, Gp, G,
                       chunk_frames, ctl, final_tile ? 1 : 0, window / chunk_frames, hop / chunk_frames, stream_window_slots(window, hop),
                       max_windows, state, head, power_w, argmax_w, latest_power, latest_argmax, Ghp);
    return hipGetLastError();
}

}  // namespace micloc
