// Streaming form of the time-resolved read-out: power and arg-max per window WHILE the recording arrives
// (micloc_stream_localize_tile_windows_f64).  The rule -- window bounds, when a window is emitted, its value -- is stated in
// full in include/micloc_hip.h ("streaming windows"); utils.windows_complete restates the emission count for Python.
//
// The kernel runs between the accumulate and the commit of a tile.  It sees what stream_accumulate_kernel (beamform.hip) sees:
// partial [B][nwin][Gp], the rows of sum_t y^2 of the chunks that became final in this call at the window-relative rows
// [lo, hi) (ctl[4], ctl[5]); ctl[0] = chunks done before this call (absolute), ctl[6] = chunks done after it.  Which windows the call
// opens, feeds and emits -- also at the end of the recording -- is StreamWindowWalk of readout_rows.h, shared with the Xylo stream's
// window kernel; at most K = ceil(window / hop) windows have started and are not complete.  Window n keeps {total, open-block sum} (two
// rows of G doubles) in slot n % K of state [B][K][2][G]; the fill of its open block is (chunks of the window so far) %
// STREAM_BLOCK_CHUNKS and needs no word of its own.  Every open window takes the new rows it covers in ascending order (BlockedSum) --
// the additions of window_power_kernel<1> (windows.hip) on the whole recording, to the bit, in O(K G) memory per trial.  A window that
// is emitted is divided by its frame count, written to row n % max_windows of the outputs and, if it is the newest of this call, to
// latest_*; its arg-max is block_first_max.
//
// One workgroup per trial, the windows of a call in a loop inside the kernel: the grid depends on B only, no launch argument
// on time, so the launch is part of the tile's graph.  No atomics, no host synchronisation.
//
// The complex Beamformer's stream (stream_complex.hip) emits its windows through the same kernel: its rows are folded, columns
// [0, Ghp) Re and [Ghp, Gp) Im, and its control words carry the same meaning.  PAIRS = 1 adds both halves per chunk, s += Re; s += Im,
// the additions of window_power_kernel with complex_pairs = 1 (windows.hip); PAIRS = 0 is the real read-out, which never reads Ghp.
#include "readout_rows.h"

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
    const StreamWindowWalk walk(ctl, final_tile, CH, wchunks, hchunks, nwin);
    if (!walk.ok) return;
    const double *pb = partial + (size_t)b * nwin * Gp;
    for (int n = walk.n0; n <= walk.n_started; ++n) {
        const StreamWindowWalk::Window w = walk.window(n);
        double *tot = state + (((size_t)b * K + n % K) * 2) * G, *blk = tot + G;
        const size_t row = (size_t)b * max_windows + n % max_windows;
        double best = -1.0;
        int bi = RO_NONE;
        for (int g = col; g < G; g += SW_COLS) {
            BlockedSum sum{0.0, 0.0, (w.ca - w.c0) % STREAM_BLOCK_CHUNKS};
            if (w.ca > w.c0) {  // the window opened in an earlier call
                sum.total = tot[g];
                sum.s = blk[g];
            }
            for (int ch = w.ca; ch < w.cb; ++ch) {
                const double *r = pb + (size_t)walk.row(ch) * Gp + g;
                if (PAIRS)
                    sum.add(r[0], r[Ghp]);
                else
                    sum.add(r[0]);
            }
            if (!w.emit) {
                tot[g] = sum.total;
                blk[g] = sum.s;
                continue;
            }
            const double p = sum.close() / (double)w.frames;
            if (power_w) power_w[row * G + g] = p;
            if (w.newest && latest_power) latest_power[(size_t)b * G + g] = p;
            if (p > best) {
                best = p;
                bi = g;
            }
            tot[g] = 0.0;
            blk[g] = 0.0;
        }
        if (!w.emit) continue;  // (uniform over the workgroup)
        const int32_t a = block_first_max<SW_COLS, double, true>(best, bi, sv, si, col);  // (trailing barrier: the next window rewrites sv / si)
        if (col == 0) {
            if (argmax_w) argmax_w[row] = a;
            if (w.newest && latest_argmax) latest_argmax[b] = a;
        }
    }
    if (b == 0 && col == 0) head[0] = walk.head();
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
