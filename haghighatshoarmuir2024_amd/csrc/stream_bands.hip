// The band sum of a wideband STREAM (micloc_stream_band_sum_f64): after the F band chains of a tile have run -- each one
// StreamingLocalizer's launch sequence on its slice of filterbank_tile_kernel's output (filterbank.hip) -- ONE launch adds the bands.
// The rule is stated in full in include/micloc_hip.h ("wideband streaming").
//
// stream_band_sum_kernel, one workgroup per trial (the grid depends on B only, no argument on time: part of the tile's graph):
//   * running read-out: power[b][g] = ((p_0 + p_1) + p_2) + ... over the bands' running power [B][G], __dadd_rn in ascending band order
//     from p_0, arg-max by band_sum_kernel's scan and block_first_max of readout_rows.h (a NaN never wins, a row of NaN gives 0);
//   * windows: band f keeps its windows in a ring [B][Kb][G], window n in row n % Kb, and counts them in a device word.  With
//     `emitted` wideband windows so far, window n is emitted -- the ascending band sum of the bands' rows, into row n % max_windows of
//     the outputs -- for n = emitted .. min_f count_f - 1.  A band that leads by more than Kb windows has overwritten the rows of
//     the windows n < count_f - Kb: those are given up (counted as failures, nothing written), never summed from a row that holds a
//     later window (ready_windows of readout_rows.h, shared with the Xylo stream's read-out).
// The F running-power pointers, ring pointers and count pointers travel by value in the kernel argument: no device table.
// State block: int words {0: windows emitted or given up, 1: windows given up, 2 / 3: what this launch adds to them}.  Every workgroup
// reads word 0; workgroup 0 writes words 2 / 3 only, and stream_bands_commit_kernel (one thread, the next launch on the stream) folds
// them into words 0 / 1 -- the read is ordered against the write by the launch boundary, as stream_window_kernel's count is against
// the commit of its tile.  No atomics, no host synchronisation.
#include "readout_rows.h"

namespace micloc {

namespace {

constexpr int SB_COLS = 256;

__global__ __launch_bounds__(SB_COLS) void stream_band_sum_kernel(const StreamBandsArgs args, int F, int G, int windowed, int Kb, int max_windows,
                                                                   int *__restrict__ state, double *__restrict__ power,
                                                                   int32_t *__restrict__ argmax, double *__restrict__ power_w,
                                                                   int32_t *__restrict__ argmax_w, double *__restrict__ latest_power,
                                                                   int32_t *__restrict__ latest_argmax)
{
    __shared__ double sv[SB_COLS];
    __shared__ int si[SB_COLS];
    const size_t b = blockIdx.x;
    const int col = threadIdx.x;
    {  // the running read-out
        double best = 0.0;
        int bi = RO_NONE;
        for (int g = col; g < G; g += SB_COLS) {
            double s = args.power[0][b * G + g];
            for (int f = 1; f < F; ++f) s = __dadd_rn(s, args.power[f][b * G + g]);
            if (power) power[b * G + g] = s;
            if (s == s && (bi == RO_NONE || s > best)) {  // ascending g per thread: the first maximum; a NaN never wins
                best = s;
                bi = g;
            }
        }
        const int a = block_first_max<SB_COLS, double, true>(best, bi, sv, si, col);  // (trailing barrier: the next row rewrites sv / si)
        if (col == 0 && argmax) argmax[b] = a;
    }
    if (!windowed) return;
    const int emitted = state[0];
    // windows below rw.lo have left the ring of the band that leads: given up
    const ReadyWindows rw = ready_windows(F, emitted, Kb, [&](int f) { return args.count[f][0]; });
    for (int n = rw.lo; n < rw.hi; ++n) {  // (uniform over the workgroup)
        const size_t in_row = (b * Kb + n % Kb) * (size_t)G;
        const size_t out_row = b * max_windows + n % max_windows;
        const bool newest = n == rw.hi - 1;
        double best = 0.0;
        int bi = RO_NONE;
        for (int g = col; g < G; g += SB_COLS) {
            double s = args.rows[0][in_row + g];
            for (int f = 1; f < F; ++f) s = __dadd_rn(s, args.rows[f][in_row + g]);
            if (power_w) power_w[out_row * G + g] = s;
            if (newest && latest_power) latest_power[b * G + g] = s;
            if (s == s && (bi == RO_NONE || s > best)) {
                best = s;
                bi = g;
            }
        }
        const int a = block_first_max<SB_COLS, double, true>(best, bi, sv, si, col);  // (trailing barrier: the next row rewrites sv / si)
        if (col == 0) {
            if (argmax_w) argmax_w[out_row] = a;
            if (newest && latest_argmax) latest_argmax[b] = a;
        }
    }
    if (b == 0 && col == 0) {
        const int next = rw.lo > rw.hi ? rw.lo : rw.hi;  // never below `emitted`: lo >= emitted
        state[2] = next - emitted;
        state[3] = rw.given(next);
    }
}

__global__ void stream_bands_commit_kernel(int *__restrict__ state)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state[0] += state[2];
        state[1] += state[3];
        state[2] = 0;
        state[3] = 0;
    }
}

}  // namespace

hipError_t launch_stream_band_sum(const StreamBandsArgs &args, int F, int B, int G, int windowed, int Kb, int max_windows, void *state,
                                  double *power, int32_t *argmax, double *power_w, int32_t *argmax_w, double *latest_power,
                                  int32_t *latest_argmax, hipStream_t stream)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || B < 1 || G < 1 || !state || (windowed && (Kb < 1 || max_windows < 1))) return hipErrorInvalidValue;
    int *st = reinterpret_cast<int *>(state);
    hipLaunchKernelGGL(stream_band_sum_kernel, dim3((unsigned)B), dim3(SB_COLS), 0, stream, args, F, G, windowed ? 1 : 0, Kb, max_windows, st, power,
                       argmax, power_w, argmax_w, latest_power, latest_argmax);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !windowed) return e;
    hipLaunchKernelGGL(stream_bands_commit_kernel, dim3(1), dim3(64), 0, stream, st);
    return hipGetLastError();
}

}  // namespace micloc
