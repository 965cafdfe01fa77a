// Streaming multi-source read-out (micloc_stream_peaks_tile_f64): the K strongest peaks of a stream's running power row and of every window
// the stream has emitted since this read-out last ran, behind a tile's own read-out and inside the tile's graph.  The rule is stated in
// full in include/micloc_hip.h ("streaming, multi-source"); the row rule is peaks_rows.h's.
//
// The stream's window read-out has left c windows counted in a device word (window n in row n % max_windows of window_power); this
// read-out keeps r, "windows whose peaks are read", in a state of its own.  stream_peaks_kernel, grid (B, STREAM_PEAKS_SLOTS), one wave per
// workgroup: workgroup (b, s) walks the windows n = n_lo + s, n_lo + s + SLOTS, ... < c with n_lo = max(r, c - max_windows), applies the
// rule to row n % max_windows of trial b's ring and writes row n % max_windows of the peak rings; the workgroup that meets window c - 1
// writes latest_* as well.  The running row of trial b rides on the last slot, which has a window of its own only when a tile emits at
// least SLOTS of them.  Nothing in the launch depends on the tile or on time: c and r are read from the device, so any number of new
// windows -- 0, 1, more than SLOTS, more than max_windows -- is one and the same launch.
//
// Hazards.  No atomics, no host synchronisation.  Within the launch every workgroup READS c, r, its rows of power / window_power and
// doa, and WRITES rows of the peak arrays that no other workgroup touches: the windows of [n_lo, c) are at most max_windows consecutive
// numbers, so they sit in distinct ring rows, and each (b, n) belongs to one workgroup.  r and the skipped count are written by
// stream_peaks_commit_kernel, a launch of its own (one thread) behind the read-out: no workgroup reads a word another workgroup of the same
// launch writes.  The count word is written by the stream's own launches in front of this one.
#include "peaks_rows.h"
#include "stream_peaks.h"

namespace micloc {

namespace {

// the windows a launch reads: [lo, c)
__device__ __forceinline__ void stream_peaks_span(const int32_t *__restrict__ count, const int *__restrict__ st, int max_windows, int *lo, int *c)
{
    int cc = *count, r = st[0];
    if (cc < 0) cc = 0;
    if (r < 0) r = 0;
    const int first = cc - max_windows;  // (cc >= 0, max_windows >= 1: no overflow)
    *lo = r > first ? r : first;
    *c = cc;
}

}  // namespace

__global__ __launch_bounds__(PKR_WAVE) void stream_peaks_kernel(const double *__restrict__ power, const double *__restrict__ window_power,
                                                                const int32_t *__restrict__ count, const int *__restrict__ st, int G, int max_windows,
                                                                const double *__restrict__ doa, int kind, int K, double min_sep, double rel,
                                                                int32_t *__restrict__ peaks, double *__restrict__ peak_power,
                                                                int32_t *__restrict__ window_peaks, double *__restrict__ window_peak_power,
                                                                int32_t *__restrict__ latest_peaks, double *__restrict__ latest_peak_power)
{
    extern __shared__ double spk_lds[];
    const int b = blockIdx.x;
    const int slot = blockIdx.y;

    if (window_power) {
        int lo, c;
        stream_peaks_span(count, st, max_windows, &lo, &c);
        // n < c <= INT_MAX; lo + slot may pass INT_MAX only when it is >= c as well: walk in 64 bits
        for (long long n = (long long)lo + slot; n < c; n += STREAM_PEAKS_SLOTS) {
            const size_t row = (size_t)b * max_windows + (size_t)(n % max_windows);
            const bool newest = n == (long long)c - 1;
            peaks_row(window_power + row * G, G, doa, kind, K, min_sep, rel, window_peaks + row * K,
                      window_peak_power ? window_peak_power + row * K : nullptr, newest && latest_peaks ? latest_peaks + (size_t)b * K : nullptr,
                      newest && latest_peak_power ? latest_peak_power + (size_t)b * K : nullptr, spk_lds);
        }
    }
    if (power && slot == STREAM_PEAKS_SLOTS - 1)
        peaks_row(power + (size_t)b * G, G, doa, kind, K, min_sep, rel, peaks + (size_t)b * K, peak_power ? peak_power + (size_t)b * K : nullptr,
                  nullptr, nullptr, spk_lds);
}

// behind the read-out: r = c, skipped += the windows whose rows were overwritten before they were read
__global__ __launch_bounds__(64) void stream_peaks_commit_kernel(const int32_t *__restrict__ count, int *__restrict__ st, int max_windows)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int c = *count, r = st[0];
    if (c < 0) c = 0;
    if (r < 0) r = 0;
    const int lost = c - max_windows - r;
    if (lost > 0) st[1] += lost;
    st[0] = c;
}

hipError_t launch_stream_peaks(const double *power, const double *window_power, const int32_t *window_count, int B, int G, int max_windows,
                               const double *doa, int kind, int K, double min_sep, double rel, void *pk_state, int32_t *peaks, double *peak_power,
                               int32_t *window_peaks, double *window_peak_power, int32_t *latest_peaks, double *latest_peak_power,
                               hipStream_t stream)
{
    // G <= 4096 (checked by the API): at most 48 KiB, within the default dynamic-LDS limit (as launch_doa_peaks)
    const size_t dyn = peaks_row_lds_bytes(G, kind);
    int *st = reinterpret_cast<int *>(pk_state);
    hipLaunchKernelGGL(stream_peaks_kernel, dim3(B, STREAM_PEAKS_SLOTS), dim3(PKR_WAVE), dyn, stream, power, window_power, window_count, st, G,
                       max_windows, doa, kind, K, min_sep, rel, peaks, peak_power, window_peaks, window_peak_power, latest_peaks, latest_peak_power);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !window_power) return e;
    hipLaunchKernelGGL(stream_peaks_commit_kernel, dim3(1), dim3(64), 0, stream, window_count, st, max_windows);
    return hipGetLastError();
}

}  // namespace micloc
