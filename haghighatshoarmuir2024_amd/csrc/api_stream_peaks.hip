// C-ABI of libmicloc_hip.so (see include/micloc_hip.h for the contract): the multi-source read-out of a stream, "streaming, multi-source" --
// its state, the launch sequence behind a tile (stream_peaks.hip) and its two counters.
#include "api_internal.h"
#include "stream_peaks.h"

using namespace micloc;

extern "C" {

size_t micloc_stream_peaks_state_bytes(void) { return STREAM_PEAKS_STATE_BYTES; }

int micloc_stream_peaks_reset(void *pk_state, size_t pk_bytes, void *stream)
{
    if (!pk_state) return MICLOC_ERR_INVALID;
    if (bad_ws(pk_state, pk_bytes, STREAM_PEAKS_STATE_BYTES)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(pk_state));
    HIP_TRY(launch_zero_fill(pk_state, STREAM_PEAKS_STATE_BYTES, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_peaks_tile_f64(const double *power, const double *window_power, const int32_t *window_count, int B, int G, int max_windows,
                                 const double *doa_list, int grid_kind, int K, double min_separation, double rel_threshold, void *pk_state,
                                 size_t pk_bytes, int32_t *peaks, double *peak_power, int32_t *window_peaks, double *window_peak_power,
                                 int32_t *latest_peaks, double *latest_peak_power, void *stream)
{
    // the limits of micloc_doa_peaks_f64, before any device work
    if (!doa_list || bad_batch(B) || G < 1 || G > 4096 || K < 1 || K > 16 || max_windows < 0) return MICLOC_ERR_INVALID;
    if (grid_kind < MICLOC_GRID_LINEAR || grid_kind > MICLOC_GRID_CIRCULAR_CLOSED) return MICLOC_ERR_INVALID;
    if (!(min_separation >= 0.0) || !(rel_threshold >= 0.0) || isinf(rel_threshold)) return MICLOC_ERR_INVALID;
    const bool windows = window_power != nullptr && max_windows > 0;
    if (!windows && !power) return MICLOC_ERR_INVALID;  // nothing to read
    if (power && !peaks) return MICLOC_ERR_INVALID;
    if (windows && (!window_count || !window_peaks)) return MICLOC_ERR_INVALID;
    if (bad_ws(pk_state, pk_bytes, STREAM_PEAKS_STATE_BYTES)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(pk_state));
    HIP_TRY(launch_stream_peaks(power, windows ? window_power : nullptr, window_count, B, G, max_windows, doa_list, grid_kind, K, min_separation,
                                rel_threshold, pk_state, peaks, peak_power, window_peaks, window_peak_power, latest_peaks, latest_peak_power,
                                (hipStream_t)stream));
    return MICLOC_OK;
}

/* status[0] = windows whose peaks are read, [1] = windows skipped: their rows were overwritten before they were read (synchronises the
 * stream) */
int micloc_stream_peaks_status(const void *pk_state, int *status2, void *stream)
{
    if (!pk_state || !status2) return MICLOC_ERR_INVALID;
    int w[2];
    HIP_TRY(hipMemcpyAsync(w, pk_state, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status2[0] = w[0];
    status2[1] = w[1];
    return MICLOC_OK;
}

}  // extern "C"
