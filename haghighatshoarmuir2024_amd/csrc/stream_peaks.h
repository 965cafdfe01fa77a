// The multi-source read-out of a stream (stream_peaks.hip): what its C-ABI unit (api_stream_peaks.hip) calls.
#pragma once
#include "micloc_internal.h"

namespace micloc {

// pk_state: int words {windows whose peaks are read, windows skipped}, the rest of the 256 bytes reserved; zero-filled once
constexpr size_t STREAM_PEAKS_STATE_BYTES = 256;
// window slots of a launch: grid (B, STREAM_PEAKS_SLOTS), whatever the tile (MICLOC_STREAM_PEAKS_SLOTS of include/micloc_hip.h)
constexpr int STREAM_PEAKS_SLOTS = MICLOC_STREAM_PEAKS_SLOTS;

// The read-out behind a tile: the rule of peaks_rows.h on power [B][G] (NULL: skipped) into peaks / peak_power [B][K], and on the rows of
// window_power [B][max_windows][G] of the windows [max(r, c - max_windows), c), c = *window_count, r = word 0 of pk_state, into the same rows
// of window_peaks / window_peak_power [B][max_windows][K], window c - 1 also into latest_peaks / latest_peak_power [B][K]; then the commit
// launch.  window_power == NULL: the running rows only.  peak_power, window_peak_power and latest_* may be NULL.
hipError_t launch_stream_peaks(const double *power, const double *window_power, const int32_t *window_count, int B, int G, int max_windows,
                               const double *doa, int kind, int K, double min_sep, double rel, void *pk_state, int32_t *peaks, double *peak_power,
                               int32_t *window_peaks, double *window_peak_power, int32_t *latest_peaks, double *latest_peak_power,
                               hipStream_t stream);

}  // namespace micloc
