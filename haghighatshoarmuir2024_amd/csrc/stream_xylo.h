// What csrc/stream_xylo.hip (the packed integer LIF resumable across launches, its windows, the read-out over the bands) offers to the
// C-ABI unit api_xylo_stream.hip.  A header of its own: micloc_internal.h is among the sources that committed measurement records pin.
#pragma once
#include "micloc_internal.h"

namespace micloc {

constexpr int XYLO_STREAM_CHUNK = 256;                      // frames per chunk of a band's stream: what a window and a hop are multiples of
constexpr size_t XYLO_STREAM_READOUT_STATE_BYTES = 256;     // int words {emitted, given up, pending emitted, pending given up}
size_t xylo_stream_state_bytes(int B, int N);               // [B][Npad / 2] x {isyn, vmem, total0, total1}: 16 bytes per lane pair
size_t xylo_stream_chunk_bytes(int B, int N, int chunk_rows);  // chunk_counts [B][chunk_rows][N] ints
// the frames [t0, t0 + n) of raster [B][stride_frames][tc] by value (ctl == NULL), or the chunk range of a band's control words `ctl`;
// state in, state out, counts [B][N] rewritten (an empty range: nothing); ws: xylo_upload's; chunk_counts may be NULL
hipError_t launch_xylo_resume(const int8_t *raster, int tc, int stride_frames, int B, int t0, int n, const int *ctl, int Cin, int N, int max_spikes,
                              uint8_t *spikes_out, int T_out, int32_t *counts, void *state, void *ws, int32_t *chunk_counts, int chunk_rows,
                              hipStream_t stream);
// win_state of a band: [256 B: int windows emitted][acc [B][ceil(window / hop)][N] ints][ring [B][Kb][N] ints]
size_t xylo_stream_window_state_bytes(int B, int N, int window, int hop, int Kb);
// between launch_xylo_resume and launch_stream_commit of a tile: the new chunk rows onto the open windows, finished windows into the ring
hipError_t launch_xylo_stream_windows(const int32_t *chunk_counts, int B, int chunk_rows, int N, const int *ctl, int final_tile, int window, int hop,
                                      int Kb, void *win_state, hipStream_t stream);
struct XyloReadoutArgs {
    const int32_t *counts[MICLOC_MAX_BANDS];
    const int *ctl[MICLOC_MAX_BANDS];
    const int *head[MICLOC_MAX_BANDS];  // (filled by the launcher from the bands' win_state)
    const int32_t *ring[MICLOC_MAX_BANDS];
};
int xylo_stream_readout_max_grid();
// behind every band's tile: counts [B][F G], rate [B][G], peak [B]; window > 0: the windows every band has emitted, window n in row
// n % max_windows of wcounts [B][max_windows][F G] / wrate [B][max_windows][G] / wpeak [B][max_windows], the newest also in l* (may be NULL)
hipError_t launch_xylo_stream_readout(XyloReadoutArgs a, void *const *win_states, int F, int B, int G, double fs, int win, int window, int hop, int Kb,
                                      int max_windows, void *state, int32_t *counts, double *rate, int32_t *peak, int32_t *wcounts, double *wrate,
                                      int32_t *wpeak, int32_t *lcounts, double *lrate, int32_t *lpeak, hipStream_t stream);

// ---- the tracked stream (include/micloc_hip.h "streaming, Xylo tracking") ----
size_t xylo_stream_track_state_bytes(int B, int N);           // [B][Npad / 2] x {e0, e1} doubles, the lane order of the LIF state
size_t xylo_stream_track_pairs_bytes(int B, int N, int cap);  // 256 up to 512 neurons, else one (value, index) pair per position and block
// launch_xylo_resume's range and state hand-off (no spikes_out) with the tracked read-out: the envelope in front of the range in and out
// (env_state), frame t of the range into row t % R of index / peak [B][R], the newest also into latest_*, env_last [B][N] and counts [B][N]
// rewritten (an empty range: nothing).  cap: positions per trial of `pairs` (a stream: the raster window's frames; by value: >= n).
hipError_t launch_xylo_track_resume(const int8_t *raster, int tc, int stride_frames, int B, int t0, int n, const int *ctl, int Cin, int N,
                                    int max_spikes, int32_t *counts, void *state, void *env_state, void *ws, int32_t *chunk_counts, int chunk_rows,
                                    double a_rise, double i_rise, double a_fall, int R, int32_t *index, double *peak, int32_t *latest_index,
                                    double *latest_peak, double *env_last, void *pairs, int cap, hipStream_t stream);

}  // namespace micloc
