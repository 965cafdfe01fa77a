// What the time-resolved read-out of the one-shot Xylo LIF -- the chunk-count kernels and the window sums of csrc/xylo.hip, rate and peak
// of the window rows in csrc/sweep.hip -- offers to the C-ABI unit api_track.hip (include/micloc_hip.h "time-resolved DoA, Xylo"; DESIGN
// 4.25).  A header of its own, as xylo_track.h: micloc_internal.h is among the sources that committed measurement records pin.
#pragma once
#include "micloc_internal.h"

namespace micloc {

// the counts per chunk of 256 frames: int32 [B][ceil(T / 256)][N]
size_t xylo_windows_chunk_bytes(int B, int T, int N);
// workgroups over the (trial, window) pairs of the two window kernels: one each, or a fixed number that strides over them
unsigned xylo_window_grid(unsigned pairs);
// launch_xylo_resident's routing with the chunk-count kernels, then the window sums: two launches whatever B and nW.  window, hop:
// multiples of 256, hop <= window; nW = window_count(T, window, hop), B nW < 2^31; window_counts [B][nW][N]; rate [B][N] may be NULL; ws:
// xylo_upload's.  No host access, no synchronisation (graph-capturable).
hipError_t launch_xylo_windows(const void *spikes_in, int ternary_C, int B, int T, int Cin, int N, int w_rec, int max_spikes, int window, int hop,
                               int nW, int32_t *window_counts, int32_t *rate, void *ws, int32_t *chunk_counts, hipStream_t stream);
// window_counts [B nW][F G] -> window_rate [B nW][G], window_peak [B nW] (either may be NULL): one launch
hipError_t launch_xylo_window_readout(const int32_t *window_counts, int B, int nW, int T, int window, int hop, int G, int F, double fs, int win,
                                      double *window_rate, int32_t *window_peak, hipStream_t stream);

}  // namespace micloc
