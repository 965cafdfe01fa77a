// The tracking rule while the recording arrives (stream_track.hip): what its C-ABI unit (api_stream.hip) calls.
#pragma once
#include "micloc_internal.h"

namespace micloc {

// state: the envelope e[t-1][g] in front of the next frame, [B][track_col_groups(G) * 64] doubles, zero-filled once
size_t stream_track_state_bytes(int B, int G);
size_t stream_track_pairs_bytes(int B, int cap, int G);  // (value, index) pairs [B][cap][ceil(G / 64)]; 256 with one column group
int stream_track_halo(const NeuronTab &nt);              // rows of LIF history in front of a chunk: they must fit one chunk of the stream
// between the accumulate (and the window read-out) and the commit / the slide of a tile: ctl is the head of the stream's state.  src: the
// raster window [B][cap][C] (real bf_mat; CH = the stream's chunk length) or the staging array [B][C][cap] (complex).  Frame t of the
// range goes to row t % R of index / peak [B][R], the newest one also to latest_index / latest_peak [B].
hipError_t launch_stream_track(const BeamformW &W, const NeuronTab &nt, int is_complex, const void *src, const int *ctl, int B, int cap, int CH,
                               int G, double a_rise, double i_rise, double a_fall, double *state, int R, int32_t *index, double *peak,
                               int32_t *latest_index, double *latest_peak, void *pairs, hipStream_t stream);

}  // namespace micloc
