// What the tracking form of the packed integer LIF (the envelope and the per-frame arg-max on its step counts; csrc/xylo.hip) offers to
// the C-ABI unit api_track.hip.  A header of its own: micloc_internal.h is among the sources that committed measurement records pin.
#pragma once
#include "micloc_internal.h"

namespace micloc {

// the (value, index) pairs of n rows x neuron blocks in one workspace: pval [n] doubles, then pidx [n] int32, each rounded to 256 bytes
inline size_t xylo_track_al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t xylo_track_pairs_size(size_t n) { return xylo_track_al256(n * sizeof(double)) + xylo_track_al256(n * sizeof(int32_t)); }
inline void xylo_track_pairs_split(void *pairs, size_t n, double *&pval, int32_t *&pidx)
{
    pval = reinterpret_cast<double *>(pairs);
    pidx = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(pairs) + xylo_track_al256(n * sizeof(double)));
}

// the network and input the fused kernel serves (beside a 16-byte aligned raster, which the call itself checks)
bool xylo_track_fused(int ternary_C, int Cin, int w_rec, int max_spikes);
// scratch of the fused call: nothing to speak of up to 512 neurons, else one (value, index) pair per frame and 512-neuron block
size_t xylo_track_pairs_bytes(int B, int T, int N);
// raster int8 [B][T][ternary_C], ws: xylo_upload's; index [B][T], peak [B][T] / env_last [B][N] / rate [B][N] may be NULL.  No host
// access, no synchronisation (graph-capturable).
hipError_t launch_xylo_track(const int8_t *raster, int ternary_C, int B, int T, int Cin, int N, int max_spikes, double a_rise, double i_rise,
                             double a_fall, int32_t *index, double *peak, double *env_last, int32_t *rate, void *ws, void *pairs,
                             hipStream_t stream);

}  // namespace micloc
