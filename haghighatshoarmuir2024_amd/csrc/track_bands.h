// Wideband moving-target tracking (the rule: include/micloc_hip.h, "wideband moving-target tracking"): what track.hip offers to the C-ABI
// unit that runs the tracking read-out of a set of plans, api_track.hip.  Only those two include this header.
#pragma once
#include "micloc_internal.h"

namespace micloc {

// What the band kernels read per band; by value as a kernel argument (no device table).  src: band f's raster [B][T][C] (real bf_mat) or
// its planar band-passed rows [B][C][Ts] (complex); tab / NK: its neuron table (real bf_mat only); Wp / GT: its packed bf_mat.
struct TrackBandsArgs {
    const void *src[MICLOC_MAX_BANDS];
    const double *tab[MICLOC_MAX_BANDS];
    const double *Wp[MICLOC_MAX_BANDS];
    int NK[MICLOC_MAX_BANDS];
    int GT[MICLOC_MAX_BANDS];
};

// true: the band kernels serve this set -- every plan is track_fused_eligible and the LDS of a workgroup, sized for the largest NK, fits
bool track_bands_fused_eligible(const BeamformW *const *W, const NeuronTab *const *nt, int F, int is_complex);

// F bands of B trials -> index [B][T], peak [B][T] (may be NULL), env_last [B][G] (may be NULL).  C: channels (2 x microphones), NKmax: the
// largest NK of `a` (0 for complex), pairs: track_pairs_bytes(B, T, G).  One kernel launch, then track_combine_kernel when G > 64.
hipError_t launch_track_bands_fused(const TrackBandsArgs &a, int F, int NKmax, int is_complex, int C, int B, int T, int Ts, int G, double a_rise,
                                    double i_rise, double a_fall, int32_t *index, double *peak, double *env_last, void *pairs,
                                    hipStream_t stream);

// the band sum of the two-step route: m[i] = |y[i]| (first) or m[i] + |y[i]| in one rounded add, i < n; |.| = fabs, or hypot(re, im) of
// interleaved pairs (is_complex) -- the expressions of the fused kernels' magnitude tile
hipError_t launch_track_bands_magnitude(const double *y, int is_complex, size_t n, int first, double *m, hipStream_t stream);

}  // namespace micloc
