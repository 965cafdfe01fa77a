// Wideband tracking while the recording arrives (stream_track_bands.hip; the rule: include/micloc_hip.h "wideband streaming, tracking"):
// what its C-ABI unit (api_stream.hip) calls.
#pragma once
#include "track_bands.h"

namespace micloc {

// the head of the tracked state in front of the envelope rows: STB_HEAD_BYTES of int words
constexpr size_t STB_HEAD_BYTES = 256;
constexpr int STB_FRONT = 0;  // the tracked frontier in absolute frames: every frame below it has been emitted
constexpr int STB_F0 = 1;     // the range of the current tile in rows of the raster windows, [STB_F0, STB_F1) ...
constexpr int STB_F1 = 2;
constexpr int STB_ABS0 = 3;   // ... whose row 0 is this absolute frame

// the heads of the SNN bands' localize states (loc_state of micloc_stream_localize_tile_f64), by value as a kernel argument
struct TrackBandsCtl {
    const int *ctl[MICLOC_MAX_BANDS];
};

// [head][B][track_col_groups(G) * 64] doubles, zero-filled once
size_t stream_track_bands_state_bytes(int B, int G);

// SNN bands, behind the last band's localize step of a tile (commit and tick included): one thread writes the frontier words from the bands'
// committed chunk counts, then the band kernel tracks the frames between the previous frontier and the new one from the bands' raster windows
// a.src[f] = [B][cap][C], then (G > 64) the combine.  CH: the bands' chunk length; pairs: stream_track_pairs_bytes(B, cap, G).
hipError_t launch_stream_track_bands(const TrackBandsArgs &a, const TrackBandsCtl &c, int F, int NKmax, int C, int B, int cap, int CH, int G,
                                     double a_rise, double i_rise, double a_fall, void *track_state, int R, int32_t *index, double *peak,
                                     int32_t *latest_index, double *latest_peak, void *pairs, hipStream_t stream);

// complex bands, in front of the slide of a tile: a.src[f] = band f's rows [B][C][cap] of the one staging array; ctl: the head of the complex
// stream's state, whose words give the range as for the single-plan stream
hipError_t launch_stream_track_bands_complex(const TrackBandsArgs &a, int F, const int *ctl, int C, int B, int cap, int G, double a_rise,
                                             double i_rise, double a_fall, void *track_state, int R, int32_t *index, double *peak,
                                             int32_t *latest_index, double *latest_peak, void *pairs, hipStream_t stream);

}  // namespace micloc
