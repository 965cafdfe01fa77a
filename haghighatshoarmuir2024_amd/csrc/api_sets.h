// What the C-ABI units of the entries that take a SET of plans share (api_bands.hip, api_stream.hip, api_track.hip): the rule of the set --
// its pointers, and what its plans must have in common -- and the tracking workspace and run of a set, of which a single plan is the set of
// one.  Each entry keeps the order of its statuses (include/micloc_hip.h) by the order in which it calls these.
#pragma once
#include "api_internal.h"

namespace micloc {

// ---- the rule of a set -----------------------------------------------------------------------------------------------------------
// MICLOC_ERR_INVALID for no set, a band count outside 1 .. MICLOC_MAX_BANDS or a NULL member; reads no plan
inline int set_pointers(const micloc_plan *const *plans, int F)
{
    if (!plans || F < 1 || F > MICLOC_MAX_BANDS) return MICLOC_ERR_INVALID;
    for (int f = 0; f < F; ++f)
        if (!plans[f]) return MICLOC_ERR_INVALID;
    return MICLOC_OK;
}

// MICLOC_ERR_NOT_SET for a plan without bf_mat or (with_ntab) without neuron kernel
inline int set_tables(const micloc_plan *const *plans, int F, bool with_W, bool with_ntab)
{
    for (int f = 0; f < F; ++f)
        if ((with_W && !plans[f]->d_W) || (with_ntab && !plans[f]->d_ntab)) return MICLOC_ERR_NOT_SET;
    return MICLOC_OK;
}

// what an entry asks the plans of its set to share
enum SetPart : unsigned {
    SET_GRID = 1,     // the array and the DoA grid: device, M, G_out
    SET_REAL = 2,     // every bf_mat real
    SET_COMPLEX = 4,  // every bf_mat complex
    SET_CHAIN = 8,    // one STHT launch, one band-pass launch and one chunking for all bands: W.GT, W.CT, L, the STHT taps' bits, iir.n
    SET_FRONT = 16,   // the first two of those launches alone, which read no bf_mat: device, M, L, the taps, iir.n
};

// MICLOC_ERR_SHAPE for a plan that differs from plans[0] in a part that is asked for; set_pointers has passed
inline int set_shares(const micloc_plan *const *plans, int F, unsigned parts)
{
    const micloc_plan *p0 = plans[0];
    for (int f = 0; f < F; ++f) {
        const micloc_plan *p = plans[f];
        if ((parts & (SET_GRID | SET_FRONT)) && (p->device != p0->device || p->M != p0->M)) return MICLOC_ERR_SHAPE;
        if ((parts & SET_GRID) && p->G_out != p0->G_out) return MICLOC_ERR_SHAPE;
        if ((parts & (SET_REAL | SET_COMPLEX)) && (p->W_is_complex != 0) != ((parts & SET_COMPLEX) != 0)) return MICLOC_ERR_SHAPE;
        if ((parts & SET_CHAIN) && (p->W.GT != p0->W.GT || p->W.CT != p0->W.CT)) return MICLOC_ERR_SHAPE;
        if ((parts & (SET_CHAIN | SET_FRONT)) && (p->L != p0->L || p->taps_host != p0->taps_host || p->iir.n != p0->iir.n)) return MICLOC_ERR_SHAPE;
    }
    return MICLOC_OK;
}

// the complex one-shot loaders (bands_complex.hip) index a trial's T x M samples with 32 bits
inline bool trial_over_32_bits(const micloc_plan *p, int T) { return (unsigned long long)T * (unsigned long long)p->M > 0xffffffffull; }

// ---- the tracking workspace and run of a set (api_track.hip) -----------------------------------------------------------------------
// [ xf (banded) | the front end: h, then (real bf_mat) the encoder scratch, shared by the bands, which run one after the other on the stream,
// and every band's raster -- (complex) every band's planar rows, h and pre | the tracking region ].  Not the pipeline's per-chunk sums, not the
// planar array the set's kind never writes.  Tracking region of fused sets: the (value, index) pairs, the only part that knows G.  Other
// sets (the two-step route): one band's y, (banded) the band sum m, and the envelope for as many trials at a time as the caller's buffer
// holds, one at least.  A single plan is the set of one that is not banded: no filterbank output xf, no band sum m.
struct TrackLayout : FrontOffsets {
    size_t xf, raster, base, per_trial, min_total;  // raster: bytes of one band's raster; per_trial == 0: fused
    int NKmax;
};

// the plans hold their tables and share what the entries ask for (bands: set_shares); B and T are in range
TrackLayout track_layout(const micloc_plan *const *plans, int F, bool cpx, bool banded, int B, int T);

// src[f]: band f's raster [B][T][C] (real bf_mat) or planar band-passed rows [B][C][Ts] (complex).  Fused: launch_track_fused, banded (also
// at F == 1) launch_track_bands_fused.  Two-step: per band beamforming with y stored -- banded: and the band sum m by the rule --, then
// envelope_kernel on y / m and the row read-out.
int track_run(const micloc_plan *const *plans, int F, bool cpx, bool banded, const void *const *src, int B, int T, int Ts, double a_rise,
              double i_rise, double a_fall, int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, const TrackLayout &L,
              hipStream_t st);

}  // namespace micloc
