// C-ABI of libmicloc_hip.so (see include/micloc_hip.h for the contract and reference citations):
// moving-target tracking, the per-step arg-max of the envelope of the beamformer output (track.hip) -- the workspace layout and the run of a
// set of plans, which the wideband entries of api_bands.hip share (api_sets.h), and the entries of a single plan, the set of one -- and of
// the Xylo network's spike counts (the tracking form of the packed walk, stream_xylo.hip); beside that one-shot Xylo read-out, the other:
// counts, rate and peak per time window (xylo.hip, sweep.hip).
#include "api_sets.h"
#include "track_bands.h"
#include "xylo_track.h"
#include "xylo_windows.h"

using namespace micloc;

namespace {

// the two-step route's loop: body(b0, nb) for as many trials at a time as the caller's buffer holds (fit), one at least
template <class Body>
int sub_batches(int B, size_t fit, Body body)
{
    const int nb_max = fit > (size_t)B ? B : (int)fit;
    for (int b0 = 0; b0 < B; b0 += nb_max) {
        const int rc = body(b0, B - b0 < nb_max ? B - b0 : nb_max);
        if (rc != MICLOC_OK) return rc;
    }
    return MICLOC_OK;
}

// the two-step route's tail for the trials b0 .. b0 + nb: envelope_kernel on `in` (kind: MICLOC_ENV_*), then the row read-out
int envelope_rows(const void *in, int kind, int b0, int nb, int T, int G, double a_rise, double i_rise, double a_fall, double *env, int32_t *index,
                  double *peak_env, double *env_last, hipStream_t st)
{
    HIP_TRY(launch_envelope_track(in, kind, nb, T, G, a_rise, i_rise, a_fall, env, nullptr, st));
    HIP_TRY(launch_track_rows(env, nb, T, G, index + (size_t)b0 * T, peak_env ? peak_env + (size_t)b0 * T : nullptr,
                              env_last ? env_last + (size_t)b0 * G : nullptr, st));
    return MICLOC_OK;
}

bool bands_track_fused(const micloc_plan *const *plans, int F, bool cpx)
{
    const BeamformW *W[MICLOC_MAX_BANDS];
    const NeuronTab *nt[MICLOC_MAX_BANDS];
    for (int f = 0; f < F; ++f) {
        W[f] = &plans[f]->W;
        nt[f] = &plans[f]->ntab;
    }
    return track_bands_fused_eligible(W, nt, F, cpx);
}

// the checks and the layout of the four single-plan entries in the header's order; in: the entry's input array, Ts: the planar stage
// entry's argument (else NULL)
int track_checked(const micloc_plan *p, bool cpx, const void *in, int B, int T, const int *Ts, const int32_t *index, const void *ws,
                  size_t ws_bytes, TrackLayout *L)
{
    if (!p || !index || bad_batch(B)) return MICLOC_ERR_INVALID;
    if (T < 1 || (long long)B * T > 0x7fffffffll) return MICLOC_ERR_SHAPE;
    if (!in) return MICLOC_ERR_INVALID;
    if (Ts && *Ts != micloc_padded_T(T)) return MICLOC_ERR_SHAPE;
    const int rc = plan_kind(p, cpx);
    if (rc != MICLOC_OK) return rc;
    *L = track_layout(&p, 1, cpx, false, B, T);
    return bad_ws(ws, ws_bytes, L->min_total) ? MICLOC_ERR_WORKSPACE : MICLOC_OK;
}

}  // namespace

namespace micloc {

TrackLayout track_layout(const micloc_plan *const *plans, int F, bool cpx, bool banded, int B, int T)
{
    const micloc_plan *p0 = plans[0];
    const size_t Ts = (size_t)micloc_padded_T(T);
    TrackLayout L{};
    size_t off = 0;
    L.xf = off;
    if (banded) off += align256((size_t)F * B * T * p0->M * sizeof(double));
    L.h = off;
    if (cpx) {
        const size_t planar = align256((size_t)F * B * p0->C * Ts * sizeof(double));
        off += planar;
        L.pre = off;
        off += planar;
    } else {
        off += align256((size_t)B * p0->C * Ts * sizeof(double));
        size_t scratch = 0;
        for (int f = 0; f < F; ++f) {
            const size_t n = rzcc_scratch_bytes(B * p0->C, T, plans[f]->robust_width, plans[f]->chunk_frames);
            if (n > scratch) scratch = n;
            if (plans[f]->ntab.NK > L.NKmax) L.NKmax = plans[f]->ntab.NK;
        }
        L.scratch = off;
        off += align256(scratch);
        L.spikes = off;
        L.raster = align256((size_t)B * T * p0->C);
        off += (size_t)F * L.raster;
    }
    L.base = off;
    if (banded ? bands_track_fused(plans, F, cpx) : track_fused_eligible(p0->W, p0->ntab, cpx)) {
        L.min_total = L.base + align256(track_pairs_bytes(B, T, p0->G_out));
    } else {
        const size_t cell = (size_t)T * p0->G_out * sizeof(double);
        L.per_trial = align256(cpx ? 2 * cell : cell) + (banded ? 2 : 1) * align256(cell);
        L.min_total = L.base + L.per_trial;
    }
    return L;
}

int track_run(const micloc_plan *const *plans, int F, bool cpx, bool banded, const void *const *src, int B, int T, int Ts, double a_rise,
              double i_rise, double a_fall, int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, const TrackLayout &L,
              hipStream_t st)
{
    const micloc_plan *p0 = plans[0];
    const int G = p0->G_out, C = p0->C;
    unsigned char *reg = static_cast<unsigned char *>(ws) + L.base;
    if (L.per_trial == 0 && !banded) {
        HIP_TRY(launch_track_fused(p0->W, p0->ntab, cpx, src[0], B, T, Ts, G, a_rise, i_rise, a_fall, index, peak_env, env_last, reg, st));
        return MICLOC_OK;
    }
    if (L.per_trial == 0) {
        TrackBandsArgs a{};
        for (int f = 0; f < F; ++f) {
            a.src[f] = src[f];
            a.tab[f] = plans[f]->ntab.tab;
            a.Wp[f] = plans[f]->W.Wp;
            a.NK[f] = plans[f]->ntab.NK;
            a.GT[f] = plans[f]->W.GT;
        }
        HIP_TRY(launch_track_bands_fused(a, F, L.NKmax, cpx, C, B, T, Ts, G, a_rise, i_rise, a_fall, index, peak_env, env_last, reg, st));
        return MICLOC_OK;
    }
    // the two-step route, over sub-batches of independent trials
    const size_t cell = (size_t)T * G * sizeof(double);
    return sub_batches(B, (ws_bytes - L.base) / L.per_trial, [&](int b0, int nb) {
        double *y = reinterpret_cast<double *>(reg);
        unsigned char *after_y = reg + (size_t)nb * align256(cpx ? 2 * cell : cell);
        double *m = reinterpret_cast<double *>(after_y);  // (banded)
        double *env = reinterpret_cast<double *>(banded ? after_y + (size_t)nb * align256(cell) : after_y);
        for (int f = 0; f < F; ++f) {
            const micloc_plan *p = plans[f];
            int nch = 0;
            if (cpx)
                HIP_TRY(launch_planar_beamform(p->W, static_cast<const double *>(src[f]) + (size_t)b0 * C * Ts, nb, T, Ts, y, 1, nullptr, st, &nch));
            else
                HIP_TRY(launch_lif_beamform(p->W, p->ntab, static_cast<const int8_t *>(src[f]) + (size_t)b0 * T * C, nb, T, y, nullptr, st, &nch));
            if (banded) HIP_TRY(launch_track_bands_magnitude(y, cpx, (size_t)nb * T * G, f == 0, m, st));
        }
        return envelope_rows(banded ? m : y, !banded && cpx ? MICLOC_ENV_C128 : MICLOC_ENV_F64, b0, nb, T, G, a_rise, i_rise, a_fall, env, index,
                             peak_env, env_last, st);
    });
}

}  // namespace micloc

namespace {

// ---- Xylo ----
// ws of micloc_xylo_lif_track_i16.  Fused networks: the pairs.  Others (the two-step route): the uint8 raster [T][N] and its envelope
// [T][N] doubles for as many trials at a time as the caller's buffer holds, one at least.
struct XyloTrackLayout {
    size_t per_trial, raster, min_total;  // per_trial == 0: fused
};

bool xylo_track_served(int ternary_C, int Cin, int N, int w_rec)
{
    return !(Cin < 1 || Cin > 64 || N < 1 || ternary_C < 0 || (ternary_C > 0 && Cin != 2 * ternary_C) || (w_rec != 0 && N > 1024));
}

XyloTrackLayout xylo_track_layout(bool fused, int B, int T, int N)
{
    XyloTrackLayout t{};
    if (fused) {
        t.min_total = xylo_track_pairs_bytes(B, T, N);
    } else {
        t.raster = align256((size_t)T * N);
        t.per_trial = t.raster + align256((size_t)T * N * sizeof(double));
        t.min_total = t.per_trial;
    }
    return t;
}

}  // namespace

extern "C" {

int micloc_xylo_track_is_fused(int ternary_C, int Cin, int N, int w_rec, int max_spikes)
{
    if (max_spikes < 1) return MICLOC_ERR_INVALID;
    if (Cin > 64 && N >= 1) return 0;  // (no Xylo kernel takes more than 64 input channels: the call itself answers MICLOC_ERR_SHAPE)
    if (!xylo_track_served(ternary_C, Cin, N, w_rec)) return MICLOC_ERR_SHAPE;
    return xylo_track_fused(ternary_C, Cin, w_rec, max_spikes) ? 1 : 0;
}

size_t micloc_xylo_track_workspace_bytes(int ternary_C, int Cin, int N, int w_rec, int B, int T)
{
    if (!xylo_track_served(ternary_C, Cin, N, w_rec) || bad_batch(B) || T < 1 || (long long)B * T > 0x7fffffffll) return 0;
    return xylo_track_layout(xylo_track_fused(ternary_C, Cin, w_rec, 1), B, T, N).min_total;
}

int micloc_xylo_lif_track_i16(const void *spikes_in, int ternary_C, int B, int T, int Cin, int N, int w_rec, int max_spikes, double a_rise,
                              double i_rise, double a_fall, int32_t *index, double *peak_env, double *env_last, int32_t *rate, void *net_ws,
                              size_t net_ws_bytes, void *ws, size_t ws_bytes, void *stream)
{
    if (!spikes_in || !index || bad_batch(B) || max_spikes < 1) return MICLOC_ERR_INVALID;
    if (T < 1 || N < 1 || (long long)B * T > 0x7fffffffll || !xylo_track_served(ternary_C, Cin, N, w_rec)) return MICLOC_ERR_SHAPE;
    if (bad_ws(net_ws, net_ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    // (an unaligned ternary raster is served by the general kernel: the two-step route, if its workspace is there)
    const bool fused = xylo_track_fused(ternary_C, Cin, w_rec, max_spikes) && (reinterpret_cast<uintptr_t>(spikes_in) & 15) == 0;
    const XyloTrackLayout lay = xylo_track_layout(fused, B, T, N);
    if (bad_ws(ws, ws_bytes, lay.min_total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(net_ws));
    hipStream_t st = (hipStream_t)stream;
    if (fused) {
        HIP_TRY(launch_xylo_track(static_cast<const int8_t *>(spikes_in), ternary_C, B, T, Cin, N, max_spikes, a_rise, i_rise, a_fall, index,
                                  peak_env, env_last, rate, net_ws, ws, st));
        return MICLOC_OK;
    }
    // the two-step route over sub-batches of independent trials: the LIF with its raster stored, envelope_kernel, the row read-out
    const int Crow = ternary_C > 0 ? ternary_C : Cin;
    return sub_batches(B, ws_bytes / lay.per_trial, [&](int b0, int nb) {
        uint8_t *raster = static_cast<uint8_t *>(ws);
        double *env = reinterpret_cast<double *>(static_cast<unsigned char *>(ws) + align256((size_t)nb * T * N));
        HIP_TRY(launch_xylo_resident(static_cast<const uint8_t *>(spikes_in) + (size_t)b0 * T * Crow, ternary_C, nb, T, Cin, N, w_rec, max_spikes,
                                     raster, rate ? rate + (size_t)b0 * N : nullptr, net_ws, st));
        return envelope_rows(raster, MICLOC_ENV_U8, b0, nb, T, N, a_rise, i_rise, a_fall, env, index, peak_env, env_last, st);
    });
}

size_t micloc_track_workspace_bytes(const micloc_plan *p, int B, int T)
{
    if (!p || bad_batch(B) || T < 1 || (long long)B * T > 0x7fffffffll || plan_kind(p, p->W_is_complex) != MICLOC_OK) return 0;
    return track_layout(&p, 1, p->W_is_complex, false, B, T).min_total;
}

int micloc_track_is_fused(const micloc_plan *p)
{
    if (!p) return MICLOC_ERR_INVALID;
    if (plan_kind(p, p->W_is_complex) != MICLOC_OK) return MICLOC_ERR_NOT_SET;
    return track_fused_eligible(p->W, p->ntab, p->W_is_complex) ? 1 : 0;
}

int micloc_lif_beamform_track_f64(const micloc_plan *p, const int8_t *spikes, int B, int T, double a_rise, double i_rise, double a_fall,
                                  int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream)
{
    TrackLayout L;
    const int rc = track_checked(p, false, spikes, B, T, nullptr, index, ws, ws_bytes, &L);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(p->device);
    const void *src = spikes;
    return track_run(&p, 1, false, false, &src, B, T, 0, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, L, (hipStream_t)stream);
}

int micloc_beamform_c128_track_f64(const micloc_plan *p, const double *pre, int B, int T, int Ts, double a_rise, double i_rise, double a_fall,
                                   int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream)
{
    TrackLayout L;
    const int rc = track_checked(p, true, pre, B, T, &Ts, index, ws, ws_bytes, &L);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(p->device);
    const void *src = pre;
    return track_run(&p, 1, true, false, &src, B, T, Ts, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, L, (hipStream_t)stream);
}

// the first two launches of the plan's pipeline entry (micloc_snn_pipeline_f64 / micloc_beamformer_pipeline_f64), then the tracking read-out
// of their raster / planar rows
static int pipeline_track(const micloc_plan *p, bool cpx, const double *x, int B, int T, double a_rise, double i_rise, double a_fall, int32_t *index,
                          double *peak_env, double *env_last, void *ws, size_t ws_bytes, hipStream_t st)
{
    TrackLayout L;
    const int rc = track_checked(p, cpx, x, B, T, nullptr, index, ws, ws_bytes, &L);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(p->device);
    const Front f = front_end(p, cpx, x, B, T, ws, L, nullptr, MICLOC_STAGE_ALL, st);
    if (f.rc != MICLOC_OK) return f.rc;
    return track_run(&p, 1, cpx, false, &f.src, B, T, f.Ts, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, L, st);
}

int micloc_snn_pipeline_track_f64(const micloc_plan *p, const double *x, int B, int T, double a_rise, double i_rise, double a_fall,
                                  int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream)
{
    return pipeline_track(p, false, x, B, T, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, (hipStream_t)stream);
}

int micloc_beamformer_pipeline_track_f64(const micloc_plan *p, const double *x, int B, int T, double a_rise, double i_rise, double a_fall,
                                         int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream)
{
    return pipeline_track(p, true, x, B, T, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, (hipStream_t)stream);
}

// ---- time-resolved DoA, Xylo: counts, rate and peak per window (the rule: include/micloc_hip.h; every refusal in front of any launch) ----
int micloc_xylo_window_quantum(void) { return 256; }

size_t micloc_xylo_windows_workspace_bytes(int B, int T, int N)
{
    if (bad_batch(B) || T < 1 || N < 1) return 0;
    return align256(xylo_windows_chunk_bytes(B, T, N));
}

// window_args' statuses for the quantum of 256 frames, and hop <= window (a window past the recording would hold no frame)
static int xylo_window_args(int T, int window, int hop, int B, int *nW)
{
    const int rc = window_args(T, window, hop, micloc_xylo_window_quantum(), B, nW);
    if (rc != MICLOC_OK) return rc;
    return hop > window ? MICLOC_ERR_SHAPE : MICLOC_OK;
}

int micloc_xylo_lif_windows_i16(const void *spikes_in, int ternary_channels, int B, int T, int Cin, int N, int w_rec, int max_spikes, int window,
                                int hop, int32_t *window_counts, int32_t *counts, void *net_ws, size_t net_ws_bytes, void *ws, size_t ws_bytes,
                                void *stream)
{
    if (!spikes_in || !window_counts || bad_batch(B) || T < 1 || Cin < 1 || N < 1 || max_spikes < 1) return MICLOC_ERR_INVALID;
    if (!xylo_track_served(ternary_channels, Cin, N, w_rec)) return MICLOC_ERR_SHAPE;  // (the shapes micloc_xylo_lif_resident_i16 refuses)
    int nW = 0;
    const int rc = xylo_window_args(T, window, hop, B, &nW);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(net_ws, net_ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, xylo_windows_chunk_bytes(B, T, N))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(net_ws));
    HIP_TRY(launch_xylo_windows(spikes_in, ternary_channels, B, T, Cin, N, w_rec, max_spikes, window, hop, nW, window_counts, counts, net_ws,
                                reinterpret_cast<int32_t *>(ws), (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_xylo_window_readout(const int32_t *window_counts, int B, int T, int window, int hop, int G, int bands, double fs, int win_size,
                               double *window_rate, int32_t *window_peak, void *stream)
{
    if (!window_counts || bad_batch(B) || T < 1 || G < 1 || bands < 1 || !(fs > 0.0) || (!window_rate && !window_peak)) return MICLOC_ERR_INVALID;
    if (window_peak && (win_size < 1 || win_size % 2 != 1 || win_size > G / 2 || G > 16384)) return MICLOC_ERR_INVALID;  // micloc_peak_location_i32's rule
    int nW = 0;
    const int rc = xylo_window_args(T, window, hop, B, &nW);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(device_of(window_counts));
    HIP_TRY(launch_xylo_window_readout(window_counts, B, nW, T, window, hop, G, bands, fs, win_size, window_rate, window_peak, (hipStream_t)stream));
    return MICLOC_OK;
}

}  // extern "C"
