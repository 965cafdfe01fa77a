// C-ABI of libmicloc_hip.so (see include/micloc_hip.h for the contract and reference citations):
// moving-target tracking, the per-step arg-max of the envelope of the beamformer output (track.hip) and of the Xylo network's spike
// counts (the tracking form of the packed walk, stream_xylo.hip) -- and, beside that one-shot Xylo read-out, the other: counts, rate and
// peak per time window (xylo.hip, sweep.hip).
#include "api_internal.h"
#include "xylo_track.h"
#include "xylo_windows.h"

using namespace micloc;

namespace {

// Workspace of the four tracking calls: [ what the first two pipeline stages need | the tracking region ] -- the STHT output, then the
// encoder scratch and the raster (real bf_mat) or the band-passed rows (complex); not the pipeline's per-chunk sums, not the
// planar array the plan's kind never writes.  Tracking region of fused plans: the (value, index) pairs.  Other plans (the two-step
// route): y and its envelope for as many trials at a time as the caller's buffer holds, one at least.
struct TrackLayout : FrontOffsets {
    size_t base, per_trial, min_total;  // per_trial == 0: fused
};

TrackLayout track_layout(const micloc_plan *p, int B, int T)
{
    TrackLayout t{};
    const size_t planar = align256((size_t)B * p->C * micloc_padded_T(T) * sizeof(double));
    size_t off = 0;
    t.h = off;
    off += planar;
    if (p->W_is_complex) {
        t.pre = off;
        off += planar;
    } else {
        t.scratch = off;
        off += align256(rzcc_scratch_bytes(B * p->C, T, p->robust_width, p->chunk_frames));
        t.spikes = off;
        off += align256((size_t)B * T * p->C);
    }
    t.base = off;
    if (track_fused_eligible(p->W, p->ntab, p->W_is_complex)) {
        t.min_total = t.base + align256(track_pairs_bytes(B, T, p->G_out));
    } else {
        const size_t cell = (size_t)T * p->G_out * sizeof(double);
        t.per_trial = align256(p->W_is_complex ? 2 * cell : cell) + align256(cell);
        t.min_total = t.base + t.per_trial;
    }
    return t;
}

// the argument checks of a tracking entry; in: its input array
int track_args(const micloc_plan *p, const void *in, int B, int T, const int32_t *index)
{
    if (!p || !index || bad_batch(B)) return MICLOC_ERR_INVALID;
    if (T < 1 || (long long)B * T > 0x7fffffffll) return MICLOC_ERR_SHAPE;
    return in ? MICLOC_OK : MICLOC_ERR_INVALID;
}

// src: the spike raster (real bf_mat) or the planar band-passed rows [B][C][Ts] (complex)
int track_run(const micloc_plan *p, const void *src, int B, int T, int Ts, double a_rise, double i_rise, double a_fall, int32_t *index,
              double *peak_env, double *env_last, void *ws, size_t ws_bytes, const TrackLayout &lay, hipStream_t st)
{
    const int G = p->G_out, cpx = p->W_is_complex;
    unsigned char *reg = static_cast<unsigned char *>(ws) + lay.base;
    if (lay.per_trial == 0) {
        HIP_TRY(launch_track_fused(p->W, p->ntab, cpx, src, B, T, Ts, G, a_rise, i_rise, a_fall, index, peak_env, env_last, reg, st));
        return MICLOC_OK;
    }
    // the two-step route, over sub-batches of independent trials: beamforming with y stored, envelope_kernel, the row read-out
    size_t fit = (ws_bytes - lay.base) / lay.per_trial;
    const int nb_max = fit > (size_t)B ? B : (int)fit;
    const size_t cell = (size_t)T * G * sizeof(double);
    for (int b0 = 0; b0 < B; b0 += nb_max) {
        const int nb = B - b0 < nb_max ? B - b0 : nb_max;
        double *y = reinterpret_cast<double *>(reg);
        double *env = reinterpret_cast<double *>(reg + (size_t)nb * align256(cpx ? 2 * cell : cell));
        int nch = 0;
        if (cpx)
            HIP_TRY(launch_planar_beamform(p->W, static_cast<const double *>(src) + (size_t)b0 * p->C * Ts, nb, T, Ts, y, 1, nullptr, st, &nch));
        else
            HIP_TRY(launch_lif_beamform(p->W, p->ntab, static_cast<const int8_t *>(src) + (size_t)b0 * T * p->C, nb, T, y, nullptr, st, &nch));
        HIP_TRY(launch_envelope_track(y, cpx ? MICLOC_ENV_C128 : MICLOC_ENV_F64, nb, T, G, a_rise, i_rise, a_fall, env, nullptr, st));
        HIP_TRY(launch_track_rows(env, nb, T, G, index + (size_t)b0 * T, peak_env ? peak_env + (size_t)b0 * T : nullptr,
                                  env_last ? env_last + (size_t)b0 * G : nullptr, st));
    }
    return MICLOC_OK;
}

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
    const size_t fit = ws_bytes / lay.per_trial;
    const int nb_max = fit > (size_t)B ? B : (int)fit;
    const int Crow = ternary_C > 0 ? ternary_C : Cin;
    for (int b0 = 0; b0 < B; b0 += nb_max) {
        const int nb = B - b0 < nb_max ? B - b0 : nb_max;
        uint8_t *raster = static_cast<uint8_t *>(ws);
        double *env = reinterpret_cast<double *>(static_cast<unsigned char *>(ws) + align256((size_t)nb * T * N));
        HIP_TRY(launch_xylo_resident(static_cast<const uint8_t *>(spikes_in) + (size_t)b0 * T * Crow, ternary_C, nb, T, Cin, N, w_rec, max_spikes,
                                     raster, rate ? rate + (size_t)b0 * N : nullptr, net_ws, st));
        HIP_TRY(launch_envelope_track(raster, MICLOC_ENV_U8, nb, T, N, a_rise, i_rise, a_fall, env, nullptr, st));
        HIP_TRY(launch_track_rows(env, nb, T, N, index + (size_t)b0 * T, peak_env ? peak_env + (size_t)b0 * T : nullptr,
                                  env_last ? env_last + (size_t)b0 * N : nullptr, st));
    }
    return MICLOC_OK;
}

size_t micloc_track_workspace_bytes(const micloc_plan *p, int B, int T)
{
    if (!p || bad_batch(B) || T < 1 || (long long)B * T > 0x7fffffffll || plan_kind(p, p->W_is_complex) != MICLOC_OK) return 0;
    return track_layout(p, B, T).min_total;
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
    int rc = track_args(p, spikes, B, T, index);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(p->device);
    rc = plan_kind(p, false);
    if (rc != MICLOC_OK) return rc;
    const TrackLayout lay = track_layout(p, B, T);
    if (bad_ws(ws, ws_bytes, lay.min_total)) return MICLOC_ERR_WORKSPACE;
    return track_run(p, spikes, B, T, 0, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, lay, (hipStream_t)stream);
}

int micloc_beamform_c128_track_f64(const micloc_plan *p, const double *pre, int B, int T, int Ts, double a_rise, double i_rise, double a_fall,
                                   int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream)
{
    int rc = track_args(p, pre, B, T, index);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(p->device);
    if (Ts != micloc_padded_T(T)) return MICLOC_ERR_SHAPE;
    rc = plan_kind(p, true);
    if (rc != MICLOC_OK) return rc;
    const TrackLayout lay = track_layout(p, B, T);
    if (bad_ws(ws, ws_bytes, lay.min_total)) return MICLOC_ERR_WORKSPACE;
    return track_run(p, pre, B, T, Ts, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, lay, (hipStream_t)stream);
}

// the first two launches of micloc_snn_pipeline_f64, then the tracking read-out of their raster
int micloc_snn_pipeline_track_f64(const micloc_plan *p, const double *x, int B, int T, double a_rise, double i_rise, double a_fall,
                                  int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream)
{
    int rc = track_args(p, x, B, T, index);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(p->device);
    rc = plan_kind(p, false);
    if (rc != MICLOC_OK) return rc;
    const TrackLayout lay = track_layout(p, B, T);
    if (bad_ws(ws, ws_bytes, lay.min_total)) return MICLOC_ERR_WORKSPACE;
    const Front f = front_end(p, false, x, B, T, ws, lay, nullptr, MICLOC_STAGE_ALL, (hipStream_t)stream);
    if (f.rc != MICLOC_OK) return f.rc;
    return track_run(p, f.src, B, T, f.Ts, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, lay, (hipStream_t)stream);
}

int micloc_beamformer_pipeline_track_f64(const micloc_plan *p, const double *x, int B, int T, double a_rise, double i_rise, double a_fall,
                                         int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream)
{
    int rc = track_args(p, x, B, T, index);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(p->device);
    rc = plan_kind(p, true);
    if (rc != MICLOC_OK) return rc;
    const TrackLayout lay = track_layout(p, B, T);
    if (bad_ws(ws, ws_bytes, lay.min_total)) return MICLOC_ERR_WORKSPACE;
    const Front f = front_end(p, true, x, B, T, ws, lay, nullptr, MICLOC_STAGE_ALL, (hipStream_t)stream);
    if (f.rc != MICLOC_OK) return f.rc;
    return track_run(p, f.src, B, T, f.Ts, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, lay, (hipStream_t)stream);
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
