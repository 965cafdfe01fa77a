// C-ABI of libmicloc_hip.so (see include/micloc_hip.h for the contract and reference citations):
// moving-target tracking, the per-step arg-max of the envelope of the beamformer output (track.hip).
#include "api_internal.h"

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

}  // namespace

extern "C" {

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

}  // extern "C"
