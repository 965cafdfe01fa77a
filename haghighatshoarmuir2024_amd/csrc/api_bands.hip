// C-ABI of libmicloc_hip.so (see include/micloc_hip.h for the contract and reference citations): the wideband batch entries -- the
// filterbank, the band sum, and the pipelines of F bands, SNN (one chain per band) and complex (every band's chain in one batch), with
// the entries of their moving-target tracking read-out (a DoA per frame over all bands): the checks and the front ends, in front of the
// layout and the run of api_track.hip.  What the plans of a set must share: api_sets.h.
#include "api_sets.h"

using namespace micloc;

// ---- what api_stream.hip takes from this unit (api_internal.h) -------------------------------------------------------------------
namespace micloc {

int filterbank_coef(const double *b, const double *a, int F, int n, FilterbankCoef *co)
{
    if (!b || !a || F < 1 || F > MICLOC_MAX_BANDS || n < 1 || n > MICLOC_MAX_IIR) return MICLOC_ERR_INVALID;
    memset(co, 0, sizeof(*co));
    co->n = n;
    for (int f = 0; f < F; ++f) {
        const double a0 = a[(size_t)f * n];
        if (a0 == 0.0) return MICLOC_ERR_INVALID;
        for (int i = 0; i < n; ++i) {
            co->b[f][i] = b[(size_t)f * n + i] / a0;
            co->a[f][i] = a[(size_t)f * n + i] / a0;
        }
    }
    return MICLOC_OK;
}

void cbands_coef(const micloc_plan *const *plans, int F, FilterbankCoef *co)
{
    memset(co, 0, sizeof(*co));
    co->n = plans[0]->iir.n;
    for (int f = 0; f < F; ++f)
        for (int i = 0; i < MICLOC_MAX_IIR; ++i) {
            co->b[f][i] = plans[f]->iir.b[i];
            co->a[f][i] = plans[f]->iir.a[i];
        }
}

}  // namespace micloc

// ---- wideband: filterbank, one SNN chain per band, band sum (filterbank.hip) ---------------------------------------------------
namespace {

struct BandsLayout {
    size_t xf, band_power, pipe, pipe_bytes, total;
    int nW;       // windows per trial (1 for whole recordings)
    long long R;  // rows of the band sum
};

// argument checks of the band pipeline in the header's order; fills the layout
int bands_layout(const micloc_plan *const *plans, int F, int B, int T, int window, int hop, bool own_band_power, BandsLayout *L)
{
    if (set_pointers(plans, F) != MICLOC_OK || bad_batch(B) || T < 1 || window < 0 || hop < 0) return MICLOC_ERR_INVALID;
    if (set_tables(plans, F, true, true) != MICLOC_OK) return MICLOC_ERR_NOT_SET;
    if (set_shares(plans, F, SET_GRID | SET_REAL) != MICLOC_OK) return MICLOC_ERR_SHAPE;
    const micloc_plan *p0 = plans[0];
    L->nW = 1;
    if (window > 0) {
        if (hop == 0) hop = window;
        for (int f = 0; f < F; ++f) {
            const int rc = window_args(T, window, hop, window_quantum(plans[f]), B, &L->nW);
            if (rc != MICLOC_OK) return rc;
        }
    }
    L->R = (long long)B * L->nW;
    size_t off = 0;
    L->xf = off;
    off += align256((size_t)F * B * T * p0->M * sizeof(double));
    L->band_power = off;
    if (own_band_power) off += align256((size_t)F * L->R * p0->G_out * sizeof(double));
    L->pipe = off;
    L->pipe_bytes = 0;
    for (int f = 0; f < F; ++f) {
        const size_t n = micloc_workspace_bytes(plans[f], B, T);  // (the pipeline's ws_layout(...).total: the arguments are checked above)
        if (n > L->pipe_bytes) L->pipe_bytes = n;
    }
    off += L->pipe_bytes;
    L->total = off;
    return MICLOC_OK;
}

}  // namespace

extern "C" {

int micloc_filterbank_f64(const double *b, const double *a, int F, int n, const double *x, int B, int T, int M, double *xf, void *stream)
{
    FilterbankCoef co;
    const int rc = filterbank_coef(b, a, F, n, &co);
    if (rc != MICLOC_OK) return rc;
    if (!x || !xf || B < 1 || T < 1 || M < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(xf));
    HIP_TRY(launch_filterbank(co, x, F, B, T, M, xf, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_band_sum_f64(const double *band_power, int F, int R, int G, double *power, int32_t *argmax, void *stream)
{
    if (!band_power || (!power && !argmax) || F < 1 || F > MICLOC_MAX_BANDS || R < 1 || G < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(power ? (const void *)power : (const void *)argmax));
    HIP_TRY(launch_band_sum(band_power, F, R, G, power, argmax, (hipStream_t)stream));
    return MICLOC_OK;
}

size_t micloc_snn_bands_workspace_bytes(const micloc_plan *const *plans, int F, int B, int T, int window, int hop)
{
    BandsLayout L{};
    // (sized for a caller that passes band_power == NULL: enough for either form)
    return bands_layout(plans, F, B, T, window, hop, true, &L) == MICLOC_OK ? L.total : 0;
}

int micloc_snn_pipeline_bands_f64(const micloc_plan *const *plans, int F, const double *fb_b, const double *fb_a, int fb_n, const double *x,
                                  int B, int T, int window, int hop, double *band_power, double *power, int32_t *argmax, void *ws,
                                  size_t ws_bytes, void *stream)
{
    if (!plans || !x || (!power && !argmax)) return MICLOC_ERR_INVALID;
    FilterbankCoef co;
    int rc = filterbank_coef(fb_b, fb_a, F, fb_n, &co);
    if (rc != MICLOC_OK) return rc;
    BandsLayout L{};
    rc = bands_layout(plans, F, B, T, window, hop, band_power == nullptr, &L);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(ws, ws_bytes, L.total)) return MICLOC_ERR_WORKSPACE;
    if (window > 0 && hop == 0) hop = window;
    const micloc_plan *p0 = plans[0];
    DeviceGuard guard(p0->device);
    unsigned char *base = reinterpret_cast<unsigned char *>(ws);
    double *xf = reinterpret_cast<double *>(base + L.xf);
    double *bp = band_power ? band_power : reinterpret_cast<double *>(base + L.band_power);
    void *pipe = base + L.pipe;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_filterbank(co, x, F, B, T, p0->M, xf, st));
    const size_t band_in = (size_t)B * T * p0->M, band_out = (size_t)L.R * p0->G_out;
    for (int f = 0; f < F; ++f) {  // one after the other on the stream: they share `pipe`
        rc = window > 0 ? micloc_snn_pipeline_windows_f64(plans[f], xf + f * band_in, B, T, window, hop, nullptr, bp + f * band_out, nullptr, nullptr,
                                                          nullptr, pipe, L.pipe_bytes, stream)
                        : micloc_snn_pipeline_f64(plans[f], xf + f * band_in, B, T, nullptr, nullptr, bp + f * band_out, nullptr, pipe, L.pipe_bytes,
                                                  stream);
        if (rc != MICLOC_OK) return rc;
    }
    HIP_TRY(launch_band_sum(bp, F, L.R, p0->G_out, power, argmax, st));
    return MICLOC_OK;
}

}  // extern "C"

// ---- wideband, complex Beamformer: every band's chain in one batch (bands_complex.hip) ---------------------------------------------------
namespace {

struct CBandsLayout {
    size_t xf, h, pre, partial, band_power, total;
    int nW;       // windows per trial (1 for whole recordings)
    int q;        // the plans' common window quantum (window > 0)
    long long R;  // rows of the band sum
};

// argument checks of the complex band pipeline in the header's order; fills the layout
int cbands_layout(const micloc_plan *const *plans, int F, int B, int T, int window, int hop, bool own_band_power, CBandsLayout *L)
{
    if (set_pointers(plans, F) != MICLOC_OK || bad_batch(B) || bad_batch(F * B) || T < 1 || window < 0 || hop < 0) return MICLOC_ERR_INVALID;
    if (set_tables(plans, F, true, false) != MICLOC_OK) return MICLOC_ERR_NOT_SET;
    const micloc_plan *p0 = plans[0];
    if (set_shares(plans, F, SET_GRID | SET_COMPLEX | SET_CHAIN) != MICLOC_OK || trial_over_32_bits(p0, T)) return MICLOC_ERR_SHAPE;
    L->nW = 1;
    L->q = 0;
    if (window > 0) {
        if (hop == 0) hop = window;
        for (int f = 0; f < F; ++f) {
            const int rc = window_args(T, window, hop, window_quantum(plans[f]), B, &L->nW);
            if (rc != MICLOC_OK) return rc;
        }
        L->q = window_quantum(p0);  // (one quantum: it depends on CT and GT only, which the plans share)
        if ((long long)F * B * L->nW > 0x7fffffffll) return MICLOC_ERR_SHAPE;
    }
    L->R = (long long)B * L->nW;
    const size_t Ts = (size_t)micloc_padded_T(T);
    const size_t planar = align256((size_t)F * B * p0->C * Ts * sizeof(double));
    size_t off = 0;
    L->xf = off;
    off += align256((size_t)F * B * T * p0->M * sizeof(double));
    L->h = off;
    off += planar;
    L->pre = off;
    off += planar;
    L->partial = off;
    off += align256(beamform_partial_bytes(F * B, T, 16 * p0->W.GT));
    L->band_power = off;
    if (own_band_power) off += align256((size_t)F * L->R * p0->G_out * sizeof(double));
    L->total = off;
    return MICLOC_OK;
}

// STHT of F * B trials in one launch (with_stht), then the band-pass of every band: one launch, or the one-shot launch per band -- the arm
// the one launch is measured against (it won at B = 1 and at B = 64, so the pipeline entry always takes the one launch)
int cbands_front(const micloc_plan *const *plans, int F, const double *xf, int B, int T, int Ts, double *h, double *pre, bool with_stht,
                 bool one_launch, hipStream_t st)
{
    const micloc_plan *p0 = plans[0];
    if (with_stht) HIP_TRY(launch_stht(p0->taps, xf, h, F * B, T, p0->M, Ts, st, false));
    if (one_launch) {
        FilterbankCoef pc;
        cbands_coef(plans, F, &pc);
        HIP_TRY(launch_bands_bandpass(pc, xf, h, F, B, T, p0->M, Ts, p0->taps.shift, pre, st));
        return MICLOC_OK;
    }
    const size_t band_rows = (size_t)B * p0->C * Ts, band_in = (size_t)B * T * p0->M;
    for (int f = 0; f < F; ++f) {
        const micloc_plan *p = plans[f];
        HIP_TRY(launch_bandpass_rzcc(p->iir, h + f * band_rows, B * p->C, p->C, T, Ts, p->robust_width, p->bipolar, pre + f * band_rows, nullptr,
                                     nullptr, st, xf + f * band_in, p->M, p->taps.shift));
    }
    return MICLOC_OK;
}

}  // namespace

extern "C" {

size_t micloc_beamformer_bands_workspace_bytes(const micloc_plan *const *plans, int F, int B, int T, int window, int hop)
{
    CBandsLayout L{};
    // (sized for a caller that passes band_power == NULL: enough for either form)
    return cbands_layout(plans, F, B, T, window, hop, true, &L) == MICLOC_OK ? L.total : 0;
}

int micloc_beamformer_pipeline_bands_f64(const micloc_plan *const *plans, int F, const double *fb_b, const double *fb_a, int fb_n,
                                         const double *x, int B, int T, int window, int hop, double *band_power, double *power, int32_t *argmax,
                                         void *ws, size_t ws_bytes, void *stream)
{
    if (!plans || !x || (!power && !argmax)) return MICLOC_ERR_INVALID;
    FilterbankCoef co;
    int rc = filterbank_coef(fb_b, fb_a, F, fb_n, &co);
    if (rc != MICLOC_OK) return rc;
    CBandsLayout L{};
    rc = cbands_layout(plans, F, B, T, window, hop, band_power == nullptr, &L);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(ws, ws_bytes, L.total)) return MICLOC_ERR_WORKSPACE;
    if (window > 0 && hop == 0) hop = window;
    const micloc_plan *p0 = plans[0];
    DeviceGuard guard(p0->device);
    double *xf = ws_doubles(ws, L.xf), *h = ws_doubles(ws, L.h), *pre = ws_doubles(ws, L.pre), *partial = ws_doubles(ws, L.partial);
    double *bp = band_power ? band_power : ws_doubles(ws, L.band_power);
    hipStream_t st = (hipStream_t)stream;
    const int Ts = micloc_padded_T(T), Gp = 16 * p0->W.GT, G = p0->G_out;
    HIP_TRY(launch_filterbank(co, x, F, B, T, p0->M, xf, st));
    rc = cbands_front(plans, F, xf, B, T, Ts, h, pre, true, true, st);
    if (rc != MICLOC_OK) return rc;
    // per band the launch of that band's own pipeline call (its bf_mat) on its B rows, into one array of chunk sums
    const size_t band_rows = (size_t)B * p0->C * Ts;
    int nch = 0;  // chunk rows per trial: known after band 0's launch, whose rows start at offset 0 whatever it is
    for (int f = 0; f < F; ++f) {
        int n = 0;
        HIP_TRY(launch_planar_beamform(plans[f]->W, pre + f * band_rows, B, T, Ts, nullptr, 1, partial + (size_t)f * B * nch * Gp, st, &n));
        if (f > 0 && n != nch) return MICLOC_ERR_INVALID;  // (never: the chunking depends on T, CT and GT only, which the plans share)
        nch = n;
    }
    if (window > 0) {
        if (nch != (T + L.q - 1) / L.q) return MICLOC_ERR_INVALID;  // the launch chose a kernel window_quantum() does not describe
        HIP_TRY(launch_window_power(partial, F * B, T, nch, Gp, G, 1, Gp / 2, L.q, window, hop, bp, nullptr, st));
    } else {
        HIP_TRY(launch_power_argmax(partial, F * B, T, nch, Gp, G, 1, Gp / 2, bp, nullptr, st));
    }
    HIP_TRY(launch_band_sum(bp, F, L.R, G, power, argmax, st));
    return MICLOC_OK;
}

int micloc_beamformer_bands_bandpass_f64(const micloc_plan *const *plans, int F, const double *xf, int B, int T, double *h, double *pre, int Ts,
                                         int with_stht, int one_launch, void *stream)
{
    if (!xf || !h || !pre || set_pointers(plans, F) != MICLOC_OK || bad_batch(B) || bad_batch(F * B) || T < 1) return MICLOC_ERR_INVALID;
    const micloc_plan *p0 = plans[0];
    if (set_shares(plans, F, SET_FRONT) != MICLOC_OK || Ts != micloc_padded_T(T) || trial_over_32_bits(p0, T)) return MICLOC_ERR_SHAPE;
    DeviceGuard guard(p0->device);
    return cbands_front(plans, F, xf, B, T, Ts, h, pre, with_stht != 0, one_launch != 0, (hipStream_t)stream);
}

}  // extern "C"

// ---- wideband moving-target tracking: a DoA per frame over all bands (track.hip; the rule: include/micloc_hip.h) ---------------------------
namespace {

// the argument checks of the header's order that read no plan: everything but `plans` itself may be a dummy
int bands_track_args(const micloc_plan *const *plans, int F, int B, int T)
{
    if (set_pointers(plans, F) != MICLOC_OK || bad_batch(B) || bad_batch(F * B)) return MICLOC_ERR_INVALID;
    if (T < 1 || (long long)B * T > 0x7fffffffll) return MICLOC_ERR_SHAPE;
    return MICLOC_OK;
}

// what the plans of a set must hold and share, then the layout; bands_track_args has passed
int bands_track_layout(const micloc_plan *const *plans, int F, bool cpx, int B, int T, TrackLayout *L)
{
    // (bf_mat as the other band entries: in front of the shapes, which a plan without bf_mat has not)
    if (set_tables(plans, F, true, false) != MICLOC_OK) return MICLOC_ERR_NOT_SET;
    if (set_shares(plans, F, SET_GRID | (cpx ? SET_COMPLEX : SET_REAL)) != MICLOC_OK) return MICLOC_ERR_SHAPE;
    if (!cpx && set_tables(plans, F, false, true) != MICLOC_OK) return MICLOC_ERR_NOT_SET;
    // complex: one STHT launch and one band-pass launch for all bands' chains, what micloc_beamformer_pipeline_bands_f64 asks for
    if (cpx && (set_shares(plans, F, SET_CHAIN) != MICLOC_OK || trial_over_32_bits(plans[0], T))) return MICLOC_ERR_SHAPE;
    *L = track_layout(plans, F, cpx, true, B, T);
    return MICLOC_OK;
}

size_t bands_track_workspace(const micloc_plan *const *plans, int F, bool cpx, int B, int T)
{
    TrackLayout L{};
    if (bands_track_args(plans, F, B, T) != MICLOC_OK || bands_track_layout(plans, F, cpx, B, T, &L) != MICLOC_OK) return 0;
    return L.min_total;
}

int bands_track_is_fused(const micloc_plan *const *plans, int F, bool cpx)
{
    TrackLayout L{};
    int rc = bands_track_args(plans, F, 1, 1);
    if (rc == MICLOC_OK) rc = bands_track_layout(plans, F, cpx, 1, 1, &L);
    if (rc != MICLOC_OK) return rc;
    return L.per_trial == 0 ? 1 : 0;
}

// the stage entries and the tails of the pipeline entries.  in: the caller's input array (checked for NULL only)
int bands_track_checked(const micloc_plan *const *plans, int F, bool cpx, const void *in, int B, int T, const int32_t *index, const void *ws,
                        size_t ws_bytes, TrackLayout *L)
{
    if (!plans || !in || !index) return MICLOC_ERR_INVALID;
    int rc = bands_track_args(plans, F, B, T);
    if (rc != MICLOC_OK) return rc;
    rc = bands_track_layout(plans, F, cpx, B, T, L);
    if (rc != MICLOC_OK) return rc;
    return bad_ws(ws, ws_bytes, L->min_total) ? MICLOC_ERR_WORKSPACE : MICLOC_OK;
}

}  // namespace

extern "C" {

size_t micloc_snn_bands_track_workspace_bytes(const micloc_plan *const *plans, int F, int B, int T)
{
    return bands_track_workspace(plans, F, false, B, T);
}

size_t micloc_beamformer_bands_track_workspace_bytes(const micloc_plan *const *plans, int F, int B, int T)
{
    return bands_track_workspace(plans, F, true, B, T);
}

int micloc_snn_bands_track_is_fused(const micloc_plan *const *plans, int F) { return bands_track_is_fused(plans, F, false); }

int micloc_beamformer_bands_track_is_fused(const micloc_plan *const *plans, int F) { return bands_track_is_fused(plans, F, true); }

int micloc_lif_beamform_bands_track_f64(const micloc_plan *const *plans, int F, const int8_t *spikes, int B, int T, double a_rise, double i_rise,
                                        double a_fall, int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream)
{
    TrackLayout L{};
    const int rc = bands_track_checked(plans, F, false, spikes, B, T, index, ws, ws_bytes, &L);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(plans[0]->device);
    const void *src[MICLOC_MAX_BANDS];
    for (int f = 0; f < F; ++f) src[f] = spikes + (size_t)f * B * T * plans[0]->C;
    return track_run(plans, F, false, true, src, B, T, 0, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, L, (hipStream_t)stream);
}

int micloc_beamform_c128_bands_track_f64(const micloc_plan *const *plans, int F, const double *pre, int B, int T, int Ts, double a_rise,
                                         double i_rise, double a_fall, int32_t *index, double *peak_env, double *env_last, void *ws,
                                         size_t ws_bytes, void *stream)
{
    TrackLayout L{};
    const int rc = bands_track_checked(plans, F, true, pre, B, T, index, ws, ws_bytes, &L);
    if (rc != MICLOC_OK) return rc;
    if (Ts != micloc_padded_T(T)) return MICLOC_ERR_SHAPE;
    DeviceGuard guard(plans[0]->device);
    const void *src[MICLOC_MAX_BANDS];
    for (int f = 0; f < F; ++f) src[f] = pre + (size_t)f * B * plans[0]->C * Ts;
    return track_run(plans, F, true, true, src, B, T, Ts, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, L, (hipStream_t)stream);
}

// the filterbank, per band the first two launches of micloc_snn_pipeline_f64 on its slice, then the tracking read-out of the F rasters
int micloc_snn_pipeline_bands_track_f64(const micloc_plan *const *plans, int F, const double *fb_b, const double *fb_a, int fb_n, const double *x,
                                        int B, int T, double a_rise, double i_rise, double a_fall, int32_t *index, double *peak_env,
                                        double *env_last, void *ws, size_t ws_bytes, void *stream)
{
    if (!plans || !x || !index) return MICLOC_ERR_INVALID;
    FilterbankCoef co;
    int rc = filterbank_coef(fb_b, fb_a, F, fb_n, &co);
    if (rc != MICLOC_OK) return rc;
    TrackLayout L{};
    rc = bands_track_checked(plans, F, false, x, B, T, index, ws, ws_bytes, &L);
    if (rc != MICLOC_OK) return rc;
    const micloc_plan *p0 = plans[0];
    DeviceGuard guard(p0->device);
    hipStream_t st = (hipStream_t)stream;
    double *xf = ws_doubles(ws, L.xf);
    HIP_TRY(launch_filterbank(co, x, F, B, T, p0->M, xf, st));
    const size_t band_in = (size_t)B * T * p0->M;
    const void *src[MICLOC_MAX_BANDS];
    for (int f = 0; f < F; ++f) {  // one after the other on the stream: they share h and the encoder scratch
        const FrontOffsets o{L.h, 0, L.scratch, L.spikes + (size_t)f * L.raster};
        const Front fr = front_end(plans[f], false, xf + f * band_in, B, T, ws, o, nullptr, MICLOC_STAGE_ALL, st);
        if (fr.rc != MICLOC_OK) return fr.rc;
        src[f] = fr.src;
    }
    return track_run(plans, F, false, true, src, B, T, 0, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, L, st);
}

// the filterbank, the STHT and the band-pass of all bands' chains as one batch (micloc_beamformer_pipeline_bands_f64's), then the
// tracking read-out of the F x B planar rows
int micloc_beamformer_pipeline_bands_track_f64(const micloc_plan *const *plans, int F, const double *fb_b, const double *fb_a, int fb_n,
                                               const double *x, int B, int T, double a_rise, double i_rise, double a_fall, int32_t *index,
                                               double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream)
{
    if (!plans || !x || !index) return MICLOC_ERR_INVALID;
    FilterbankCoef co;
    int rc = filterbank_coef(fb_b, fb_a, F, fb_n, &co);
    if (rc != MICLOC_OK) return rc;
    TrackLayout L{};
    rc = bands_track_checked(plans, F, true, x, B, T, index, ws, ws_bytes, &L);
    if (rc != MICLOC_OK) return rc;
    const micloc_plan *p0 = plans[0];
    DeviceGuard guard(p0->device);
    hipStream_t st = (hipStream_t)stream;
    const int Ts = micloc_padded_T(T);
    double *xf = ws_doubles(ws, L.xf), *h = ws_doubles(ws, L.h), *pre = ws_doubles(ws, L.pre);
    HIP_TRY(launch_filterbank(co, x, F, B, T, p0->M, xf, st));
    rc = cbands_front(plans, F, xf, B, T, Ts, h, pre, true, true, st);
    if (rc != MICLOC_OK) return rc;
    const void *src[MICLOC_MAX_BANDS];
    for (int f = 0; f < F; ++f) src[f] = pre + (size_t)f * B * p0->C * Ts;
    return track_run(plans, F, true, true, src, B, T, Ts, a_rise, i_rise, a_fall, index, peak_env, env_last, ws, ws_bytes, L, st);
}

}  // extern "C"
