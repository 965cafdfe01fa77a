// C-ABI of libmicloc_hip.so (see include/micloc_hip.h for the contract and reference citations): the wideband batch entries -- the
// filterbank, the band sum, and the pipelines of F bands, SNN (one chain per band) and complex (every band's chain in one batch).
#include "api_internal.h"

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
    if (!plans || F < 1 || F > MICLOC_MAX_BANDS || bad_batch(B) || T < 1 || window < 0 || hop < 0) return MICLOC_ERR_INVALID;
    for (int f = 0; f < F; ++f)
        if (!plans[f]) return MICLOC_ERR_INVALID;
    for (int f = 0; f < F; ++f)
        if (!plans[f]->d_ntab || !plans[f]->d_W) return MICLOC_ERR_NOT_SET;
    const micloc_plan *p0 = plans[0];
    for (int f = 0; f < F; ++f) {
        const micloc_plan *p = plans[f];
        if (p->device != p0->device || p->M != p0->M || p->G_out != p0->G_out || p->W_is_complex) return MICLOC_ERR_SHAPE;
    }
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
    if (!plans || F < 1 || F > MICLOC_MAX_BANDS || bad_batch(B) || bad_batch(F * B) || T < 1 || window < 0 || hop < 0) return MICLOC_ERR_INVALID;
    for (int f = 0; f < F; ++f)
        if (!plans[f]) return MICLOC_ERR_INVALID;
    for (int f = 0; f < F; ++f)
        if (!plans[f]->d_W) return MICLOC_ERR_NOT_SET;
    const micloc_plan *p0 = plans[0];
    for (int f = 0; f < F; ++f) {
        const micloc_plan *p = plans[f];
        if (!p->W_is_complex || p->device != p0->device || p->M != p0->M || p->G_out != p0->G_out || p->W.GT != p0->W.GT || p->W.CT != p0->W.CT ||
            p->L != p0->L || p->taps_host != p0->taps_host || p->iir.n != p0->iir.n)
            return MICLOC_ERR_SHAPE;
    }
    if ((unsigned long long)T * (unsigned long long)p0->M > 0xffffffffull) return MICLOC_ERR_SHAPE;  // (the one-shot loaders index a trial with 32 bits)
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
    if (!plans || !xf || !h || !pre) return MICLOC_ERR_INVALID;
    if (F < 1 || F > MICLOC_MAX_BANDS || bad_batch(B) || bad_batch(F * B) || T < 1) return MICLOC_ERR_INVALID;
    for (int f = 0; f < F; ++f)
        if (!plans[f]) return MICLOC_ERR_INVALID;
    const micloc_plan *p0 = plans[0];
    for (int f = 0; f < F; ++f) {
        const micloc_plan *p = plans[f];
        if (p->device != p0->device || p->M != p0->M || p->L != p0->L || p->taps_host != p0->taps_host || p->iir.n != p0->iir.n) return MICLOC_ERR_SHAPE;
    }
    if (Ts != micloc_padded_T(T) || (unsigned long long)T * (unsigned long long)p0->M > 0xffffffffull) return MICLOC_ERR_SHAPE;
    DeviceGuard guard(p0->device);
    return cbands_front(plans, F, xf, B, T, Ts, h, pre, with_stht != 0, one_launch != 0, (hipStream_t)stream);
}

}  // extern "C"
