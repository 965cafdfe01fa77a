// C-ABI of libmicloc_hip.so (see include/micloc_hip.h for the contract and reference citations): version and last error, the plan, the
// CU-range streams, the stage entries and the one-shot pipelines with their power, window and covariance read-outs.
#include "api_internal.h"

using namespace micloc;

// ---- what the other units take from this one (api_internal.h) -------------------------------------------------------------------
namespace micloc {

thread_local int g_last_hip = 0;

// Frames per row of partial sums of the kernel family beamform_nchunks_ct describes (the general kernel): the largest T that is one chunk.
static int gen_chunk_frames(int CT)
{
    for (int c = 256; c <= 4096; c += 256)
        if (beamform_nchunks_ct(c, CT) == 1 && beamform_nchunks_ct(c + 1, CT) == 2) return c;
    return 0;
}

// The chunk length of the power-only launch that serves this plan and bf_mat: launch_lif_beamform (real bf_mat) or
// launch_planar_beamform with complex output pairs.  The latter takes its bf_mat-stationary kernel (256-frame chunks, the finest
// chunking of any kernel: see beamform_partial_bytes) for one channel tile -- a complex table always has an even number of DoA
// tiles -- and the general kernel otherwise.  window_readout() checks the result against the nchunks the launch reports.
int window_quantum(const micloc_plan *p)
{
    if (!p->W_is_complex) return lif_beamform_chunk_frames(p->W, p->ntab);
    if (p->W.CT == 1 && (p->W.GT & 1) == 0) return 256;
    return gen_chunk_frames(p->W.CT);
}

// The spikes-only encoder launch: the three-slot form of rzcc_sweep.hip where the launch has its shape, rzcc.hip's kernels otherwise
// (same spikes, same scratch either way).
static hipError_t bandpass_rzcc_spikes(const IirCoef &coef, const double *h, int nlanes, int C, int T, int Ts, int robust_width, int bipolar,
                                       int8_t *spikes, void *scratch, hipStream_t stream, const double *xin, int M, int shift,
                                       int chunk_frames, int phases)
{
    hipError_t e = hipSuccess;
    if (launch_bandpass_rzcc_sweep(coef, h, nlanes, C, T, Ts, robust_width, bipolar, spikes, scratch, stream, xin, M, shift, chunk_frames,
                                   phases, &e))
        return e;
    return launch_bandpass_rzcc(coef, h, nlanes, C, T, Ts, robust_width, bipolar, nullptr, spikes, scratch, stream, xin, M, shift,
                                chunk_frames, phases);
}

// ---- the front end of the pipeline entries ---------------------------------------------------------------------------------------
// STHT, then the band-pass stage, into the workspace regions at `o`.  Real bf_mat (cpx false): the raster, in `spikes` when the caller
// wants it, with the plan's encoder chunking and only the launches that `stages` (MICLOC_STAGE_* bits) selects.  Complex: the planar rows.
Front front_end(const micloc_plan *p, bool cpx, const double *x, int B, int T, void *ws, const FrontOffsets &o, int8_t *spikes, int stages,
                hipStream_t st)
{
    Front f{MICLOC_OK, nullptr, micloc_padded_T(T)};
    double *h = ws_doubles(ws, o.h);
    // the in-phase channels are the rolled input frames: the band-pass kernel reads them from x directly
    hipError_t e = (stages & MICLOC_STAGE_STHT) ? launch_stht(p->taps, x, h, B, T, p->M, f.Ts, st, false) : hipSuccess;
    if (cpx) {
        double *pre = ws_doubles(ws, o.pre);
        f.src = pre;
        if (e == hipSuccess)
            e = launch_bandpass_rzcc(p->iir, h, B * p->C, p->C, T, f.Ts, p->robust_width, p->bipolar, pre, nullptr, nullptr, st, x, p->M,
                                     p->taps.shift);
    } else {
        int8_t *spk = spikes ? spikes : static_cast<int8_t *>(ws) + o.spikes;
        f.src = spk;
        const int phases = (stages & MICLOC_STAGE_ENCODE) ? RZ_PHASE_ALL
                                                          : ((stages & MICLOC_STAGE_ENCODE_SCAN) ? RZ_PHASE_SCAN : 0) |
                                                                ((stages & MICLOC_STAGE_ENCODE_REST) ? RZ_PHASE_ENCODE : 0);
        if (e == hipSuccess && phases)
            e = bandpass_rzcc_spikes(p->iir, h, B * p->C, p->C, T, f.Ts, p->robust_width, p->bipolar, spk,
                                     static_cast<char *>(ws) + o.scratch, st, x, p->M, p->taps.shift, p->chunk_frames, phases);
    }
    if (e != hipSuccess) f.rc = hip_failed(e);
    return f;
}

}  // namespace micloc

namespace {

// Uploads a host table.  A table that fits the existing allocation is overwritten in place (device pointer unchanged:
// hipGraphs captured against this plan stay valid IF the caller keeps the table's shape -- set_W / set_neuron_kernel bump
// the generation themselves when the shape changes); otherwise the buffer is re-allocated and *generation is bumped.
int upload(double **dptr, size_t *cap, int *generation, const std::vector<double> &host)
{
    const size_t n = host.empty() ? 1 : host.size();
    if (!*dptr || *cap < n) {
        if (*dptr) {
            HIP_TRY(hipFree(*dptr));
            *dptr = nullptr;
            *cap = 0;
        }
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(dptr), n * sizeof(double)));
        *cap = n;
        ++*generation;
    }
    if (!host.empty()) HIP_TRY(hipMemcpy(*dptr, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
    return MICLOC_OK;
}

int pad_ct(int C)
{
    int ct = (C + 15) / 16;
    if (ct > 4 && ct <= 8) ct = 8;
    return ct;
}

struct WsLayout : FrontOffsets {
    size_t partial, total;
};

WsLayout ws_layout(const micloc_plan *p, int B, int T)
{
    WsLayout w{};
    const size_t Ts = (size_t)micloc_padded_T(T);
    const size_t planar = align256((size_t)B * p->C * Ts * sizeof(double));
    int Gp = p->W.GT > 0 ? 16 * p->W.GT : 16;
    size_t off = 0;
    w.h = off;
    off += planar;
    w.pre = off;
    off += planar;
    w.scratch = off;
    off += rzcc_scratch_bytes(B * p->C, T, p->robust_width, p->chunk_frames);
    w.spikes = off;
    off += align256((size_t)B * T * p->C);
    w.partial = off;
    {
        const size_t pb = beamform_partial_bytes(B, T, Gp);
        const int ct = pad_ct(p->C);
        const size_t pc = ct <= 8 ? cov_partial_bytes(B, T, ct) : 0;
        off += pb > pc ? pb : pc;
    }
    w.total = off;
    return w;
}

// ---- windowed read-out (windows.hip) ----------------------------------------------------------------------------------
// both read-outs of one buffer of partial sums: the windows, and (on request) the ordinary whole-recording power / arg-max
int window_readout(const micloc_plan *p, const double *partial, int B, int T, int nch, int quantum, int window, int hop, double *power_w,
                   int32_t *argmax_w, double *power, int32_t *argmax, hipStream_t st)
{
    if (nch != (T + quantum - 1) / quantum) return MICLOC_ERR_INVALID;  // the launch chose a kernel window_quantum() does not describe
    const int Gp = 16 * p->W.GT, cp = p->W_is_complex ? 1 : 0;
    HIP_TRY(launch_window_power(partial, B, T, nch, Gp, p->G_out, cp, cp ? Gp / 2 : 0, quantum, window, hop, power_w, argmax_w, st));
    if (power || argmax) HIP_TRY(launch_power_argmax(partial, B, T, nch, Gp, p->G_out, cp, cp ? Gp / 2 : 0, power, argmax, st));
    return MICLOC_OK;
}

// The one-shot power launch: the fixed-shape kernel of beamform_lean.hip where the plan and the call have its shape, the general kernels
// otherwise (same bits in `partial` either way).  Windows, streaming, tracking and y stay with launch_lif_beamform.
hipError_t lif_beamform_oneshot(const BeamformW &W, const NeuronTab &nt, const int8_t *spikes, int B, int T, double *y, double *partial,
                                hipStream_t stream, int *nchunks)
{
    hipError_t e = hipSuccess;
    if (launch_lif_beamform_lean(W, nt, spikes, B, T, y, partial, stream, nchunks, &e)) return e;
    return launch_lif_beamform(W, nt, spikes, B, T, y, partial, stream, nchunks);
}

// the kind check of a window entry, then the window rule: the plan's quantum (> 0), or the status (< 0) of the check that failed
int window_check(const micloc_plan *p, bool cpx, int B, int T, int window, int hop)
{
    int rc = plan_kind(p, cpx), nW = 0;
    if (rc != MICLOC_OK) return rc;
    const int q = window_quantum(p);
    rc = window_args(T, window, hop, q, B, &nW);
    return rc == MICLOC_OK ? q : rc;
}

// The rule of the two covariance entries: the neuron kernel always, a real bf_mat only for the power, at most 128 channels.
int cov_check(const micloc_plan *p, bool want_power)
{
    if (!p->d_ntab) return MICLOC_ERR_NOT_SET;
    if (want_power && (!p->d_W || p->W_is_complex)) return p->d_W ? MICLOC_ERR_SHAPE : MICLOC_ERR_NOT_SET;
    return pad_ct(p->C) > 8 ? MICLOC_ERR_SHAPE : MICLOC_OK;
}

// ---- the tails: from Front::src (or a caller's array of that kind) to one read-out; the fourth, track_run, is api_track.hip's ------------
// y and / or power and arg-max; `partial` (the chunk sums) is read only when one of the latter two is wanted
int power_tail(const micloc_plan *p, const void *src, int B, int T, int Ts, double *y, double *power, int32_t *argmax, double *partial,
               hipStream_t st)
{
    const int Gp = 16 * p->W.GT, cpx = p->W_is_complex ? 1 : 0;
    if (!power && !argmax) partial = nullptr;
    int nch = 0;
    if (cpx)
        HIP_TRY(launch_planar_beamform(p->W, static_cast<const double *>(src), B, T, Ts, y, 1, partial, st, &nch));
    else
        HIP_TRY(lif_beamform_oneshot(p->W, p->ntab, static_cast<const int8_t *>(src), B, T, y, partial, st, &nch));
    if (partial) HIP_TRY(launch_power_argmax(partial, B, T, nch, Gp, p->G_out, cpx, cpx ? Gp / 2 : 0, power, argmax, st));
    return MICLOC_OK;
}

// the power-only launch, then both read-outs of its partial sums
int window_tail(const micloc_plan *p, const void *src, int B, int T, int Ts, int quantum, int window, int hop, double *power_w,
                int32_t *argmax_w, double *power, int32_t *argmax, double *partial, hipStream_t st)
{
    int nch = 0;
    if (p->W_is_complex)
        HIP_TRY(launch_planar_beamform(p->W, static_cast<const double *>(src), B, T, Ts, nullptr, 1, partial, st, &nch));
    else
        HIP_TRY(launch_lif_beamform(p->W, p->ntab, static_cast<const int8_t *>(src), B, T, nullptr, partial, st, &nch));
    return window_readout(p, partial, B, T, nch, quantum, window, hop, power_w, argmax_w, power, argmax, st);
}

// membrane covariance of the frames t >= t_start and, on request, the power in its covariance form
int cov_tail(const micloc_plan *p, const int8_t *spikes, int B, int T, int t_start, double *cov, double *power, int32_t *argmax, double *partial,
             hipStream_t st)
{
    const int CT = pad_ct(p->C);
    const bool want_power = power || argmax;
    HIP_TRY(launch_lif_cov(p->ntab, spikes, B, T, p->C, CT, t_start, partial, st));
    HIP_TRY(launch_cov_power(partial, B, T, CT, p->C, T - t_start, want_power ? p->W.Wp : nullptr, want_power ? 16 * p->W.GT : 16,
                             want_power ? p->G_out : 0, cov, power, argmax, st));
    return MICLOC_OK;
}

}  // namespace

extern "C" {

int micloc_abi_version(void) { return MICLOC_ABI_VERSION; }

int micloc_last_hip_error(void) { return g_last_hip; }

const char *micloc_status_string(int status)
{
    switch (status) {
        case MICLOC_OK: return "ok";
        case MICLOC_ERR_INVALID: return "invalid argument";
        case MICLOC_ERR_SHAPE: return "shape mismatch";
        case MICLOC_ERR_WORKSPACE: return "workspace too small or misaligned (256-byte alignment required)";
        case MICLOC_ERR_NOT_SET: return "neuron kernel or beamforming matrix not set on the plan";
        case MICLOC_ERR_HIP: return "HIP runtime error (see micloc_last_hip_error)";
        case MICLOC_ERR_NO_DEVICE: return "no usable HIP device";
        default: return "unknown status";
    }
}

int micloc_padded_T(int T) { return T <= 0 ? 8 : (T + 7) & ~7; }

int micloc_plan_create(const micloc_config *cfg, micloc_plan **out)
{
    if (!cfg || !out) return MICLOC_ERR_INVALID;
    *out = nullptr;
    if (cfg->num_mic <= 0 || cfg->stht_len <= 0 || !cfg->stht_kernel) return MICLOC_ERR_INVALID;
    if (cfg->iir_len < 1 || cfg->iir_len > MICLOC_MAX_IIR || !cfg->iir_b || !cfg->iir_a) return MICLOC_ERR_INVALID;
    if (cfg->iir_a[0] == 0.0 || cfg->robust_width < 1) return MICLOC_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev)
        return MICLOC_ERR_NO_DEVICE;
    {
        // the code objects in this library are gfx950 only
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return MICLOC_ERR_NO_DEVICE;
    }

    micloc_plan *p = new (std::nothrow) micloc_plan();
    if (!p) return MICLOC_ERR_INVALID;
    p->device = cfg->device;
    p->M = cfg->num_mic;
    p->C = 2 * cfg->num_mic;
    p->L = cfg->stht_len;
    p->robust_width = cfg->robust_width;
    p->bipolar = cfg->bipolar ? 1 : 0;
    p->iir.n = cfg->iir_len;
    for (int i = 0; i < MICLOC_MAX_IIR; ++i) {
        p->iir.b[i] = i < cfg->iir_len ? cfg->iir_b[i] / cfg->iir_a[0] : 0.0;
        p->iir.a[i] = i < cfg->iir_len ? cfg->iir_a[i] / cfg->iir_a[0] : 0.0;
    }

    // compact tap table: delays klo, klo + kstep, ... ; exact-zero taps are dropped when every second tap is zero
    const int L = cfg->stht_len;
    int klo = -1, khi = -1;
    for (int k = 0; k < L; ++k)
        if (cfg->stht_kernel[k] != 0.0) {
            if (klo < 0) klo = k;
            khi = k;
        }
    SthtTaps tp{};
    std::vector<double> compact;
    if (klo < 0) {
        tp.klo = 0;
        tp.kstep = 2;
        tp.ngroups = 0;
        compact.assign(4, 0.0);
    } else {
        bool stride2 = true;
        for (int k = klo; k <= khi; ++k)
            if (((k - klo) & 1) && cfg->stht_kernel[k] != 0.0) stride2 = false;
        tp.kstep = stride2 ? 2 : 1;
        tp.klo = klo;
        const int ntaps = (khi - klo) / tp.kstep + 1;
        const int U = STHT_R / tp.kstep;
        tp.ngroups = (ntaps + U - 1) / U;
        compact.assign((size_t)(tp.ngroups + 1) * U, 0.0);  // +1 all-zero group: the kernel prefetches one group ahead
        for (int j = 0; j < ntaps; ++j) compact[j] = cfg->stht_kernel[klo + j * tp.kstep];
    }
    {
        const int U = STHT_R / tp.kstep;
        const int kmax = tp.klo + (tp.ngroups * U > 0 ? (tp.ngroups * U - 1) * tp.kstep : 0);
        tp.halo = tp.klo + STHT_R * ((kmax - tp.klo + STHT_R - 1) / STHT_R);
        tp.shift = L / 2;
    }
    if (stht_lds_bytes(tp, p->M) > 160 * 1024) {
        delete p;
        return MICLOC_ERR_INVALID;  // kernel too long for the LDS-staged tile
    }

    DeviceGuard guard(p->device);
    int rc = upload(&p->d_taps, &p->taps_cap, &p->generation, compact);
    if (rc != MICLOC_OK) {
        delete p;
        return rc;
    }
    tp.taps = p->d_taps;
    p->taps = tp;
    p->taps_host = compact;
    *out = p;
    return MICLOC_OK;
}

void micloc_plan_destroy(micloc_plan *p)
{
    if (!p) return;
    DeviceGuard guard(p->device);
    if (p->d_taps) (void)hipFree(p->d_taps);
    if (p->d_ntab) (void)hipFree(p->d_ntab);
    if (p->d_W) (void)hipFree(p->d_W);
    delete p;
}

int micloc_plan_set_neuron_kernel(micloc_plan *p, const double *nir, int n)
{
    if (!p || !nir || n < 1) return MICLOC_ERR_INVALID;
    const int NK = (n + 15 + 3) / 4;
    if ((size_t)(256 + 4 * NK) * 16 * pad_ct(p->C) > 96 * 1024) return MICLOC_ERR_INVALID;  // the int8 spike tile of a sub-chunk must fit in LDS
    std::vector<double> tab((size_t)4 * NK + 16, 0.0);
    for (int k = 0; k < n; ++k) tab[(size_t)k + 15] = nir[k];
    DeviceGuard guard(p->device);
    // the table may be in use by queued kernels: replace it only after the device went idle
    HIP_TRY(hipDeviceSynchronize());
    int rc = upload(&p->d_ntab, &p->ntab_cap, &p->generation, tab);
    if (rc != MICLOC_OK) return rc;
    if (p->ntab.tab && (p->ntab.n != n || p->ntab.NK != NK)) ++p->generation;  // captured graphs hold n / NK by value
    p->ntab.tab = p->d_ntab;
    p->ntab.n = n;
    p->ntab.NK = NK;
    return MICLOC_OK;
}

static int set_W(micloc_plan *p, const std::vector<double> &Wp, int CT, int GT, int C, int Gcols, int is_complex,
                 int G_out)
{
    DeviceGuard guard(p->device);
    HIP_TRY(hipDeviceSynchronize());
    int rc = upload(&p->d_W, &p->W_cap, &p->generation, Wp);
    if (rc != MICLOC_OK) return rc;
    // same allocation, other shape: a captured graph would read the new table with the old stride and dimensions
    if (p->W.Wp && (p->W.CT != CT || p->W.GT != GT || p->W.C != C || p->W.G != Gcols || p->W_is_complex != is_complex || p->G_out != G_out))
        ++p->generation;
    p->W.Wp = p->d_W;
    p->W.CT = CT;
    p->W.GT = GT;
    p->W.C = C;
    p->W.G = Gcols;
    p->W.complex_pairs = is_complex;
    p->W_is_complex = is_complex;
    p->G_out = G_out;
    return MICLOC_OK;
}

int micloc_plan_set_bf_mat(micloc_plan *p, const double *W, int C, int G)
{
    if (!p || !W || G < 1) return MICLOC_ERR_INVALID;
    if (C != p->C) return MICLOC_ERR_SHAPE;
    const int CT = pad_ct(C);
    if (CT > 8) return MICLOC_ERR_INVALID;
    const int GT = (G + 15) / 16;
    const int Gp = 16 * GT;
    // (+16: the general kernel streams bf_mat in slabs of two DoA tiles and reads a whole slab even when the last one is half empty)
    std::vector<double> Wp((size_t)16 * CT * Gp + 16, 0.0);
    for (int c = 0; c < C; ++c)
        for (int g = 0; g < G; ++g) Wp[(size_t)c * Gp + g] = W[(size_t)c * G + g];
    return set_W(p, Wp, CT, GT, C, G, 0, G);
}

int micloc_plan_set_bf_mat_c128(micloc_plan *p, const double *Wre, const double *Wim, int M, int G)
{
    if (!p || !Wre || !Wim || G < 1) return MICLOC_ERR_INVALID;
    if (M != p->M) return MICLOC_ERR_SHAPE;
    const int C = 2 * M;
    const int CT = pad_ct(C);
    if (CT > 8) return MICLOC_ERR_INVALID;
    const int Ghp = 16 * ((G + 15) / 16);  // Gp / 16 is even by construction
    const int Gp = 2 * Ghp;
    // (hr + j hi)(wr - j wi):  re = [hr hi] . [wr; wi]   im = [hr hi] . [-wi; wr]
    std::vector<double> Wp((size_t)16 * CT * Gp + 16, 0.0);
    for (int m = 0; m < M; ++m)
        for (int g = 0; g < G; ++g) {
            const double wr = Wre[(size_t)m * G + g], wi = Wim[(size_t)m * G + g];
            Wp[(size_t)m * Gp + g] = wr;
            Wp[(size_t)(M + m) * Gp + g] = wi;
            Wp[(size_t)m * Gp + Ghp + g] = -wi;
            Wp[(size_t)(M + m) * Gp + Ghp + g] = wr;
        }
    return set_W(p, Wp, CT, Gp / 16, C, 2 * G, 1, G);
}

int micloc_plan_generation(const micloc_plan *p) { return p ? p->generation : -1; }

// ---- streams restricted to a part of every XCD ------------------------------------------------------------------------
int micloc_stream_create_cu_range(int device, int cu_lo, int cu_hi, void **stream)
{
    if (!stream || device < 0) return MICLOC_ERR_INVALID;
    *stream = nullptr;
    DeviceGuard guard(device);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return MICLOC_ERR_INVALID;
    // gfx950: 8 XCDs; bit i of the mask is compute unit i / 8 of XCD i % 8 (measured: tools/dev/cu_mask_probe.hip), and an XCD
    // whose bits are all clear is NOT excluded -- it runs the stream on all of its compute units -- so a range is given per XCD
    // The layout was measured on the unpartitioned device (SPX: 256 compute units in 8 XCDs) and holds for that only: a partition
    // (CPX: 32 compute units, one XCD) has the same arch name and a mask that means something else -- refuse, callers fall back to
    // ordinary streams (runtime.StreamPipeline / sweep: scan_lane = 0).
    constexpr int NXCD = 8;
    const int ncu = prop.multiProcessorCount;
    if (ncu != 256) return MICLOC_ERR_INVALID;
    const int per = ncu / NXCD;
    if (cu_lo < 0 || cu_hi > per || cu_lo >= cu_hi) return MICLOC_ERR_INVALID;
    std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
    for (int c = cu_lo; c < cu_hi; ++c)
        for (int x = 0; x < NXCD; ++x) {
            const int bit = c * NXCD + x;
            mask[bit / 32] |= 1u << (bit % 32);
        }
    hipStream_t st = nullptr;
    HIP_TRY(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
    *stream = st;
    return MICLOC_OK;
}

int micloc_stream_destroy(void *stream)
{
    if (!stream) return MICLOC_ERR_INVALID;
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_plan_set_encoder_chunk(micloc_plan *p, int chunk_frames)
{
    if (!p) return MICLOC_ERR_INVALID;
    p->chunk_frames = chunk_frames;
    return MICLOC_OK;
}

int micloc_plan_encoder_chunks(const micloc_plan *p, int B, int T)
{
    if (!p || bad_batch(B) || T < 1) return MICLOC_ERR_INVALID;
    return rzcc_chunks(B * p->C, T, p->robust_width, p->chunk_frames);
}

size_t micloc_workspace_bytes(const micloc_plan *p, int B, int T)
{
    if (!p || bad_batch(B) || T < 1) return 0;
    return ws_layout(p, B, T).total;
}

size_t micloc_lif_beamform_workspace_bytes(const micloc_plan *p, int B, int T)
{
    if (!p || bad_batch(B) || T < 1 || p->W.GT < 1) return 0;
    return align256(beamform_partial_bytes(B, T, 16 * p->W.GT));
}

// ---- stages ----------------------------------------------------------------------------------------------
int micloc_stht_f64(const micloc_plan *p, const double *x, int B, int T, double *h, int Ts, void *stream)
{
    if (!p || !x || !h || bad_batch(B) || T < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);  // launches and stream belong to the plan's device, whatever the caller's current one
    if (Ts != micloc_padded_T(T)) return MICLOC_ERR_SHAPE;
    HIP_TRY(launch_stht(p->taps, x, h, B, T, p->M, Ts, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_bandpass_rzcc_f64(const micloc_plan *p, const double *h, int B, int T, int Ts, double *pre,
                             int8_t *spikes, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !h || bad_batch(B) || T < 1 || (!pre && !spikes)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);  // launches and stream belong to the plan's device, whatever the caller's current one
    if (Ts != micloc_padded_T(T)) return MICLOC_ERR_SHAPE;
    const int nl = B * p->C;
    if (spikes && bad_ws(ws, ws_bytes, rzcc_scratch_bytes(nl, T, p->robust_width, p->chunk_frames))) return MICLOC_ERR_WORKSPACE;
    if (spikes && !pre)
        HIP_TRY(bandpass_rzcc_spikes(p->iir, h, nl, p->C, T, Ts, p->robust_width, p->bipolar, spikes, ws, (hipStream_t)stream, nullptr, 0, 0,
                                     p->chunk_frames, RZ_PHASE_ALL));
    else
        HIP_TRY(launch_bandpass_rzcc(p->iir, h, nl, p->C, T, Ts, p->robust_width, p->bipolar, pre, spikes, ws,
                                     (hipStream_t)stream, nullptr, 0, 0, p->chunk_frames));
    return MICLOC_OK;
}

int micloc_lif_beamform_f64(const micloc_plan *p, const int8_t *spikes, int B, int T, double *y, double *power,
                            int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !spikes || bad_batch(B) || T < 1 || (!y && !power && !argmax)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);  // launches and stream belong to the plan's device, whatever the caller's current one
    const int rc = plan_kind(p, false);
    if (rc != MICLOC_OK) return rc;
    if ((power || argmax) && bad_ws(ws, ws_bytes, beamform_partial_bytes(B, T, 16 * p->W.GT))) return MICLOC_ERR_WORKSPACE;
    return power_tail(p, spikes, B, T, 0, y, power, argmax, ws_doubles(ws, 0), (hipStream_t)stream);
}

int micloc_beamform_c128_f64(const micloc_plan *p, const double *pre, int B, int T, int Ts, double *y, double *power,
                             int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !pre || bad_batch(B) || T < 1 || (!y && !power && !argmax)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);  // launches and stream belong to the plan's device, whatever the caller's current one
    if (Ts != micloc_padded_T(T)) return MICLOC_ERR_SHAPE;
    const int rc = plan_kind(p, true);
    if (rc != MICLOC_OK) return rc;
    if ((power || argmax) && bad_ws(ws, ws_bytes, beamform_partial_bytes(B, T, 16 * p->W.GT))) return MICLOC_ERR_WORKSPACE;
    return power_tail(p, pre, B, T, Ts, y, power, argmax, ws_doubles(ws, 0), (hipStream_t)stream);
}

// ---- pipelines -------------------------------------------------------------------------------------------
int micloc_snn_pipeline_f64(const micloc_plan *p, const double *x, int B, int T, int8_t *spikes, double *y,
                            double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    return micloc_snn_pipeline_stages_f64(p, x, B, T, spikes, y, power, argmax, ws, ws_bytes, stream, MICLOC_STAGE_ALL);
}

int micloc_snn_pipeline_stages_f64(const micloc_plan *p, const double *x, int B, int T, int8_t *spikes, double *y,
                                   double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream, int stages)
{
    if (!p || !x || bad_batch(B) || T < 1 || (!spikes && !y && !power && !argmax)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);  // launches and stream belong to the plan's device, whatever the caller's current one
    if (stages <= 0 || (stages & ~(MICLOC_STAGE_ALL | MICLOC_STAGE_ENCODE_SCAN | MICLOC_STAGE_ENCODE_REST))) return MICLOC_ERR_INVALID;
    const bool want_bf = y || power || argmax;  // a call for the raster alone needs no table
    const int rc = want_bf ? plan_kind(p, false) : MICLOC_OK;
    if (rc != MICLOC_OK) return rc;
    const WsLayout w = ws_layout(p, B, T);
    if (bad_ws(ws, ws_bytes, w.total)) return MICLOC_ERR_WORKSPACE;
    const Front f = front_end(p, false, x, B, T, ws, w, spikes, stages, (hipStream_t)stream);
    if (f.rc != MICLOC_OK) return f.rc;
    if (!want_bf || !(stages & MICLOC_STAGE_BEAMFORM)) return MICLOC_OK;
    return power_tail(p, f.src, B, T, f.Ts, y, power, argmax, ws_doubles(ws, w.partial), (hipStream_t)stream);
}

int micloc_beamformer_pipeline_f64(const micloc_plan *p, const double *x, int B, int T, double *y, double *power,
                                   int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !x || bad_batch(B) || T < 1 || (!y && !power && !argmax)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);  // launches and stream belong to the plan's device, whatever the caller's current one
    const int rc = plan_kind(p, true);
    if (rc != MICLOC_OK) return rc;
    const WsLayout w = ws_layout(p, B, T);
    if (bad_ws(ws, ws_bytes, w.total)) return MICLOC_ERR_WORKSPACE;
    const Front f = front_end(p, true, x, B, T, ws, w, nullptr, MICLOC_STAGE_ALL, (hipStream_t)stream);
    if (f.rc != MICLOC_OK) return f.rc;
    return power_tail(p, f.src, B, T, f.Ts, y, power, argmax, ws_doubles(ws, w.partial), (hipStream_t)stream);
}

// ---- time-resolved DoA: power and arg-max per window ------------------------------------------------------------------
int micloc_window_quantum(const micloc_plan *p)
{
    if (!p) return MICLOC_ERR_INVALID;
    if (plan_kind(p, p->W_is_complex) != MICLOC_OK) return MICLOC_ERR_NOT_SET;
    const int q = window_quantum(p);
    return q > 0 ? q : MICLOC_ERR_INVALID;
}

int micloc_window_count(int T, int window, int hop, int quantum)
{
    int nW = 0;
    const int rc = window_args(T, window, hop, quantum, 1, &nW);
    return rc == MICLOC_OK ? nW : rc;
}

size_t micloc_window_workspace_bytes(const micloc_plan *p, int B, int T, int window, int hop, int pipeline)
{
    if (!p || bad_batch(B) || T < 1 || micloc_window_quantum(p) < 1) return 0;
    int nW = 0;
    if (window_args(T, window, hop, window_quantum(p), B, &nW) != MICLOC_OK) return 0;
    return pipeline ? ws_layout(p, B, T).total : align256(beamform_partial_bytes(B, T, 16 * p->W.GT));
}

int micloc_lif_beamform_windows_f64(const micloc_plan *p, const int8_t *spikes, int B, int T, int window, int hop, double *power_w,
                                    int32_t *argmax_w, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !spikes || bad_batch(B) || T < 1 || (!power_w && !argmax_w)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    const int q = window_check(p, false, B, T, window, hop);
    if (q < 0) return q;
    if (bad_ws(ws, ws_bytes, beamform_partial_bytes(B, T, 16 * p->W.GT))) return MICLOC_ERR_WORKSPACE;
    return window_tail(p, spikes, B, T, 0, q, window, hop, power_w, argmax_w, power, argmax, ws_doubles(ws, 0), (hipStream_t)stream);
}

int micloc_beamform_c128_windows_f64(const micloc_plan *p, const double *pre, int B, int T, int Ts, int window, int hop, double *power_w,
                                     int32_t *argmax_w, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !pre || bad_batch(B) || T < 1 || (!power_w && !argmax_w)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    if (Ts != micloc_padded_T(T)) return MICLOC_ERR_SHAPE;
    const int q = window_check(p, true, B, T, window, hop);
    if (q < 0) return q;
    if (bad_ws(ws, ws_bytes, beamform_partial_bytes(B, T, 16 * p->W.GT))) return MICLOC_ERR_WORKSPACE;
    return window_tail(p, pre, B, T, Ts, q, window, hop, power_w, argmax_w, power, argmax, ws_doubles(ws, 0), (hipStream_t)stream);
}

// the launches of micloc_snn_pipeline_f64 up to the raster, then both read-outs of the partial sums
int micloc_snn_pipeline_windows_f64(const micloc_plan *p, const double *x, int B, int T, int window, int hop, int8_t *spikes,
                                    double *power_w, int32_t *argmax_w, double *power, int32_t *argmax, void *ws, size_t ws_bytes,
                                    void *stream)
{
    if (!p || !x || bad_batch(B) || T < 1 || (!power_w && !argmax_w)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    const int q = window_check(p, false, B, T, window, hop);
    if (q < 0) return q;
    const WsLayout w = ws_layout(p, B, T);
    if (bad_ws(ws, ws_bytes, w.total)) return MICLOC_ERR_WORKSPACE;
    const Front f = front_end(p, false, x, B, T, ws, w, spikes, MICLOC_STAGE_ALL, (hipStream_t)stream);
    if (f.rc != MICLOC_OK) return f.rc;
    return window_tail(p, f.src, B, T, f.Ts, q, window, hop, power_w, argmax_w, power, argmax, ws_doubles(ws, w.partial), (hipStream_t)stream);
}

int micloc_beamformer_pipeline_windows_f64(const micloc_plan *p, const double *x, int B, int T, int window, int hop, double *power_w,
                                           int32_t *argmax_w, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !x || bad_batch(B) || T < 1 || (!power_w && !argmax_w)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    const int q = window_check(p, true, B, T, window, hop);
    if (q < 0) return q;
    const WsLayout w = ws_layout(p, B, T);
    if (bad_ws(ws, ws_bytes, w.total)) return MICLOC_ERR_WORKSPACE;
    const Front f = front_end(p, true, x, B, T, ws, w, nullptr, MICLOC_STAGE_ALL, (hipStream_t)stream);
    if (f.rc != MICLOC_OK) return f.rc;
    return window_tail(p, f.src, B, T, f.Ts, q, window, hop, power_w, argmax_w, power, argmax, ws_doubles(ws, w.partial), (hipStream_t)stream);
}

// ---- fp32-MFMA variant of the beamforming tail ---------------------------------------------------------------------
int micloc_lif_beamform_f32(const micloc_plan *p, const int8_t *spikes, int B, int T, double *power, int32_t *argmax,
                            void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !spikes || bad_batch(B) || T < 1 || (!power && !argmax)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);  // launches and stream belong to the plan's device, whatever the caller's current one
    const int rc = plan_kind(p, false);
    if (rc != MICLOC_OK) return rc;
    if (p->W.CT > 4) return MICLOC_ERR_SHAPE;
    const int Gp = 16 * p->W.GT;
    if (bad_ws(ws, ws_bytes, beamform_partial_bytes(B, T, Gp))) return MICLOC_ERR_WORKSPACE;
    double *partial = reinterpret_cast<double *>(ws);
    int nch = 0;
    HIP_TRY(launch_lif_beamform_f32(p->W, p->ntab, spikes, B, T, partial, (hipStream_t)stream, &nch));
    HIP_TRY(launch_power_argmax(partial, B, T, nch, Gp, p->G_out, 0, 0, power, argmax, (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- covariance-form power and membrane covariance ------------------------------------------------------------
int micloc_lif_covariance_f64(const micloc_plan *p, const int8_t *spikes, int B, int T, int t_start, double *cov,
                              double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !spikes || bad_batch(B) || T < 1 || t_start < 0 || t_start >= T || (!cov && !power && !argmax))
        return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);  // launches and stream belong to the plan's device, whatever the caller's current one
    const int rc = cov_check(p, power || argmax);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(ws, ws_bytes, cov_partial_bytes(B, T, pad_ct(p->C)))) return MICLOC_ERR_WORKSPACE;
    return cov_tail(p, spikes, B, T, t_start, cov, power, argmax, ws_doubles(ws, 0), (hipStream_t)stream);
}

int micloc_snn_pipeline_cov_f64(const micloc_plan *p, const double *x, int B, int T, int t_start, int8_t *spikes,
                                double *cov, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !x || bad_batch(B) || T < 1 || t_start < 0 || t_start >= T || (!cov && !power && !argmax))
        return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);  // launches and stream belong to the plan's device, whatever the caller's current one
    const int rc = cov_check(p, power || argmax);
    if (rc != MICLOC_OK) return rc;
    const WsLayout w = ws_layout(p, B, T);
    if (bad_ws(ws, ws_bytes, w.total)) return MICLOC_ERR_WORKSPACE;
    const Front f = front_end(p, false, x, B, T, ws, w, spikes, MICLOC_STAGE_ALL, (hipStream_t)stream);
    if (f.rc != MICLOC_OK) return f.rc;
    return cov_tail(p, static_cast<const int8_t *>(f.src), B, T, t_start, cov, power, argmax, ws_doubles(ws, w.partial), (hipStream_t)stream);
}

}  // extern "C"
