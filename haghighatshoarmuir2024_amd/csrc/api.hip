// C-ABI of libmicloc_hip.so (see include/micloc_hip.h for the contract and reference citations).
#include <math.h>
#include <string.h>

#include <new>
#include <vector>

#include "micloc_internal.h"

using namespace micloc;

static thread_local int g_last_hip = 0;

// (a failed runtime call also leaves its code in HIP's sticky "last error": clear it, or the next, unrelated launch
// check -- hipGetLastError() after a successful launch -- would report it again)
static int hip_failed(hipError_t e)
{
    g_last_hip = (int)e;
    (void)hipGetLastError();
    return MICLOC_ERR_HIP;
}

#define HIP_TRY(expr)                                \
    do {                                             \
        hipError_t _e = (expr);                      \
        if (_e != hipSuccess) return hip_failed(_e); \
    } while (0)

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct micloc_plan {
    int device = 0;
    int M = 0, C = 0, L = 0;
    int robust_width = 1, bipolar = 0;
    IirCoef iir{};
    // STHT taps
    double *d_taps = nullptr;
    SthtTaps taps{};
    std::vector<double> taps_host;  // the compact table as uploaded: two plans run ONE STHT launch only when theirs are the same bits
    // neuron kernel
    double *d_ntab = nullptr;
    NeuronTab ntab{};
    // beamforming matrices
    double *d_W = nullptr;
    BeamformW W{};
    int W_is_complex = 0;
    int G_out = 0;  // DoA grid size seen by the caller
    // bumped whenever a captured hipGraph of this plan becomes stale: a device table was re-allocated (the graph holds the
    // old pointer) or replaced by one of another shape (the graph holds the old dimensions BY VALUE: W.GT / W.G / W.CT,
    // ntab.n / NK are kernel arguments, and the packed bf_mat layout depends on Gp)
    int generation = 0;
    int chunk_frames = 0;  // encoder time chunking: 0 automatic, < 0 off, > 0 owned frames per chunk
    size_t taps_cap = 0, ntab_cap = 0, W_cap = 0;  // allocated doubles
};

namespace {

struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
            changed = hipSetDevice(dev) == hipSuccess;
        }
    }
    ~DeviceGuard()
    {
        if (changed) (void)hipSetDevice(prev);
    }
};

// Device that owns a device pointer (plan-less entry points: their launches belong to the device of their buffers and
// stream, whatever the caller's current device is).  Falls back to the current device for pointers HIP does not know.
int device_of(const void *ptr)
{
    hipPointerAttribute_t at;
    int dev = 0;
    if (ptr && hipPointerGetAttributes(&at, ptr) == hipSuccess) return at.device;
    (void)hipGetLastError();
    (void)hipGetDevice(&dev);
    return dev;
}

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

// where the front end of a pipeline entry (STHT, band-pass / RZCC) keeps its arrays in the caller's workspace
struct FrontOffsets {
    size_t h, pre, scratch, spikes;
};

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

// trials map to gridDim.y / gridDim.z, which HIP limits to 65535
bool bad_batch(int B) { return B < 1 || B > 65535; }

bool bad_ws(const void *ws, size_t have, size_t need)
{
    return ws == nullptr || have < need || (reinterpret_cast<uintptr_t>(ws) & 255) != 0;
}

double *ws_doubles(void *ws, size_t offset) { return reinterpret_cast<double *>(static_cast<unsigned char *>(ws) + offset); }

// ---- windowed read-out (windows.hip) ----------------------------------------------------------------------------------
// Frames per row of partial sums of the kernel family beamform_nchunks_ct describes (the general kernel): the largest T that is one chunk.
int gen_chunk_frames(int CT)
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

// MICLOC_OK and *nW, or the status of the window rule's argument errors
int window_args(int T, int window, int hop, int quantum, int B, int *nW)
{
    if (T < 1 || quantum < 1) return MICLOC_ERR_INVALID;
    if (window < 1 || hop < 1 || window % quantum != 0 || hop % quantum != 0) return MICLOC_ERR_SHAPE;
    const long long n = window_count(T, window, hop);
    if (n * (long long)B > 0x7fffffffll) return MICLOC_ERR_SHAPE;
    *nW = (int)n;
    return MICLOC_OK;
}

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

// The one-shot power launch: the fixed-shape kernel of beamform_lean.hip where the plan and the call have its shape, the general kernels
// otherwise (same bits in `partial` either way).  Windows, streaming, tracking and y stay with launch_lif_beamform.
hipError_t lif_beamform_oneshot(const BeamformW &W, const NeuronTab &nt, const int8_t *spikes, int B, int T, double *y, double *partial,
                                hipStream_t stream, int *nchunks)
{
    hipError_t e = hipSuccess;
    if (launch_lif_beamform_lean(W, nt, spikes, B, T, y, partial, stream, nchunks, &e)) return e;
    return launch_lif_beamform(W, nt, spikes, B, T, y, partial, stream, nchunks);
}

// MICLOC_OK when the plan holds what an entry for a complex / a real bf_mat reads: the matrix of that kind and, for a real one, the neuron kernel
int plan_kind(const micloc_plan *p, bool cpx)
{
    if (!p->d_W || (!cpx && !p->d_ntab)) return MICLOC_ERR_NOT_SET;
    return (p->W_is_complex != 0) == cpx ? MICLOC_OK : MICLOC_ERR_SHAPE;
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

// ---- the front end of the pipeline entries ---------------------------------------------------------------------------------------
struct Front {
    int rc;
    const void *src;  // what the tails below read: the spike raster (real bf_mat) or the planar band-passed rows [B][C][Ts] (complex)
    int Ts;
};

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

// ---- the tails: from Front::src (or a caller's array of that kind) to one read-out; the fourth, track_run, is further down ----------------
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

}  // extern "C"

// ---- wideband: filterbank, one SNN chain per band, band sum (filterbank.hip) ---------------------------------------------------
namespace {

// host [F][n] coefficient rows -> the kernel's table, divided by a[0] as micloc_lfilter_f64 does
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
        const size_t n = ws_layout(plans[f], B, T).total;
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

// the plans' band-pass rows as one table (already divided by a[0] at plan creation)
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

extern "C" {

// ---- wideband streaming: filterbank state carry (filterbank.hip), band sum per tile (stream_bands.hip) ------------------------------
size_t micloc_filterbank_stream_state_bytes(int F, int n, int B, int M)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || n < 1 || n > MICLOC_MAX_IIR || B < 1 || M < 1) return 0;
    return filterbank_stream_state_bytes(F, n, B, M);
}

int micloc_filterbank_stream_reset(void *fb_state, size_t bytes, void *stream)
{
    if (!fb_state) return MICLOC_ERR_INVALID;
    if (bad_ws(fb_state, bytes, 256)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(fb_state));
    HIP_TRY(launch_zero_fill(fb_state, bytes, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_filterbank_tile_f64(const double *b, const double *a, int F, int n, const double *x_tile, int B, int n_frames, int M, void *fb_state,
                               size_t fb_bytes, double *xf_tile, void *stream)
{
    FilterbankCoef co;
    const int rc = filterbank_coef(b, a, F, n, &co);
    if (rc != MICLOC_OK) return rc;
    if (!x_tile || !xf_tile || !fb_state || B < 1 || n_frames < 1 || M < 1) return MICLOC_ERR_INVALID;
    if (bad_ws(fb_state, fb_bytes, filterbank_stream_state_bytes(F, n, B, M))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(xf_tile));
    HIP_TRY(launch_filterbank_tile(co, x_tile, F, B, n_frames, M, xf_tile, reinterpret_cast<double *>(fb_state), (hipStream_t)stream));
    return MICLOC_OK;
}

size_t micloc_stream_bands_state_bytes(void) { return STREAM_BANDS_STATE_BYTES; }

int micloc_stream_bands_reset(void *bands_state, size_t bytes, void *stream)
{
    if (!bands_state) return MICLOC_ERR_INVALID;
    if (bad_ws(bands_state, bytes, STREAM_BANDS_STATE_BYTES)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(bands_state));
    HIP_TRY(launch_zero_fill(bands_state, STREAM_BANDS_STATE_BYTES, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_band_sum_f64(int F, int B, int G, const double *const *band_power, int window, int Kb, int max_windows,
                               const double *const *band_window_power, const int32_t *const *band_window_count, void *bands_state,
                               size_t bands_bytes, double *power, int32_t *argmax, double *window_power, int32_t *window_argmax,
                               double *latest_power, int32_t *latest_argmax, void *stream)
{
    if (!band_power || !bands_state || (!power && !argmax) || F < 1 || F > MICLOC_MAX_BANDS || bad_batch(B) || G < 1 || window < 0)
        return MICLOC_ERR_INVALID;
    if (window > 0 && (!band_window_power || !band_window_count || !window_argmax || max_windows < 1 || Kb < 1)) return MICLOC_ERR_INVALID;
    StreamBandsArgs args{};
    for (int f = 0; f < F; ++f) {
        if (!band_power[f]) return MICLOC_ERR_INVALID;
        args.power[f] = band_power[f];
        if (window > 0) {
            if (!band_window_power[f] || !band_window_count[f]) return MICLOC_ERR_INVALID;
            args.rows[f] = band_window_power[f];
            args.count[f] = band_window_count[f];
        }
    }
    if (bad_ws(bands_state, bands_bytes, STREAM_BANDS_STATE_BYTES)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(bands_state));
    HIP_TRY(launch_stream_band_sum(args, F, B, G, window > 0, Kb, max_windows, bands_state, power, argmax, window_power, window_argmax, latest_power,
                                   latest_argmax, (hipStream_t)stream));
    return MICLOC_OK;
}

/* status[0] = wideband windows emitted (or given up) so far, [1] = windows given up because a band's ring had overwritten them
 * (synchronises the stream) */
int micloc_stream_bands_status(const void *bands_state, int *status2, void *stream)
{
    if (!bands_state || !status2) return MICLOC_ERR_INVALID;
    int w[2];
    HIP_TRY(hipMemcpyAsync(w, bands_state, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status2[0] = w[0];
    status2[1] = w[1];
    return MICLOC_OK;
}

// ---- moving-target tracking: per-step arg-max of the envelope of the beamformer output (track.hip) ---------------------
}  // extern "C"

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

// ---- streaming: the band-pass / RZCC stage tile by tile, exact state hand-off -----------------------------------
size_t micloc_stream_state_bytes(const micloc_plan *p, int B)
{
    if (!p || bad_batch(B)) return 0;
    return rzcc_stream_state_bytes(B * p->C);
}

int micloc_stream_overflow(const void *state, int *count, void *stream)
{
    if (!state || !count) return MICLOC_ERR_INVALID;
    HIP_TRY(hipMemcpyAsync(count, state, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return MICLOC_OK;
}

// ---- streaming localisation: LIF + beamforming + power as the spikes become final ---------------------------------------------
// loc_state: [256 B: 64 control ints][acc: B x 2 x G doubles]
size_t micloc_stream_localize_state_bytes(const micloc_plan *p, int B)
{
    if (!p || bad_batch(B) || p->G_out < 1) return 0;
    return 256 + align256((size_t)B * 2 * p->G_out * sizeof(double));
}

int micloc_stream_chunk_frames(const micloc_plan *p)
{
    if (!p || !p->d_ntab || !p->d_W) return MICLOC_ERR_NOT_SET;
    return lif_beamform_chunk_frames(p->W, p->ntab);
}

size_t micloc_stream_localize_workspace_bytes(const micloc_plan *p, int B, int window_frames)
{
    if (!p || bad_batch(B) || window_frames < 1 || p->W.GT < 1) return 0;
    return align256(beamform_partial_bytes(B, window_frames, 16 * p->W.GT));
}

// ---- clocked streaming: the same stages with the absolute time in a device word ----------------------------------------------
// One tile = begin_tile (clock + window slide) -> STHT of [history | tile] (micloc_stht_f64) -> wrap_rows -> encode_tile ->
// localize_tile (which ends with the clock's tick).  No call takes an absolute time: every launch of a tile of n frames has the
// same arguments, so the sequence can be captured into ONE hipGraph and replayed per tile (StreamingLocalizer.capture).
int micloc_stream_reset(const micloc_plan *p, int B, void *enc_state, size_t enc_bytes, void *loc_state, size_t loc_bytes, int8_t *window,
                        int window_frames, void *stream)
{
    if (!p || !enc_state || !loc_state || !window || bad_batch(B) || window_frames < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    if (bad_ws(enc_state, enc_bytes, rzcc_stream_state_bytes(B * p->C))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(loc_state, loc_bytes, micloc_stream_localize_state_bytes(p, B))) return MICLOC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_zero_fill(enc_state, 256, st));  // overflow counter (the encoder's own state is written by the first tile)
    HIP_TRY(launch_zero_fill(loc_state, micloc_stream_localize_state_bytes(p, B), st));  // control words, clock, accumulators
    HIP_TRY(launch_zero_fill(window, (size_t)B * window_frames * p->C, st));
    return MICLOC_OK;
}

int micloc_stream_begin_tile(const micloc_plan *p, void *loc_state, int8_t *window, int8_t *scratch_window, int B, int n, int window_frames,
                             void *stream)
{
    if (!p || !loc_state || !window || !scratch_window || window == scratch_window || bad_batch(B) || n < 1 || window_frames < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    if (!p->d_ntab || !p->d_W) return MICLOC_ERR_NOT_SET;
    const int CH = lif_beamform_chunk_frames(p->W, p->ntab);
    if (window_frames % CH != 0 || n > window_frames) return MICLOC_ERR_SHAPE;
    HIP_TRY(launch_stream_begin_tile(reinterpret_cast<int *>(loc_state), window, scratch_window, B, (size_t)window_frames * p->C, p->C, n, window_frames,
                                     CH, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_wrap_rows_f64(const micloc_plan *p, const void *loc_state, double *h, int B, int Ts, int first_col, int n, const double *wrap_tail,
                                void *stream)
{
    if (!p || !loc_state || !h || bad_batch(B) || n < 1 || first_col < 0 || first_col + n > Ts) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    HIP_TRY(launch_stht_wrap_rows(h, wrap_tail, B, p->M, Ts, first_col, n, p->L / 2, reinterpret_cast<const int *>(loc_state), (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_encode_tile_f64(const micloc_plan *p, const double *h, int B, int T_tile, int row_stride, int final_tile, int8_t *window,
                                  int window_frames, void *enc_state, size_t enc_bytes, const void *loc_state, void *stream)
{
    if (!p || !h || !window || !loc_state || bad_batch(B) || T_tile < 1 || window_frames < T_tile || row_stride < T_tile) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    if (!final_tile && T_tile % 16 != 0) return MICLOC_ERR_SHAPE;
    if (bad_ws(enc_state, enc_bytes, rzcc_stream_state_bytes(B * p->C))) return MICLOC_ERR_WORKSPACE;
    HIP_TRY(launch_stream_encode(p->iir, h, B * p->C, p->C, T_tile, row_stride, p->robust_width, p->bipolar, window, window_frames, 0, 0,
                                 final_tile, enc_state, (hipStream_t)stream, 0, reinterpret_cast<const int *>(loc_state)));
    return MICLOC_OK;
}

// ---- the localize step of a tile, with or without the streaming windows: the time-resolved read-out of the same chunk rows, emitted
// while the recording arrives ----------------------------------------------------------------------------------------------------
// win_state: [256 B: int windows emitted][B][ceil(window / hop)][2][G] doubles (stream_windows.hip), for the SNN stream and the complex one
namespace {

// MICLOC_OK and *CH, or the status of a plan that cannot serve the SNN stream's localize step (p non-NULL)
int stream_plan_args(const micloc_plan *p, int *CH)
{
    *CH = 0;
    if (!p->d_ntab || !p->d_W) return MICLOC_ERR_NOT_SET;
    if (p->W_is_complex) return MICLOC_ERR_SHAPE;
    *CH = lif_beamform_chunk_frames(p->W, p->ntab);
    return MICLOC_OK;
}

// the window-argument rule of both streams; rc: the status of the stream's own plan check, which gave the chunk length *CH (read only
// behind rc == MICLOC_OK, so the check may be an argument of the same call)
int stream_window_args(int rc, int window, int hop, int max_windows, const int *CH)
{
    if (window < 1 || hop < 1 || max_windows < 1) return MICLOC_ERR_INVALID;
    if (rc != MICLOC_OK) return rc;
    if (window % *CH != 0 || hop % *CH != 0 || hop > window) return MICLOC_ERR_SHAPE;
    return MICLOC_OK;
}

// the tail of both *_window_reset entries; rc: stream_window_args' status
int stream_window_zero(int rc, const micloc_plan *p, int B, void *win_state, size_t win_bytes, int window, int hop, void *stream)
{
    if (rc != MICLOC_OK) return rc;
    const size_t need = stream_window_state_bytes(B, p->G_out, window, hop);
    if (bad_ws(win_state, win_bytes, need)) return MICLOC_ERR_WORKSPACE;
    HIP_TRY(launch_zero_fill(win_state, need, (hipStream_t)stream));
    return MICLOC_OK;
}

// the launches of a tile behind the encoder: horizon, LIF + beamforming of the chunks that became final, accumulation, (the window
// read-out in front of the commit,) commit, tick.  win_state == nullptr: no read-out; loc_state, power and argmax end with the same bits
// either way.
int stream_localize(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *raster, int B, int window_frames,
                    int final_tile, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *win_state, size_t win_bytes, int window,
                    int hop, int max_windows, double *window_power, int32_t *window_argmax, double *latest_power, int32_t *latest_argmax,
                    void *stream)
{
    if (!p || !enc_state || !loc_state || !raster || bad_batch(B) || window_frames < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    int CH;
    int rc = stream_plan_args(p, &CH);
    if (win_state) rc = stream_window_args(rc, window, hop, max_windows, &CH);
    if (rc != MICLOC_OK) return rc;
    if (window_frames % CH != 0) return MICLOC_ERR_SHAPE;
    const int G = p->G_out, Gp = 16 * p->W.GT;
    if (bad_ws(loc_state, loc_bytes, micloc_stream_localize_state_bytes(p, B))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, beamform_partial_bytes(B, window_frames, Gp))) return MICLOC_ERR_WORKSPACE;
    if (win_state && bad_ws(win_state, win_bytes, stream_window_state_bytes(B, G, window, hop))) return MICLOC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int *ctl = reinterpret_cast<int *>(loc_state);
    double *acc = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(loc_state) + 256);
    const int nwin = window_frames / CH;
    HIP_TRY(launch_stream_horizon(enc_state, B * p->C, p->bipolar, 0, final_tile ? 1 : 0, CH, 0, nwin, ctl, st, 1));
    BeamformW W = p->W;
    W.chunk_range = ctl + 4;
    double *partial = reinterpret_cast<double *>(ws);
    int nch = 0;
    // the whole window as the launch shape; the kernel takes the frames that exist from the control words
    HIP_TRY(launch_lif_beamform(W, p->ntab, raster, B, window_frames, nullptr, partial, st, &nch));
    HIP_TRY(launch_stream_accumulate(partial, B, nch, Gp, G, ctl + 4, ctl, acc, ctl + 8, power, argmax, st));
    if (win_state)
        HIP_TRY(launch_stream_windows(partial, B, nch, Gp, G, 0, 0, CH, ctl, final_tile ? 1 : 0, window, hop, max_windows, win_state, window_power,
                                      window_argmax, latest_power, latest_argmax, st));
    HIP_TRY(launch_stream_commit(ctl, STREAM_BLOCK_CHUNKS, st));
    HIP_TRY(launch_stream_tick(ctl, st));
    return MICLOC_OK;
}

}  // namespace

int micloc_stream_localize_tile_f64(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window, int B,
                                    int window_frames, int final_tile, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    return stream_localize(p, enc_state, loc_state, loc_bytes, window, B, window_frames, final_tile, power, argmax, ws, ws_bytes, nullptr, 0, 0, 0, 0,
                           nullptr, nullptr, nullptr, nullptr, stream);
}

size_t micloc_stream_window_state_bytes(const micloc_plan *p, int B, int window, int hop, int max_windows)
{
    int CH;
    if (!p || bad_batch(B) || p->G_out < 1 || stream_window_args(stream_plan_args(p, &CH), window, hop, max_windows, &CH) != MICLOC_OK) return 0;
    return stream_window_state_bytes(B, p->G_out, window, hop);
}

int micloc_stream_window_reset(const micloc_plan *p, int B, void *win_state, size_t win_bytes, int window, int hop, int max_windows, void *stream)
{
    if (!p || !win_state || bad_batch(B)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    int CH;
    const int rc = stream_plan_args(p, &CH);
    return stream_window_zero(stream_window_args(rc, window, hop, max_windows, &CH), p, B, win_state, win_bytes, window, hop, stream);
}

int micloc_stream_localize_tile_windows_f64(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window_raster,
                                            int B, int window_frames, int final_tile, double *power, int32_t *argmax, void *ws, size_t ws_bytes,
                                            void *win_state, size_t win_bytes, int window, int hop, int max_windows, double *window_power,
                                            int32_t *window_argmax, double *latest_power, int32_t *latest_argmax, void *stream)
{
    if (!win_state || !window_argmax) return MICLOC_ERR_INVALID;
    return stream_localize(p, enc_state, loc_state, loc_bytes, window_raster, B, window_frames, final_tile, power, argmax, ws, ws_bytes, win_state,
                           win_bytes, window, hop, max_windows, window_power, window_argmax, latest_power, latest_argmax, stream);
}

/* windows emitted so far (synchronises the stream) */
int micloc_stream_window_count(const void *win_state, int *count, void *stream)
{
    if (!win_state || !count) return MICLOC_ERR_INVALID;
    HIP_TRY(hipMemcpyAsync(count, win_state, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return MICLOC_OK;
}

/* device address of the count word micloc_stream_window_count reads (for kernels that follow a band's windows: stream_bands.hip) */
const int32_t *micloc_stream_window_count_ptr(const void *win_state) { return reinterpret_cast<const int32_t *>(win_state); }

/* status[0] = chunks beamformed, [1] = frames beamformed, [2] = window-lag failures, [3] = chunks in the open reduction block
 * (synchronises the stream) */
int micloc_stream_localize_status(const void *loc_state, int *status4, void *stream)
{
    if (!loc_state || !status4) return MICLOC_ERR_INVALID;
    int ctl[16];
    HIP_TRY(hipMemcpyAsync(ctl, loc_state, sizeof(ctl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status4[0] = ctl[0];
    status4[1] = ctl[8];
    status4[2] = ctl[13];
    status4[3] = ctl[1];
    return MICLOC_OK;
}

// ---- streaming, complex Beamformer (stream_complex.hip; the rule: include/micloc_hip.h) ------------------------------------------------
// state: [256 B control words][DF2T words][carry][acc] (stream_complex_layout); ws: [staging [B][2M][Ks CH]][partial [B][Ks][Gp]]
namespace {

struct ScArgs {
    int CH, Ks, S, Gp;
    StreamComplexLayout L;
    size_t ws_partial, ws_total;
};

// MICLOC_OK and *a, or the status of the rule's argument errors (p non-NULL, B checked)
int sc_args(const micloc_plan *p, int B, int max_tile, ScArgs *a)
{
    *a = ScArgs{};
    if (!p->d_W) return MICLOC_ERR_NOT_SET;
    if (!p->W_is_complex) return MICLOC_ERR_SHAPE;
    const int CH = window_quantum(p);
    if (CH < 1) return MICLOC_ERR_INVALID;
    a->CH = CH;
    a->Gp = 16 * p->W.GT;
    a->L = stream_complex_layout(B, p->C, p->G_out, p->iir.n, CH);
    if (max_tile > 0) {
        if ((long long)max_tile + 2ll * CH > 0x7fffffffll) return MICLOC_ERR_SHAPE;
        a->Ks = stream_complex_chunks(max_tile, CH);
        a->S = a->Ks * CH;
        a->ws_partial = align256((size_t)B * p->C * a->S * sizeof(double));
        a->ws_total = a->ws_partial + align256(beamform_partial_bytes(B, a->S, a->Gp));
    }
    return MICLOC_OK;
}

// the launches behind the band-pass of a tile: contraction, accumulation, (windows,) slide + commit -- one chain on one stream
int sc_localize(const micloc_plan *p, const ScArgs &a, void *state, int B, int final_tile, double *power, int32_t *argmax, void *ws,
                void *win_state, int window, int hop, int max_windows, double *window_power, int32_t *window_argmax, double *latest_power,
                int32_t *latest_argmax, hipStream_t st)
{
    double *staging = reinterpret_cast<double *>(ws);
    double *partial = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(ws) + a.ws_partial);
    int nch = 0;
    // the staging array as a recording of Ks whole chunks: the launch shape depends on max_tile only; the rows past the valid ones are never read
    HIP_TRY(launch_planar_beamform(p->W, staging, B, a.S, a.S, nullptr, 1, partial, st, &nch));
    if (nch != a.Ks) return MICLOC_ERR_INVALID;  // the launch chose a kernel window_quantum() does not describe
    HIP_TRY(launch_stream_complex_accumulate(partial, B, a.Ks, a.Gp, p->G_out, a.CH, final_tile, state, a.L, power, argmax, st));
    if (win_state)
        HIP_TRY(launch_stream_windows(partial, B, a.Ks, a.Gp, p->G_out, 1, a.Gp / 2, a.CH, reinterpret_cast<const int *>(state), final_tile ? 1 : 0,
                                      window, hop, max_windows, win_state, window_power, window_argmax, latest_power, latest_argmax, st));
    HIP_TRY(launch_stream_complex_slide(staging, B * p->C, a.S, a.CH, state, a.L, st));
    return MICLOC_OK;
}

}  // namespace

size_t micloc_stream_complex_state_bytes(const micloc_plan *p, int B)
{
    ScArgs a;
    if (!p || bad_batch(B) || sc_args(p, B, 0, &a) != MICLOC_OK) return 0;
    return a.L.total;
}

size_t micloc_stream_complex_workspace_bytes(const micloc_plan *p, int B, int max_tile)
{
    ScArgs a;
    if (!p || bad_batch(B) || max_tile < 1 || sc_args(p, B, max_tile, &a) != MICLOC_OK) return 0;
    return a.ws_total;
}

int micloc_stream_complex_reset(const micloc_plan *p, int B, void *state, size_t state_bytes, void *stream)
{
    if (!p || !state || bad_batch(B)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    const int rc = sc_args(p, B, 0, &a);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, a.L.total)) return MICLOC_ERR_WORKSPACE;
    HIP_TRY(launch_zero_fill(state, a.L.total, (hipStream_t)stream));  // clock, zero DF2T state (lfilter's), empty carry, accumulators
    return MICLOC_OK;
}

int micloc_stream_complex_bandpass_tile_f64(const micloc_plan *p, const double *h, int B, int n, int row_stride, int first_col, int max_tile,
                                            void *state, size_t state_bytes, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !h || !state || !ws || bad_batch(B) || n < 1 || max_tile < 1 || first_col < 0 || row_stride < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    const int rc = sc_args(p, B, max_tile, &a);
    if (rc != MICLOC_OK) return rc;
    if (n > max_tile || (long long)first_col + n > row_stride) return MICLOC_ERR_SHAPE;
    if (bad_ws(state, state_bytes, a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, a.ws_total)) return MICLOC_ERR_WORKSPACE;
    HIP_TRY(launch_stream_complex_bandpass(p->iir, h + first_col, B * p->C, n, (size_t)row_stride, reinterpret_cast<double *>(ws), a.S, a.CH,
                                           state, a.L, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_complex_localize_tile_f64(const micloc_plan *p, void *state, size_t state_bytes, int B, int max_tile, int final_tile,
                                            double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !state || !ws || bad_batch(B) || max_tile < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    const int rc = sc_args(p, B, max_tile, &a);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, a.ws_total)) return MICLOC_ERR_WORKSPACE;
    return sc_localize(p, a, state, B, final_tile, power, argmax, ws, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

size_t micloc_stream_complex_window_state_bytes(const micloc_plan *p, int B, int window, int hop, int max_windows)
{
    ScArgs a;
    if (!p || bad_batch(B) || stream_window_args(sc_args(p, B, 0, &a), window, hop, max_windows, &a.CH) != MICLOC_OK) return 0;
    return stream_window_state_bytes(B, p->G_out, window, hop);
}

int micloc_stream_complex_window_reset(const micloc_plan *p, int B, void *win_state, size_t win_bytes, int window, int hop, int max_windows,
                                       void *stream)
{
    if (!p || !win_state || bad_batch(B)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    const int rc = sc_args(p, B, 0, &a);
    return stream_window_zero(stream_window_args(rc, window, hop, max_windows, &a.CH), p, B, win_state, win_bytes, window, hop, stream);
}

int micloc_stream_complex_localize_tile_windows_f64(const micloc_plan *p, void *state, size_t state_bytes, int B, int max_tile, int final_tile,
                                                    double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *win_state, size_t win_bytes,
                                                    int window, int hop, int max_windows, double *window_power, int32_t *window_argmax,
                                                    double *latest_power, int32_t *latest_argmax, void *stream)
{
    if (!p || !state || !ws || !win_state || !window_argmax || bad_batch(B) || max_tile < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    const int rc = stream_window_args(sc_args(p, B, max_tile, &a), window, hop, max_windows, &a.CH);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, a.ws_total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(win_state, win_bytes, stream_window_state_bytes(B, p->G_out, window, hop))) return MICLOC_ERR_WORKSPACE;
    return sc_localize(p, a, state, B, final_tile, power, argmax, ws, win_state, window, hop, max_windows, window_power, window_argmax,
                       latest_power, latest_argmax, (hipStream_t)stream);
}

/* status[0] = chunks contracted, [1] = frames contracted, [2] = carry fill, [3] = frames pushed (synchronises the stream) */
int micloc_stream_complex_status(const void *state, int *status4, void *stream)
{
    if (!state || !status4) return MICLOC_ERR_INVALID;
    int ctl[STREAM_CLK_T + 1];
    HIP_TRY(hipMemcpyAsync(ctl, state, sizeof(ctl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status4[0] = ctl[0];
    status4[1] = ctl[8];
    status4[2] = ctl[2];
    status4[3] = ctl[STREAM_CLK_T];
    return MICLOC_OK;
}

// ---- wideband streaming, complex Beamformer (stream_bands_complex.hip; the rule: include/micloc_hip.h) ----------------------------------
// The complex stream above for F * B rows.  state: stream_complex_layout(F * B); ws: [staging [F B][2M][Ks CH]][partial [F B][Ks][Gp]]
// [running band power [F B][G]]; win_state: [the window state of F * B rows, the band sum's words at byte SCB_BANDS_WORDS of its 256-B head][band ring [F B][Kb][G]]
}  // extern "C"

namespace {

struct ScbArgs {
    ScArgs a;  // the complex stream's arguments for F * B rows
    int FB;
    size_t ws_band_power, ws_total;
    // windows (scb_window_args)
    int Kb;
    size_t win_ring, win_total;
};

// the window kernel keeps its count in int word 0 of win_state's 256-B head and touches no other word of it: the band sum's four words
// {emitted, given up, pending emitted, pending given up} live further on in the same head, zero-filled with it
constexpr size_t SCB_BANDS_WORDS = 64;

// argument checks of the wideband complex stream in the header's order (max_tile == 0: the state's layout only)
int scb_args(const micloc_plan *const *plans, int F, int B, int max_tile, ScbArgs *s)
{
    *s = ScbArgs{};
    if (!plans || F < 1 || F > MICLOC_MAX_BANDS || bad_batch(B) || bad_batch(F * B) || max_tile < 0) return MICLOC_ERR_INVALID;
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
    s->FB = F * B;
    const int rc = sc_args(p0, s->FB, max_tile, &s->a);  // (one chunk length: it depends on CT and GT only, which the plans share)
    if (rc != MICLOC_OK) return rc;
    s->ws_band_power = s->a.ws_total;
    s->ws_total = s->a.ws_total + align256((size_t)s->FB * p0->G_out * sizeof(double));
    return MICLOC_OK;
}

// the window rule of the streams, then the layout of win_state; rc: scb_args' status with max_tile >= 1
int scb_window_args(int rc, const micloc_plan *const *plans, int window, int hop, int max_windows, ScbArgs *s)
{
    rc = stream_window_args(rc, window, hop, max_windows, &s->a.CH);
    if (rc != MICLOC_OK) return rc;
    s->Kb = stream_bands_ring_depth(s->a.Ks, hop / s->a.CH);
    s->win_ring = stream_window_state_bytes(s->FB, plans[0]->G_out, window, hop);
    s->win_total = s->win_ring + align256((size_t)s->FB * s->Kb * plans[0]->G_out * sizeof(double));
    return MICLOC_OK;
}

// the launches behind the band-pass of a tile: contraction per band, accumulation, (windows,) slide + commit over the F * B rows, band sum
int scb_localize(const micloc_plan *const *plans, int F, int B, const ScbArgs &s, void *state, int final_tile, double *band_power, double *power,
                 int32_t *argmax, void *ws, void *win_state, int window, int hop, int max_windows, double *window_power, int32_t *window_argmax,
                 double *latest_power, int32_t *latest_argmax, hipStream_t st)
{
    const micloc_plan *p0 = plans[0];
    const ScArgs &a = s.a;
    const int G = p0->G_out;
    double *staging = ws_doubles(ws, 0), *partial = ws_doubles(ws, a.ws_partial);
    double *bp = band_power ? band_power : ws_doubles(ws, s.ws_band_power);
    // per band the contraction of 4.16's tile (that band's bf_mat) on its B rows of the one staging array, into one array of chunk rows
    const size_t band_rows = (size_t)B * p0->C * a.S, band_partial = (size_t)B * a.Ks * a.Gp;
    for (int f = 0; f < F; ++f) {
        int nch = 0;
        HIP_TRY(launch_planar_beamform(plans[f]->W, staging + f * band_rows, B, a.S, a.S, nullptr, 1, partial + f * band_partial, st, &nch));
        if (nch != a.Ks) return MICLOC_ERR_INVALID;  // the launch chose a kernel window_quantum() does not describe
    }
    HIP_TRY(launch_stream_complex_accumulate(partial, s.FB, a.Ks, a.Gp, G, a.CH, final_tile, state, a.L, bp, nullptr, st));
    unsigned char *wbase = reinterpret_cast<unsigned char *>(win_state);
    double *ring = win_state ? reinterpret_cast<double *>(wbase + s.win_ring) : nullptr;
    if (win_state)  // every band's windows into its rows of the ring, window n in row n % Kb; the one count word serves all bands
        HIP_TRY(launch_stream_windows(partial, s.FB, a.Ks, a.Gp, G, 1, a.Gp / 2, a.CH, reinterpret_cast<const int *>(state), final_tile ? 1 : 0, window,
                                      hop, s.Kb, win_state, ring, nullptr, nullptr, nullptr, st));
    HIP_TRY(launch_stream_complex_slide(staging, s.FB * p0->C, a.S, a.CH, state, a.L, st));
    StreamBandsArgs args{};
    for (int f = 0; f < F; ++f) {
        args.power[f] = bp + (size_t)f * B * G;
        if (win_state) {
            args.rows[f] = ring + (size_t)f * B * s.Kb * G;
            args.count[f] = reinterpret_cast<const int32_t *>(win_state);
        }
    }
    // (without windows the band sum reads no word of its state: the stream's own stands in for the non-NULL pointer the launcher wants)
    HIP_TRY(launch_stream_band_sum(args, F, B, G, win_state != nullptr, s.Kb, max_windows, win_state ? (void *)(wbase + SCB_BANDS_WORDS) : state, power,
                                   argmax, window_power, window_argmax, latest_power, latest_argmax, st));
    return MICLOC_OK;
}

}  // namespace

extern "C" {

size_t micloc_stream_complex_bands_state_bytes(const micloc_plan *const *plans, int F, int B)
{
    ScbArgs s;
    return scb_args(plans, F, B, 0, &s) == MICLOC_OK ? s.a.L.total : 0;
}

size_t micloc_stream_complex_bands_workspace_bytes(const micloc_plan *const *plans, int F, int B, int max_tile)
{
    ScbArgs s;
    if (max_tile < 1 || scb_args(plans, F, B, max_tile, &s) != MICLOC_OK) return 0;
    return s.ws_total;
}

int micloc_stream_complex_bands_reset(const micloc_plan *const *plans, int F, int B, void *state, size_t state_bytes, void *stream)
{
    if (!plans || !state) return MICLOC_ERR_INVALID;
    ScbArgs s;
    const int rc = scb_args(plans, F, B, 0, &s);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, s.a.L.total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(plans[0]->device);
    HIP_TRY(launch_zero_fill(state, s.a.L.total, (hipStream_t)stream));  // clock, zero DF2T state, empty carry, accumulators
    return MICLOC_OK;
}

int micloc_stream_complex_bands_bandpass_tile_f64(const micloc_plan *const *plans, int F, const double *h, int B, int n, int row_stride,
                                                  int first_col, int max_tile, int chains_per_workgroup, void *state, size_t state_bytes, void *ws,
                                                  size_t ws_bytes, void *stream)
{
    if (!plans || !h || !state || !ws || n < 1 || max_tile < 1 || first_col < 0 || row_stride < 1) return MICLOC_ERR_INVALID;
    if (chains_per_workgroup != 0 && chains_per_workgroup != 16 && chains_per_workgroup != 32 && chains_per_workgroup != 64) return MICLOC_ERR_INVALID;
    ScbArgs s;
    const int rc = scb_args(plans, F, B, max_tile, &s);
    if (rc != MICLOC_OK) return rc;
    if (n > max_tile || (long long)first_col + n > row_stride) return MICLOC_ERR_SHAPE;
    if (bad_ws(state, state_bytes, s.a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, s.ws_total)) return MICLOC_ERR_WORKSPACE;
    const micloc_plan *p0 = plans[0];
    DeviceGuard guard(p0->device);
    FilterbankCoef pc;
    cbands_coef(plans, F, &pc);
    HIP_TRY(launch_stream_bands_bandpass(pc, h + first_col, F, B * p0->C, n, (size_t)row_stride, ws_doubles(ws, 0), s.a.S, s.a.CH, state, s.a.L,
                                         chains_per_workgroup, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_complex_bands_localize_tile_f64(const micloc_plan *const *plans, int F, void *state, size_t state_bytes, int B, int max_tile,
                                                  int final_tile, double *band_power, double *power, int32_t *argmax, void *ws, size_t ws_bytes,
                                                  void *stream)
{
    if (!plans || !state || !ws || max_tile < 1) return MICLOC_ERR_INVALID;
    ScbArgs s;
    const int rc = scb_args(plans, F, B, max_tile, &s);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, s.a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, s.ws_total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(plans[0]->device);
    return scb_localize(plans, F, B, s, state, final_tile, band_power, power, argmax, ws, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr,
                        (hipStream_t)stream);
}

size_t micloc_stream_complex_bands_window_state_bytes(const micloc_plan *const *plans, int F, int B, int max_tile, int window, int hop,
                                                      int max_windows)
{
    ScbArgs s;
    if (max_tile < 1 || scb_window_args(scb_args(plans, F, B, max_tile, &s), plans, window, hop, max_windows, &s) != MICLOC_OK) return 0;
    return s.win_total;
}

int micloc_stream_complex_bands_window_reset(const micloc_plan *const *plans, int F, int B, int max_tile, void *win_state, size_t win_bytes,
                                             int window, int hop, int max_windows, void *stream)
{
    if (!plans || !win_state || max_tile < 1) return MICLOC_ERR_INVALID;
    ScbArgs s;
    const int rc = scb_window_args(scb_args(plans, F, B, max_tile, &s), plans, window, hop, max_windows, &s);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(win_state, win_bytes, s.win_total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(plans[0]->device);
    HIP_TRY(launch_zero_fill(win_state, s.win_total, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_complex_bands_localize_tile_windows_f64(const micloc_plan *const *plans, int F, void *state, size_t state_bytes, int B,
                                                          int max_tile, int final_tile, double *band_power, double *power, int32_t *argmax,
                                                          void *ws, size_t ws_bytes, void *win_state, size_t win_bytes, int window, int hop,
                                                          int max_windows, double *window_power, int32_t *window_argmax, double *latest_power,
                                                          int32_t *latest_argmax, void *stream)
{
    if (!plans || !state || !ws || !win_state || !window_argmax || max_tile < 1) return MICLOC_ERR_INVALID;
    ScbArgs s;
    const int rc = scb_window_args(scb_args(plans, F, B, max_tile, &s), plans, window, hop, max_windows, &s);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, s.a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, s.ws_total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(win_state, win_bytes, s.win_total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(plans[0]->device);
    return scb_localize(plans, F, B, s, state, final_tile, band_power, power, argmax, ws, win_state, window, hop, max_windows, window_power,
                        window_argmax, latest_power, latest_argmax, (hipStream_t)stream);
}

/* status[0 .. 3] = micloc_stream_complex_status' words of the F * B rows; [4] = wideband windows emitted or given up, [5] = given up
 * (0 and 0 with win_state == NULL) (synchronises the stream) */
int micloc_stream_complex_bands_status(const void *state, const void *win_state, int *status6, void *stream)
{
    if (!state || !status6) return MICLOC_ERR_INVALID;
    int ctl[STREAM_CLK_T + 1], w[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(ctl, state, sizeof(ctl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (win_state)
        HIP_TRY(hipMemcpyAsync(w, reinterpret_cast<const unsigned char *>(win_state) + SCB_BANDS_WORDS, sizeof(w), hipMemcpyDeviceToHost,
                               (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status6[0] = ctl[0];
    status6[1] = ctl[8];
    status6[2] = ctl[2];
    status6[3] = ctl[STREAM_CLK_T];
    status6[4] = w[0];
    status6[5] = w[1];
    return MICLOC_OK;
}

// ---- stand-alone operators -------------------------------------------------------------------------------
size_t micloc_rzcc_workspace_bytes(int B, int T, int C) { return micloc_rzcc_workspace_bytes_ex(B, T, C, 1, 0); }

size_t micloc_rzcc_workspace_bytes_ex(int B, int T, int C, int robust_width, int chunk_frames)
{
    if (B < 1 || T < 1 || C < 1 || robust_width < 1) return 0;
    const size_t planar = align256((size_t)B * C * micloc_padded_T(T) * sizeof(double));
    return planar + rzcc_scratch_bytes(B * C, T, robust_width, chunk_frames);
}

int micloc_rzcc_encode_f64(const double *sig, int B, int T, int C, int robust_width, int bipolar, int8_t *spikes,
                           void *ws, size_t ws_bytes, void *stream)
{
    return micloc_rzcc_encode_ex_f64(sig, B, T, C, robust_width, bipolar, 0, spikes, ws, ws_bytes, stream);
}

int micloc_rzcc_encode_ex_f64(const double *sig, int B, int T, int C, int robust_width, int bipolar, int chunk_frames,
                              int8_t *spikes, void *ws, size_t ws_bytes, void *stream)
{
    if (!sig || !spikes || bad_batch(B) || T < 1 || C < 1 || robust_width < 1) return MICLOC_ERR_INVALID;
    // (the automatic choice does not depend on robust_width: micloc_rzcc_workspace_bytes(B, T, C) covers chunk_frames 0)
    if (bad_ws(ws, ws_bytes, micloc_rzcc_workspace_bytes_ex(B, T, C, robust_width, chunk_frames))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(spikes));
    const int Ts = micloc_padded_T(T);
    unsigned char *base = reinterpret_cast<unsigned char *>(ws);
    double *planar = reinterpret_cast<double *>(base);
    void *scratch = base + align256((size_t)B * C * Ts * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_pack_planar(sig, planar, B, T, C, Ts, st));
    IirCoef id{};
    id.n = 1;
    id.b[0] = 1.0;  // fma(1, x, +0) == x: the identity filter keeps the stream bit-exact
    id.a[0] = 1.0;
    HIP_TRY(launch_bandpass_rzcc(id, planar, B * C, C, T, Ts, robust_width, bipolar ? 1 : 0, nullptr, spikes, scratch,
                                 st, nullptr, 0, 0, chunk_frames));
    return MICLOC_OK;
}

size_t micloc_lfilter_workspace_bytes(int B, int T, int C)
{
    if (B < 1 || T < 1 || C < 1) return 0;
    return 2 * align256((size_t)B * C * micloc_padded_T(T) * sizeof(double));
}

int micloc_lfilter_f64(const double *b, const double *a, int n, const double *x, int B, int T, int C, double *y,
                       void *ws, size_t ws_bytes, void *stream)
{
    if (!b || !a || !x || !y || n < 1 || n > MICLOC_MAX_IIR || bad_batch(B) || T < 1 || C < 1 || a[0] == 0.0)
        return MICLOC_ERR_INVALID;
    if (bad_ws(ws, ws_bytes, micloc_lfilter_workspace_bytes(B, T, C))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(y));
    const int Ts = micloc_padded_T(T);
    const size_t planar_bytes = align256((size_t)B * C * Ts * sizeof(double));
    unsigned char *base = reinterpret_cast<unsigned char *>(ws);
    double *pin = reinterpret_cast<double *>(base);
    double *pout = reinterpret_cast<double *>(base + planar_bytes);
    IirCoef co{};
    co.n = n;
    for (int i = 0; i < n; ++i) {
        co.b[i] = b[i] / a[0];
        co.a[i] = a[i] / a[0];
    }
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_pack_planar(x, pin, B, T, C, Ts, st));
    HIP_TRY(launch_bandpass_rzcc(co, pin, B * C, C, T, Ts, 1, 0, pout, nullptr, nullptr, st));
    HIP_TRY(launch_unpack_planar(pout, y, B, T, C, Ts, st));
    return MICLOC_OK;
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

// ---- Gram matrix of a planar signal (complex covariance of Beamformer.design_from_template) ------------------------------
size_t micloc_planar_gram_workspace_bytes(int B, int T, int C, int t_start)
{
    if (B < 1 || T < 1 || C < 1 || t_start < 0 || t_start >= T) return 0;
    return align256(planar_gram_partial_bytes(B, T, C, t_start));
}

int micloc_planar_gram_f64(const double *planar, int B, int C, int T, int Ts, int t_start, int normalise, double *gram, void *ws,
                           size_t ws_bytes, void *stream)
{
    if (!planar || !gram || bad_batch(B) || C < 1 || C > 128 || T < 1 || t_start < 0 || t_start >= T) return MICLOC_ERR_INVALID;
    if (Ts < T) return MICLOC_ERR_SHAPE;
    if (bad_ws(ws, ws_bytes, planar_gram_partial_bytes(B, T, C, t_start))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(gram));
    HIP_TRY(launch_planar_gram(planar, B, C, T, Ts, t_start, normalise, gram, reinterpret_cast<double *>(ws), (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- array-signal synthesis (noise-free part of apply_to_template) -------------------------------------------
int micloc_synth_delay_f64(const double *time, const double *sig, const double *slopes, int T, const double *delays,
                           int B, int M, double fs, double *x, void *stream)
{
    if (!time || !sig || !slopes || !delays || !x || T < 2 || bad_batch(B) || M < 1 || !(fs > 0.0)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(x));
    HIP_TRY(launch_synth(time, sig, slopes, T, delays, B, M, fs, x, (hipStream_t)stream));
    return MICLOC_OK;
}

static int synth_args_from_abi(const micloc_synth_args *a, SynthArgs *out)
{
    if (!a || !a->time || !a->sig || !a->slopes || !a->x || a->T < 2 || bad_batch(a->B) || a->K < 1 || a->M < 1 || !(a->fs > 0.0))
        return MICLOC_ERR_INVALID;
    if (a->mode != MICLOC_SYNTH_APPLY_TO_TEMPLATE && a->mode != MICLOC_SYNTH_SIGNAL_FROM_TEMPLATE) return MICLOC_ERR_INVALID;
    if (!a->delays && (!a->doa || !a->r_vec || !a->theta_vec || !(a->speed > 0.0))) return MICLOC_ERR_INVALID;
    SynthArgs k{};
    k.time = a->time;
    k.sig = a->sig;
    k.slopes = a->slopes;
    k.T = a->T;
    k.B = a->B;
    k.K = a->K;
    k.M = a->M;
    k.delays = a->delays;
    k.doa = a->doa;
    k.moving = a->moving ? 1 : 0;
    k.r_vec = a->r_vec;
    k.theta_vec = a->theta_vec;
    k.speed = a->speed;
    k.shift = a->shift;
    k.gain = a->gain;
    k.mode = a->mode;
    k.inv_step = a->fs;
    k.x = a->x;
    *out = k;
    return MICLOC_OK;
}

int micloc_synth_targets_f64(const micloc_synth_args *a, void *stream)
{
    SynthArgs k{};
    const int rc = synth_args_from_abi(a, &k);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(device_of(a->x));
    HIP_TRY(launch_synth_targets(k, (hipStream_t)stream));
    return MICLOC_OK;
}

size_t micloc_synth_awgn_workspace_bytes(int B, int T, int M, int K)
{
    if (B < 1 || T < 1 || M < 1 || K < 1) return 0;
    return synth_awgn_ws_bytes(B, (size_t)T * M, K, M);
}

int micloc_synth_awgn_f64(const micloc_synth_args *a, const double *snr_db, uint64_t seed, uint32_t substream, const uint32_t *epoch,
                          uint32_t first_trial, void *ws, size_t ws_bytes, void *stream)
{
    SynthArgs k{};
    const int rc = synth_args_from_abi(a, &k);
    if (rc != MICLOC_OK) return rc;
    if (!snr_db) return MICLOC_ERR_INVALID;
    if (((size_t)k.T * k.M + 1) / 2 > 0xFFFFFFFFull || (uint64_t)first_trial + (uint64_t)k.B > 0xFFFFFFFFull) return MICLOC_ERR_INVALID;
    if (bad_ws(ws, ws_bytes, synth_awgn_ws_bytes(k.B, (size_t)k.T * k.M, k.K, k.M))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(a->x));
    HIP_TRY(launch_synth_awgn(k, snr_db, seed, substream, epoch, first_trial, ws, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_delay_min_f64(const double *doa, int B, int K, int moving_T, const double *r_vec, const double *theta_vec, int M,
                         double speed, double *shift, void *stream)
{
    if (!doa || !r_vec || !theta_vec || !shift || bad_batch(B) || K < 1 || moving_T < 1 || M < 1 || !(speed > 0.0)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(shift));
    HIP_TRY(launch_delay_min(doa, B, K, moving_T, r_vec, theta_vec, M, speed, shift, (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- counter-based random numbers ----------------------------------------------------------------------------
int micloc_uniform_f64(double *out, size_t n, uint64_t seed, uint32_t substream, const uint32_t *epoch, double lo, double hi,
                       void *stream)
{
    if (!out || n < 1 || (n + 1) / 2 > 0xFFFFFFFFull) return MICLOC_ERR_INVALID;  // the pair index is one counter word
    DeviceGuard guard(device_of(out));
    HIP_TRY(launch_uniform(out, n, seed, substream, epoch, lo, hi, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_counter_add_u32(uint32_t *counter, uint32_t inc, void *stream)
{
    if (!counter) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(counter));
    HIP_TRY(launch_counter_add(counter, inc, (hipStream_t)stream));
    return MICLOC_OK;
}

size_t micloc_awgn_workspace_bytes(int B, int T, int M)
{
    if (B < 1 || T < 1 || M < 1) return 0;
    return awgn_ws_bytes(B, (size_t)T * M);
}

int micloc_awgn_f64(double *x, int B, int T, int M, const double *snr_db, const double *sigma, uint64_t seed, uint32_t substream,
                    const uint32_t *epoch, uint32_t first_trial, void *ws, size_t ws_bytes, void *stream)
{
    if (!x || bad_batch(B) || T < 1 || M < 1 || (!snr_db && !sigma)) return MICLOC_ERR_INVALID;
    // counter words: pair index < 2^32; trial ids stay below the uniform generator's reserved word 0xFFFFFFFF
    if (((size_t)T * M + 1) / 2 > 0xFFFFFFFFull || (uint64_t)first_trial + (uint64_t)B > 0xFFFFFFFFull) return MICLOC_ERR_INVALID;
    if (!sigma && bad_ws(ws, ws_bytes, awgn_ws_bytes(B, (size_t)T * M))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(x));
    HIP_TRY(launch_awgn(x, B, (size_t)T * M, M, snr_db, sigma, seed, substream, epoch, first_trial, ws, (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- per-trial DoA error and per-SNR mean absolute error ------------------------------------------------------
int micloc_doa_error_f64(const int32_t *argmax, const double *doa_list, int G, const double *doa_true, int B, int groups,
                         double *err, double *mae, void *stream)
{
    if (!argmax || !doa_list || !doa_true || G < 1 || bad_batch(B) || groups < 1 || B % groups != 0 || (!err && !mae))
        return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(argmax));
    HIP_TRY(launch_doa_error(argmax, doa_list, G, doa_true, B, groups, err, mae, (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- Xylo integer LIF (BASELINE config 4; parity unpinned, see xylo.hip) ------------------------------------
size_t micloc_xylo_workspace_bytes(int Cin, int N)
{
    if (Cin < 1 || N < 1) return 0;
    return xylo_ws_bytes(Cin, N);
}

int micloc_xylo_lif_i16(const uint8_t *spikes_in, int B, int T, int Cin, const int8_t *W_in, int N, int w_rec,
                        const uint8_t *dash_syn, const uint8_t *dash_mem, const int16_t *thr, int max_spikes,
                        uint8_t *spikes_out, int32_t *rate, void *ws, size_t ws_bytes, void *stream)
{
    if (!spikes_in || !W_in || !dash_syn || !dash_mem || !thr || bad_batch(B) || T < 1 || Cin < 1 || N < 1 || max_spikes < 1 ||
        (!spikes_out && !rate))
        return MICLOC_ERR_INVALID;
    if (Cin > 64 || (w_rec != 0 && N > 1024)) return MICLOC_ERR_SHAPE;
    for (int g = 0; g < N; ++g)
        if (thr[g] <= 0 || dash_syn[g] > 15 || dash_mem[g] > 15) return MICLOC_ERR_INVALID;
    if (bad_ws(ws, ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ws));
    HIP_TRY(launch_xylo(spikes_in, B, T, Cin, W_in, N, w_rec, dash_syn, dash_mem, thr, max_spikes, spikes_out, rate, ws,
                        (hipStream_t)stream));
    return MICLOC_OK;
}

// Two-phase form of the same network: constants uploaded once, then any number of launches that touch no host memory
// and never synchronise (capturable into a HIP graph).  `ternary_channels` > 0: the input is the encoder's int8 raster.
int micloc_xylo_upload(int Cin, const int8_t *W_in, int N, const uint8_t *dash_syn, const uint8_t *dash_mem, const int16_t *thr,
                       void *ws, size_t ws_bytes, void *stream)
{
    if (!W_in || !dash_syn || !dash_mem || !thr || Cin < 1 || N < 1) return MICLOC_ERR_INVALID;
    if (Cin > 64) return MICLOC_ERR_SHAPE;
    for (int g = 0; g < N; ++g)
        if (thr[g] <= 0 || dash_syn[g] > 15 || dash_mem[g] > 15) return MICLOC_ERR_INVALID;
    if (bad_ws(ws, ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ws));
    HIP_TRY(xylo_upload(Cin, W_in, N, dash_syn, dash_mem, thr, ws, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_xylo_lif_resident_i16(const void *spikes_in, int ternary_channels, int B, int T, int Cin, int N, int w_rec,
                                 int max_spikes, uint8_t *spikes_out, int32_t *rate, void *ws, size_t ws_bytes, void *stream)
{
    if (!spikes_in || bad_batch(B) || T < 1 || Cin < 1 || N < 1 || max_spikes < 1 || (!spikes_out && !rate)) return MICLOC_ERR_INVALID;
    if (Cin > 64 || (w_rec != 0 && N > 1024)) return MICLOC_ERR_SHAPE;
    if (ternary_channels < 0 || (ternary_channels > 0 && Cin != 2 * ternary_channels)) return MICLOC_ERR_SHAPE;
    if (bad_ws(ws, ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ws));
    HIP_TRY(launch_xylo_resident(spikes_in, ternary_channels, B, T, Cin, N, w_rec, max_spikes, spikes_out, rate, ws, (hipStream_t)stream));
    return MICLOC_OK;
}

size_t micloc_xylo_sweep_scratch_bytes(int B)
{
    if (bad_batch(B)) return 0;
    return xylo_sweep_scratch_bytes(B);
}

int micloc_xylo_lif_sweep_i16(const int8_t *raster, int ternary_channels, int B, int T, int Cin, int N, int max_spikes, int32_t *rate,
                              void *ws, size_t ws_bytes, void *scratch, size_t scratch_bytes, int workers_per_cu, void *stream)
{
    if (!raster || !rate || bad_batch(B) || T < 1 || Cin < 1 || N < 1 || max_spikes < 1 || workers_per_cu < 0 || workers_per_cu > 8) return MICLOC_ERR_INVALID;
    if (Cin > 64 || ternary_channels < 1 || Cin != 2 * ternary_channels) return MICLOC_ERR_SHAPE;
    if (bad_ws(ws, ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(scratch, scratch_bytes, xylo_sweep_scratch_bytes(B))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ws));
    HIP_TRY(launch_xylo_sweep(raster, ternary_channels, B, T, Cin, N, max_spikes, rate, ws, scratch, workers_per_cu, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_xylo_sweep_status(const void *scratch, int *status2, void *stream)
{
    if (!scratch || !status2) return MICLOC_ERR_INVALID;
    int ctl[2];
    HIP_TRY(hipMemcpyAsync(ctl, scratch, sizeof(ctl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status2[0] = ctl[0];
    status2[1] = ctl[1];
    return MICLOC_OK;
}

int micloc_design_vectors_f64(const double *cov, int n_doa, int C, int bipolar, double rel_prec, double *bf_mat, int G, int g0,
                              void *stream)
{
    if (!cov || !bf_mat || n_doa < 1 || C < 2 || G < 1 || g0 < 0 || g0 + n_doa > G || !(rel_prec > 0.0)) return MICLOC_ERR_INVALID;
    if (C > 128 || (C > 32 && (C & 1)) || (bipolar && (C & 1))) return MICLOC_ERR_SHAPE;  // (the one-sided kernel pairs all columns: even C)
    DeviceGuard guard(device_of(bf_mat));
    HIP_TRY(launch_design_vec(cov, n_doa, C, bipolar ? 1 : 0, rel_prec, bf_mat, G, g0, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_pack_events_u8(const int8_t *raster, int B, int T, int C, int band, int bands, int mode, uint8_t *out, void *stream)
{
    if (!raster || !out || bad_batch(B) || T < 1 || C < 1 || bands < 1 || band < 0 || band >= bands) return MICLOC_ERR_INVALID;
    if (mode != MICLOC_PACK_TERNARY && mode != MICLOC_PACK_UNIPOLAR && mode != MICLOC_PACK_BIPOLAR) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(out));
    const int stride = bands * C * (mode == MICLOC_PACK_BIPOLAR ? 2 : 1);
    HIP_TRY(launch_pack_events(raster, (size_t)B * T, C, out, stride, band * C, bands * C + band * C, mode, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_rate_from_counts_f64(const int32_t *counts, int B, int G, int bands, int T, double fs, double *rate, void *stream)
{
    if (!counts || !rate || bad_batch(B) || G < 1 || bands < 1 || T < 1 || !(fs > 0.0) || (long long)B * G > 0x7fffffffll) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(rate));
    HIP_TRY(launch_rate_from_counts(counts, B, G, bands, T, fs, rate, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_envelope_track_f64(const double *y, int B, int T, int G, double a_rise, double i_rise, double a_fall, double *env, int32_t *index,
                              void *stream)
{
    if (!y || !env || bad_batch(B) || T < 1 || G < 1 || (long long)B * T > 0x7fffffffll * 4) return MICLOC_ERR_INVALID;
    // 1 - 1/w and 1/w of window lengths w >= 1 (utils.py:34): finite, in [0, 1]
    if (!(a_rise >= 0.0 && a_rise <= 1.0 && i_rise >= 0.0 && i_rise <= 1.0 && a_fall >= 0.0 && a_fall <= 1.0)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(env));
    HIP_TRY(launch_envelope_track(y, MICLOC_ENV_F64, B, T, G, a_rise, i_rise, a_fall, env, index, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_envelope_track_any(const void *y, int kind, int B, int T, int G, double a_rise, double i_rise, double a_fall, double *env, int32_t *index,
                              void *stream)
{
    if (!y || !env || bad_batch(B) || T < 1 || G < 1 || (long long)B * T > 0x7fffffffll * 4) return MICLOC_ERR_INVALID;
    if (kind < MICLOC_ENV_F64 || kind > MICLOC_ENV_I64) return MICLOC_ERR_INVALID;
    if (!(a_rise >= 0.0 && a_rise <= 1.0 && i_rise >= 0.0 && i_rise <= 1.0 && a_fall >= 0.0 && a_fall <= 1.0)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(env));
    HIP_TRY(launch_envelope_track(y, kind, B, T, G, a_rise, i_rise, a_fall, env, index, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_peak_location_i32(const int32_t *rate, int B, int G, int bands, int win_size, int32_t *index, void *stream)
{
    if (!rate || !index || bad_batch(B) || G < 1 || bands < 1) return MICLOC_ERR_INVALID;
    if (win_size < 1 || win_size % 2 != 1 || win_size > G / 2 || G > 16384) return MICLOC_ERR_INVALID;  // utils.py:96-107
    DeviceGuard guard(device_of(index));
    HIP_TRY(launch_peak_location(rate, B, G, bands, win_size, index, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_doa_peaks_f64(const double *power, int B, int G, const double *doa_list, int grid_kind, int K, double min_separation,
                         double rel_threshold, int32_t *index, double *value, void *stream)
{
    if (!power || !doa_list || !index || bad_batch(B) || G < 1 || G > 4096 || K < 1 || K > 16) return MICLOC_ERR_INVALID;
    if (grid_kind < MICLOC_GRID_LINEAR || grid_kind > MICLOC_GRID_CIRCULAR_CLOSED) return MICLOC_ERR_INVALID;
    if (!(min_separation >= 0.0) || !(rel_threshold >= 0.0) || isinf(rel_threshold)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(index));
    HIP_TRY(launch_doa_peaks(power, B, G, doa_list, grid_kind, K, min_separation, rel_threshold, index, value, (hipStream_t)stream));
    return MICLOC_OK;
}

}  // extern "C"

namespace {

bool music_dims(int B, int T, int M, int L, int hop, int S, int N, int nbin, int G, int k, MusicDims *d)
{
    if (bad_batch(B) || T < 1 || M < 1 || L < 1 || hop < 1 || S < 1 || N < 2 || nbin < 1 || nbin > N || nbin > 8192 || G < 1 || k < 0)
        return false;
    d->B = B, d->T = T, d->M = M, d->S = S, d->L = L, d->hop = hop, d->N = N;
    d->Np = (N + 63) / 64 * 64;
    d->Fmax = (L < T ? L : T) / N;
    d->nbin = nbin;
    d->Cp = (2 * nbin + 15) / 16 * 16;
    d->G = G;
    d->ksel = (k == 0 || k > nbin) ? nbin : k;
    return true;
}

// every slice starts inside the signal and holds at least one frame (the last slice is the shortest)
bool music_slices_ok(const MusicDims &d)
{
    const long long last = (long long)(d.S - 1) * d.hop;
    if (last >= d.T) return false;
    const long long len = d.T - last < d.L ? d.T - last : d.L;
    return len >= d.N && d.Fmax >= 1;
}

size_t music_ws(const MusicDims &d)
{
    const MusicBuffers L = music_layout(d);
    return align256(L.xf_bytes) + align256(L.X_bytes) + align256(L.sel_bytes) + align256(L.spec_bytes);
}

}  // namespace

extern "C" {

size_t micloc_music_workspace_bytes(int B, int T, int M, int L, int hop, int S, int N, int nbin, int G, int k)
{
    MusicDims d{};
    if (!music_dims(B, T, M, L, hop, S, N, nbin, G, k, &d)) return 0;
    return music_ws(d);
}

int micloc_music_f64(const double *x, int B, int T, int M, const double *b, const double *a, int n, int L, int hop, int S, int N,
                     const double *W, int nbin, const double *steer_re, const double *steer_im, int G, int k, int32_t *sel, double *spec,
                     double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    MusicDims d{};
    if (!x || !b || !a || !W || !steer_re || !steer_im || n < 1 || n > MICLOC_MAX_IIR || a[0] == 0.0 ||
        !music_dims(B, T, M, L, hop, S, N, nbin, G, k, &d))
        return MICLOC_ERR_INVALID;
    if (!music_slices_ok(d)) return MICLOC_ERR_SHAPE;
    if (bad_ws(ws, ws_bytes, music_ws(d))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(x));
    IirCoef co{};
    co.n = n;
    for (int i = 0; i < n; ++i) {
        co.b[i] = b[i] / a[0];
        co.a[i] = a[i] / a[0];
    }
    const MusicBuffers Lb = music_layout(d);
    unsigned char *base = reinterpret_cast<unsigned char *>(ws);
    double *xf = reinterpret_cast<double *>(base);
    base += align256(Lb.xf_bytes);
    double *X = reinterpret_cast<double *>(base);
    base += align256(Lb.X_bytes);
    int32_t *sel_ws = reinterpret_cast<int32_t *>(base);
    base += align256(Lb.sel_bytes);
    double *spec_ws = reinterpret_cast<double *>(base);
    HIP_TRY(launch_music(d, co, x, W, steer_re, steer_im, xf, X, sel ? sel : sel_ws, spec ? spec : spec_ws, power, argmax, (hipStream_t)stream));
    return MICLOC_OK;
}

}  // extern "C"
