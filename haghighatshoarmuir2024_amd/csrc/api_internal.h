// What the units of the C-ABI (api_*.hip; contract: include/micloc_hip.h) share: the plan, the last-error word, the argument rules that more
// than one surface applies.  No kernel and no launch macro here or in any api_*.hip: they call the launch_* functions of micloc_internal.h.
#pragma once
#include <math.h>
#include <string.h>

#include <new>
#include <vector>

#include "micloc_internal.h"

struct micloc_plan {
    int device = 0;
    int M = 0, C = 0, L = 0;
    int robust_width = 1, bipolar = 0;
    micloc::IirCoef iir{};
    // STHT taps
    double *d_taps = nullptr;
    micloc::SthtTaps taps{};
    std::vector<double> taps_host;  // the compact table as uploaded: two plans run ONE STHT launch only when theirs are the same bits
    // neuron kernel
    double *d_ntab = nullptr;
    micloc::NeuronTab ntab{};
    // beamforming matrices
    double *d_W = nullptr;
    micloc::BeamformW W{};
    int W_is_complex = 0;
    int G_out = 0;  // DoA grid size seen by the caller
    // bumped whenever a captured hipGraph of this plan becomes stale: a device table was re-allocated (the graph holds the
    // old pointer) or replaced by one of another shape (the graph holds the old dimensions BY VALUE: W.GT / W.G / W.CT,
    // ntab.n / NK are kernel arguments, and the packed bf_mat layout depends on Gp)
    int generation = 0;
    int chunk_frames = 0;  // encoder time chunking: 0 automatic, < 0 off, > 0 owned frames per chunk
    size_t taps_cap = 0, ntab_cap = 0, W_cap = 0;  // allocated doubles
};

namespace micloc {

// what micloc_last_hip_error reports: one word per thread and library (defined in api_plan.hip), written by a failure in any unit
extern thread_local int g_last_hip;

// (a failed runtime call also leaves its code in HIP's sticky "last error": clear it, or the next, unrelated launch
// check -- hipGetLastError() after a successful launch -- would report it again)
inline int hip_failed(hipError_t e)
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

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

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
inline int device_of(const void *ptr)
{
    hipPointerAttribute_t at;
    int dev = 0;
    if (ptr && hipPointerGetAttributes(&at, ptr) == hipSuccess) return at.device;
    (void)hipGetLastError();
    (void)hipGetDevice(&dev);
    return dev;
}

// trials map to gridDim.y / gridDim.z, which HIP limits to 65535
inline bool bad_batch(int B) { return B < 1 || B > 65535; }

inline bool bad_ws(const void *ws, size_t have, size_t need)
{
    return ws == nullptr || have < need || (reinterpret_cast<uintptr_t>(ws) & 255) != 0;
}

inline double *ws_doubles(void *ws, size_t offset) { return reinterpret_cast<double *>(static_cast<unsigned char *>(ws) + offset); }

// MICLOC_OK when the plan holds what an entry for a complex / a real bf_mat reads: the matrix of that kind and, for a real one, the neuron kernel
inline int plan_kind(const micloc_plan *p, bool cpx)
{
    if (!p->d_W || (!cpx && !p->d_ntab)) return MICLOC_ERR_NOT_SET;
    return (p->W_is_complex != 0) == cpx ? MICLOC_OK : MICLOC_ERR_SHAPE;
}

// ---- the window rule (api_plan.hip) ---------------------------------------------------------------------------------------------
// the chunk length of the power-only launch that serves this plan and bf_mat: what a window and a hop are multiples of
int window_quantum(const micloc_plan *p);

// MICLOC_OK and *nW, or the status of the window rule's argument errors
inline int window_args(int T, int window, int hop, int quantum, int B, int *nW)
{
    if (T < 1 || quantum < 1) return MICLOC_ERR_INVALID;
    if (window < 1 || hop < 1 || window % quantum != 0 || hop % quantum != 0) return MICLOC_ERR_SHAPE;
    const long long n = window_count(T, window, hop);
    if (n * (long long)B > 0x7fffffffll) return MICLOC_ERR_SHAPE;
    *nW = (int)n;
    return MICLOC_OK;
}

// ---- the front end of the pipeline entries (api_plan.hip) --------------------------------------------------------------------------
// where it (STHT, band-pass / RZCC) keeps its arrays in the caller's workspace
struct FrontOffsets {
    size_t h, pre, scratch, spikes;
};

struct Front {
    int rc;
    const void *src;  // what the tails read: the spike raster (real bf_mat) or the planar band-passed rows [B][C][Ts] (complex)
    int Ts;
};

Front front_end(const micloc_plan *p, bool cpx, const double *x, int B, int T, void *ws, const FrontOffsets &o, int8_t *spikes, int stages,
                hipStream_t st);

// ---- the coefficient tables of a set of bands (api_bands.hip) ---------------------------------------------------------------------
// host [F][n] coefficient rows -> the filterbank kernel's table, divided by a[0] as micloc_lfilter_f64 does
int filterbank_coef(const double *b, const double *a, int F, int n, FilterbankCoef *co);

// the plans' band-pass rows as one table (already divided by a[0] at plan creation)
void cbands_coef(const micloc_plan *const *plans, int F, FilterbankCoef *co);

}  // namespace micloc
