// Xylo integer LIF as a STREAM: xylo_lif_pk_kernel's arithmetic (xylo.hip: ternary raster in, input currents on the int8 matrix
// cores, two neurons per lane in packed 16-bit words, the fast step with one second-spike test per 16 steps and the exact re-walk),
// resumable ACROSS LAUNCHES.  PARITY UNPINNED like xylo.hip: HIP == oracle_xylo_lif bit for bit, the oracle is not checked against
// XyloSim.
//
// The one-shot kernel starts every trial from zero state at frame 0.  Here a launch integrates the frames [t0, t1) of every trial:
// a wave loads (isyn, vmem, total0, total1) of its lanes from the per-trial state [B][Npad / 2] (16 bytes per lane pair) at its
// start, stores them back at its end and writes the running counts [B][N].  Zero state comes from a reset (a zero fill), never from
// the kernel.  The range comes by value, or (ctl != NULL) from the control words of a band's stream: the window-relative chunk range
// ctl[4], ctl[5] of rz_stream_horizon_kernel in chunks of 256 frames, cut at ctl[10], the frames of the window that exist -- as
// beamform_ws_kernel reads chunk_range -- so that no launch argument of a tile depends on time.  An empty range returns at once and
// rewrites nothing.  t0 is a multiple of 16 frames (the contract that keeps the 16-byte tile loads aligned); t1 is arbitrary and the
// ragged tail takes the path of the one-shot kernel's last partial tile.  The raster's trial stride is an argument of its own (the
// `cap` frames of a raster window, or T).
//
// One workgroup per (neuron block of 512, trial).  No persistent workgroups, no tickets, no wait on another workgroup: the state is
// handed over between launches on one stream, nowhere else.
//
// The windowed read-out: the launch also writes the count of every chunk it finishes to chunk_counts [B][chunk_rows][N] at the
// chunk's window-relative row; xylo_stream_window_kernel folds those rows into the open windows (integers: no ordering contract),
// and xylo_stream_readout_kernel turns the bands' counts into rate and peak (the expressions of rate_from_counts_kernel and
// peak_location_kernel, sweep.hip).
//
// The lane's constants, the step functions, the MFMA `produce`, the staging loop and the walk over a range are XpLif of xylo_rows.h,
// the one-shot kernel's; here are the range, the state's load and store and the counts.
//
// At the end of the file stands the tracking form of the packed walk as a stream, xylo_lif_track_stream_kernel: this file's range and
// state around the tap of the one-shot xylo_lif_track_kernel (xylo.hip), which xylo_track_rows.h holds for both.
#include "readout_rows.h"
#include "stream_xylo.h"
#include "xylo_rows.h"
#include "xylo_track.h"
#include "xylo_track_rows.h"

namespace micloc {

namespace {

constexpr int SX_CH = XYLO_STREAM_CHUNK;
constexpr int SX_MAXG = 4096;  // DoA grid of the read-out (its band sums live in LDS)

// The range of xylo_lif_stream_kernel below as a function, for its tracking form xylo_lif_track_stream_kernel at the end of the file; the
// chunk counts as a function are xp_chunk_done of xylo_rows.h, shared with the one-shot chunk-count kernel of xylo.hip.  The counting
// kernel keeps its own text of both, and of the state's load and store: it is the live loop's kernel, and with these functions in it its 12 000-frame tile measured 1 % slower at equal registers (with the state helpers as well: 82 VGPRs
// instead of 80, five waves per SIMD instead of six); DESIGN 4.24.
// The frames of a launch: [t_lo, t_hi) by value, or (ctl != NULL) the range of this tile, decided on the device by the horizon launch in
// front.  false: an empty range (uniform over the launch; the caller returns in front of every barrier and rewrites nothing).
__device__ __forceinline__ bool sx_range(const int *__restrict__ ctl, int chunk_rows, int &t_lo, int &t_hi)
{
    if (ctl) {
        const int lo = ctl[4], hi = ctl[5], exist = ctl[10];
        if (lo < 0 || hi > chunk_rows) return false;  // (never: the horizon flags a window that does not hold the range and leaves it empty)
        t_lo = lo * SX_CH;
        t_hi = hi * SX_CH < exist ? hi * SX_CH : exist;
    }
    return t_hi > t_lo;
}

template <int KQ, bool WANT_OUT>
__global__ __launch_bounds__(XP_WAVES * 64) void xylo_lif_stream_kernel(const int8_t *__restrict__ raster, int tc, int stride_frames, int Cin,
                                                                         const long *__restrict__ Wb /*[Npad][4 KQ]*/, int N,
                                                                         const uint8_t *__restrict__ dash_syn,
                                                                         const uint8_t *__restrict__ dash_mem,
                                                                         const short *__restrict__ thr, int max_spikes,
                                                                         uint8_t *__restrict__ spikes_out, int T_out, int *__restrict__ counts,
                                                                         int4_t *__restrict__ state, int t_lo, int t_hi,
                                                                         const int *__restrict__ ctl, int *__restrict__ chunk_counts,
                                                                         int chunk_rows)
{
    if (ctl) {  // the range of this tile, decided on the device by the horizon launch in front
        const int lo = ctl[4], hi = ctl[5], exist = ctl[10];
        if (lo < 0 || hi > chunk_rows) return;  // (never: the horizon flags a window that does not hold the range and leaves it empty)
        t_lo = lo * SX_CH;
        t_hi = hi * SX_CH < exist ? hi * SX_CH : exist;
    }
    if (t_hi <= t_lo) return;  // uniform over the launch, in front of every barrier: nothing is rewritten

    __shared__ __attribute__((aligned(16))) unsigned char tile[XP_TT][32 * KQ];
    extern __shared__ __attribute__((aligned(16))) int cur_dyn[];  // [waves][4][64][4]
    const int b = blockIdx.y;
    XpLif<KQ, WANT_OUT> lif;
    lif.init(tile, cur_dyn, blockIdx.x * XP_NEUR, Wb, N, dash_syn, dash_mem, thr, max_spikes);
    const int n0 = lif.n0, n1 = lif.n1;
    const bool act0 = lif.act0, act1 = lif.act1;

    // the trial's state of this lane pair: [B][Npad / 2] words of 16 bytes, neuron block major, then wave, then lane
    int4_t *st = state + (((size_t)b * gridDim.x + blockIdx.x) * XP_WAVES + lif.wv) * 64 + lif.l;
    const int4_t sv = *st;
    lif.isyn = xp_s2(sv[0]);
    lif.vmem = xp_s2(sv[1]);
    lif.total0 = sv[2];
    lif.total1 = sv[3];
    int chunk0 = lif.total0, chunk1 = lif.total1;  // the totals at the start of the open chunk
    if constexpr (WANT_OUT) lif.ob = spikes_out + (size_t)b * T_out * N;

    lif.run_range(raster + (size_t)b * stride_frames * tc, raster + (size_t)gridDim.y * stride_frames * tc, tc, Cin, t_lo, t_hi,
                  [&](int t0, int steps) {
                      // a chunk of the stream ends with this tile (the recording's last one may be ragged): its count, for the
                      // windowed read-out
                      if (chunk_counts && (((t0 + steps) & (SX_CH - 1)) == 0 || t0 + steps == t_hi)) {
                          int *cc = chunk_counts + ((size_t)b * chunk_rows + (t0 >> 8)) * N;
                          if (act0) cc[n0] = lif.total0 - chunk0;
                          if (act1) cc[n1] = lif.total1 - chunk1;
                          chunk0 = lif.total0;
                          chunk1 = lif.total1;
                      }
                  });
    *st = int4_t{xp_i(lif.isyn), xp_i(lif.vmem), lif.total0, lif.total1};
    if (act0) counts[(size_t)b * N + n0] = lif.total0;
    if (act1) counts[(size_t)b * N + n1] = lif.total1;
}

static_assert(SX_CH == 256 && SX_CH == XP_CHUNK, "the chunk row of a tile is t0 >> 8 (xp_chunk_done, xylo_rows.h)");

// ---- the windows of one band: stream_window_kernel's schedule (StreamWindowWalk, readout_rows.h) on integer counts, between the LIF
// launch and the commit of a tile.  chunk_counts [B][chunk_rows][N] holds the chunks that became final in this call.  Window n keeps its
// sum so far in slot n % K of acc [B][K][N]; a window that is emitted goes to row n % Kb of ring [B][Kb][N] and head[0] becomes the
// number of windows emitted.
__global__ __launch_bounds__(256) void xylo_stream_window_kernel(const int *__restrict__ chunk_counts, int chunk_rows, int N,
                                                                  const int *__restrict__ ctl, int final_tile, int wchunks, int hchunks, int K,
                                                                  int Kb, int *__restrict__ acc, int *__restrict__ head, int *__restrict__ ring)
{
    const int b = blockIdx.x;
    const StreamWindowWalk walk(ctl, final_tile, SX_CH, wchunks, hchunks, chunk_rows);
    if (!walk.ok) return;
    const int *cb_ = chunk_counts + (size_t)b * chunk_rows * N;
    for (int n = walk.n0; n <= walk.n_started; ++n) {
        const StreamWindowWalk::Window w = walk.window(n);
        int *slot = acc + ((size_t)b * K + n % K) * N;
        int *row = ring + ((size_t)b * Kb + n % Kb) * N;
        for (int g = threadIdx.x; g < N; g += 256) {
            int total = w.ca > w.c0 ? slot[g] : 0;  // (the window opened in an earlier call)
            for (int ch = w.ca; ch < w.cb; ++ch) total += cb_[(size_t)walk.row(ch) * N + g];
            if (w.emit) {
                row[g] = total;
                slot[g] = 0;
            } else {
                slot[g] = total;
            }
        }
    }
    if (b == 0 && threadIdx.x == 0) head[0] = walk.head();
}

// ---- the read-out over the bands -----------------------------------------------------------------------------------------------------
// peak_location_kernel's estimator (sweep.hip) on the band sums pw[G] in LDS: box-car of `win` samples by a full, non-circular
// convolution, first maximum (block_first_max, readout_rows.h), minus win / 2, modulo G.  Every thread of the workgroup calls it.
__device__ int sx_peak(const long long *pw, int G, int win, long long *bestv, int *besti)
{
    long long bv = -1;
    int bi = RO_NONE;
    for (int n = threadIdx.x; n < G + win - 1; n += 256) {
        long long s = 0;
        for (int k = 0; k < win; ++k) {
            const int g = n - k;
            if (g >= 0 && g < G) s += pw[g];
        }
        if (s > bv) {
            bv = s;
            bi = n;
        }
    }
    int idx = block_first_max<256>(bv, bi, bestv, besti, (int)threadIdx.x) - win / 2;
    idx %= G;
    return idx < 0 ? idx + G : idx;
}

// One workgroup per trial.  Running: counts [B][F G] gathered from the bands, rate[b][g] = mean over the bands of counts_f / frames_f *
// fs in rate_from_counts_kernel's expression and band order (frames_f: ctl_f[8], the frames band f has integrated; a band that has
// integrated none contributes its zero counts over one frame), peak[b].  Windowed: the windows [emitted, min_f head_f) that every band
// has emitted, from the bands' rings, over the frames the window holds; a window a band's ring has overwritten is counted as given up.
// The new counts go to state[2], state[3]; xylo_stream_readout_commit_kernel makes them state[0], state[1] (every workgroup reads them).
__global__ __launch_bounds__(256) void xylo_stream_readout_kernel(XyloReadoutArgs a, int F, int G, double fs, int win, int windowed, int window,
                                                                   int hop, int Kb, int max_windows, int *__restrict__ state,
                                                                   int32_t *__restrict__ counts, double *__restrict__ rate,
                                                                   int32_t *__restrict__ peak, int32_t *__restrict__ wcounts,
                                                                   double *__restrict__ wrate, int32_t *__restrict__ wpeak,
                                                                   int32_t *__restrict__ lcounts, double *__restrict__ lrate,
                                                                   int32_t *__restrict__ lpeak)
{
    __shared__ long long pw[SX_MAXG];
    __shared__ long long bestv[256];
    __shared__ int besti[256];
    const int b = blockIdx.x;
    for (int g = threadIdx.x; g < G; g += 256) {
        double s = 0.0;
        long long ps = 0;
        for (int f = 0; f < F; ++f) {
            const int c = a.counts[f][(size_t)b * G + g];
            const int fr = a.ctl[f][8];
            const double T = fr > 0 ? (double)fr : 1.0;
            s += (double)c / T * fs;
            ps += c;
            counts[((size_t)b * F + f) * G + g] = c;
        }
        rate[(size_t)b * G + g] = s / (double)F;
        pw[g] = ps;
    }
    __syncthreads();
    const int idx = sx_peak(pw, G, win, bestv, besti);
    if (threadIdx.x == 0) peak[b] = idx;
    if (!windowed) return;
    const int emitted = state[0];
    // a window below rw.lo has been overwritten in the ring of the band that leads: given up (uniform over the launch)
    const ReadyWindows rw = ready_windows(F, emitted, Kb, [&](int f) { return a.head[f][0]; });
    const long long Tend = a.ctl[0][STREAM_CLK_T];  // frames pushed (the bands share the clock; the tick is behind every band's tile)
    for (int n = rw.lo; n < rw.hi; ++n) {
        long long frames = Tend - (long long)n * hop;
        frames = frames > window ? window : (frames < 1 ? 1 : frames);
        const size_t row = (size_t)b * max_windows + n % max_windows;
        const bool newest = n == rw.hi - 1;
        __syncthreads();  // pw is rewritten
        for (int g = threadIdx.x; g < G; g += 256) {
            double s = 0.0;
            long long ps = 0;
            for (int f = 0; f < F; ++f) {
                const int c = a.ring[f][((size_t)b * Kb + n % Kb) * G + g];
                s += (double)c / (double)frames * fs;
                ps += c;
                wcounts[(row * F + f) * G + g] = c;
                if (newest && lcounts) lcounts[((size_t)b * F + f) * G + g] = c;
            }
            const double r = s / (double)F;
            wrate[row * G + g] = r;
            if (newest && lrate) lrate[(size_t)b * G + g] = r;
            pw[g] = ps;
        }
        __syncthreads();
        const int wi = sx_peak(pw, G, win, bestv, besti);
        if (threadIdx.x == 0) {
            wpeak[row] = wi;
            if (newest && lpeak) lpeak[b] = wi;
        }
    }
    if (b == 0 && threadIdx.x == 0) {
        const int next = rw.hi > emitted ? rw.hi : emitted;
        state[2] = next;
        state[3] = state[1] + rw.given(next);
    }
}

__global__ void xylo_stream_readout_commit_kernel(int *__restrict__ state)
{
    state[0] = state[2];
    state[1] = state[3];
}

size_t sx_al(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

size_t xylo_stream_state_bytes(int B, int N) { return (size_t)B * (xp_npad(N) / 2) * sizeof(int4_t); }

size_t xylo_stream_chunk_bytes(int B, int N, int chunk_rows) { return sx_al((size_t)B * chunk_rows * N * sizeof(int)); }

// raster: int8 [B][stride_frames][tc], 16-byte aligned; ws: xylo_upload's.  ctl == NULL: the frames [t0, t0 + n) by value.
hipError_t launch_xylo_resume(const int8_t *raster, int tc, int stride_frames, int B, int t0, int n, const int *ctl, int Cin, int N, int max_spikes,
                              uint8_t *spikes_out, int T_out, int32_t *counts, void *state, void *ws, int32_t *chunk_counts, int chunk_rows,
                              hipStream_t stream)
{
    if (Cin > 64 || Cin != 2 * tc || max_spikes < 1 || (reinterpret_cast<uintptr_t>(raster) & 15) != 0) return hipErrorInvalidValue;
    if (!ctl && n < 1) return hipSuccess;  // an empty range: nothing is launched, nothing rewritten
    const XyloWs w = xylo_ws(ws, Cin, N);
    const XpShape sh = xp_shape(N, tc);
    const dim3 grid(sh.nblk, B), block(sh.waves * 64);
    int4_t *stp = reinterpret_cast<int4_t *>(state);
#define SX_LAUNCH(KQ, WO)                                                                                                              \
    hipLaunchKernelGGL((xylo_lif_stream_kernel<KQ, WO>), grid, block, sh.lds, stream, raster, tc, stride_frames, Cin, w.dWb, N, w.dds, \
                       w.ddm, w.dth, max_spikes, spikes_out, T_out, counts, stp, t0, t0 + n, ctl, chunk_counts, chunk_rows)
    if (xp_kq(Cin) == 1) {
        if (spikes_out)
            SX_LAUNCH(1, true);
        else
            SX_LAUNCH(1, false);
    } else {
        if (spikes_out)
            SX_LAUNCH(2, true);
        else
            SX_LAUNCH(2, false);
    }
#undef SX_LAUNCH
    return hipGetLastError();
}

// win_state: [256 B: int windows emitted][acc [B][K][N] ints][ring [B][Kb][N] ints], K = stream_window_slots
size_t xylo_stream_window_state_bytes(int B, int N, int window, int hop, int Kb)
{
    return 256 + sx_al((size_t)B * stream_window_slots(window, hop) * N * sizeof(int)) + sx_al((size_t)B * Kb * N * sizeof(int));
}

static int *sx_ring(void *win_state, int B, int N, int window, int hop)
{
    return reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(win_state) + 256 +
                                   sx_al((size_t)B * stream_window_slots(window, hop) * N * sizeof(int)));
}

hipError_t launch_xylo_stream_windows(const int32_t *chunk_counts, int B, int chunk_rows, int N, const int *ctl, int final_tile, int window, int hop,
                                      int Kb, void *win_state, hipStream_t stream)
{
    if (window < 1 || hop < 1 || hop > window || window % SX_CH != 0 || hop % SX_CH != 0 || Kb < 1) return hipErrorInvalidValue;
    int *head = reinterpret_cast<int *>(win_state);
    int *acc = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(win_state) + 256);
    hipLaunchKernelGGL(xylo_stream_window_kernel, dim3(B), dim3(256), 0, stream, chunk_counts, chunk_rows, N, ctl, final_tile ? 1 : 0, window / SX_CH,
                       hop / SX_CH, stream_window_slots(window, hop), Kb, acc, head, sx_ring(win_state, B, N, window, hop));
    return hipGetLastError();
}

int xylo_stream_readout_max_grid() { return SX_MAXG; }

// a.counts / a.ctl: every band's counts [B][G] and control words; windowed: a.head / a.ring are filled here from win_states
hipError_t launch_xylo_stream_readout(XyloReadoutArgs a, void *const *win_states, int F, int B, int G, double fs, int win, int window, int hop, int Kb,
                                      int max_windows, void *state, int32_t *counts, double *rate, int32_t *peak, int32_t *wcounts, double *wrate,
                                      int32_t *wpeak, int32_t *lcounts, double *lrate, int32_t *lpeak, hipStream_t stream)
{
    if (G > SX_MAXG || F < 1 || F > MICLOC_MAX_BANDS) return hipErrorInvalidValue;
    const int windowed = window > 0;
    for (int f = 0; f < F; ++f) {
        a.head[f] = windowed ? reinterpret_cast<const int *>(win_states[f]) : nullptr;
        a.ring[f] = windowed ? sx_ring(win_states[f], B, G, window, hop) : nullptr;
    }
    int *st = reinterpret_cast<int *>(state);
    hipLaunchKernelGGL(xylo_stream_readout_kernel, dim3(B), dim3(256), 0, stream, a, F, G, fs, win, windowed, window, hop, Kb, max_windows, st, counts,
                       rate, peak, wcounts, wrate, wpeak, lcounts, lrate, lpeak);
    if (windowed) hipLaunchKernelGGL(xylo_stream_readout_commit_kernel, dim3(1), dim3(1), 0, stream, st);
    return hipGetLastError();
}

// ==== the tracking walk as a STREAM: xylo_lif_stream_kernel's range, early return and state hand-off around xylo_lif_track_kernel's tap,
// pair tile and combine over the waves (include/micloc_hip.h "streaming, Xylo tracking") ===================================
// The walk hands its tap first = (position in the range's raster == 0).  In a stream that position is relative to the raster WINDOW; the
// rule's e[0] = m[0] belongs to ABSOLUTE frame 0 alone.  The stream's tap wraps the one-shot tap and lets `first` through only where
// position 0 is absolute frame 0: the window's base word ctl[STREAM_CLK_BASE], written by the clock launch in front of the tile, is 0 (by
// value: the raster is the recording, always).  No flag the kernel writes for itself is read (4.21's rule).
struct XpTrackStreamTap : XpTrackTap {
    bool at_origin;
    __device__ __forceinline__ void begin(int off_, bool first_) { XpTrackTap::begin(off_, first_ && at_origin); }
};

struct XyloTrackSink {
    int R;  // ring depth
    int32_t *index;
    double *peak;
    int32_t *latest_index;
    double *latest_peak;
};

// a finished row of trial b: frame `abs` into its ring row, the newest frame of the launch also into the latest words
__device__ __forceinline__ void xylo_track_ring_store(const XyloTrackSink &o, int b, int abs, bool newest, double best, int bi)
{
    const size_t r = (size_t)b * o.R + (size_t)((unsigned)abs % (unsigned)o.R);  // (abs >= 0: the clock's)
    const int idx = bi == RO_NONE ? 0 : bi;
    o.index[r] = idx;
    o.peak[r] = best;
    if (newest) {
        o.latest_index[b] = idx;
        o.latest_peak[b] = best;
    }
}

// grid (neuron blocks, trials), the range and the state of xylo_lif_stream_kernel; env_state [B][Npad / 2] x {e0, e1}, the lane order of
// `state`.  Position p of the range's raster is absolute frame abs0 + p.  One neuron block: the workgroup writes ring row (abs0 + p) % R
// itself; more: the pairs go to pval / pidx [B][cap][blocks] at p - p0 (p0: 0 in a stream, the by-value range's start otherwise) and
// xylo_track_stream_combine_kernel finishes them.
template <int KQ>
__global__ __launch_bounds__(XP_WAVES * 64) void xylo_lif_track_stream_kernel(const int8_t *__restrict__ raster, int tc, int stride_frames, int Cin,
                                                                               const long *__restrict__ Wb /*[Npad][4 KQ]*/, int N,
                                                                               const uint8_t *__restrict__ dash_syn,
                                                                               const uint8_t *__restrict__ dash_mem,
                                                                               const short *__restrict__ thr, int max_spikes,
                                                                               int *__restrict__ counts, int4_t *__restrict__ state,
                                                                               double2 *__restrict__ env_state, int t_lo, int t_hi,
                                                                               const int *__restrict__ ctl, int *__restrict__ chunk_counts,
                                                                               int chunk_rows, double a_rise, double i_rise, double a_fall,
                                                                               const XyloTrackSink out, double *__restrict__ env_last,
                                                                               double *__restrict__ pval, int32_t *__restrict__ pidx, int cap)
{
    const int p0 = ctl ? 0 : t_lo;
    if (!sx_range(ctl, chunk_rows, t_lo, t_hi)) return;  // uniform over the launch, in front of every barrier: nothing is rewritten
    const int abs0 = ctl ? ctl[STREAM_CLK_BASE] : 0;

    __shared__ __attribute__((aligned(16))) unsigned char tile[XP_TT][32 * KQ];
    extern __shared__ __attribute__((aligned(16))) int cur_dyn[];  // [waves][4][64][4]
    __shared__ double sv[XP_WAVES][XP_TT];
    __shared__ int si[XP_WAVES][XP_TT];
    const int b = blockIdx.y, nblk = gridDim.x, blk = blockIdx.x;
    XpLif<KQ, false, XpTrackStreamTap> lif;
    lif.init(tile, cur_dyn, blk * XP_NEUR, Wb, N, dash_syn, dash_mem, thr, max_spikes);
    XpTrackStreamTap &tap = lif.tap;
    xp_track_tap_init(lif, a_rise, i_rise, a_fall, sv, si);
    tap.at_origin = abs0 == 0;
    // the trial's state of this lane pair, as xylo_lif_stream_kernel's; its envelopes in the same order
    const size_t lane = (((size_t)b * nblk + blk) * XP_WAVES + lif.wv) * 64 + lif.l;
    const int4_t sw = state[lane];
    lif.isyn = xp_s2(sw[0]);
    lif.vmem = xp_s2(sw[1]);
    lif.total0 = sw[2];
    lif.total1 = sw[3];
    const double2 ev = env_state[lane];
    tap.e0 = ev.x, tap.e1 = ev.y;
    int chunk0 = lif.total0, chunk1 = lif.total1;
    const int tid = lif.tid, nthreads = lif.nthreads, waves = nthreads >> 6;

    lif.run_range(raster + (size_t)b * stride_frames * tc, raster + (size_t)gridDim.y * stride_frames * tc, tc, Cin, t_lo, t_hi,
                  [&](int t0, int steps) {
                      xp_chunk_done(lif, chunk_counts, chunk_rows, b, t0, steps, t_hi, chunk0, chunk1);
                      xp_track_rows(sv, si, waves, tid, nthreads, steps, [&](int f, double best, int bi) {
                          const int p = t0 + f;
                          if (nblk == 1) {
                              xylo_track_ring_store(out, b, abs0 + p, p == t_hi - 1, best, bi);
                          } else {
                              const size_t e = ((size_t)b * cap + (p - p0)) * nblk + blk;
                              pval[e] = best;
                              pidx[e] = bi;
                          }
                      });
                  });
    state[lane] = int4_t{xp_i(lif.isyn), xp_i(lif.vmem), lif.total0, lif.total1};
    env_state[lane] = double2{tap.e0, tap.e1};
    if (lif.act0) {
        counts[(size_t)b * N + lif.n0] = lif.total0;
        env_last[(size_t)b * N + lif.n0] = tap.e0;
    }
    if (lif.act1) {
        counts[(size_t)b * N + lif.n1] = lif.total1;
        env_last[(size_t)b * N + lif.n1] = tap.e1;
    }
}

// one thread per position of the pair scratch; positions outside the launch's range (the same words) return
__global__ __launch_bounds__(256) void xylo_track_stream_combine_kernel(const double *__restrict__ pval, const int32_t *__restrict__ pidx,
                                                                        const int *__restrict__ ctl, int chunk_rows, int t_lo, int t_hi, int cap,
                                                                        int nblk, const XyloTrackSink out)
{
    const int p0 = ctl ? 0 : t_lo;
    if (!sx_range(ctl, chunk_rows, t_lo, t_hi)) return;
    const int abs0 = ctl ? ctl[STREAM_CLK_BASE] : 0;
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const int p = p0 + j;
    if (j >= cap || p < t_lo || p >= t_hi) return;
    const size_t e = ((size_t)b * cap + j) * nblk;
    double best;
    int bi;
    xylo_track_combine_row(pval + e, pidx + e, nblk, best, bi);
    xylo_track_ring_store(out, b, abs0 + p, p == t_hi - 1, best, bi);
}

size_t xylo_stream_track_state_bytes(int B, int N) { return (size_t)B * (xp_npad(N) / 2) * sizeof(double2); }

size_t xylo_stream_track_pairs_bytes(int B, int N, int cap)
{
    const int nblk = xp_npad(N) / XP_NEUR;
    return nblk == 1 ? 256 : xylo_track_pairs_size((size_t)B * cap * nblk);  // (one block writes the ring itself; never 0: that is "bad arguments")
}

// launch_xylo_resume's range and state with the tracked read-out; cap: the positions per trial of the pair scratch (a stream: the raster
// window's frames; by value: n)
hipError_t launch_xylo_track_resume(const int8_t *raster, int tc, int stride_frames, int B, int t0, int n, const int *ctl, int Cin, int N,
                                    int max_spikes, int32_t *counts, void *state, void *env_state, void *ws, int32_t *chunk_counts, int chunk_rows,
                                    double a_rise, double i_rise, double a_fall, int R, int32_t *index, double *peak, int32_t *latest_index,
                                    double *latest_peak, double *env_last, void *pairs, int cap, hipStream_t stream)
{
    if (Cin > 64 || Cin != 2 * tc || max_spikes < 1 || R < 1 || (reinterpret_cast<uintptr_t>(raster) & 15) != 0) return hipErrorInvalidValue;
    if (!ctl && n < 1) return hipSuccess;  // an empty range: nothing is launched, nothing rewritten
    if (cap < (ctl ? stride_frames : n)) return hipErrorInvalidValue;
    const XyloWs w = xylo_ws(ws, Cin, N);
    const XpShape sh = xp_shape(N, tc);
    const dim3 grid(sh.nblk, B), block(sh.waves * 64);
    const XyloTrackSink out{R, index, peak, latest_index, latest_peak};
    double *pval = nullptr;
    int32_t *pidx = nullptr;
    if (sh.nblk > 1) xylo_track_pairs_split(pairs, (size_t)B * cap * sh.nblk, pval, pidx);
    int4_t *stp = reinterpret_cast<int4_t *>(state);
    double2 *esp = reinterpret_cast<double2 *>(env_state);
    if (xp_kq(Cin) == 1)
        hipLaunchKernelGGL(xylo_lif_track_stream_kernel<1>, grid, block, sh.lds, stream, raster, tc, stride_frames, Cin, w.dWb, N, w.dds, w.ddm, w.dth,
                           max_spikes, counts, stp, esp, t0, t0 + n, ctl, chunk_counts, chunk_rows, a_rise, i_rise, a_fall, out, env_last, pval, pidx,
                           cap);
    else
        hipLaunchKernelGGL(xylo_lif_track_stream_kernel<2>, grid, block, sh.lds, stream, raster, tc, stride_frames, Cin, w.dWb, N, w.dds, w.ddm, w.dth,
                           max_spikes, counts, stp, esp, t0, t0 + n, ctl, chunk_counts, chunk_rows, a_rise, i_rise, a_fall, out, env_last, pval, pidx,
                           cap);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || sh.nblk == 1) return e;
    hipLaunchKernelGGL(xylo_track_stream_combine_kernel, dim3((unsigned)((cap + 255) / 256), B), dim3(256), 0, stream, pval, pidx, ctl, chunk_rows, t0,
                       t0 + n, cap, sh.nblk, out);
    return hipGetLastError();
}


}  // namespace micloc
