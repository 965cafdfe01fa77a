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
// The step functions, the MFMA `produce` and the staging loop are copies of xylo.hip's (its kernels are left as they are).
#include "stream_xylo.h"

namespace micloc {

namespace {

typedef short sx_short2 __attribute__((ext_vector_type(2)));
typedef int sx_int4 __attribute__((ext_vector_type(4)));

constexpr int SX_WAVES = 4;  // 4 x 128 = 512 neurons per workgroup
constexpr int SX_TT = 128;   // time steps staged per LDS tile
constexpr int SX_NEUR = SX_WAVES * 128;
constexpr int SX_CH = XYLO_STREAM_CHUNK;
constexpr int SX_MAXG = 4096;  // DoA grid of the read-out (its band sums live in LDS)

__device__ __forceinline__ sx_short2 sx_s2(int w) { return __builtin_bit_cast(sx_short2, w); }
__device__ __forceinline__ int sx_i(sx_short2 v) { return __builtin_bit_cast(int, v); }

// v - max(v >> dash, min(v, 1)): the "at least one LSB" decay, exact in packed 16 bit (xylo.hip)
__device__ __forceinline__ sx_short2 sx_decay(sx_short2 v, sx_short2 dash)
{
    const sx_short2 one = {1, 1};
    return v - __builtin_elementwise_max(v >> dash, __builtin_elementwise_min(v, one));
}

// exact floor(v / th) for 0 < th <= v <= 32767: fp32 quotient, corrected by +-1
__device__ __forceinline__ int sx_div(int v, int th)
{
    int n = (int)((float)v * __builtin_amdgcn_rcpf((float)th));
    n = n * th > v ? n - 1 : n;
    n = (n + 1) * th <= v ? n + 1 : n;
    return n;
}

template <int KQ, bool WANT_OUT>
__global__ __launch_bounds__(SX_WAVES * 64) void xylo_lif_stream_kernel(const int8_t *__restrict__ raster, int tc, int stride_frames, int Cin,
                                                                         const long *__restrict__ Wb /*[Npad][4 KQ]*/, int N,
                                                                         const uint8_t *__restrict__ dash_syn,
                                                                         const uint8_t *__restrict__ dash_mem,
                                                                         const short *__restrict__ thr, int max_spikes,
                                                                         uint8_t *__restrict__ spikes_out, int T_out, int *__restrict__ counts,
                                                                         sx_int4 *__restrict__ state, int t_lo, int t_hi,
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

    __shared__ __attribute__((aligned(16))) unsigned char tile[SX_TT][32 * KQ];
    extern __shared__ __attribute__((aligned(16))) int cur_dyn[];  // [waves][4][64][4]
    int(*cur)[4][64][4] = reinterpret_cast<int(*)[4][64][4]>(cur_dyn);
    int8_t *raw = reinterpret_cast<int8_t *>(cur_dyn);  // staging area for the raster bytes of a tile (between barriers)
    const int tid = threadIdx.x;
    const int nthreads = blockDim.x;
    const int wv = tid >> 6, l = tid & 63, lc = l & 15, q = l >> 4;
    const int b = blockIdx.y;
    const int nbase = blockIdx.x * SX_NEUR + wv * 128;

    // weight fragments of the wave's 8 column tiles: lane (q, lc) holds channels 8 q .. 8 q + 7 (+ 32 kq) of neuron 16 j + lc
    long Bw[8][KQ];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int kq = 0; kq < KQ; ++kq) Bw[j][kq] = Wb[(size_t)(nbase + 16 * j + lc) * (4 * KQ) + 4 * kq + q];

    const int n0 = nbase + 32 * q + lc, n1 = n0 + 16;
    const bool act0 = n0 < N, act1 = n1 < N;
    auto clamp15 = [](int d) { return d > 15 ? 15 : d; };
    const sx_short2 ds = {(short)(act0 ? clamp15(dash_syn[n0]) : 0), (short)(act1 ? clamp15(dash_syn[n1]) : 0)};
    const sx_short2 dm = {(short)(act0 ? clamp15(dash_mem[n0]) : 0), (short)(act1 ? clamp15(dash_mem[n1]) : 0)};
    const sx_short2 th = {(short)(act0 ? thr[n0] : 32767), (short)(act1 ? thr[n1] : 32767)};
    const int th_hi = (int)th.y << 16;  // v.hi >= th.hi  <=>  (int)word >= th.hi << 16

    // the trial's state of this lane pair: [B][Npad / 2] words of 16 bytes, neuron block major, then wave, then lane
    sx_int4 *st = state + (((size_t)b * gridDim.x + blockIdx.x) * SX_WAVES + wv) * 64 + l;
    const sx_int4 sv = *st;
    sx_short2 isyn = sx_s2(sv[0]), vmem = sx_s2(sv[1]);
    int total0 = sv[2], total1 = sv[3];
    int chunk0 = total0, chunk1 = total1;  // the totals at the start of the open chunk

    const int8_t *sb = raster + (size_t)b * stride_frames * tc;
    const int8_t *rend = raster + (size_t)gridDim.y * stride_frames * tc;
    uint8_t *ob = WANT_OUT ? spikes_out + (size_t)b * T_out * N : nullptr;

    // currents of 16 steps (tile16 `i` of the staged rows) -> the wave's LDS slice, ONE slice per wave: the 16 steps of a tile are in
    // registers before the next tile's currents overwrite them (the LDS operations of a wave execute in order)
    auto produce = [&](int i) {
        sx_int4 acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = sx_int4{0, 0, 0, 0};
#pragma unroll
        for (int kq = 0; kq < KQ; ++kq) {
            const long a = *reinterpret_cast<const long *>(&tile[16 * i + lc][32 * kq + 8 * q]);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = __builtin_amdgcn_mfma_i32_16x16x32_i8(a, Bw[j][kq], acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sx_int4 pk;
#pragma unroll
            for (int r = 0; r < 4; ++r) pk[r] = (int)__builtin_amdgcn_perm((unsigned)acc[2 * k + 1][r], (unsigned)acc[2 * k][r], 0x05040100u);
            *reinterpret_cast<sx_int4 *>(&cur[wv][q][16 * k + lc][0]) = pk;  // steps 4 q .. 4 q + 3 of pair lane 16 k + lc
        }
    };

    sx_short2 cnt = {0, 0};
    sx_short2 vmx = {-32768, -32768};
    // the fast step keeps the largest membrane word it left behind; one test per 16 steps decides whether some step needs the exact
    // sequence, and such a group is walked again from its saved state with the per-step test (`step`)
    auto step_fast = [&](int in_word, int t) {
        sx_short2 i2 = sx_decay(isyn, ds);
        sx_short2 v2 = sx_decay(vmem, dm);
        i2 = __builtin_elementwise_add_sat(i2, sx_s2(in_word));
        v2 = __builtin_elementwise_add_sat(v2, i2);
        const sx_short2 d = __builtin_elementwise_sub_sat(v2, th);
        const sx_short2 fifteen = {15, 15};
        const sx_short2 m = d >> fifteen;  // all ones: below threshold
        const int vw = (sx_i(m) & sx_i(v2)) | (~sx_i(m) & sx_i(d));
        cnt += m;
        vmx = __builtin_elementwise_max(vmx, sx_s2(vw));
        if constexpr (WANT_OUT) {
            const size_t row = (size_t)t * N;
            if (act0) ob[row + n0] = (uint8_t)(1 + m.x);
            if (act1) ob[row + n1] = (uint8_t)(1 + m.y);
        }
        isyn = i2;
        vmem = sx_s2(vw);
    };
    auto step = [&](int in_word, int t) {
        sx_short2 i2 = sx_decay(isyn, ds);
        sx_short2 v2 = sx_decay(vmem, dm);
        i2 = __builtin_elementwise_add_sat(i2, sx_s2(in_word));
        v2 = __builtin_elementwise_add_sat(v2, i2);
        const sx_short2 d = __builtin_elementwise_sub_sat(v2, th);
        const sx_short2 fifteen = {15, 15};
        const sx_short2 m = d >> fifteen;  // all ones: below threshold
        int vw = (sx_i(m) & sx_i(v2)) | (~sx_i(m) & sx_i(d));
        cnt += m;
        int extra0 = 0, extra1 = 0;
        // a second spike in the same step (v >= 2 th): exact 32-bit sequence, per half
        const bool again = ((short)vw >= th.x) | (vw >= th_hi);
        if (__builtin_expect(__any(again), 0)) {
            int lo = (short)vw, hi = vw >> 16;
            if (lo >= th.x) {
                int more = sx_div(lo, th.x);
                more = more < max_spikes - 1 ? more : max_spikes - 1;
                extra0 = more;
                lo -= more * th.x;
            }
            if (hi >= th.y) {
                int more = sx_div(hi, th.y);
                more = more < max_spikes - 1 ? more : max_spikes - 1;
                extra1 = more;
                hi -= more * th.y;
            }
            vw = (lo & 0xffff) | (hi << 16);
            total0 += extra0;
            total1 += extra1;
        }
        if constexpr (WANT_OUT) {
            const size_t row = (size_t)t * N;
            if (act0) ob[row + n0] = (uint8_t)(1 + m.x + extra0);
            if (act1) ob[row + n1] = (uint8_t)(1 + m.y + extra1);
        }
        isyn = i2;
        vmem = sx_s2(vw);
    };

    for (int t0 = t_lo; t0 < t_hi; t0 += SX_TT) {
        const int steps = (t_hi - t0) < SX_TT ? (t_hi - t0) : SX_TT;
        __syncthreads();  // every wave is done with the previous tile and with its slice of `cur`
        // the steps x tc raster bytes of this tile are contiguous: 16-byte loads into LDS (the slices of `cur` are idle between these
        // barriers), then the +1 / -1 split from there (channel c < tc: +1 events, tc + c: -1 events, zero padded to 32 KQ)
        {
            const int8_t *src = sb + (size_t)t0 * tc;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(src) & ~(uintptr_t)15;  // >= raster: the launcher checks its alignment
            const int off = (int)(reinterpret_cast<uintptr_t>(src) - a0);
            const int nvec = (off + steps * tc + 15) >> 4;
            const uint4 *vsrc = reinterpret_cast<const uint4 *>(a0);
            for (int e = tid; e < nvec; e += nthreads) {
                uint4 v;
                if (reinterpret_cast<const int8_t *>(vsrc + e + 1) <= rend) {
                    v = vsrc[e];
                } else {  // the last vector of the whole raster: only the bytes that exist
                    unsigned w4[4] = {0u, 0u, 0u, 0u};
                    const int8_t *p = reinterpret_cast<const int8_t *>(vsrc + e);
                    for (int i = 0; i < 16 && p + i < rend; ++i) w4[i >> 2] |= (unsigned)(unsigned char)p[i] << (8 * (i & 3));
                    v = uint4{w4[0], w4[1], w4[2], w4[3]};
                }
                reinterpret_cast<uint4 *>(raw)[e] = v;
            }
            __syncthreads();
            unsigned *tile32 = reinterpret_cast<unsigned *>(&tile[0][0]);
            for (int e = tid; e < SX_TT * 8 * KQ; e += nthreads) {
                const int r = e / (8 * KQ), k = e % (8 * KQ);
                unsigned w = 0;
                if (r < steps) {
                    const int8_t *row = raw + off + r * tc;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = 4 * k + i;
                        if (c < 2 * tc && c < Cin) {
                            const int sv1 = c < tc ? row[c] : -row[c - tc];
                            w |= (unsigned)(sv1 > 0) << (8 * i);
                        }
                    }
                }
                tile32[e] = w;
            }
        }
        __syncthreads();
        const int ntile = (steps + 15) >> 4;
        cnt = sx_short2{0, 0};
        produce(0);
        for (int i = 0; i < ntile; ++i) {
            const int jn = steps - 16 * i < 16 ? steps - 16 * i : 16;
            const sx_int4 *cw = reinterpret_cast<const sx_int4 *>(&cur[wv][0][l][0]);
            sx_int4 in4[4];
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) in4[t4] = cw[64 * t4];
            if (i + 1 < ntile) produce(i + 1);  // (overwrites the slice: after the reads above, in program order)
            if (jn == 16) {
                const sx_short2 isyn_s = isyn, vmem_s = vmem, cnt_s = cnt;
                vmx = sx_short2{-32768, -32768};
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) step_fast(in4[t4][r], t0 + 16 * i + 4 * t4 + r);
                }
                const sx_short2 fifteen = {15, 15};
                const sx_short2 below = __builtin_elementwise_sub_sat(vmx, th) >> fifteen;  // all ones: never reached th again
                if (__builtin_expect(__any(sx_i(below) != -1), 0)) {
                    isyn = isyn_s;
                    vmem = vmem_s;
                    cnt = cnt_s;
#pragma unroll
                    for (int t4 = 0; t4 < 4; ++t4) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) step(in4[t4][r], t0 + 16 * i + 4 * t4 + r);
                    }
                }
            } else {  // the last steps of the range
                for (int j = 0; j < jn; ++j) {
                    int w_in = 0;
#pragma unroll
                    for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
                        for (int r = 0; r < 4; ++r) w_in = (j == 4 * t4 + r) ? in4[t4][r] : w_in;
                    step(w_in, t0 + 16 * i + j);
                }
            }
        }
        total0 += steps + cnt.x;
        total1 += steps + cnt.y;
        // a chunk of the stream ends with this tile (the recording's last one may be ragged): its count, for the windowed read-out
        if (chunk_counts && (((t0 + steps) & (SX_CH - 1)) == 0 || t0 + steps == t_hi)) {
            int *cc = chunk_counts + ((size_t)b * chunk_rows + (t0 >> 8)) * N;
            if (act0) cc[n0] = total0 - chunk0;
            if (act1) cc[n1] = total1 - chunk1;
            chunk0 = total0;
            chunk1 = total1;
        }
    }
    *st = sx_int4{sx_i(isyn), sx_i(vmem), total0, total1};
    if (act0) counts[(size_t)b * N + n0] = total0;
    if (act1) counts[(size_t)b * N + n1] = total1;
}

static_assert(SX_CH == 256, "the chunk row of a tile is t0 >> 8");

// ---- the windows of one band: stream_window_kernel's bookkeeping (stream_windows.hip) on integer counts -------------------------------
// between the LIF launch and the commit of a tile.  chunk_counts [B][chunk_rows][N] holds the chunks that became final in this call at
// the window-relative rows [lo, hi); ctl[0] = chunks done before this call, ctl[6] = after it.  Window n keeps its sum so far in slot
// n % K of acc [B][K][N]; a window whose last chunk arrived (or, on the final tile, which the end of the recording cuts) goes to row
// n % Kb of ring [B][Kb][N] and head[0] becomes the number of windows emitted.
__global__ __launch_bounds__(256) void xylo_stream_window_kernel(const int *__restrict__ chunk_counts, int chunk_rows, int N,
                                                                  const int *__restrict__ ctl, int final_tile, int wchunks, int hchunks, int K,
                                                                  int Kb, int *__restrict__ acc, int *__restrict__ head, int *__restrict__ ring)
{
    const int b = blockIdx.x;
    const int done = ctl[0], lo = ctl[4], hi = ctl[5], ready = ctl[6];
    const int T = ctl[STREAM_CLK_TEND];
    const bool ended = final_tile && (long long)ready * SX_CH >= T;
    if (ready - done != hi - lo || hi < lo || lo < 0 || hi > chunk_rows) return;  // (never: the horizon writes both)
    const int n0 = done < wchunks ? 0 : (done - wchunks) / hchunks + 1;  // first window not emitted before this call
    const int n_started = ready > 0 ? (ready - 1) / hchunks : -1;        // last window that holds a chunk
    long long n_emit;                                                    // windows emitted after this call
    if (ended)
        n_emit = T <= (long long)wchunks * SX_CH ? 1 : 1 + ((long long)T - (long long)wchunks * SX_CH + (long long)hchunks * SX_CH - 1) / ((long long)hchunks * SX_CH);
    else
        n_emit = ready < wchunks ? 0 : (ready - wchunks) / hchunks + 1;
    const int *cb_ = chunk_counts + (size_t)b * chunk_rows * N;
    for (int n = n0; n <= n_started; ++n) {
        const int c0 = n * hchunks;
        const int ca = done > c0 ? done : c0;
        const int cb = ready - c0 < wchunks ? ready : c0 + wchunks;
        const bool emit = n < n_emit;
        int *slot = acc + ((size_t)b * K + n % K) * N;
        int *row = ring + ((size_t)b * Kb + n % Kb) * N;
        for (int g = threadIdx.x; g < N; g += 256) {
            int total = ca > c0 ? slot[g] : 0;  // (the window opened in an earlier call)
            for (int ch = ca; ch < cb; ++ch) total += cb_[(size_t)(lo + ch - done) * N + g];
            if (emit) {
                row[g] = total;
                slot[g] = 0;
            } else {
                slot[g] = total;
            }
        }
    }
    if (b == 0 && threadIdx.x == 0) head[0] = (int)(n_emit > 0x7fffffffll ? 0x7fffffffll : n_emit);
}

// ---- the read-out over the bands -----------------------------------------------------------------------------------------------------
// peak_location_kernel's estimator (sweep.hip) on the band sums pw[G] in LDS: box-car of `win` samples by a full, non-circular
// convolution, first maximum, minus win / 2, modulo G.  Every thread of the workgroup calls it; thread 0 returns the index.
__device__ int sx_peak(const long long *pw, int G, int win, long long *bestv, int *besti)
{
    long long bv = -1;
    int bi = 0x7fffffff;
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
    bestv[threadIdx.x] = bv;
    besti[threadIdx.x] = bi;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const long long ov = bestv[threadIdx.x + h];
            const int oi = besti[threadIdx.x + h];
            if (ov > bestv[threadIdx.x] || (ov == bestv[threadIdx.x] && oi < besti[threadIdx.x])) {
                bestv[threadIdx.x] = ov;
                besti[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    int idx = besti[0] - win / 2;
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
    int newc = 0x7fffffff;
    for (int f = 0; f < F; ++f) newc = a.head[f][0] < newc ? a.head[f][0] : newc;
    const long long Tend = a.ctl[0][STREAM_CLK_T];  // frames pushed (the bands share the clock; the tick is behind every band's tile)
    int given = 0;
    for (int n = emitted; n < newc; ++n) {
        bool lost = false;
        for (int f = 0; f < F; ++f) lost = lost || a.head[f][0] - n > Kb;
        if (lost) {  // (uniform over the launch)
            ++given;
            continue;
        }
        long long frames = Tend - (long long)n * hop;
        frames = frames > window ? window : (frames < 1 ? 1 : frames);
        const size_t row = (size_t)b * max_windows + n % max_windows;
        const bool newest = n == newc - 1;
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
        state[2] = newc > emitted ? newc : emitted;
        state[3] = state[1] + given;
    }
}

__global__ void xylo_stream_readout_commit_kernel(int *__restrict__ state)
{
    state[0] = state[2];
    state[1] = state[3];
}

int sx_npad(int N) { return ((N + SX_NEUR - 1) / SX_NEUR) * SX_NEUR; }
size_t sx_al(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

size_t xylo_stream_state_bytes(int B, int N) { return (size_t)B * (sx_npad(N) / 2) * sizeof(sx_int4); }

size_t xylo_stream_chunk_bytes(int B, int N, int chunk_rows) { return sx_al((size_t)B * chunk_rows * N * sizeof(int)); }

// raster: int8 [B][stride_frames][tc], 16-byte aligned; ws: xylo_upload's.  ctl == NULL: the frames [t0, t0 + n) by value.
hipError_t launch_xylo_resume(const int8_t *raster, int tc, int stride_frames, int B, int t0, int n, const int *ctl, int Cin, int N, int max_spikes,
                              uint8_t *spikes_out, int T_out, int32_t *counts, void *state, void *ws, int32_t *chunk_counts, int chunk_rows,
                              hipStream_t stream)
{
    if (Cin > 64 || Cin != 2 * tc || max_spikes < 1 || (reinterpret_cast<uintptr_t>(raster) & 15) != 0) return hipErrorInvalidValue;
    if (!ctl && n < 1) return hipSuccess;  // an empty range: nothing is launched, nothing rewritten
    // xylo_upload's layout (xylo.hip): [packed dwords][dash_syn][dash_mem][thresholds][neuron-major byte matrix]
    unsigned char *base = reinterpret_cast<unsigned char *>(ws);
    const int nq = (Cin + 3) / 4;
    const size_t off = sx_al((size_t)nq * N * sizeof(int));
    const size_t seg = sx_al((size_t)N * 2);
    const uint8_t *dds = base + off;
    const uint8_t *ddm = base + off + seg;
    const short *dth = reinterpret_cast<const short *>(base + off + 2 * seg);
    const long *dWb = reinterpret_cast<const long *>(base + off + 3 * seg);
    const int nblk = sx_npad(N) / SX_NEUR;
    const int waves = nblk > 1 ? SX_WAVES : (N + 127) / 128;  // as many waves as hold neurons, the same in every workgroup
    const dim3 grid(nblk, B), block(waves * 64);
    size_t lds = (size_t)waves * 4 * 64 * 4 * sizeof(int);
    const size_t rawb = (size_t)SX_TT * tc + 48;
    lds = lds > rawb ? lds : rawb;
    sx_int4 *stp = reinterpret_cast<sx_int4 *>(state);
#define SX_LAUNCH(KQ, WO)                                                                                                                \
    hipLaunchKernelGGL((xylo_lif_stream_kernel<KQ, WO>), grid, block, lds, stream, raster, tc, stride_frames, Cin, dWb, N, dds, ddm, dth, \
                       max_spikes, spikes_out, T_out, counts, stp, t0, t0 + n, ctl, chunk_counts, chunk_rows)
    if (Cin <= 32) {
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

// win_state: [256 B: int windows emitted][acc [B][K][N] ints][ring [B][Kb][N] ints], K = ceil(window / hop)
size_t xylo_stream_window_state_bytes(int B, int N, int window, int hop, int Kb)
{
    const int K = (window + hop - 1) / hop;
    return 256 + sx_al((size_t)B * K * N * sizeof(int)) + sx_al((size_t)B * Kb * N * sizeof(int));
}

static int *sx_ring(void *win_state, int B, int N, int window, int hop)
{
    const int K = (window + hop - 1) / hop;
    return reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(win_state) + 256 + sx_al((size_t)B * K * N * sizeof(int)));
}

hipError_t launch_xylo_stream_windows(const int32_t *chunk_counts, int B, int chunk_rows, int N, const int *ctl, int final_tile, int window, int hop,
                                      int Kb, void *win_state, hipStream_t stream)
{
    if (window < 1 || hop < 1 || hop > window || window % SX_CH != 0 || hop % SX_CH != 0 || Kb < 1) return hipErrorInvalidValue;
    int *head = reinterpret_cast<int *>(win_state);
    int *acc = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(win_state) + 256);
    hipLaunchKernelGGL(xylo_stream_window_kernel, dim3(B), dim3(256), 0, stream, chunk_counts, chunk_rows, N, ctl, final_tile ? 1 : 0, window / SX_CH,
                       hop / SX_CH, (window + hop - 1) / hop, Kb, acc, head, sx_ring(win_state, B, N, window, hop));
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

}  // namespace micloc
