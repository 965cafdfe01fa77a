// Xylo-A2 (SYNS61201) hidden-layer integer LIF on gfx950 -- BASELINE config 4.
//
// PARITY UNPINNED.  In the reference this stage is rockpool's XyloSim (C++/pybind `xylosim`, third party, not
// vendored, unpinned in setup.py:19, not installed in the build image) called from
// micloc/xylo_snn_localization.py:269-290 (from_config) and :358-377 (xylo_process).  The kernel follows the
// published Xylo update rule exactly as restated in oracle/micloc_oracle.c (oracle_xylo_lif): bit-shift decay with
// the "at least 1 LSB" rule, 8-bit weights, saturating 16-bit synaptic current and membrane, subtractive reset
// with a per-step spike cap, one shared recurrent weight.  HIP == oracle bit for bit; oracle != checked
// against XyloSim.
//
// Two kernels.  xylo_lif_kernel (general: spike counts in, recurrence): lane = hidden neuron, workgroup = one trial x
// up to 1024 neurons, sequential over time (integer state recurrences); the input channels are packed 4 x int8 per dword
// and contracted with v_dot4_i32_i8; input spike rows are staged 256 steps at a time in LDS and read as wave-uniform
// (broadcast) dwords.  xylo_lif_pk_kernel (the sweep: binary events, no recurrence): two neurons per lane in packed
// 16-bit arithmetic, input currents from the int8 matrix cores -- the lane's walk is XpLif of xylo_rows.h, shared with the stream's
// kernel (stream_xylo.hip); here are its two launch forms.
// Each has a CHUNK-COUNT form for the time-resolved read-out (xylo_lif_kernel<REC, NQ, true>, xylo_lif_pk_chunks_kernel: the same walk,
// which also leaves the spike count of every 256 frames), and xylo_window_kernel adds those rows per window: "time-resolved DoA" below,
// PARITY UNPINNED like everything here.
// At the end of the file stands the packed walk's TRACKING form, xylo_lif_track_kernel (the envelope of the counts and the first maximum
// over the neurons per frame), around the tap of xylo_track_rows.h.
#include <vector>

#include "micloc_internal.h"
#include "xylo_rows.h"
#include "xylo_track.h"
#include "xylo_track_rows.h"
#include "xylo_windows.h"

// (the recurrent instantiations keep a barrier inside the step loop, which the requested unrolling skips)
#pragma clang diagnostic ignored "-Wpass-failed"

namespace micloc {

constexpr int XY_TT = 256;   // time steps staged per LDS tile
static_assert(XY_TT == XP_CHUNK, "a staged tile of the general kernel is one chunk of the windowed read-out");
constexpr int XY_MAXQ = 16;  // up to 64 input channels

__device__ __forceinline__ int xy_sat16(int v) { return v > 32767 ? 32767 : (v < -32768 ? -32768 : v); }

// v - dv with dv = v >> dash, "at least one LSB" while v != 0.  The arithmetic shift of a negative value is never 0
// (-1 at least), so the rule only ever fires for 0 < v < 2^dash, where it sets dv = 1:  dv = max(v >> dash, min(v, 1))
// (v > 0: max(., 1);  v = 0: 0;  v < 0: v >> dash >= v).  Three instructions instead of seven.
__device__ __forceinline__ int xy_decay(int v, int dash)
{
    const int dv = max(v >> dash, min(v, 1));
    return v - dv;
}

// NQ = dwords of packed input per step (compile time: the contraction unrolls into NQ v_dot4 with no branches; the
// staged row is read with wide, wave-uniform LDS loads).
// CHUNKS: the chunk-count form (the windowed read-out, "time-resolved DoA" below).  The staged tile is one chunk of XP_CHUNK frames, and at
// its end the lane also writes its count since the previous tile to chunk_counts [B][ceil(T / XP_CHUNK)][N]; rate may be NULL; no raster out.
template <bool REC, int NQ, bool CHUNKS = false>
__global__ __launch_bounds__(1024) void xylo_lif_kernel(const uint8_t *__restrict__ spikes_in, int ternary_C, int T, int Cin,
                                                         const int *__restrict__ Wpk /*[nq][N]*/, int nq, int N, int w_rec,
                                                         const uint8_t *__restrict__ dash_syn,
                                                         const uint8_t *__restrict__ dash_mem,
                                                         const short *__restrict__ thr, int max_spikes,
                                                         uint8_t *__restrict__ spikes_out, int *__restrict__ rate,
                                                         int *__restrict__ chunk_counts)
{
    __shared__ __attribute__((aligned(16))) int tile[XY_TT][NQ];
    __shared__ int wsum[2][16];
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    const bool act = g < N;
    int w[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) w[k] = (act && k < nq) ? Wpk[(size_t)k * N + g] : 0;
    const int ds = act ? dash_syn[g] : 0, dm = act ? dash_mem[g] : 0;
    const int th = act ? thr[g] : 32767;
    int isyn = 0, vmem = 0, total = 0, prev_total = 0;
    [[maybe_unused]] int chunk_total = 0;  // CHUNKS: `total` at the start of the tile
    // ternary_C > 0: the input is the encoder's int8 raster [B][T][ternary_C] in {-1, 0, +1}; channel c carries its +1
    // events, channel ternary_C + c its -1 events (Demo.spike_encoding's split, xylo_snn_localization.py:350-354)
    const int Crow = ternary_C > 0 ? ternary_C : Cin;
    const uint8_t *sb = spikes_in + (size_t)b * T * Crow;
    const int8_t *sbt = reinterpret_cast<const int8_t *>(sb);
    [[maybe_unused]] uint8_t *ob = nullptr;
    if constexpr (!CHUNKS) ob = spikes_out ? spikes_out + (size_t)b * T * N : nullptr;
    const int nwaves = blockDim.x >> 6;

    for (int t0 = 0; t0 < T; t0 += XY_TT) {
        const int steps = (T - t0) < XY_TT ? (T - t0) : XY_TT;
        __syncthreads();
        // stage `steps` rows of Cin bytes, zero padded to NQ dwords
        uint8_t *tb = reinterpret_cast<uint8_t *>(&tile[0][0]);
        for (int e = threadIdx.x; e < steps * NQ * 4; e += blockDim.x) {
            const int r = e / (NQ * 4), c = e % (NQ * 4);
            uint8_t v = 0;
            if (c < Cin) {
                if (ternary_C > 0)
                    v = c < ternary_C ? (uint8_t)(sbt[(size_t)(t0 + r) * Crow + c] > 0) : (uint8_t)(sbt[(size_t)(t0 + r) * Crow + c - ternary_C] < 0);
                else
                    v = sb[(size_t)(t0 + r) * Cin + c];
            }
            tb[e] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < steps; ++j) {
            int in = 0;
#pragma unroll
            for (int k = 0; k < NQ; ++k) in = __builtin_amdgcn_sdot4(w[k], tile[j][k], in, false);
            int i2 = xy_decay(isyn, ds);
            int v2 = xy_decay(vmem, dm);
            i2 = xy_sat16(i2 + in + (REC ? w_rec * prev_total : 0));
            v2 = xy_sat16(v2 + i2);
            // subtractive reset until below threshold or until the per-step cap: almost always zero or one spike, so the
            // first one is branch-free and only a wave in which some neuron still sits above threshold takes the division
            int n = v2 >= th ? 1 : 0;
            v2 -= n ? th : 0;
            if (__builtin_expect(__any(v2 >= th), 0)) {  // (cap >= 1 by the API contract)
                if (v2 >= th) {
                    int more = xy_div(v2, th);
                    more = more < max_spikes - 1 ? more : max_spikes - 1;
                    n += more;
                    v2 -= more * th;
                }
            }
            isyn = i2;
            vmem = v2;
            total += n;
            if constexpr (!CHUNKS)
                if (ob && act) ob[(size_t)(t0 + j) * N + g] = (uint8_t)n;
            if (REC) {
                // block-wide sum of this step's spikes feeds every neuron at the next step
                int s = n;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                const int p = j & 1;
                if ((threadIdx.x & 63) == 0) wsum[p][threadIdx.x >> 6] = s;
                __syncthreads();
                int tot = 0;
                for (int k2 = 0; k2 < nwaves; ++k2) tot += wsum[p][k2];
                prev_total = tot;
            }
        }
        if constexpr (CHUNKS) {
            if (act) chunk_counts[((size_t)b * ((T + XY_TT - 1) / XY_TT) + t0 / XY_TT) * N + g] = total - chunk_total;  // CHUNKS
            chunk_total = total;                                                                                      // CHUNKS
        }
    }
    if (rate && act) rate[(size_t)b * N + g] = total;
}

// QUEUE (the sweep: counts only): the launch is a fixed set of PERSISTENT workgroups -- four per CU, twelve waves on four SIMDs --
// that take (trial, time chunk) tickets from a device counter, trial fastest, so that every trial advances chunk by chunk and the
// integer state of a trial (two packed words and two counts per lane) is handed from one workgroup to the next through memory.
// A trial is a serial chain of T steps and all chains are equally long: launched as one workgroup per trial, 1100 x 3 waves land
// on 1024 SIMDs as three waves here and four there, and the launch lasts as long as the SIMDs that got four (80 % balance,
// tools/wave_placement.hip).  With tickets every SIMD holds the same three waves from start to end and the chip as a whole works
// off ceil(chunks x trials / 1024) rounds.  A ticket's predecessor (same trial, previous chunk) was handed out `trials` tickets
// earlier to a workgroup that is RUNNING (tickets are only taken by resident workgroups), so the wait for it always ends; it is
// bounded all the same (a worker that gives up sets the error word and the launch drains).
constexpr int XQ_CTL = 64;         // control ints in front of the per-trial chunk counters: [0] ticket, [1] error
constexpr int XQ_SPIN_MAX = 1 << 24;  // x (s_sleep 8 + one coherent load, ~2 us): half a minute -- a predecessor on a crowded chip takes milliseconds

template <int KQ, bool WANT_OUT, bool QUEUE = false>
__global__ __launch_bounds__(XP_WAVES * 64) void xylo_lif_pk_kernel(const int8_t *__restrict__ raster, int tc, int T, int Cin,
                                                                     const long *__restrict__ Wb /*[Npad][4 KQ]*/, int N,
                                                                     const uint8_t *__restrict__ dash_syn,
                                                                     const uint8_t *__restrict__ dash_mem,
                                                                     const short *__restrict__ thr, int max_spikes,
                                                                     uint8_t *__restrict__ spikes_out, int *__restrict__ rate,
                                                                     int *__restrict__ qctl, int4_t *__restrict__ qstate, int Lc, int ntrials)
{
    __shared__ __attribute__((aligned(16))) unsigned char tile[XP_TT][32 * KQ];
    extern __shared__ __attribute__((aligned(16))) int cur_dyn[];  // [waves][4][64][4]: only the waves that hold neurons
    XpLif<KQ, WANT_OUT> lif;
    lif.init(tile, cur_dyn, QUEUE ? 0 : blockIdx.x * XP_NEUR, Wb, N, dash_syn, dash_mem, thr, max_spikes);  // (QUEUE: one neuron block, N <= 512)
    const int tid = lif.tid, wv = lif.wv, l = lif.l;
    const int n0 = lif.n0, n1 = lif.n1;
    const bool act0 = lif.act0, act1 = lif.act1;
    const int8_t *rend = raster + (size_t)(QUEUE ? ntrials : (int)gridDim.y) * T * tc;
    auto none = [](int, int) {};
    if constexpr (!QUEUE) {
        const int b = blockIdx.y;
        if constexpr (WANT_OUT) lif.ob = spikes_out + (size_t)b * T * N;
        lif.run_range(raster + (size_t)b * T * tc, rend, tc, Cin, 0, T, none);
        if (rate) {
            if (act0) rate[(size_t)b * N + n0] = lif.total0;
            if (act1) rate[(size_t)b * N + n1] = lif.total1;
        }
    } else {
        __shared__ int s_ticket;
        const int nchunks = (T + Lc - 1) / Lc;
        const int nitems = nchunks * ntrials;
        // (one barrier in front of the write keeps the previous ticket's readers ahead of it, one behind publishes the new one;
        //  the value is made a scalar: every branch on it is a scalar branch, no lane can leave a wave early)
        auto next_ticket = [&]() {
            __syncthreads();
            if (tid == 0) s_ticket = atomicAdd(&qctl[0], 1);
            __syncthreads();
            return __builtin_amdgcn_readfirstlane(s_ticket);
        };
        for (int ticket = next_ticket(); ticket < nitems; ticket = next_ticket()) {  // (the counter only grows: every worker leaves)
            const int chunk = ticket / ntrials;
            const int b = ticket - chunk * ntrials;
            int4_t *st = qstate + ((size_t)b * XP_WAVES + wv) * 64 + l;
            if (chunk > 0) {
                if (tid == 0) {
                    int spins = 0;
                    while (__hip_atomic_load(&qctl[XQ_CTL + b], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < chunk) {
                        __builtin_amdgcn_s_sleep(8);
                        if (++spins > XQ_SPIN_MAX) {  // never seen; keeps a broken launch from hanging the device
                            atomicExch(&qctl[1], 1);
                            break;
                        }
                    }
                }
                __syncthreads();
                __threadfence();  // acquire for every lane: the state below was written by another workgroup, maybe on another XCD
                const int4_t v = *st;
                lif.isyn = xp_s2(v[0]);
                lif.vmem = xp_s2(v[1]);
                lif.total0 = v[2];
                lif.total1 = v[3];
            } else {
                lif.isyn = short2_t{0, 0};
                lif.vmem = short2_t{0, 0};
                lif.total0 = lif.total1 = 0;
            }
            const int t_lo = chunk * Lc;
            const int t_hi = t_lo + Lc < T ? t_lo + Lc : T;
            lif.run_range(raster + (size_t)b * T * tc, rend, tc, Cin, t_lo, t_hi, none);
            if (chunk + 1 < nchunks) {
                *st = int4_t{xp_i(lif.isyn), xp_i(lif.vmem), lif.total0, lif.total1};
                __threadfence();  // release: the state is visible device-wide before the chunk counter says so
                __syncthreads();
                if (tid == 0) __hip_atomic_store(&qctl[XQ_CTL + b], chunk + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                // a worker that gave up waiting (never seen) went on from an unwritten state: whatever is finished after that is marked,
                // not returned as plausible counts (the host side raises at its next synchronisation point, XyloNetwork.check)
                const bool broken = __hip_atomic_load(&qctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                if (act0) rate[(size_t)b * N + n0] = broken ? -1 : lif.total0;
                if (act1) rate[(size_t)b * N + n1] = broken ? -1 : lif.total1;
            }
        }
    }
}

__global__ void xylo_queue_reset_kernel(int *qctl, int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) qctl[i] = 0;
}

size_t xylo_ws_bytes(int Cin, int N) { return xylo_ws(nullptr, Cin, N).bytes; }

// Uploads the packed weights and per-neuron constants into `ws` (synchronises the stream once).
hipError_t xylo_upload(int Cin, const int8_t *W_in_host, int N, const uint8_t *dash_syn_host, const uint8_t *dash_mem_host,
                       const int16_t *thr_host, void *ws, hipStream_t stream)
{
    const int nq = (Cin + 3) / 4;
    if (nq > XY_MAXQ) return hipErrorInvalidValue;
    const XyloWs w = xylo_ws(ws, Cin, N);
    // pack 4 input channels per dword: byte i of word k = W_in[4k + i][g]
    std::vector<int> pk((size_t)nq * N, 0);
    for (int k = 0; k < nq; ++k)
        for (int g = 0; g < N; ++g) {
            unsigned v = 0;
            for (int i = 0; i < 4; ++i) {
                const int c = 4 * k + i;
                const unsigned byte = c < Cin ? (unsigned char)W_in_host[(size_t)c * N + g] : 0u;
                v |= byte << (8 * i);
            }
            pk[(size_t)k * N + g] = (int)v;
        }
    hipError_t e = hipMemcpyAsync(w.dW, pk.data(), pk.size() * sizeof(int), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemcpyAsync(w.dds, dash_syn_host, (size_t)N, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(w.ddm, dash_mem_host, (size_t)N, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(w.dth, thr_host, (size_t)N * 2, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    std::vector<int8_t> wb;
    if (Cin <= 64) {
        // neuron-major bytes for the matrix-core form: Wb[n][c], rows of 32 KQ bytes, neurons padded to whole workgroups
        const int row = 32 * xp_kq(Cin);
        wb.assign((size_t)xp_npad(N) * row, 0);
        for (int c = 0; c < Cin; ++c)
            for (int g = 0; g < N; ++g) wb[(size_t)g * row + c] = W_in_host[(size_t)c * N + g];
        if ((e = hipMemcpyAsync(w.dWb, wb.data(), wb.size(), hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    }
    return hipStreamSynchronize(stream);  // `pk` / `wb` are host temporaries
}

// The general form's launch, with the chunk counts (chunk_counts != NULL: no raster) or without.  Without recurrence the neurons are
// independent: as few, as full workgroups as possible (N = 360 -> one of 384 threads instead of 256 + 104: every wave of the launch
// issues the same instructions whether its lanes are used or not).
static void xylo_launch_general(const XyloWs &w, const uint8_t *sp, int ternary_C, int B, int T, int Cin, int N, int w_rec, int max_spikes,
                                uint8_t *spikes_out, int32_t *rate, int32_t *chunk_counts, hipStream_t stream)
{
    const int nq = (Cin + 3) / 4;
    const int nblocks = w_rec != 0 ? 1 : (N + 511) / 512;
    const int per = (N + nblocks - 1) / nblocks;
    const dim3 block(((per + 63) / 64) * 64), grid(nblocks, B);
#define XY_KERNEL(REC, NQ, CHUNKS)                                                                                                    \
    hipLaunchKernelGGL((xylo_lif_kernel<REC, NQ, CHUNKS>), grid, block, 0, stream, sp, ternary_C, T, Cin, w.dW, nq, N, REC ? w_rec : 0, \
                       w.dds, w.ddm, w.dth, max_spikes, spikes_out, rate, chunk_counts)
#define XY_LAUNCH(NQ)                      \
    do {                                   \
        if (chunk_counts && w_rec != 0)    \
            XY_KERNEL(true, NQ, true);     \
        else if (chunk_counts)             \
            XY_KERNEL(false, NQ, true);    \
        else if (w_rec != 0)               \
            XY_KERNEL(true, NQ, false);    \
        else                               \
            XY_KERNEL(false, NQ, false);   \
    } while (0)
    if (nq <= 2)
        XY_LAUNCH(2);
    else if (nq <= 4)
        XY_LAUNCH(4);
    else if (nq <= 7)
        XY_LAUNCH(7);
    else if (nq <= 8)
        XY_LAUNCH(8);
    else
        XY_LAUNCH(16);
#undef XY_LAUNCH
#undef XY_KERNEL
}

// Runs the network whose constants xylo_upload placed in `ws`: no host access, no synchronisation (graph-capturable).
hipError_t launch_xylo_resident(const void *spikes_in, int ternary_C, int B, int T, int Cin, int N, int w_rec, int max_spikes,
                                uint8_t *spikes_out, int32_t *rate, void *ws, hipStream_t stream)
{
    const int nq = (Cin + 3) / 4;
    if (nq > XY_MAXQ) return hipErrorInvalidValue;
    const XyloWs w = xylo_ws(ws, Cin, N);
    const uint8_t *sp = reinterpret_cast<const uint8_t *>(spikes_in);
    if (w_rec != 0 && N > 1024) return hipErrorInvalidValue;
    if (w_rec == 0 && ternary_C > 0 && Cin <= 64 && max_spikes >= 1 && (reinterpret_cast<uintptr_t>(spikes_in) & 15) == 0) {
        // binary events, independent neurons: two neurons per lane, input currents on the matrix cores
        const XpShape sh = xp_shape(N, ternary_C);
        const dim3 pgrid(sh.nblk, B), pblock(sh.waves * 64);
        const int8_t *rs = reinterpret_cast<const int8_t *>(spikes_in);
#define XP_LAUNCH(KQ, WO)                                                                                                      \
    hipLaunchKernelGGL((xylo_lif_pk_kernel<KQ, WO>), pgrid, pblock, sh.lds, stream, rs, ternary_C, T, Cin, w.dWb, N, w.dds, w.ddm, \
                       w.dth, max_spikes, spikes_out, rate, nullptr, nullptr, 0, B)
        if (xp_kq(Cin) == 1) {
            if (spikes_out)
                XP_LAUNCH(1, true);
            else
                XP_LAUNCH(1, false);
        } else {
            if (spikes_out)
                XP_LAUNCH(2, true);
            else
                XP_LAUNCH(2, false);
        }
#undef XP_LAUNCH
        return hipGetLastError();
    }
    xylo_launch_general(w, sp, ternary_C, B, T, Cin, N, w_rec, max_spikes, spikes_out, rate, nullptr, stream);
    return hipGetLastError();
}

// ---- time-resolved DoA: the counts per window of `window` frames every `hop` frames (include/micloc_hip.h "time-resolved DoA, Xylo";
// DESIGN 4.25) ----------------------------------------------------------------------------------------------------------------------------
// The LIF walks a trial ONCE, without a reset between windows, and leaves the count of every chunk of 256 frames -- the stream's quantum --
// in chunk_counts [B][ceil(T / 256)][N]; xylo_window_kernel adds the chunk rows of every window.  Integers: no ordering contract.
//
// The chunk-count form of the packed one-shot launch (xylo_lif_pk_kernel<KQ, false>: one workgroup per trial and neuron block): the walk is
// XpLif's, `done` is the stream's (xp_chunk_done, xylo_rows.h).
template <int KQ>
__global__ __launch_bounds__(XP_WAVES * 64) void xylo_lif_pk_chunks_kernel(const int8_t *__restrict__ raster, int tc, int T, int Cin,
                                                                            const long *__restrict__ Wb /*[Npad][4 KQ]*/, int N,
                                                                            const uint8_t *__restrict__ dash_syn,
                                                                            const uint8_t *__restrict__ dash_mem,
                                                                            const short *__restrict__ thr, int max_spikes, int *__restrict__ rate,
                                                                            int *__restrict__ chunk_counts /*[B][chunk_rows][N]*/, int chunk_rows)
{
    __shared__ __attribute__((aligned(16))) unsigned char tile[XP_TT][32 * KQ];
    extern __shared__ __attribute__((aligned(16))) int cur_dyn[];  // [waves][4][64][4]: only the waves that hold neurons
    XpLif<KQ, false> lif;
    lif.init(tile, cur_dyn, blockIdx.x * XP_NEUR, Wb, N, dash_syn, dash_mem, thr, max_spikes);
    const int b = blockIdx.y;
    int chunk0 = 0, chunk1 = 0;  // the totals at the start of the open chunk
    lif.run_range(raster + (size_t)b * T * tc, raster + (size_t)gridDim.y * T * tc, tc, Cin, 0, T,
                  [&](int t0, int steps) { xp_chunk_done(lif, chunk_counts, chunk_rows, b, t0, steps, T, chunk0, chunk1); });
    if (rate) {
        if (lif.act0) rate[(size_t)b * N + lif.n0] = lif.total0;
        if (lif.act1) rate[(size_t)b * N + lif.n1] = lif.total1;
    }
}

// window_counts[b][n][g] = sum of the chunk rows [n hchunks, min(n hchunks + wchunks, chunk_rows)) of trial b.  Workgroup = 256 adjacent
// neurons of one (trial, window): every row is read with coalesced loads, every output has one writer (no atomics).
__global__ __launch_bounds__(256) void xylo_window_kernel(const int *__restrict__ chunk_counts, int chunk_rows, int N, int nW, unsigned pairs,
                                                           int wchunks, int hchunks, int *__restrict__ window_counts)
{
    const int g = blockIdx.y * 256 + threadIdx.x;
    if (g >= N) return;
    for (unsigned bw = blockIdx.x; bw < pairs; bw += gridDim.x) {  // (trial, window) pairs, B nW of them
        const int b = (int)(bw / (unsigned)nW), n = (int)(bw - (unsigned)b * (unsigned)nW);
        const int c0 = n * hchunks;  // (< chunk_rows: window n starts inside the recording)
        const int c1 = chunk_rows - c0 < wchunks ? chunk_rows : c0 + wchunks;
        const int *rows = chunk_counts + (size_t)b * chunk_rows * N + g;
        int total = 0;
        for (int c = c0; c < c1; ++c) total += rows[(size_t)c * N];
        window_counts[(size_t)bw * N + g] = total;
    }
}

// workgroups over the (trial, window) pairs of the two window kernels: one each, or a fixed number that strides over them (a grid's
// x extent times the workgroup size stays below 2^32)
unsigned xylo_window_grid(unsigned pairs) { return pairs < (1u << 20) ? pairs : (1u << 20); }

size_t xylo_windows_chunk_bytes(int B, int T, int N) { return (size_t)B * ((T + XP_CHUNK - 1) / XP_CHUNK) * N * sizeof(int); }

// launch_xylo_resident's routing with the chunk-count forms, then the window sums: two launches whatever B and nW; no host access, no
// synchronisation (graph-capturable).  window, hop: multiples of XP_CHUNK, hop <= window; nW: window_count(T, window, hop); B nW < 2^31.
hipError_t launch_xylo_windows(const void *spikes_in, int ternary_C, int B, int T, int Cin, int N, int w_rec, int max_spikes, int window, int hop,
                               int nW, int32_t *window_counts, int32_t *rate, void *ws, int32_t *chunk_counts, hipStream_t stream)
{
    const int nq = (Cin + 3) / 4;
    if (nq > XY_MAXQ || (w_rec != 0 && N > 1024) || max_spikes < 1) return hipErrorInvalidValue;
    if (window < 1 || hop < 1 || hop > window || window % XP_CHUNK != 0 || hop % XP_CHUNK != 0 || nW < 1) return hipErrorInvalidValue;
    const XyloWs w = xylo_ws(ws, Cin, N);
    const int chunk_rows = (T + XP_CHUNK - 1) / XP_CHUNK;
    if (w_rec == 0 && ternary_C > 0 && Cin <= 64 && (reinterpret_cast<uintptr_t>(spikes_in) & 15) == 0) {
        const XpShape sh = xp_shape(N, ternary_C);
        const dim3 pgrid(sh.nblk, B), pblock(sh.waves * 64);
        const int8_t *rs = reinterpret_cast<const int8_t *>(spikes_in);
        if (xp_kq(Cin) == 1)
            hipLaunchKernelGGL(xylo_lif_pk_chunks_kernel<1>, pgrid, pblock, sh.lds, stream, rs, ternary_C, T, Cin, w.dWb, N, w.dds, w.ddm, w.dth,
                               max_spikes, rate, chunk_counts, chunk_rows);
        else
            hipLaunchKernelGGL(xylo_lif_pk_chunks_kernel<2>, pgrid, pblock, sh.lds, stream, rs, ternary_C, T, Cin, w.dWb, N, w.dds, w.ddm, w.dth,
                               max_spikes, rate, chunk_counts, chunk_rows);
    } else {
        xylo_launch_general(w, reinterpret_cast<const uint8_t *>(spikes_in), ternary_C, B, T, Cin, N, w_rec, max_spikes, nullptr, rate, chunk_counts,
                            stream);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned pairs = (unsigned)B * (unsigned)nW;
    hipLaunchKernelGGL(xylo_window_kernel, dim3(xylo_window_grid(pairs), (N + 255) / 256), dim3(256), 0, stream, chunk_counts, chunk_rows, N, nW,
                       pairs, window / XP_CHUNK, hop / XP_CHUNK, window_counts);
    return hipGetLastError();
}

// ---- the sweep's form: counts only, ternary raster, no recurrence -> persistent workgroups on a ticket queue -----------------
static bool xylo_sweep_queued(const void *raster, int Cin, int N)
{
    return Cin <= 64 && N <= XP_NEUR && (reinterpret_cast<uintptr_t>(raster) & 15) == 0;
}

size_t xylo_sweep_scratch_bytes(int B)
{
    // [XQ_CTL control ints][B chunk counters] | [B][XP_WAVES][64] int4 hand-over state
    return (((size_t)(XQ_CTL + B) * sizeof(int) + 255) & ~(size_t)255) + (size_t)B * XP_WAVES * 64 * sizeof(int4_t);
}

constexpr int XQ_CHUNK = 2048;  // steps per ticket (16 staged tiles): ~0.3 ms of work against a few microseconds of hand-over

hipError_t launch_xylo_sweep(const int8_t *raster, int ternary_C, int B, int T, int Cin, int N, int max_spikes, int32_t *rate, void *ws,
                             void *scratch, int workers_per_cu, hipStream_t stream)
{
    if (!xylo_sweep_queued(raster, Cin, N) || max_spikes < 1)
        return launch_xylo_resident(raster, ternary_C, B, T, Cin, N, 0, max_spikes, nullptr, rate, ws, stream);
    const XyloWs w = xylo_ws(ws, Cin, N);
    const XpShape sh = xp_shape(N, ternary_C);  // (one neuron block)
    int *qctl = reinterpret_cast<int *>(scratch);
    int4_t *qstate = reinterpret_cast<int4_t *>(reinterpret_cast<unsigned char *>(scratch) + (((size_t)(XQ_CTL + B) * sizeof(int) + 255) & ~(size_t)255));
    static int num_cu = 0;  // (one device model per process: the library's code objects are gfx950 only)
    if (num_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return hipErrorInvalidDevice;
        num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    const int nchunks = (T + XQ_CHUNK - 1) / XQ_CHUNK;
    const long long nitems = (long long)nchunks * B;
    // four workgroups per CU: with three waves each every SIMD holds three; never more workers than trials (a worker beyond that
    // could only wait for a predecessor)
    int workers = (workers_per_cu > 0 ? workers_per_cu : 4) * num_cu;
    workers = workers > B ? B : workers;
    workers = (long long)workers > nitems ? (int)nitems : workers;
    hipLaunchKernelGGL(xylo_queue_reset_kernel, dim3((XQ_CTL + B + 255) / 256), dim3(256), 0, stream, qctl, XQ_CTL + B);
    if (xp_kq(Cin) == 1)
        hipLaunchKernelGGL((xylo_lif_pk_kernel<1, false, true>), dim3(workers), dim3(sh.waves * 64), sh.lds, stream, raster, ternary_C, T, Cin, w.dWb,
                           N, w.dds, w.ddm, w.dth, max_spikes, nullptr, rate, qctl, qstate, XQ_CHUNK, B);
    else
        hipLaunchKernelGGL((xylo_lif_pk_kernel<2, false, true>), dim3(workers), dim3(sh.waves * 64), sh.lds, stream, raster, ternary_C, T, Cin, w.dWb,
                           N, w.dds, w.ddm, w.dth, max_spikes, nullptr, rate, qctl, qstate, XQ_CHUNK, B);
    return hipGetLastError();
}

hipError_t launch_xylo(const uint8_t *spikes_in, int B, int T, int Cin, const int8_t *W_in_host, int N, int w_rec,
                       const uint8_t *dash_syn_host, const uint8_t *dash_mem_host, const int16_t *thr_host,
                       int max_spikes, uint8_t *spikes_out, int32_t *rate, void *ws, hipStream_t stream)
{
    hipError_t e0 = xylo_upload(Cin, W_in_host, N, dash_syn_host, dash_mem_host, thr_host, ws, stream);
    if (e0 != hipSuccess) return e0;
    return launch_xylo_resident(spikes_in, 0, B, T, Cin, N, w_rec, max_spikes, spikes_out, rate, ws, stream);
}

// ==== the tracking form of the packed walk: Envelope.evolve of the spike counts and the first maximum over the neurons, per frame ========
// The tap, its set-up and the two combines are xylo_track_rows.h's, shared with the walk as a stream (stream_xylo.hip); here are the
// one-shot range -- every trial from zero state at frame 0 -- and what the call leaves.  include/micloc_hip.h, "Xylo moving-target
// tracking", has the rule; DESIGN 4.23 the structure.
// grid (neuron blocks, trials) as xylo_lif_pk_kernel's one-shot form.  One neuron block: pval / pidx are peak_env (may be NULL) and index
// [B][T]; more: the pairs [B T][blocks] that xylo_track_combine_kernel reduces.
template <int KQ>
__global__ __launch_bounds__(XP_WAVES * 64) void xylo_lif_track_kernel(const int8_t *__restrict__ raster, int tc, int T, int Cin,
                                                                        const long *__restrict__ Wb /*[Npad][4 KQ]*/, int N,
                                                                        const uint8_t *__restrict__ dash_syn,
                                                                        const uint8_t *__restrict__ dash_mem,
                                                                        const short *__restrict__ thr, int max_spikes, double a_rise,
                                                                        double i_rise, double a_fall, double *__restrict__ pval,
                                                                        int32_t *__restrict__ pidx, double *__restrict__ env_last,
                                                                        int *__restrict__ rate)
{
    __shared__ __attribute__((aligned(16))) unsigned char tile[XP_TT][32 * KQ];
    extern __shared__ __attribute__((aligned(16))) int cur_dyn[];  // [waves][4][64][4]: only the waves that hold neurons
    __shared__ double sv[XP_WAVES][XP_TT];
    __shared__ int si[XP_WAVES][XP_TT];
    XpLif<KQ, false, XpTrackTap> lif;
    lif.init(tile, cur_dyn, blockIdx.x * XP_NEUR, Wb, N, dash_syn, dash_mem, thr, max_spikes);
    XpTrackTap &tap = lif.tap;
    xp_track_tap_init(lif, a_rise, i_rise, a_fall, sv, si);
    tap.e0 = tap.e1 = 0.0;
    const int b = blockIdx.y, nblk = gridDim.x, blk = blockIdx.x;
    const int tid = lif.tid, nthreads = lif.nthreads, waves = nthreads >> 6;
    const int8_t *rend = raster + (size_t)gridDim.y * T * tc;
    auto done = [&](int t0, int steps) {
        xp_track_rows(sv, si, waves, tid, nthreads, steps, [&](int f, double best, int bi) {
            const size_t row = (size_t)b * T + t0 + f;
            if (nblk == 1) {
                pidx[row] = bi == RO_NONE ? 0 : bi;
                if (pval) pval[row] = best;
            } else {
                pval[row * nblk + blk] = best;
                pidx[row * nblk + blk] = bi;
            }
        });
    };
    lif.run_range(raster + (size_t)b * T * tc, rend, tc, Cin, 0, T, done);
    if (env_last) {
        if (lif.act0) env_last[(size_t)b * N + lif.n0] = tap.e0;
        if (lif.act1) env_last[(size_t)b * N + lif.n1] = tap.e1;
    }
    if (rate) {
        if (lif.act0) rate[(size_t)b * N + lif.n0] = lif.total0;
        if (lif.act1) rate[(size_t)b * N + lif.n1] = lif.total1;
    }
}

// the pairs of a frame over the neuron blocks -> index, peak
__global__ __launch_bounds__(256) void xylo_track_combine_kernel(const double *__restrict__ pval, const int32_t *__restrict__ pidx, size_t rows,
                                                                 int nblk, int32_t *__restrict__ index, double *__restrict__ peak)
{
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    double best;
    int bi;
    xylo_track_combine_row(pval + row * nblk, pidx + row * nblk, nblk, best, bi);
    index[row] = bi == RO_NONE ? 0 : bi;
    if (peak) peak[row] = best;
}

bool xylo_track_fused(int ternary_C, int Cin, int w_rec, int max_spikes)
{
    return w_rec == 0 && ternary_C > 0 && Cin <= 64 && max_spikes >= 1;  // (and a 16-byte aligned raster: the caller's check)
}

size_t xylo_track_pairs_bytes(int B, int T, int N)
{
    const int nblk = xp_npad(N) / XP_NEUR;
    return nblk == 1 ? 256 : xylo_track_pairs_size((size_t)B * T * nblk);  // (one block writes the results itself; never 0: that is "bad arguments")
}

hipError_t launch_xylo_track(const int8_t *raster, int ternary_C, int B, int T, int Cin, int N, int max_spikes, double a_rise, double i_rise,
                             double a_fall, int32_t *index, double *peak, double *env_last, int32_t *rate, void *ws, void *pairs,
                             hipStream_t stream)
{
    if (!xylo_track_fused(ternary_C, Cin, 0, max_spikes) || (reinterpret_cast<uintptr_t>(raster) & 15) != 0) return hipErrorInvalidValue;
    const XyloWs w = xylo_ws(ws, Cin, N);
    const XpShape sh = xp_shape(N, ternary_C);
    double *pval = peak;
    int32_t *pidx = index;
    const size_t rows = (size_t)B * T;
    if (sh.nblk > 1) xylo_track_pairs_split(pairs, rows * sh.nblk, pval, pidx);
    const dim3 grid(sh.nblk, B), block(sh.waves * 64);
    if (xp_kq(Cin) == 1)
        hipLaunchKernelGGL(xylo_lif_track_kernel<1>, grid, block, sh.lds, stream, raster, ternary_C, T, Cin, w.dWb, N, w.dds, w.ddm, w.dth,
                           max_spikes, a_rise, i_rise, a_fall, pval, pidx, env_last, rate);
    else
        hipLaunchKernelGGL(xylo_lif_track_kernel<2>, grid, block, sh.lds, stream, raster, ternary_C, T, Cin, w.dWb, N, w.dds, w.ddm, w.dth,
                           max_spikes, a_rise, i_rise, a_fall, pval, pidx, env_last, rate);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || sh.nblk == 1) return e;
    hipLaunchKernelGGL(xylo_track_combine_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, pval, pidx, rows, sh.nblk, index,
                       peak);
    return hipGetLastError();
}

}  // namespace micloc
