// What the packed Xylo LIF kernels share -- the one-shot xylo_lif_pk_kernel of xylo.hip (one workgroup per trial, or persistent
// workgroups on a ticket queue) and the resumable xylo_lif_stream_kernel of stream_xylo.hip: the shape of a workgroup, the lane's
// constants and state, the matrix-core `produce`, the two step functions, the staging loop of a 128-step tile, the walk over a range
// of frames and the count of a 256-frame chunk for the windowed read-outs (xp_chunk_done); on the host the layout of xylo_upload's workspace and the launch shape.  Stated once, so that a frame has the same bits
// whether its trial was walked in one launch, handed from ticket to ticket or cut at launch borders.  PARITY UNPINNED like xylo.hip.
//
// ---------------------------------------------------------------------------------------------------------------
// Packed form (binary input events, no recurrence): two neurons per lane in 16-bit halves.
//
// The state is 16 bit by definition, so every step of the rule has a packed instruction that is exact on it:
//   decay              v - max(v >> dash, min(v, 1))       v_pk_ashrrev_i16 / v_pk_min_i16 / v_pk_max_i16 / v_pk_sub_i16
//   sat16(a + b)       both operands 16 bit                v_pk_add_i16 clamp
//   first spike        d = sat(v - th); m = d >> 15 (all ones below threshold); v = m ? v : d; count += m
//                                                          v_pk_sub_i16 clamp / v_pk_ashrrev_i16 / v_bfi_b32 / v_pk_add_i16
// (a shift count above 15 acts like 15 on a 16-bit value, so dash is clamped; the spike count of a 128-step tile is
// 128 + the sum of the m's and is widened to 32 bit per tile).  9 instructions per neuron-step instead of ~41.
//
// The input current in[t][n] = sum_c W_in[c][n] s[t][c] is a plain matrix product of the event raster with the weight
// matrix, identical for every trial: it runs on the matrix cores (v_mfma_i32_16x16x32_i8, one instruction per 16 steps x
// 16 neurons; |in| <= 64 x 127 fits 16 bit because the events are 0/1).  A wave owns 128 neurons = 8 column tiles, whose
// weight fragments it keeps in registers; lane (q, lc) integrates neurons 32 q + lc and 32 q + 16 + lc of the wave.  The
// accumulators of column tiles 2k and 2k + 1 hold exactly those two neurons in lane (., lc), so one v_perm_b32 per step
// packs them; the wave parks the packed currents of the next 16 steps in its own LDS slice ([4 steps][lane], 16 B per
// lane: conflict-free both ways) while it integrates the current 16, and no barrier is needed inside a 128-step tile.
// The rare second spike within one step (v >= 2 th) leaves the packed path for the exact 32-bit sequence.
// ---------------------------------------------------------------------------------------------------------------
#pragma once
#include "micloc_internal.h"

namespace micloc {

typedef short short2_t __attribute__((ext_vector_type(2)));
typedef int int4_t __attribute__((ext_vector_type(4)));

constexpr int XP_WAVES = 4;                  // 4 x 128 = 512 neurons per workgroup
constexpr int XP_TT = 128;                   // time steps staged per LDS tile: 4 KB + 4 KB per wave = 16 KB for the sweep's 360
                                             // neurons: all 1100 trials are resident at once (4-5 workgroups per CU)
constexpr int XP_NEUR = XP_WAVES * 128;

__device__ __forceinline__ short2_t xp_s2(int w) { return __builtin_bit_cast(short2_t, w); }
__device__ __forceinline__ int xp_i(short2_t v) { return __builtin_bit_cast(int, v); }

// v - max(v >> dash, min(v, 1)): the "at least one LSB" decay (xy_decay, xylo.hip), exact in packed 16 bit
__device__ __forceinline__ short2_t xp_decay(short2_t v, short2_t dash)
{
    const short2_t one = {1, 1};
    return v - __builtin_elementwise_max(v >> dash, __builtin_elementwise_min(v, one));
}

// exact floor(v / th) for 0 < th <= v <= 32767 without the integer-division sequence: fp32 quotient, corrected by +-1
__device__ __forceinline__ int xy_div(int v, int th)
{
    int n = (int)((float)v * __builtin_amdgcn_rcpf((float)th));
    n = n * th > v ? n - 1 : n;
    n = (n + 1) * th <= v ? n + 1 : n;
    return n;
}

// What a launch form may hang on the walk to see every step's FINAL spike counts (the tracking kernel of stream_xylo.hip: XpTrackTap).  A tap
// with `on` gets, exactly once per step and in step order, the packed counts of the lane's two neurons (low half: n0, high half: n1):
//   begin(off, first)   in front of a run of steps: `off` = position of its first step in the staged tile, `first` = that step is frame 0
//   put(j, cw)          step j (a compile-time index after unrolling) of a whole 16-step group; a group that is walked again calls it
//                       again for every j, and only the last call counts
//   group()             the 16 counts of the group are final
//   single(j, cw)       step j of the ragged last group of a range: final at once (those steps run the exact sequence)
// XpNoTap is the walk of the counting and the streaming kernels: nothing is called, nothing is kept.
struct XpNoTap {
    static constexpr bool on = false;
    __device__ __forceinline__ void begin(int, bool) {}
    __device__ __forceinline__ void put(int, int) {}
    __device__ __forceinline__ void group() {}
    __device__ __forceinline__ void single(int, int) {}
};

// One lane of a packed workgroup: its constants, its two neurons' state and the walk over a range of frames.  The kernels declare the
// LDS (tile [XP_TT][32 KQ] static, cur_dyn dynamic: xp_shape) and own everything around run_range: where the state comes from and goes.
template <int KQ, bool WANT_OUT, class Tap = XpNoTap>
struct XpLif {
    Tap tap;
    long Bw[8][KQ];  // weight fragments of the wave's 8 column tiles: lane (q, lc) holds channels 8 q .. 8 q + 7 (+ 32 kq) of neuron 16 j + lc
    short2_t ds, dm, th;
    int th_hi;  // v.hi >= th.hi  <=>  (int)word >= th.hi << 16
    int n0, n1;
    bool act0, act1;
    short2_t isyn, vmem, cnt, vmx;
    int total0, total1;
    int N, max_spikes;
    int tid, nthreads, wv, l, lc, q;
    uint8_t *ob;  // WANT_OUT: the trial's spikes_out [T][N], set by the kernel
    unsigned char (*tile)[32 * KQ];
    int (*cur)[4][64][4];  // [waves][4][64][4]: only the waves that hold neurons
    int8_t *raw;           // staging area for the raster bytes of a tile (the slices of `cur`, between barriers)

    // zero state; nblock: the first neuron of the workgroup
    __device__ __forceinline__ void init(unsigned char (*tile_)[32 * KQ], int *cur_dyn, int nblock, const long *__restrict__ Wb /*[Npad][4 KQ]*/,
                                         int N_, const uint8_t *__restrict__ dash_syn, const uint8_t *__restrict__ dash_mem,
                                         const short *__restrict__ thr, int max_spikes_)
    {
        tile = tile_;
        cur = reinterpret_cast<int(*)[4][64][4]>(cur_dyn);
        raw = reinterpret_cast<int8_t *>(cur_dyn);
        N = N_;
        max_spikes = max_spikes_;
        tid = threadIdx.x;
        nthreads = blockDim.x;
        wv = tid >> 6, l = tid & 63, lc = l & 15, q = l >> 4;
        const int nbase = nblock + wv * 128;
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int kq = 0; kq < KQ; ++kq) Bw[j][kq] = Wb[(size_t)(nbase + 16 * j + lc) * (4 * KQ) + 4 * kq + q];
        n0 = nbase + 32 * q + lc, n1 = n0 + 16;
        act0 = n0 < N, act1 = n1 < N;
        auto clamp15 = [](int d) { return d > 15 ? 15 : d; };
        ds = short2_t{(short)(act0 ? clamp15(dash_syn[n0]) : 0), (short)(act1 ? clamp15(dash_syn[n1]) : 0)};
        dm = short2_t{(short)(act0 ? clamp15(dash_mem[n0]) : 0), (short)(act1 ? clamp15(dash_mem[n1]) : 0)};
        th = short2_t{(short)(act0 ? thr[n0] : 32767), (short)(act1 ? thr[n1] : 32767)};
        th_hi = (int)th.y << 16;
        isyn = vmem = cnt = short2_t{0, 0};
        vmx = short2_t{-32768, -32768};
        total0 = total1 = 0;
        ob = nullptr;
    }

    // currents of 16 steps (tile16 `i` of the staged rows) -> the wave's LDS slice.  ONE slice per wave (4 KB): the 16 steps of
    // a tile are read into registers before the next tile's currents overwrite them (LDS operations of a wave execute in
    // order), so a workgroup takes 16 instead of 28 KB and a CU that holds four or five of them still has room for a
    // workgroup of the stages in front (the chunked encoder: 80 KB) -- with 28 KB the three stages of the sweep took turns.
    __device__ __forceinline__ void produce(int i)
    {
        int4_t acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = int4_t{0, 0, 0, 0};
#pragma unroll
        for (int kq = 0; kq < KQ; ++kq) {
            const long a = *reinterpret_cast<const long *>(&tile[16 * i + lc][32 * kq + 8 * q]);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = __builtin_amdgcn_mfma_i32_16x16x32_i8(a, Bw[j][kq], acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int4_t pk;
#pragma unroll
            for (int r = 0; r < 4; ++r) pk[r] = (int)__builtin_amdgcn_perm((unsigned)acc[2 * k + 1][r], (unsigned)acc[2 * k][r], 0x05040100u);
            *reinterpret_cast<int4_t *>(&cur[wv][q][16 * k + lc][0]) = pk;  // steps 4 q .. 4 q + 3 of pair lane 16 k + lc
        }
    }

    // The second-spike test (v >= th again after the reset: two compares, a scalar or and a branch per step) is not run per step
    // in whole tiles: the steps only keep the largest membrane word they left behind, one test per 16 steps decides, and a group in
    // which some step did need the exact sequence is walked again from its saved state with the per-step test (`step` below).
    __device__ __forceinline__ void step_fast(int in_word, int t, int j)
    {
        short2_t i2 = xp_decay(isyn, ds);
        short2_t v2 = xp_decay(vmem, dm);
        i2 = __builtin_elementwise_add_sat(i2, xp_s2(in_word));
        v2 = __builtin_elementwise_add_sat(v2, i2);
        const short2_t d = __builtin_elementwise_sub_sat(v2, th);
        const short2_t fifteen = {15, 15};
        const short2_t m = d >> fifteen;  // all ones: below threshold
        const int vw = (xp_i(m) & xp_i(v2)) | (~xp_i(m) & xp_i(d));
        cnt += m;
        vmx = __builtin_elementwise_max(vmx, xp_s2(vw));
        if constexpr (Tap::on) tap.put(j, xp_i(m + short2_t{1, 1}));
        if constexpr (WANT_OUT) {
            const size_t row = (size_t)t * N;
            if (act0) ob[row + n0] = (uint8_t)(1 + m.x);
            if (act1) ob[row + n1] = (uint8_t)(1 + m.y);
        }
        isyn = i2;
        vmem = xp_s2(vw);
    }

    template <bool RAGGED = false>
    __device__ __forceinline__ void step(int in_word, int t, int j)
    {
        short2_t i2 = xp_decay(isyn, ds);
        short2_t v2 = xp_decay(vmem, dm);
        i2 = __builtin_elementwise_add_sat(i2, xp_s2(in_word));
        v2 = __builtin_elementwise_add_sat(v2, i2);
        const short2_t d = __builtin_elementwise_sub_sat(v2, th);
        const short2_t fifteen = {15, 15};
        const short2_t m = d >> fifteen;  // all ones: below threshold
        int vw = (xp_i(m) & xp_i(v2)) | (~xp_i(m) & xp_i(d));
        cnt += m;
        int extra0 = 0, extra1 = 0;
        // a second spike in the same step (v >= 2 th): exact 32-bit sequence, per half
        const bool again = ((short)vw >= th.x) | (vw >= th_hi);
        if (__builtin_expect(__any(again), 0)) {
            int lo = (short)vw, hi = vw >> 16;
            if (lo >= th.x) {
                int more = xy_div(lo, th.x);
                more = more < max_spikes - 1 ? more : max_spikes - 1;
                extra0 = more;
                lo -= more * th.x;
            }
            if (hi >= th.y) {
                int more = xy_div(hi, th.y);
                more = more < max_spikes - 1 ? more : max_spikes - 1;
                extra1 = more;
                hi -= more * th.y;
            }
            vw = (lo & 0xffff) | (hi << 16);
            total0 += extra0;
            total1 += extra1;
        }
        if constexpr (Tap::on) {
            const int cw = xp_i(m + short2_t{1, 1}) + extra0 + (extra1 << 16);  // (counts <= 31: no carry between the halves)
            if constexpr (RAGGED)
                tap.single(j, cw);
            else
                tap.put(j, cw);
        }
        if constexpr (WANT_OUT) {
            const size_t row = (size_t)t * N;
            if (act0) ob[row + n0] = (uint8_t)(1 + m.x + extra0);
            if (act1) ob[row + n1] = (uint8_t)(1 + m.y + extra1);
        }
        isyn = i2;
        vmem = xp_s2(vw);
    }

    // The frames [t_lo, t_hi) of the trial whose raster rows [frame][tc] begin at sb, in tiles of XP_TT; rend: the end of the whole
    // raster allocation, which is 16-byte aligned (the 16-byte loads round a tile's start down and never read at or past rend).
    // done(t0, steps): called by every thread after the totals of the tile [t0, t0 + steps) are in total0 / total1.
    template <class Done>
    __device__ __forceinline__ void run_range(const int8_t *sb, const int8_t *rend, int tc, int Cin, int t_lo, int t_hi, Done done)
    {
        for (int t0 = t_lo; t0 < t_hi; t0 += XP_TT) {
            const int steps = (t_hi - t0) < XP_TT ? (t_hi - t0) : XP_TT;
            __syncthreads();  // every wave is done with the previous tile and with its slice of `cur`
            // the steps x tc raster bytes of this tile are contiguous: one 16-byte load per thread into LDS (the slices of `cur`
            // are idle between these barriers), then the +1 / -1 split from there (channel c < tc: +1 events, tc + c: -1
            // events, zero padded to 32 KQ).  A byte-wise gather from global memory costs one exposed latency per element.
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
                for (int e = tid; e < XP_TT * 8 * KQ; e += nthreads) {
                    const int r = e / (8 * KQ), k = e % (8 * KQ);
                    unsigned w = 0;
                    if (r < steps) {
                        const int8_t *row = raw + off + r * tc;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int c = 4 * k + i;
                            if (c < 2 * tc && c < Cin) {
                                const int sv = c < tc ? row[c] : -row[c - tc];
                                w |= (unsigned)(sv > 0) << (8 * i);
                            }
                        }
                    }
                    tile32[e] = w;
                }
            }
            __syncthreads();
            const int ntile = (steps + 15) >> 4;
            cnt = short2_t{0, 0};
            produce(0);
            for (int i = 0; i < ntile; ++i) {
                const int jn = steps - 16 * i < 16 ? steps - 16 * i : 16;
                const int4_t *cw = reinterpret_cast<const int4_t *>(&cur[wv][0][l][0]);
                int4_t in4[4];
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) in4[t4] = cw[64 * t4];
                if (i + 1 < ntile) produce(i + 1);  // (overwrites the slice: after the reads above, in program order)
                if constexpr (Tap::on) tap.begin(16 * i, t0 + 16 * i == 0);
                if (jn == 16) {
                    const short2_t isyn_s = isyn, vmem_s = vmem, cnt_s = cnt;
                    vmx = short2_t{-32768, -32768};
#pragma unroll
                    for (int t4 = 0; t4 < 4; ++t4) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) step_fast(in4[t4][r], t0 + 16 * i + 4 * t4 + r, 4 * t4 + r);
                    }
                    const short2_t fifteen = {15, 15};
                    const short2_t below = __builtin_elementwise_sub_sat(vmx, th) >> fifteen;  // all ones: never reached th again
                    if (__builtin_expect(__any(xp_i(below) != -1), 0)) {
                        isyn = isyn_s;
                        vmem = vmem_s;
                        cnt = cnt_s;
#pragma unroll
                        for (int t4 = 0; t4 < 4; ++t4) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) step(in4[t4][r], t0 + 16 * i + 4 * t4 + r, 4 * t4 + r);
                        }
                    }
                    if constexpr (Tap::on) tap.group();
                } else {  // the last steps of the range
                    for (int j = 0; j < jn; ++j) {
                        int w_in = 0;
#pragma unroll
                        for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
                            for (int r = 0; r < 4; ++r) w_in = (j == 4 * t4 + r) ? in4[t4][r] : w_in;
                        step<true>(w_in, t0 + 16 * i + j, j);
                    }
                }
            }
            total0 += steps + cnt.x;
            total1 += steps + cnt.y;
            done(t0, steps);
        }
    }
};

// run_range's `done` for the windowed read-outs (the stream's tracking kernel, stream_xylo.hip; the one-shot chunk-count kernel,
// xylo.hip): a chunk of XP_CHUNK frames ends with the tile [t0, t0 + steps) (the recording's last one may be ragged): its count goes to
// row t0 / XP_CHUNK of chunk_counts [B][chunk_rows][N].  chunk0 / chunk1: the totals at the start of the open chunk.
constexpr int XP_CHUNK = 256;
static_assert(XP_CHUNK == 256 && XP_CHUNK % XP_TT == 0, "the chunk row of a tile is t0 >> 8; a chunk ends with a tile");

template <class Lif>
__device__ __forceinline__ void xp_chunk_done(const Lif &lif, int *__restrict__ chunk_counts, int chunk_rows, int b, int t0, int steps, int t_hi,
                                              int &chunk0, int &chunk1)
{
    if (chunk_counts && (((t0 + steps) & (XP_CHUNK - 1)) == 0 || t0 + steps == t_hi)) {
        int *cc = chunk_counts + ((size_t)b * chunk_rows + (t0 >> 8)) * lif.N;
        if (lif.act0) cc[lif.n0] = lif.total0 - chunk0;
        if (lif.act1) cc[lif.n1] = lif.total1 - chunk1;
        chunk0 = lif.total0;
        chunk1 = lif.total1;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
inline int xp_npad(int N) { return ((N + XP_NEUR - 1) / XP_NEUR) * XP_NEUR; }
inline int xp_kq(int Cin) { return Cin <= 32 ? 1 : 2; }

// xylo_upload's workspace: [packed dwords [nq][N]][dash_syn][dash_mem][thresholds], each padded to 256 bytes, and for Cin <= 64 the
// neuron-major byte matrix [Npad][32 KQ] of the packed form
struct XyloWs {
    int *dW;
    uint8_t *dds, *ddm;
    short *dth;
    long *dWb;
    size_t bytes;
};

inline XyloWs xylo_ws(void *ws, int Cin, int N)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const int nq = (Cin + 3) / 4;
    const size_t off = al((size_t)nq * N * sizeof(int)), seg = al((size_t)N * 2);
    const size_t wb = Cin <= 64 ? al((size_t)xp_npad(N) * 32 * xp_kq(Cin)) : 0;
    const uintptr_t base = reinterpret_cast<uintptr_t>(ws);  // (ws == NULL: only `bytes` is asked for)
    return XyloWs{reinterpret_cast<int *>(base),
                  reinterpret_cast<uint8_t *>(base + off),
                  reinterpret_cast<uint8_t *>(base + off + seg),
                  reinterpret_cast<short *>(base + off + 2 * seg),
                  reinterpret_cast<long *>(base + off + 3 * seg),
                  off + 3 * seg + wb};
}

// The packed launch: as many waves as hold neurons (N = 360: 3, not 4), the same in every workgroup of the launch; dynamic LDS = the
// waves' current slices or the raw raster bytes of a tile (+ 15 of the rounded-down start, + 15 of the rounded-up end), whichever is more
struct XpShape {
    int nblk, waves;
    size_t lds;
};

inline XpShape xp_shape(int N, int tc)
{
    const int nblk = xp_npad(N) / XP_NEUR;
    const int waves = nblk > 1 ? XP_WAVES : (N + 127) / 128;
    const size_t slices = (size_t)waves * 4 * 64 * 4 * sizeof(int), rawb = (size_t)XP_TT * tc + 48;
    return XpShape{nblk, waves, slices > rawb ? slices : rawb};
}

}  // namespace micloc
