// The sweep's encoder launch: band-pass IIR + RZCC spike encoder in a form of which a CU holds three workgroups.
//
// This is the wave pipeline of rzcc.hip's bandpass_rzcc_fast_kernel (read the description there: loader, filter, detect and two
// select waves over 16-step tiles, flagged units redone by a list-based kernel) written out for ONE kind of launch: spikes only, one
// pass over the stream (no time chunks), not streaming, 64 streams per workgroup, order-2 Butterworth band-pass (five
// coefficients) -- the headline sweep's, where three streams run their launches of 241 workgroups next to each other's beamformer.
// rzcc.hip's form takes 75 904 B of LDS and 123 VGPRs, two workgroups per CU.  Here a workgroup takes 51 584 B and 84 VGPRs:
//
//   * 32 candidate ring entries per stream instead of 64.  The detect wave checks the space a tile REALLY needs (its events, at
//     least the three slots of the unconditional stores) against what the select waves still hold, instead of reserving a whole
//     tile of sixteen appends: the sweep's streams need at most about 15 of the 32 (tools/dev/ring_demand.py,
//     tests/test_ring_depth_cpu.py).  A lane that has stopped appending stores nothing, so it cannot overwrite an entry a select
//     wave still reads.
//   * the loader waves keep the 64 stream bases in a 512-byte LDS table instead of sixteen register pairs per lane, read back four
//     at a time just in front of the loads; the loaders' LDS accesses are hand-issued with immediate offsets.
//   * the widest register form of the cluster resolution is 8 (longer clusters take the list walk: same rule, same ties).
//
// Why a file of its own: rzcc.hip is one of the hot-path sources whose hash the newest committed profile round records
// (tests/test_profiles_manifest.py), so it changes only together with a new round of profiles.  Until the next round folds this form
// back into rzcc.hip's template, the pieces both files need (filter step, cluster resolution, fallback kernel, zero fill, scratch
// layout) exist twice; the launcher below declines if rzcc.hip's scratch size no longer matches the layout copied here.  This
// file's own measurements are tied to its hash by profiles/encoder_slots/RECORD.json (tests/test_ring_depth_cpu.py).
// The spikes are the same bits for every input: tests/test_hip_encoder_slots.py.  Everything lives in micloc::rzsweep.
#include "micloc_internal.h"

#include <type_traits>

#pragma clang diagnostic ignored "-Wpass-failed"

namespace micloc {
namespace rzsweep {

constexpr int RZ_RING_SWEEP = 32;  // candidate ring entries per stream (power of two; rzcc.hip's forms: 64)

template <int N>
struct Iir {
    double z[N > 1 ? N - 1 : 1];

    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int i = 0; i < (N > 1 ? N - 1 : 1); ++i) z[i] = 0.0;
    }

    __device__ __forceinline__ double step(const IirCoef &coef, double xin)
    {
        double y;
        if (N == 1) {
            y = __builtin_fma(coef.b[0], xin, 0.0);
        } else {
            y = __builtin_fma(coef.b[0], xin, z[0]);
#pragma unroll
            for (int i = 0; i < N - 2; ++i)
                z[i] = __builtin_fma(-coef.a[i + 1], y, __builtin_fma(coef.b[i + 1], xin, z[i + 1]));
            z[N - 2] = __builtin_fma(-coef.a[N - 1], y, coef.b[N - 1] * xin);
        }
        return y;
    }
};

// The filter coefficients arrive as kernel arguments (scalar loads).  The compiler waits for a scalar load at its first
// use; when that use sits inside the serial loop, the wait (s_waitcnt lgkmcnt(0): LDS and scalar loads share the counter)
// is re-executed every tile and drains the LDS reads issued just before it.  Touching the values once in front of the
// loop moves the wait there.
template <int N>
__device__ __forceinline__ void pin_coef(const IirCoef &coef)
{
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("; filter coefficient resident" ::"s"(coef.b[i]), "s"(coef.a[i]));
}

// Short clusters (the common case) are resolved in registers: all entries after one round of LDS reads, the rounds of the
// selection as unrolled compare / mask sequences of width W.  The list walk of resolve_cluster pays one LDS latency per
// entry it looks at, several times per round, and a wave waits for its slowest lane: dense candidate trains (order-1
// band-pass) were bound by it.  Three widths, because every round costs W compares whatever the cluster holds.
template <int W, typename WordAt, typename ValAt, typename Emit>
__device__ __forceinline__ void resolve_cluster_regs(int s, int stride, int count, int w, Emit emit, WordAt word_at, ValAt val_at,
                                                     double sgn)
{
    int P[W];
    double V[W];
#pragma unroll
    for (int u = 0; u < W; ++u) {
        const int kc = u < count ? s + u * stride : s;
        P[u] = *word_at(kc) >> 1;
        V[u] = *val_at(kc) * sgn;
    }
    unsigned alive = (1u << count) - 1u;
    while (alive) {
        int best = -1, pb = 0;
        double bv = 0.0;
#pragma unroll
        for (int u = 0; u < W; ++u) {
            if (((alive >> u) & 1u) && (best < 0 || V[u] >= bv)) {  // >= : equal priority -> the later peak wins
                best = u;
                bv = V[u];
                pb = P[u];
            }
        }
        emit(pb);
        alive &= ~(1u << best);
        // positions ascend with u: "everything closer than w" is what the outward walks with their early exit remove
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const int d = P[u] - pb;
            if ((d < 0 ? -d : d) < w) alive &= ~(1u << u);
        }
    }
}

// Greedy min-distance selection inside one cluster.  Entries live at list indices s, s+stride, ... < e;
// word >> 1 = position (the low bit is free for the caller), complemented once decided; priority = sgn * value.
// `at(i)` maps a list index to storage.
// MAXW: widest register form (16, or 8 where the kernel's register budget has no room for sixteen entries: longer clusters take
// the list walk, the same rule entry by entry).
template <int MAXW = 16, typename WordAt, typename ValAt, typename Emit>
__device__ __forceinline__ void resolve_cluster(int s, int e, int stride, int w, Emit emit, WordAt word_at, ValAt val_at,
                                                double sgn)
{
    int remaining = (e - s + stride - 1) / stride;
    // (measured on one box, encoder launch of config 2 / config 4: list walk only 0.42 / 14.7 ms; one width of 8: 0.39 / 9.2;
    // 4 + 8: 0.34 / 9.7; 2 + 4 + 8: 0.32 / 10.0; 4 + 8 + 16: 0.33 / 9.1)
    if (remaining <= 4) {
        resolve_cluster_regs<4>(s, stride, remaining, w, emit, word_at, val_at, sgn);
        return;
    }
    if (remaining <= 8) {
        resolve_cluster_regs<8>(s, stride, remaining, w, emit, word_at, val_at, sgn);
        return;
    }
    if (MAXW >= 16 && remaining <= 16) {
        resolve_cluster_regs<16>(s, stride, remaining, w, emit, word_at, val_at, sgn);
        return;
    }
    while (remaining > 0) {
        int best = -1;
        double bv = 0.0;
        // four list entries per trip: the LDS reads of a trip do not depend on each other, so their latencies overlap
        // (one read at a time left this loop latency bound on dense candidate trains: order-1 band-pass, config 4)
        for (int k = s; k < e; k += 4 * stride) {
            int wk[4];
            double vk[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kk = k + u * stride;
                const int kc = kk < e ? kk : s;
                wk[u] = *word_at(kc);
                vk[u] = *val_at(kc) * sgn;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kk = k + u * stride;
                if (kk < e && wk[u] >= 0 && (best < 0 || vk[u] >= bv)) {  // >= : equal priority -> the later peak wins (stable sort order)
                    best = kk;
                    bv = vk[u];
                }
            }
        }
        const int wb = *word_at(best);
        const int pb = wb >> 1;
        emit(pb);
        *word_at(best) = ~wb;
        --remaining;
        for (int k = best - stride; k >= s; k -= stride) {
            const int wk = *word_at(k);
            const int pk = (wk < 0 ? ~wk : wk) >> 1;
            if (pb - pk >= w) break;
            if (wk >= 0) {
                *word_at(k) = ~wk;
                --remaining;
            }
        }
        for (int k = best + stride; k < e; k += stride) {
            const int wk = *word_at(k);
            const int pk = (wk < 0 ? ~wk : wk) >> 1;
            if (pk - pb >= w) break;
            if (wk >= 0) {
                *word_at(k) = ~wk;
                --remaining;
            }
        }
    }
}

constexpr int RZ_MT = 16;  // time steps per tile of the wave pipeline (one barrier per tile)

// ---- detect-stage helper ------------------------------------------------------------------------------------------
// One step of BOTH words of the detect wave: r = 2 r + (a > b), f = 2 f + (a < b), ordered compares, through VCC inside one asm
// block.  With the compare outside (a builtin writing an SGPR pair that the add-with-carry reads and overwrites) the compiler put an
// s_nop behind every add-with-carry -- 30 of the wave's ~440 issue slots per tile; a compare writing VCC straight behind an
// add-with-carry that wrote it is an ordinary write after write.
__device__ __forceinline__ void rise_fall_step(unsigned &r, unsigned &f, double a, double b)
{
    asm("v_cmp_gt_f64 vcc, %2, %3\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\tv_cmp_lt_f64 vcc, %2, %3\n\tv_addc_co_u32_e32 %1, vcc, %1, %1, vcc"
        : "+v"(r), "+v"(f)
        : "v"(a), "v"(b)
        : "vcc");
}

// ---------------------------------------------------------------------------------------------------
// Time chunking with exact state hand-off.
//
// The serial chain of a stream (DF2T state, running sum, detector state) cannot be re-associated without changing
// bits, but it can be CHECKPOINTED: rzcc_scan_kernel walks every stream once with nothing but the band-pass and the
// running sum (the cheapest possible serial pass: two waves per 64 streams) and stores the exact state at every
// chunk boundary.  bandpass_rzcc_fast_kernel then runs one workgroup per (64 streams, chunk): it restarts the
// recurrences from the stored state -- the same operations on the same operands, hence the same bits -- and does
// the expensive part (detect + select + scatter) for its chunk, P chunks side by side.  With few, long streams
// (speech: 1750 streams x 332 157 steps) this turns a 28-workgroup latency chain into a launch that fills the chip.
//
// Chunk p owns the clusters whose FIRST candidate lies in [own_lo, own_hi).  Clusters are separated by
// same-polarity gaps >= w, so a chunk starts Vt tiles (>= w steps) early: every candidate that can chain into an
// owned cluster is seen, and a cluster whose first seen member lies before own_lo belongs to the predecessor.
// After own_hi it runs V2t more tiles to see its last cluster close; a cluster still open then, a ring overflow, or a
// detector state the scan could not pin down (a plateau longer than a tile right at the boundary) flags the
// (stream, chunk) unit, which rzcc_unit_fallback_kernel redoes serially from the same checkpoint with unbounded lists.
// ---------------------------------------------------------------------------------------------------
struct RzGeom {
    int P;    // chunks per stream (1: one pass over the whole stream, no scan kernel)
    int Lt;   // RZ_MT-step tiles owned by a chunk: chunk p owns the times [RZ_MT p Lt, RZ_MT (p+1) Lt)
    int Vt;   // look-back tiles (RZ_MT Vt >= w)
    int V2t;  // tail tiles
};

struct RzSpan {
    int m_lo, m_hi;      // tiles processed: [m_lo, m_hi)
    int own_lo, own_hi;  // owned cluster starts: [own_lo, own_hi)
    bool at_end;         // m_hi is the end of the stream
};

__host__ __device__ inline RzSpan rz_span(const RzGeom &g, int p, int NM)
{
    RzSpan s;
    s.m_lo = p == 0 ? 0 : p * g.Lt - g.Vt;
    const int hi = (p + 1) * g.Lt + g.V2t;
    s.m_hi = (p == g.P - 1 || hi > NM) ? NM : hi;
    s.own_lo = p == 0 ? 0 : p * g.Lt * RZ_MT;
    s.own_hi = p == g.P - 1 ? 0x7fffffff : (p + 1) * g.Lt * RZ_MT;
    s.at_end = s.m_hi == NM;
    return s;
}

// checkpoint q = p - 1 (state entering tile m_lo(p)):  doubles [q][N][nlanes]: DF2T state z_0..z_{N-2}, running sum;
// ints [q][3][nlanes]: direction of the last strict change (RZ_DIR_*), its time, last tile that contained one
constexpr int RZ_DIR_RISE = 1, RZ_DIR_FALL = 2, RZ_DIR_UNKNOWN = 3;

// ---- loader waves ----------------------------------------------------------------------------------------------
// 16-step x 64-stream input tiles from the planar [stream][Ts] layout (in-phase channels straight from the rolled input frames)
// into a transposed LDS tile.  Wave PHASE of two owns the tiles PHASE, PHASE + 2, ...; tile m is written to X[m % 3] during
// iteration m - 1 (tile 0 before the first barrier); `nstep` barriers after the first one; two register sets per wave keep four
// tiles of loads in flight.
// The stream bases live in a 512-byte LDS table (`tab`, one 64-bit word per stream, bit 0: the stream is read from the rolled
// input frames) instead of sixteen register pairs per lane: the kernel has 96 VGPRs, and the two register sets take 64 of them.
// Each loader wave fills the table itself before its first load -- lane l computes stream l's base, one division per lane
// instead of sixteen -- and reads it back just in front of the loads; a wave's LDS operations complete in order, so it needs no
// barrier, and the two loader waves store the same 64 words.
template <int PHASE, typename XT>
__device__ __forceinline__ void rz_loader_np(XT &X, const double *__restrict__ h, const double *__restrict__ xin, int base,
                                             int nlanes, int C, int T, int Ts, int M, int shift, int NMc, int nstep, int lane,
                                             unsigned long long *tab)
{
    constexpr int NP = 2;
    constexpr int phase = PHASE;  // compile time: the s_waitcnt vmcnt(N) in front of a tile write must be able to leave
                                  // the younger register set's loads in flight, which needs straight-line knowledge
    const int tl = lane & 15;  // time offset inside the tile
    const int sq = lane >> 4;  // stream slot 0..3 of each group of four
    constexpr int NJ = 16;     // streams per lane: stream slot 4 j + sq
    double v[2][NJ];
    {
        int g = base + lane;
        g = g < nlanes ? g : nlanes - 1;
        const int bb = g / C, cc = g - bb * C;
        const bool r = xin != nullptr && cc < M;
        const double *b0 = r ? xin + (size_t)bb * T * M + cc : h + (size_t)g * Ts;
        tab[lane] = (unsigned long long)(size_t)b0 | (r ? 1ull : 0ull);  // (doubles: the low three address bits are zero)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const int sh = shift % T;
    auto issue_loads = [&](int q, auto set) {  // own tile q (clamped: a tile past the end lands in a buffer nobody reads)
        constexpr int S = decltype(set)::value;
        int mm = phase + NP * q;
        mm = mm < NMc ? mm : NMc - 1;
        const int t = mm * RZ_MT + tl;
        const int tc = t < Ts ? t : Ts - 1;
        int tr = (t < T ? t : T - 1) - sh;
        tr = tr < 0 ? tr + T : tr;
        const unsigned i_roll = (unsigned)tr * (unsigned)M, i_lin = (unsigned)tc;  // (the launcher checks that T * M fits 32 bits)
        {
            // four bases at a time, hand-issued with one wait: left to itself the compiler reads all sixteen first (32 VGPRs).  The
            // wait also covers this wave's tile write just before (LDS operations of a wave complete in order).
            const unsigned ta = (unsigned)(size_t)(&tab[sq]);
            typedef __attribute__((address_space(1))) double gdouble;  // (a pointer made from an integer would be a flat one)
#pragma unroll
            for (int j0 = 0; j0 < NJ; j0 += 4) {
                unsigned long long e[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(e[u]) : "v"(ta), "n"((j0 + u) * 32));
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(e[3]));
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    v[S][j0 + u] = reinterpret_cast<const gdouble *>((size_t)(e[u] & ~7ull))[(e[u] & 1ull) ? i_roll : i_lin];
            }
        }
    };
    auto write_tile = [&](int buf, auto set) {
        constexpr int S = decltype(set)::value;
        {
            // one address register and immediate offsets (the compiler keeps an address per store across the unrolled loop); every
            // tile write is followed by issue_loads, whose wait completes these stores before the barrier
            const unsigned wa = (unsigned)(size_t)(&X[buf][tl][sq]);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const double vj = v[S][j];
                asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(wa), "v"(vj), "n"(j * 32));
            }
        }
    };
    using set0 = std::integral_constant<int, 0>;
    using set1 = std::integral_constant<int, 1>;
    issue_loads(0, set0{});
    issue_loads(1, set1{});
    if (phase == 0) {
        write_tile(0, set0{});
        issue_loads(2, set0{});
    }
    __syncthreads();
    // iteration k writes tile m = k + 1 if it is ours: own index q = (m - phase) / NP, register set q & 1, refilled with q + 2
    // k = 4a + i writes tile m = k + 1 if it is ours ((i + 1) % NP == phase: known at compile time)
    auto iter = [&](int k, auto pos, auto set) {
        constexpr int I = decltype(pos)::value;
        if constexpr (((I + 1) % NP) == phase) {
            const int m = k + 1;
            write_tile(m % 3, set);
            issue_loads((m - phase) / NP + 2, set);
        }
        __syncthreads();
    };
    // with NP = 2 the set index of tile m is ((m - phase) / 2) & 1: period 4 in k, fixed per (k & 3, phase)
    using p0 = std::integral_constant<int, 0>;
    using p1 = std::integral_constant<int, 1>;
    using p2 = std::integral_constant<int, 2>;
    using p3 = std::integral_constant<int, 3>;
    int k = 0;
    for (; k + 3 < nstep; k += 4) {
        iter(k, p0{}, set0{});      // m = 4a + 1: phase 1, q = 2a     -> set 0
        iter(k + 1, p1{}, set1{});  // m = 4a + 2: phase 0, q = 2a + 1 -> set 1
        iter(k + 2, p2{}, set1{});  // m = 4a + 3: phase 1, q = 2a + 1 -> set 1
        iter(k + 3, p3{}, set0{});  // m = 4a + 4: phase 0, q = 2a + 2 -> set 0
    }
    if (k < nstep) iter(k++, p0{}, set0{});
    if (k < nstep) iter(k++, p1{}, set1{});
    if (k < nstep) iter(k++, p2{}, set1{});
}

// One pass over the stream, spikes only, 64 streams per workgroup, six waves: two loaders, filter, detect, two select waves.
// RING: candidate ring entries per stream (power of two).  The detect wave checks the space a tile really needs (its events, at
// least the DET_PF slots of the unconditional stores) against what the select waves still hold, so the whole ring is usable.
template <int N, int RING>
__global__ __launch_bounds__(384, 5) void bandpass_rzcc_sweep_kernel(const double *__restrict__ h, int8_t *__restrict__ spikes,
                                                                     int *__restrict__ flag_count, int *__restrict__ flag_list,
                                                                     IirCoef coef, int nlanes, int C, int T, int Ts, int w, int bipolar,
                                                                     const double *__restrict__ xin, int M, int shift)
{
    constexpr int SW = 64;         // streams per workgroup
    constexpr int ROW = SW + 1;    // padded row of the transposed input tile (doubles)
    __shared__ __attribute__((aligned(16))) double X[3][RZ_MT][ROW];
    __shared__ double ringV[RING][SW];
    __shared__ int ringP[RING][SW];
    __shared__ int nPub[SW];
    __shared__ int polPub[SW];     // 1: the stream's first candidate is a minimum (candidates alternate from there)
    __shared__ int deadPub[SW];
    __shared__ int ovPub[SW];      // the detect wave found the ring full: unit flagged
    __shared__ int oldPub[2][SW];  // per polarity: oldest ring entry the select wave still needs
    __shared__ unsigned long long ldTab[SW];  // stream bases of the loader waves

    // hardware waves 0, 1: loaders (even / odd tiles, four tiles of global loads in flight: with one loader the pipeline ran at the
    // pace of the memory latency); then 1: filter, 2: detect, 3: select maxima, 4: select minima
    const int wave_hw = threadIdx.x >> 6;
    const int wave = wave_hw == 0 ? 0 : wave_hw - 1;
    const int lane = threadIdx.x & 63;
    const int base = xcd_walk(blockIdx.x, gridDim.x) * SW;
    const int NM = (T + RZ_MT - 1) / RZ_MT;  // tiles
    const int NSTEP = NM + 2;
    const int lane_g = base + lane;
    const bool active = lane_g < nlanes;
    const int lane_c = active ? lane_g : nlanes - 1;  // clamped: inactive lanes shadow the last stream, results unused

    if (wave_hw == 0) {
        rz_loader_np<0>(X, h, xin, base, nlanes, C, T, Ts, M, shift, NM, NSTEP, lane, ldTab);
        return;
    }
    if (wave_hw == 1) {
        rz_loader_np<1>(X, h, xin, base, nlanes, C, T, Ts, M, shift, NM, NSTEP, lane, ldTab);
        return;
    }

    if (wave == 1) {
        // ------------------------------------ filter ---------------------------------------------------
        Iir<N> iir;
        iir.init();
        double cs = 0.0;
        pin_coef<N>(coef);
        __syncthreads();
        for (int k = 0; k < NSTEP; ++k) {
            if (k < NM) {
                const int buf = k % 3;
                const int tb = k * RZ_MT;
                const int steps = (T - tb) < RZ_MT ? (T - tb) : RZ_MT;
                if (steps == RZ_MT) {
                    // the whole tile into registers with hand-issued reads and ONE wait (the compiler's own placement waits
                    // for every pair of reads in the middle of the dependent arithmetic), then arithmetic, then the stores
                    double xr[RZ_MT];
                    const unsigned addr = (unsigned)(size_t)(&X[buf][0][lane]);
#pragma unroll
                    for (int j = 0; j < RZ_MT; ++j)
                        asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(xr[j]) : "v"(addr), "n"(j * ROW * 8));
                    asm volatile("s_waitcnt lgkmcnt(0)"
                                 : "+v"(xr[0]), "+v"(xr[1]), "+v"(xr[2]), "+v"(xr[3]), "+v"(xr[4]), "+v"(xr[5]), "+v"(xr[6]), "+v"(xr[7]),
                                   "+v"(xr[8]), "+v"(xr[9]), "+v"(xr[10]), "+v"(xr[11]), "+v"(xr[12]), "+v"(xr[13]), "+v"(xr[14]),
                                   "+v"(xr[15]));
#pragma unroll
                    for (int j = 0; j < RZ_MT; ++j) {
                        cs = cs + iir.step(coef, xr[j]);
                        xr[j] = cs;
                    }
#pragma unroll
                    for (int j = 0; j < RZ_MT; ++j) X[buf][j][lane] = xr[j];
                } else {
                    for (int j = 0; j < steps; ++j) {
                        cs = cs + iir.step(coef, X[buf][j][lane]);
                        X[buf][j][lane] = cs;
                    }
                }
            }
            __syncthreads();
        }
        return;
    }

    if (wave == 2) {
        // ------------------------------------ detect ---------------------------------------------------
        // A maximum completes when c falls after a rise: plateau [left, t-1] -> position (left+t-1)>>1, priority =
        // plateau value = prev.  Minima mirror this (priority -prev).  Maxima and minima alternate strictly, so both
        // share one candidate list and the polarity of candidate i is (first polarity) ^ (i & 1).
        //
        // Bit-parallel per lane: the 16 steps of a tile give two 16-bit words per lane, R (the sum rose at step j) and F (it
        // fell) -- two fp64 compares per step, each folded into its word by one add-with-carry (word = 2 word + mask bit).
        // Everything sequential in the old formulation (direction of the last strict change, plateau start) is then a
        // handful of integer operations on whole words: the direction recurrence D_{j+1} = R_j | (D_j & ~(R_j | F_j)) is
        // the carry chain of ONE addition, events are F & D (maxima) and R & ~D & "moved before" (minima), and the few
        // events of a tile (about two) are appended in a short loop instead of sixteen unconditional ring writes.
        // About 10 instead of 17 instructions per step, no scalar-unit dependency chains.
        double prev = __builtin_nan("");  // previous value of the running sum (NaN: no event at t = 0)
        int left = 0;                     // time of the last strict change
        int n = 0;                        // candidates appended so far
        int dir = 0;                      // direction of the last strict change: 0 none yet, 1 rise, 2 fall
        int ffall = 0;                    // the stream's FIRST strict change was a fall (its first candidate is a minimum)
        bool livel = true;                // this lane may still append (ring space checked for every tile)
        nPub[lane] = 0;
        polPub[lane] = 0;
        ovPub[lane] = 0;
        __syncthreads();
        for (int k = 0; k < NSTEP; ++k) {
            if (k >= 1 && k <= NM) {
                const int m = k - 1;
                const int tbase = m * RZ_MT;  // time of the tile's first step
                const int steps = (T - tbase) < RZ_MT ? (T - tbase) : RZ_MT;
                // oldPub may be the value a select wave published before the last barrier or the one it is publishing during this
                // step (no ordering between the two waves inside a step): either is a lower bound of what the select waves still
                // read.  (Read here, used by the ring-space check below.)
                const int o0 = oldPub[0][lane], o1 = oldPub[1][lane];
                const int oldest = bipolar ? (o0 < o1 ? o0 : o1) : o0;
                // ---- A: rise / fall words (bit j = step j of the tile) ----
                double c[RZ_MT];
#pragma unroll
                for (int jj = 0; jj < RZ_MT; ++jj) c[jj] = X[m % 3][jj][lane];  // (rows past a ragged end: masked below)
                unsigned Rw = 0, Fw = 0;
#pragma unroll
                for (int jj = RZ_MT - 1; jj >= 0; --jj) {
                    const double pj = jj ? c[jj ? jj - 1 : 0] : prev;
                    rise_fall_step(Rw, Fw, c[jj], pj);  // ordered > / ordered <
                }
                const unsigned vmask = (1u << steps) - 1u;
                Rw &= vmask;
                Fw &= vmask;
                // ---- B: direction before every step, events ----
                const unsigned Sw = Rw | Fw;                        // strict changes
                const unsigned Aw = (Rw | ~Sw) & 0xFFFFu;           // generate | propagate
                const unsigned Dw = (Aw + Rw + (dir == 1 ? 1u : 0u)) ^ Aw ^ Rw;  // bit j: the last change before step j was a rise
                const unsigned low = Sw & (0u - Sw);                // lowest strict change of the tile
                const unsigned Hw = dir != 0 ? 0xFFFFu : (Sw ? (~(low | (low - 1u)) & 0xFFFFu) : 0u);  // a change happened before step j
                unsigned Ew = (Fw & Dw) | (bipolar ? (Rw & ~Dw & Hw) : 0u);
                constexpr int DET_PF = 3;
                // Ring space for THIS tile: its events, and at least the DET_PF slots the unconditional stores below touch, must lie
                // below oldest + RING.  A stream without it stops appending for good (the unit goes to the fallback kernel).
                {
                    const int ne = __builtin_popcount(Ew);
                    if (livel && n + (ne > DET_PF ? ne : DET_PF) - oldest > RING) {
                        livel = false;
                        ovPub[lane] = 1;
                    }
                }
                Ew = livel ? Ew : 0u;
                if (dir == 0 && Sw) ffall = (Fw & low) ? 1 : 0;
                // ---- C: append the events (time order; maxima and minima alternate) ----
                // The plateau value of an event is read from the LDS tile at an index only the event knows.  One event per
                // trip with that read in the middle cost a full LDS latency per event, and a wave makes as many trips as its
                // busiest lane has events: the first DET_PF events of every lane are located with integer operations, their
                // values fetched together, then appended; a lane with more events finishes in the loop below.
                {
                    int jev[DET_PF], lfv[DET_PF];
                    double vev[DET_PF];
                    const char *xt = reinterpret_cast<const char *>(&X[m % 3][0][lane]);
#pragma unroll
                    for (int u = 0; u < DET_PF; ++u) {
                        const bool has = Ew != 0u;
                        const int je = has ? __builtin_ctz(Ew) : 0;
                        Ew &= Ew - 1u;  // (0 stays 0)
                        const unsigned below = Sw & ((1u << je) - 1u);
                        lfv[u] = below ? tbase + (31 - __builtin_clz(below)) : left;
                        jev[u] = has ? je : -1;
                        // plateau value: the sum just before the step that completes the candidate
                        const double v = *reinterpret_cast<const double *>(xt + (size_t)(je > 0 ? je - 1 : 0) * ROW * 8);
                        vev[u] = je > 0 ? v : prev;
                    }
                    // unconditional stores: a live lane without a (further) event writes into its next free slot without taking it
                    // (DET_PF slots are reserved, see the ring-space check) -- one exec mask around six LDS writes.  A lane that has
                    // stopped appending stores nothing: its next slot may be one a select wave still reads.
                    if (livel) {
#pragma unroll
                        for (int u = 0; u < DET_PF; ++u) {
                            const int slot = n & (RING - 1);
                            ringP[slot][lane] = lfv[u] + tbase + jev[u] - 1;  // left + t - 1; position = word >> 1 (plateau midpoint)
                            ringV[slot][lane] = vev[u];
                            n += jev[u] >= 0 ? 1 : 0;
                        }
                    }
                }
                while (__any(Ew != 0u)) {
                    if (Ew) {
                        const int je = __builtin_ctz(Ew);
                        Ew &= Ew - 1u;
                        const unsigned below = Sw & ((1u << je) - 1u);
                        const int lf = below ? tbase + (31 - __builtin_clz(below)) : left;
                        const double val = je ? *reinterpret_cast<const double *>(reinterpret_cast<const char *>(&X[m % 3][0][lane]) +
                                                                                 (size_t)(je - 1) * ROW * 8)
                                              : prev;
                        const int slot = n & (RING - 1);
                        ringP[slot][lane] = lf + tbase + je - 1;
                        ringV[slot][lane] = val;
                        ++n;
                    }
                }
                // ---- D: state after the tile ----
                if (Sw) {
                    left = tbase + (31 - __builtin_clz(Sw));
                    dir = (Dw >> RZ_MT) & 1u ? 1 : 2;
                }
                prev = steps == RZ_MT ? c[RZ_MT - 1] : X[m % 3][steps - 1][lane];
                nPub[lane] = n;
                polPub[lane] = ffall;
            }
            __syncthreads();
        }
        return;
    }

    // ---------------------------------------- select -------------------------------------------------------
    // One wave per polarity (wave 3: maxima, wave 4: minima).  Candidates alternate strictly, so a polarity owns every
    // second ring entry from its first one on; the two waves never touch the same entry.
    const int mypol = wave - 3;
    const bool mine = bipolar || mypol == 0;
    const int stride = bipolar ? 2 : 1;
    int i_next = -1;      // next own list index to examine (-1: the stream has no candidate yet)
    int s_open = -1;      // first list index of the open cluster (-1: none)
    int l_last = 0;       // position of the last own candidate
    int s_first = 0;      // position of the open cluster's first candidate (kept in a register: no LDS read when it closes)
    bool dead = !active;  // ring overflow (or lane out of range): stop selecting; redone by the fallback kernel
    const int b = lane_c / C;
    const int ch = lane_c - b * C;
    int8_t *sp = spikes + (size_t)b * T * C + ch;
    const int8_t mark = mypol ? -1 : 1;
    const double sgn = mypol ? -1.0 : 1.0;
    auto word_at = [&](int i) { return &ringP[i & (RING - 1)][lane]; };
    auto val_at = [&](int i) { return &ringV[i & (RING - 1)][lane]; };
    // a kept peak is one byte stored into [B][T][C]
    auto emit = [&](int pos) { sp[(size_t)pos * C] = mark; };
    auto close_cluster = [&](int s, int e, int lastpos, int first) {
        if (e - s <= stride) {
            emit(lastpos);
        } else if (e - s <= 2 * stride) {
            // two candidates (the most frequent multi-candidate cluster): they lie within w of each other by construction, so the
            // better one -- the later one on a tie -- is the spike; both positions are in registers, two LDS reads for the priorities
            const double v0 = *val_at(s) * sgn, v1 = *val_at(s + stride) * sgn;
            emit(v1 >= v0 ? lastpos : first);
        } else if (e - s <= 3 * stride) {
            // three candidates p0 < p1 < p2, consecutive gaps < w: the greedy rule in closed form -- the best one (the later one on a tie) is a spike and removes its
            // neighbours; if that was an end and the other end is >= w away, the other end is a spike too.  Three priorities and
            // the middle position from LDS, no selection loop for the whole wave to sit through.
            const double v0 = *val_at(s) * sgn, v1 = *val_at(s + stride) * sgn, v2 = *val_at(s + 2 * stride) * sgn;
            const bool mid = v1 >= v0 && v2 < v1;  // arg-max with "later wins": 1 beats 0 on >=, 2 beats the best so far on >=
            if (mid) {
                emit(*word_at(s + stride) >> 1);
            } else {
                const bool last_best = v2 >= (v1 >= v0 ? v1 : v0);
                emit(last_best ? lastpos : first);
                if (lastpos - first >= w) emit(last_best ? first : lastpos);
            }
        } else {
            // longer ones: up to eight candidates in registers (sixteen do not fit this kernel's 96 VGPRs), then the list walk
            resolve_cluster<8>(s, e, stride, w, emit, word_at, val_at, sgn);
        }
    };
    if (mypol == 0) deadPub[lane] = 0;
    oldPub[mypol][lane] = 0;
    if (!mine) oldPub[mypol][lane] = 0x7fffffff;
    __syncthreads();
    for (int k = 0; k < NSTEP; ++k) {
        if (k >= 2 && mine) {
            const int n = nPub[lane];  // candidates published by the detect wave before the last barrier
            if (ovPub[lane]) dead = true;
            if (i_next < 0 && n > 0) i_next = bipolar ? (polPub[lane] ^ mypol) : 0;
            // one candidate per lane and trip.  (Fetching the words of the next four candidates up front was measured and
            // rejected: most tiles bring one new candidate per lane, the three extra reads and selects cost more than the
            // latency they hide -- select waves 1450 -> 1720 cycles per tile on config 2.)
            while (__any(!dead && i_next >= 0 && i_next < n)) {
                if (!dead && i_next >= 0 && i_next < n) {
                    const int i = i_next;
                    const int pos = *word_at(i) >> 1;
                    if (s_open >= 0 && pos - l_last >= w) {
                        close_cluster(s_open, i, l_last, s_first);
                        s_open = -1;
                    }
                    if (s_open < 0) {
                        s_open = i;
                        s_first = pos;
                    }
                    l_last = pos;
                    i_next = i + stride;
                }
            }
            // everything from the open cluster on must survive in the ring; without one, everything not yet examined
            oldPub[mypol][lane] = dead ? 0x7fffffff : (s_open >= 0 ? s_open : (i_next >= 0 ? i_next : 0));
        }
        __syncthreads();
    }
    if (active && mine) {
        if (ovPub[lane]) dead = true;
        if (!dead && s_open >= 0) close_cluster(s_open, nPub[lane], l_last, s_first);  // the stream ends here
        if (dead && atomicExch(&deadPub[lane], 1) == 0) {  // flag the unit once, whichever polarity gave up
            const int kk = atomicAdd(flag_count, 1);
            flag_list[kk] = lane_g;  // (unit id of chunk 0)
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Fallback for flagged (stream, chunk) units: serial walk from the chunk's checkpoint, unbounded candidate lists in
// global scratch (slot-major), selection afterwards.  Slow (conditional global stores in the serial loop) but exact
// for any input.  Slot s handles the flagged units s, s + nslots, ... one after the other.
// ---------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(64) void rzcc_unit_fallback_kernel(const double *__restrict__ h, int8_t *__restrict__ spikes,
                                                                 const int *__restrict__ flag_count,
                                                                 const int *__restrict__ flag_list, int *__restrict__ plist,
                                                                 double *__restrict__ vlist, int nslots, IirCoef coef,
                                                                 int nlanes, int C, int T, int Ts, int w, int bipolar,
                                                                 const double *__restrict__ xin, int M, int shift, RzGeom g,
                                                                 const double *__restrict__ ckd, const int *__restrict__ cki)
{
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= nslots) return;
    const int count = *flag_count;
    const int NMall = (T + RZ_MT - 1) / RZ_MT;
    const size_t NS = (size_t)nslots;
    const size_t nl = (size_t)nlanes;
    int *P = plist + slot;
    double *V = vlist + slot;
    const int sh = shift % T;
    auto word_at = [&](int i) { return P + (size_t)i * NS; };
    auto val_at = [&](int i) { return V + (size_t)i * NS; };

    for (int idx = slot; idx < count; idx += nslots) {
        const int unit = flag_list[idx];
        const int p = unit / nlanes;
        const int lane_g = unit - p * nlanes;
        const RzSpan span = rz_span(g, p, NMall);
        const int b = lane_g / C;
        const int ch = lane_g - b * C;
        const bool rolled = xin != nullptr && ch < M;
        const double *src = rolled ? xin + (size_t)b * T * M + ch : h + (size_t)lane_g * Ts;
        auto sample = [&](int t) {
            int tr = t - sh;
            tr = tr < 0 ? tr + T : tr;
            return rolled ? src[(size_t)tr * M] : src[t];
        };
        Iir<N> iir;
        auto load_ck = [&](int q, double &cs) {  // q < 0: the stream start
            iir.init();
            cs = 0.0;
            if (q >= 0) {
#pragma unroll
                for (int i = 0; i < N - 1; ++i) iir.z[i] = ckd[((size_t)q * N + i) * nl + lane_g];
                cs = ckd[((size_t)q * N + (N - 1)) * nl + lane_g];
            }
        };
        double c = 0.0;
        int left = 0, dir = 0;  // dir: +1 rise, -1 fall, 0 none yet
        if (p > 0) {
            const int dcode = cki[((size_t)(p - 1) * 3 + 0) * nl + lane_g];
            left = cki[((size_t)(p - 1) * 3 + 1) * nl + lane_g];
            dir = dcode == RZ_DIR_RISE ? 1 : (dcode == RZ_DIR_FALL ? -1 : 0);
            if (dcode == RZ_DIR_UNKNOWN) {
                // the last strict change lies in tile Lc, more than a tile before this chunk: walk that tile again from
                // the nearest checkpoint at or before it
                const int Lc = cki[((size_t)(p - 1) * 3 + 2) * nl + lane_g];
                int pq = (Lc + g.Vt) / g.Lt;  // largest chunk whose first tile is <= Lc
                pq = pq > p - 1 ? p - 1 : pq;
                load_ck(pq - 1, c);
                const int t0 = pq == 0 ? 0 : (pq * g.Lt - g.Vt) * RZ_MT;
                for (int t = t0; t < (Lc + 1) * RZ_MT; ++t) {
                    const double c1 = c + iir.step(coef, sample(t));
                    if (t == 0) {
                        // the first sample has no predecessor: never a strict change
                    } else if (c1 > c) {
                        dir = 1;
                        left = t;
                    } else if (c1 < c) {
                        dir = -1;
                        left = t;
                    }
                    c = c1;
                }
            }
        }
        load_ck(p - 1, c);
        double prev = p > 0 ? c : __builtin_nan("");

        // ---- candidates from the chunk start until every owned cluster has provably closed -------------------
        int n = 0;
        int lastpos[2] = {0, 0};
        bool seen[2] = {false, false};
        bool done[2] = {false, !bipolar};
        const int t_lo = span.m_lo * RZ_MT;
        auto walk = [&](int t, double xt) {
            const double y = iir.step(coef, xt);
            c = c + y;
            const bool rise = c > prev;
            const bool fall = c < prev;
            if ((fall && dir > 0) || (bipolar && rise && dir < 0)) {
                const int pol = rise ? 1 : 0;
                const int pos = (left + t - 1) >> 1;
                P[(size_t)n * NS] = ((left + t - 1) & ~1) | pol;
                V[(size_t)n * NS] = rise ? -prev : prev;
                ++n;  // n <= T - 1 < capacity T
                // a cluster that starts at or after own_hi: every owned cluster of this polarity is closed
                if ((!seen[pol] || pos - lastpos[pol] >= w) && pos >= span.own_hi) done[pol] = true;
                seen[pol] = true;
                lastpos[pol] = pos;
            }
            left = (rise || fall) ? t : left;
            dir = rise ? 1 : (fall ? -1 : dir);
            prev = c;
            // the next candidate completes at t' >= t + 1 with left' >= left: position (left' + t' - 1) >> 1 >= (left + t) >> 1
            // (a stream that has not moved at all yet: its first plateau starts at t + 1 at the earliest)
            const int nextpos = dir == 0 ? t + 1 : (left + t) >> 1;
            if (nextpos >= span.own_hi) {
                if (!seen[0] || nextpos - lastpos[0] >= w) done[0] = true;
                if (!seen[1] || nextpos - lastpos[1] >= w) done[1] = true;
            }
        };
        // The samples of FB_BLK steps are fetched together (independent loads, one wait).  With one load per step in front of
        // the conditional list stores the walk ran at one memory round trip per step (0.7 us: 8.7 ms for ONE flagged unit of a
        // 12 000-frame chunk -- more than the whole chunked pass of config 4).
        constexpr int FB_BLK = 16;
        for (int t0 = t_lo; t0 < T && !(done[0] && done[1]); t0 += FB_BLK) {
            double xs[FB_BLK];
#pragma unroll
            for (int u = 0; u < FB_BLK; ++u) xs[u] = sample(t0 + u < T ? t0 + u : T - 1);
#pragma unroll
            for (int u = 0; u < FB_BLK; ++u)
                if (t0 + u < T && !(done[0] && done[1])) walk(t0 + u, xs[u]);
        }

        // ---- clusters of each polarity; the owned ones are resolved and scattered -----------------------------
        int8_t *sp = spikes + (size_t)b * T * C + ch;
        const int stride = bipolar ? 2 : 1;
        const int first_pol = n > 0 ? (P[0] & 1) : 0;
        for (int pol = 0; pol < (bipolar ? 2 : 1); ++pol) {
            const int8_t mark = pol ? -1 : 1;
            const int i0 = bipolar ? (first_pol == pol ? 0 : 1) : 0;
            if (i0 >= n) continue;
            int s = i0;
            int plast = *word_at(i0) >> 1;
            for (int i = i0 + stride;; i += stride) {
                const bool has = i < n;
                int pi = 0;
                bool closes = true;
                if (has) {
                    pi = *word_at(i) >> 1;
                    closes = (pi - plast) >= w;
                }
                if (closes) {
                    const int e = has ? i : n;
                    const int first = *word_at(s) >> 1;
                    if (first >= span.own_lo && first < span.own_hi) {
                        if (e - s <= stride)
                            sp[(size_t)plast * C] = mark;
                        else
                            resolve_cluster(s, e, stride, w, [&](int pos) { sp[(size_t)pos * C] = mark; }, word_at, val_at, 1.0);
                    }
                    s = i;
                }
                if (!has) break;
                plast = pi;
            }
        }
    }
}

// Zero fill as an ordinary kernel.  hipMemsetAsync is avoided on purpose: captured into a HIP graph (ROCm 7.x) the
// memset NODE was observed not to be ordered before the kernel nodes that follow it -- the fallback kernel then read a
// stale flagged-stream counter and faulted on the third replay -- whereas kernel -> kernel edges are honoured.
// `extra` (may be null): a second, 256-byte block zeroed by the same launch (the encoder's counters beside its spike tensor)
__global__ __launch_bounds__(256) void zero_fill_kernel(uint4 *__restrict__ p16, size_t n16, unsigned char *__restrict__ tail,
                                                         int ntail, uint4 *__restrict__ extra)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) p16[i] = make_uint4(0, 0, 0, 0);
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0;
    if (extra && blockIdx.x == gridDim.x - 1 && threadIdx.x < 16) extra[threadIdx.x] = make_uint4(0, 0, 0, 0);
}

static hipError_t zero_fill(void *ptr, size_t bytes, hipStream_t stream, void *extra256 = nullptr)
{
    // torch / hipMalloc buffers are at least 16-byte aligned; the scatter target [B][T][C] int8 may have any size
    const size_t n16 = bytes / 16;
    const int ntail = (int)(bytes - n16 * 16);
    size_t blocks = (n16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<uint4 *>(ptr), n16,
                       reinterpret_cast<unsigned char *>(ptr) + n16 * 16, ntail, reinterpret_cast<uint4 *>(extra256));
    return hipGetLastError();
}

struct RzScratch {
    size_t count, list, ckd, cki, vlist, plist, total;
    int nslots;
};

static RzScratch rz_scratch(int nlanes, int T, int P)
{
    RzScratch s;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t off = 0;
    s.count = off;
    off += 256;
    s.list = off;
    off += al((size_t)P * nlanes * sizeof(int));
    s.ckd = off;
    off += al((size_t)(P > 1 ? P - 1 : 0) * MICLOC_MAX_IIR * nlanes * sizeof(double));
    s.cki = off;
    off += al((size_t)(P > 1 ? P - 1 : 0) * 3 * nlanes * sizeof(int));
    // fallback candidate lists: T entries per slot (a unit may have to walk to the end of its stream), at most 256 MiB
    long long slots = (256ll << 20) / (12ll * (T > 0 ? T : 1));
    if (slots < 64) slots = 64;
    if (slots > (long long)P * nlanes) slots = (long long)P * nlanes;
    if (slots > 4096) slots = 4096;
    s.nslots = (int)slots;
    s.vlist = off;
    off += al((size_t)T * s.nslots * sizeof(double));
    s.plist = off;
    off += al((size_t)T * s.nslots * sizeof(int));
    s.total = al(off);
    return s;
}

}  // namespace rzsweep

// true: the launch had this file's shape and was enqueued here (*err: its status; zero fill, encoder, fallback for flagged units -- the
// scratch layout is rzcc.hip's); false: nothing was enqueued, the caller goes to launch_bandpass_rzcc
bool launch_bandpass_rzcc_sweep(const IirCoef &coef, const double *h, int nlanes, int C, int T, int Ts, int robust_width, int bipolar,
                                int8_t *spikes, void *scratch, hipStream_t stream, const double *xin, int M, int shift, int chunk_frames,
                                int phases, hipError_t *err)
{
    using namespace rzsweep;
    constexpr int N = 5;
    if (VARIANT_RZ_TWO_SLOTS || coef.n != N || !spikes || !scratch || !(phases & RZ_PHASE_ENCODE)) return false;
    if ((unsigned long long)T * (unsigned long long)(M > 0 ? M : 1) > 0xffffffffull) return false;  // (the caller's launcher reports it)
    if (rzcc_chunks(nlanes, T, robust_width, chunk_frames) != 1) return false;
    RzGeom g;  // one chunk: the whole stream (look-back and tail tiles belong to chunked launches)
    g.P = 1;
    g.Lt = (T + RZ_MT - 1) / RZ_MT;
    g.Vt = (robust_width + RZ_MT - 1) / RZ_MT < 1 ? 1 : (robust_width + RZ_MT - 1) / RZ_MT;
    g.V2t = 4;
    const RzScratch sc = rz_scratch(nlanes, T, 1);
    // the workspace was sized by rzcc.hip's rzcc_scratch_bytes: decline if its layout is no longer the one copied here
    if (sc.total != rzcc_scratch_bytes(nlanes, T, robust_width, chunk_frames)) return false;
    unsigned char *base = reinterpret_cast<unsigned char *>(scratch);
    int *flag_count = reinterpret_cast<int *>(base + sc.count);
    int *flag_list = reinterpret_cast<int *>(base + sc.list);
    *err = zero_fill(spikes, (size_t)nlanes * T, stream, base + sc.count);  // (+ the 256-byte counter block: one launch)
    if (*err != hipSuccess) return true;
    const int nblk = (nlanes + 63) / 64;
    hipLaunchKernelGGL((bandpass_rzcc_sweep_kernel<N, RZ_RING_SWEEP>), dim3(nblk), dim3(384), 0, stream, h, spikes, flag_count, flag_list,
                       coef, nlanes, C, T, Ts, robust_width, bipolar, xin, M, shift);
    hipLaunchKernelGGL((rzcc_unit_fallback_kernel<N>), dim3((sc.nslots + 63) / 64), dim3(64), 0, stream, h, spikes, flag_count, flag_list,
                       reinterpret_cast<int *>(base + sc.plist), reinterpret_cast<double *>(base + sc.vlist), sc.nslots, coef, nlanes, C, T,
                       Ts, robust_width, bipolar, xin, M, shift, g, nullptr, nullptr);
    *err = hipGetLastError();
    return true;
}

}  // namespace micloc
