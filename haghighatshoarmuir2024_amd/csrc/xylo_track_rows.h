// What the two tracking forms of the packed Xylo LIF share -- the one-shot xylo_lif_track_kernel of xylo.hip and the resumable
// xylo_lif_track_stream_kernel of stream_xylo.hip: the tap of XpLif's walk that runs Envelope.evolve on the spike counts and leaves the
// first maximum over the neurons per frame, its set-up, the combine over the waves of a workgroup and the combine over the neuron blocks.
// Stated once, so that a frame has the same envelope bits whether its trial was walked in one launch or cut at launch borders.
// include/micloc_hip.h, "Xylo moving-target tracking", has the rule; DESIGN 4.23 the structure.  (xylo_track.h is the host side: what
// the one-shot call offers to the C-ABI unit.)
#pragma once
#include "readout_rows.h"
#include "xylo_rows.h"

namespace micloc {

// The tap of XpLif: the lane keeps the envelope of its two neurons beside isyn / vmem and the packed counts of the 16 steps of a group.
// Once the group is settled -- after the walk from the saved state, where one was needed -- the 32 envelope steps run and leave one
// (value, neuron) pair per frame and lane: the better of the lane's two neurons, n0 < n1 winning a tie.  The 16 pairs of the 64 lanes
// are folded crosswise: a lane hands half of its frames to its partner at distance 32, 16, 8 and 4 and keeps the other half, so that
// after 8 + 4 + 2 + 1 exchanges lane l holds frame l >> 2 over sixteen lanes, and wave_first_max<4> over the quad finishes it -- 17
// exchanges for 16 frames where a butterfly per frame takes 96.  `better` orders by value, then by neuron number: the lane layout
// ((q, lc) holds 32 q + lc and 32 q + 16 + lc) does not matter.  The wave's pairs go to its row of an LDS tile [waves][XP_TT]; behind
// the staged tile one thread per frame takes the waves in ascending order (a strictly larger value takes over: track_combine_row's
// rule) and writes the result.
struct XpTrackTap {
    static constexpr bool on = true;
    double a_rise, i_rise, a_fall;
    double e0, e1;  // e[t-1] of the lane's two neurons
    int cw[16];     // packed counts of the group's steps
    int n0, n1, l, off;
    bool act0, act1, first;
    double *sv;  // this wave's row of the pair tile
    int *si;

    __device__ __forceinline__ double env(double e, double m, bool f) const
    {
        const double up = __dadd_rn(__dmul_rn(a_rise, e), __dmul_rn(i_rise, m));
        const double down = __dmul_rn(a_fall, e);
        const double nx = (m >= e) ? up : down;
        return f ? m : nx;
    }
    // one step of both envelopes -> the lane's pair (a lane without neurons: RO_NONE, which never wins)
    __device__ __forceinline__ void advance(int c, bool f, double &bv, int &bi)
    {
        e0 = env(e0, (double)(c & 0xffff), f);
        e1 = env(e1, (double)(c >> 16), f);
        bv = act0 ? e0 : -1.0;
        bi = act0 ? n0 : RO_NONE;
        if (act1 && e1 > e0) {
            bv = e1;
            bi = n1;
        }
    }
    // lanes at distance D swap halves of their K + K pairs: the lower lane keeps [0, K), the upper one [K, 2 K), both in [0, K)
    template <int D, int K>
    __device__ __forceinline__ void fold(double *bv, int *bi) const
    {
        const bool up = (l & D) != 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const double ov = __shfl_xor(up ? bv[i] : bv[i + K], D, 64);
            const int oi = __shfl_xor(up ? bi[i] : bi[i + K], D, 64);
            double kv = up ? bv[i + K] : bv[i];
            int ki = up ? bi[i + K] : bi[i];
            if (better(ov, oi, kv, ki)) {
                kv = ov;
                ki = oi;
            }
            bv[i] = kv;
            bi[i] = ki;
        }
    }

    __device__ __forceinline__ void begin(int off_, bool first_) { off = off_, first = first_; }
    __device__ __forceinline__ void put(int j, int c) { cw[j] = c; }
    __device__ __forceinline__ void group()
    {
        double bv[16];
        int bi[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) advance(cw[j], first && j == 0, bv[j], bi[j]);
        fold<32, 8>(bv, bi);
        fold<16, 4>(bv, bi);
        fold<8, 2>(bv, bi);
        fold<4, 1>(bv, bi);
        wave_first_max<4>(bv[0], bi[0]);
        if ((l & 3) == 0) {
            sv[off + (l >> 2)] = bv[0];
            si[off + (l >> 2)] = bi[0];
        }
    }
    __device__ __forceinline__ void single(int j, int c)
    {
        double bv;
        int bi;
        advance(c, first && j == 0, bv, bi);
        wave_first_max<64>(bv, bi);
        if (l == 0) {
            sv[off + j] = bv;
            si[off + j] = bi;
        }
    }
};

// What the one-shot and the stream form of the tracking walk share around the tap: its set-up from the lane's constants (the envelopes
// e0 / e1 are the kernel's: zero, or the stream's state) ...
template <class Lif>
__device__ __forceinline__ void xp_track_tap_init(Lif &lif, double a_rise, double i_rise, double a_fall, double (*sv)[XP_TT], int (*si)[XP_TT])
{
    auto &tap = lif.tap;
    tap.a_rise = a_rise, tap.i_rise = i_rise, tap.a_fall = a_fall;
    tap.n0 = lif.n0, tap.n1 = lif.n1, tap.act0 = lif.act0, tap.act1 = lif.act1;
    tap.l = lif.l, tap.off = 0, tap.first = false;
    tap.sv = sv[lif.wv];
    tap.si = si[lif.wv];
}

// ... and run_range's `done`: behind the staged tile one thread per frame takes the waves' pairs in ascending order (ascending neurons: a
// strictly larger value takes over) and hands emit(f, best, bi) the result of the tile's frame f.  (The barrier at the head of the next
// tile of run_range keeps these reads in front of the next pairs.)
template <class Emit>
__device__ __forceinline__ void xp_track_rows(const double (*sv)[XP_TT], const int (*si)[XP_TT], int waves, int tid, int nthreads, int steps,
                                              Emit emit)
{
    __syncthreads();
    for (int f = tid; f < steps; f += nthreads) {
        double best = -1.0;
        int bi = RO_NONE;
        for (int w = 0; w < waves; ++w) {
            const double v = sv[w][f];
            const int i = si[w][f];
            if (i != RO_NONE && v > best) {
                best = v;
                bi = i;
            }
        }
        emit(f, best, bi);
    }
}

// the pairs of one frame over the neuron blocks, ascending = ascending neurons: only a strictly larger value takes over (counts are
// integers: every block has a winner)
__device__ __forceinline__ void xylo_track_combine_row(const double *__restrict__ pval, const int32_t *__restrict__ pidx, int nblk, double &best,
                                                       int &bi)
{
    best = -1.0;
    bi = RO_NONE;
    for (int c = 0; c < nblk; ++c) {
        const double v = pval[c];
        const int i = pidx[c];
        if (better(v, i, best, bi)) {
            best = v;
            bi = i;
        }
    }
}

}  // namespace micloc
