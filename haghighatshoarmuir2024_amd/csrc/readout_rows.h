// What the read-out kernels share: the tails that turn partial sums, counts or envelopes into a power row and a DoA index.  Three rules,
// each a promise of bit equality between entry points ("a single window >= T returns the unwindowed bits", "the stream returns the
// one-shot bits"), stated once.  DESIGN 4.22.
//
// 1. THE FIRST MAXIMUM (np.argmax) of pairs (value, index): the larger value wins; an equal value with the lower index wins; index
//    RO_NONE means "saw nothing" and never wins, and a row of nothing but RO_NONE gives index 0.  `better` is the comparison,
//    block_first_max the LDS tree over a workgroup, wave_first_max the xor butterfly over lanes, row_first_max one wave on one stored row.
//    Callers: window_power_kernel (windows.hip), stream_window_kernel (stream_windows.hip), stream_complex_accumulate_kernel
//    (stream_complex.hip), stream_band_sum_kernel (stream_bands.hip), band_sum_kernel (filterbank.hip), cov_power_kernel (covariance.hip),
//    peak_location_kernel and rows_argmax_kernel (sweep.hip), xylo_stream_readout_kernel (stream_xylo.hip), track_rows_kernel (track.hip),
//    track_chain_reduce (track_rows.h), music_first_argmax (music_rows.h, whose "nothing" is index -1).
//    The per-thread scans in front stay with their kernels: they differ on purpose (`p > best` from -1.0 where the values are >= 0 and a
//    NaN must not win; `s == s && (bi == RO_NONE || s > best)` where band sums may be negative).
//    THE ONE EXCEPTION: beamform.hip (power_argmax_kernel and its two neighbours) keeps three copies of the tree.  Its hash is pinned by
//    profiles/r6/MANIFEST.json; the copies fold in here with the next profile round.  (peaks.hip's pk_better is the same comparison on
//    candidates, no reduction of a row to its maximum; its text is pinned by the kernel profile of profiles/multisource/ and stays too.)
//
// 2. THE STREAMING WINDOW SCHEDULE: which windows a tile opens, feeds and emits (StreamWindowWalk), how many windows a recording has
//    (window_count64), how many are complete (windows_complete), and which windows every band of a wideband stream has ready
//    (ready_windows).  Callers: stream_window_kernel, xylo_stream_window_kernel (stream_xylo.hip), window_count (windows.hip),
//    stream_band_sum_kernel, xylo_stream_readout_kernel.
//
// 3. THE BLOCKED RUNNING SUM (BlockedSum): the order of additions of the one-shot time reduction (power_argmax_kernel, beamform.hip), cut
//    at any chunk border.  Callers: stream_window_kernel, stream_complex_accumulate_kernel.  window_power_kernel (windows.hip) keeps its
//    side-by-side block form: the same additions, but four blocks in flight, which this walk cannot express.
#pragma once
#include "micloc_internal.h"

namespace micloc {

constexpr int RO_NONE = 0x7fffffff;

// ---- 1. the first maximum ---------------------------------------------------------------------------------------------------------------
// (ov, oi) takes over from (mv, mi).  Two spellings stood in the kernels: this one, and `ov > mv || (ov == mv && oi < mi)` without the
// guards, which relied on the value a thread keeps while it has seen nothing (-1.0, or -1 for counts).  For every row those callers can
// produce the two agree: their scan takes a candidate only if it is > -1, so an entry with index NONE carries a value strictly below
// every real one.  (a) oi == NONE: ov = -1 is neither above mv >= -1 nor, on equality, is NONE below mi: it never won.  (b) mi == NONE
// and oi real: ov > -1 = mv: it always won.  (c) both real: the guards are idle.  The guards make that hold for any value beside NONE
// (the band sums keep 0.0 there).
template <int NONE = RO_NONE, class V>
__device__ __forceinline__ bool better(V ov, int oi, V mv, int mi)
{
    return oi != NONE && (mi == NONE || ov > mv || (ov == mv && oi < mi));
}

// Over a workgroup: the threads with `in` set are col = 0 .. COLS - 1 (COLS a power of two) and hold one pair each; sv / si are COLS
// entries of LDS.  EVERY thread of the workgroup calls it -- COLS barriers' worth: one behind the stores, one per halving -- and gets
// the index of the first maximum, 0 for a row without a winner.  TRAIL: one more barrier behind the read of the result, for callers that
// loop and rewrite sv / si; without it the caller must pass a barrier before it does.
template <int COLS, class V, bool TRAIL = false>
__device__ __forceinline__ int block_first_max(V best, int bi, V *sv, int *si, int col, bool in = true)
{
    if (in) {
        sv[col] = best;
        si[col] = bi;
    }
    __syncthreads();
    for (int s = COLS / 2; s > 0; s >>= 1) {
        if (in && col < s) {
            const V ov = sv[col + s];
            const int oi = si[col + s];
            if (better(ov, oi, sv[col], si[col])) {
                sv[col] = ov;
                si[col] = oi;
            }
        }
        __syncthreads();
    }
    const int a = si[0] == RO_NONE ? 0 : si[0];
    if (TRAIL) __syncthreads();
    return a;
}

// Over WIDTH adjacent lanes of a wave (64: the wave; 4: a quad): every lane ends with the group's first maximum, (.., RO_NONE) if none.
template <int WIDTH, class V>
__device__ __forceinline__ void wave_first_max(V &best, int &bi)
{
#pragma unroll
    for (int s = WIDTH / 2; s > 0; s >>= 1) {
        const V ov = __shfl_xor(best, s, 64);
        const int oi = __shfl_xor(bi, s, 64);
        if (better(ov, oi, best, bi)) {
            best = ov;
            bi = oi;
        }
    }
}

// One wave on one stored row r[0 .. G) of values >= 0, lane l: np.argmax(r) -- a NaN never wins, a row of NaN leaves (-1.0, RO_NONE).
__device__ __forceinline__ void row_first_max(const double *__restrict__ r, int G, int l, double &best, int &bi)
{
    best = -1.0;
    bi = RO_NONE;
    for (int g = l; g < G; g += 64) {  // ascending per lane: its first maximum
        const double v = r[g];
        if (v > best) {
            best = v;
            bi = g;
        }
    }
    wave_first_max<64>(best, bi);
}

// ---- 2. the window schedule -------------------------------------------------------------------------------------------------------------
// windows of a recording of T units (frames, or chunks): 1 if T <= window, else 1 + ceil((T - window) / hop)
__host__ __device__ inline long long window_count64(long long T, long long window, long long hop)
{
    return T <= window ? 1 : 1 + (T - window + hop - 1) / hop;
}

// windows complete once `done` chunks are in: window n is the chunks [n hchunks, n hchunks + wchunks)
__host__ __device__ inline int windows_complete(int done, int wchunks, int hchunks) { return done < wchunks ? 0 : (done - wchunks) / hchunks + 1; }

// One tile of a stream between its accumulate and its commit.  The control words: ctl[0] = chunks done before this call (absolute),
// ctl[6] = chunks done after it, [ctl[4], ctl[5]) = the rows of the new chunks in a buffer of `rows` rows, ctl[STREAM_CLK_TEND] = T, the
// frames pushed after this tile.  CH: frames per chunk.  The recording is complete once the final tile's chunks cover its T frames (a
// lag failure leaves them short: no read-out at the end).  The windows n0 .. n_started hold a new chunk or are emitted by this call;
// those below n_emit are emitted -- complete, or on the ended recording every window of window_count64(T, window, hop), cut at the
// frames it has; windows past that count started but do not exist in the rule.
struct StreamWindowWalk {
    int done, lo, ready, wchunks, hchunks, CH, T;
    bool ok, ended;
    int n0, n_started;
    long long n_emit;

    struct Window {
        int c0, ca, cb;     // first chunk of the window; the new chunks [ca, cb) it takes (ca > c0: it opened in an earlier call)
        bool emit, newest;  // emitted by this call; the last one this call emits
        long long frames;   // frames of an emitted window
    };

    __device__ __forceinline__ StreamWindowWalk(const int *__restrict__ ctl, int final_tile, int CH_, int wchunks_, int hchunks_, int rows)
        : done(ctl[0]), lo(ctl[4]), ready(ctl[6]), wchunks(wchunks_), hchunks(hchunks_), CH(CH_), T(ctl[STREAM_CLK_TEND])
    {
        const int hi = ctl[5];
        ok = !(ready - done != hi - lo || hi < lo || lo < 0 || hi > rows);  // (never false: the kernel in front writes both)
        ended = final_tile && (long long)ready * CH >= T;
        n0 = windows_complete(done, wchunks, hchunks);
        n_started = ready > 0 ? (ready - 1) / hchunks : -1;
        n_emit = ended ? window_count64(T, (long long)wchunks * CH, (long long)hchunks * CH) : windows_complete(ready, wchunks, hchunks);
    }

    __device__ __forceinline__ Window window(int n) const
    {
        Window w;
        w.c0 = n * hchunks;  // (n <= (ready - 1) / hchunks: no overflow)
        w.ca = done > w.c0 ? done : w.c0;
        w.cb = ready - w.c0 < wchunks ? ready : w.c0 + wchunks;
        w.emit = n < n_emit;
        w.newest = n == n_emit - 1;
        w.frames = (long long)T - (long long)w.c0 * CH;
        if (!ended || w.frames > (long long)wchunks * CH) w.frames = (long long)wchunks * CH;
        return w;
    }

    __device__ __forceinline__ int row(int ch) const { return lo + ch - done; }  // buffer row of the new chunk ch
    __device__ __forceinline__ int head() const { return (int)(n_emit > 0x7fffffffll ? 0x7fffffffll : n_emit); }  // windows emitted after this call
};

// The windows every band of a wideband stream has ready.  Band f has emitted count(f) windows into a ring of Kb rows, window n in row
// n % Kb; `emitted` wideband windows are behind us.  [lo, hi) = [max(emitted, max_f count(f) - Kb), min_f count(f)) can be summed; a
// window below lo has left the ring of the band that leads and is given up, never read from a row that holds a later window.  A caller
// that moves `emitted` on to `next` gives up given(next) windows.  (stream_band_sum_kernel moves to max(lo, hi) and keeps the two
// DELTAS in its state words 2 / 3; xylo_stream_readout_kernel moves to max(hi, emitted) and keeps the ABSOLUTE counts there.)
struct ReadyWindows {
    int emitted, lo, hi;
    __device__ __forceinline__ int given(int next) const { return (lo < next ? lo : next) - emitted; }
};

template <class Count>
__device__ __forceinline__ ReadyWindows ready_windows(int F, int emitted, int Kb, const Count &count)
{
    int cmin = 0x7fffffff, cmax = 0;
    for (int f = 0; f < F; ++f) {
        const int c = count(f);
        cmin = c < cmin ? c : cmin;
        cmax = c > cmax ? c : cmax;
    }
    return ReadyWindows{emitted, cmax - Kb > emitted ? cmax - Kb : emitted, cmin};
}

// ---- 3. the blocked running sum -----------------------------------------------------------------------------------------------------------
// power_argmax_kernel's order (beamform.hip): chunk sums ascend inside a block of STREAM_BLOCK_CHUNKS chunks, block sums ascend onto the
// total, the open block is added last.  `open` = chunks in the open block; {total, s} is what a stream carries between calls.
struct BlockedSum {
    double total, s;
    int open;

    __device__ __forceinline__ void step()
    {
        if (++open == STREAM_BLOCK_CHUNKS) {
            total += s;
            s = 0.0;
            open = 0;
        }
    }
    __device__ __forceinline__ void add(double v)  // one chunk
    {
        s += v;
        step();
    }
    __device__ __forceinline__ void add(double re, double im)  // one chunk of folded rows: s += Re; s += Im
    {
        s += re;
        s += im;
        step();
    }
    __device__ __forceinline__ double close() const { return open > 0 ? total + s : total; }  // the sum so far; the state is untouched
};

}  // namespace micloc
