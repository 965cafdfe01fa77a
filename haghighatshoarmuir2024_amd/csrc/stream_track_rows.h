// What the streaming tracking kernels share -- the single-plan ones of stream_track.hip and the band ones of stream_track_bands.hip: the
// range of a tile read from the stream's words, where a finished row goes (the ring, the latest words, or the pairs of a column group) and
// the combine of a position's pairs.  A kernel keeps what differs: whose words give the range, and the walk it runs over it.
#pragma once
#include "bandpass_rows.h"
#include "track_rows.h"

namespace micloc {

// the frames [f0, f1) of the window (SNN) or of the staging array (complex) that this tile made final; position p is frame abs0 + p
struct TrackSpan {
    int f0, f1, abs0;
};

template <bool COMPLEX>
__device__ __forceinline__ TrackSpan track_span(const int *__restrict__ ctl, int CH, int cap)
{
    TrackSpan s;
    if (COMPLEX) {
        const int fill = ctl[2], n = ctl[SC_N];
        s.f0 = fill;
        s.f1 = fill + n;
        s.abs0 = ctl[STREAM_CLK_T] - fill;
    } else {
        const int exist = ctl[10];
        s.f0 = ctl[4] * CH;
        s.f1 = ctl[5] * CH < exist ? ctl[5] * CH : exist;
        s.abs0 = ctl[STREAM_CLK_BASE];
    }
    if (s.f0 < 0) s.f0 = 0;  // (never: the words are the stream's own)
    if (s.f1 > cap) s.f1 = cap;
    return s;
}

struct TrackSink {
    int R;  // ring depth
    int32_t *index;
    double *peak;
    int32_t *latest_index;
    double *latest_peak;
};

// a finished row of trial b: frame `abs` into its ring row, the newest frame of the launch also into the latest words
__device__ __forceinline__ void track_ring_store(const TrackSink &o, int b, int abs, bool newest, double best, int bi)
{
    const size_t r = (size_t)b * o.R + (size_t)((unsigned)abs % (unsigned)o.R);  // (abs >= 0: the clock's)
    const int idx = track_row_index(bi);
    const double pk = track_row_peak(best, bi);
    o.index[r] = idx;
    o.peak[r] = pk;
    if (newest) {
        o.latest_index[b] = idx;
        o.latest_peak[b] = pk;
    }
}

// the emit of the stream kernels for the chunk at position cs.  Built where it is called, from the kernel's locals: one object that lives
// across the walk was not split into registers by the compiler (24 to 112 bytes of scratch per lane)
struct TrackEmit {
    const TrackSink &o;
    const TrackSpan &sp;
    int b, cg, ncg, cap, cs;
    double *__restrict__ pval;
    int32_t *__restrict__ pidx;
    __device__ __forceinline__ void operator()(int row, double best, int bi) const
    {
        const int f = cs + row;
        if (ncg == 1) {
            track_ring_store(o, b, sp.abs0 + f, f == sp.f1 - 1, best, bi);
        } else {
            const size_t e = ((size_t)b * cap + f) * ncg + cg;
            pidx[e] = bi;
            pval[e] = best;
        }
    }
};

// the combine of a tile: one thread per position of the window / the staging array; positions outside the tile's range return
__device__ __forceinline__ void track_stream_combine(const TrackSpan &sp, const double *__restrict__ pval, const int32_t *__restrict__ pidx, int cap,
                                                     int ncg, const TrackSink &out)
{
    const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (f < sp.f0 || f >= sp.f1) return;
    const size_t e = ((size_t)b * cap + f) * ncg;
    double best;
    int bi;
    track_combine_row(pval + e, pidx + e, ncg, best, bi);
    track_ring_store(out, b, sp.abs0 + f, f == sp.f1 - 1, best, bi);
}

}  // namespace micloc
