// The chunk walk over F bands (the rule: include/micloc_hip.h, "wideband moving-target tracking"), for the one-shot band kernels of
// track.hip and the streaming ones of stream_track_bands.hip: track_ws_walk / track_wsc_walk of track_rows.h with a loop over the bands
// inside a chunk, built from the same pieces.
// The launch shape of track.hip: a workgroup owns 64 DoA columns of one trial and walks it in 64-frame chunks.  Per chunk it loops over the
// bands in ascending order; band f runs the per-chunk step of the single-plan walks with ITS operands -- rows, neuron table, bf_mat --
// in that step's order, so y_f[t][g] has the bits of band f's own chain.  Band 0 stores |y_0| into the tile, every later band adds |y_f| with
// one rounded add: m = ((a_0 + a_1) + a_2) + ...  Behind the last band track_chain_reduce runs on the summed tile, unchanged.  The
// bf_mat fragments of F bands do not fit in registers: they are loaded again per band and chunk (16 KB per band and column group at
// most, which stays in L2) in front of the barrier, so the loads are in flight while the rows are staged.  No workgroup waits for
// another; nothing of size T x G exists.  (TrackBandPut of track_rows.h stores or adds.)
// The range is track_ws_walk's: the frames [f0, f1) of every band's rows, position p is frame abs0 + p -- (0, T, 0) for a whole recording,
// the frames a tile made final for a stream -- and the stride of a trial's rows is an argument of its own (the recording's T / Ts, a raster
// window's capacity, a staging array's length).
#pragma once
#include "track_bands.h"
#include "track_rows.h"

namespace micloc {

// SNN bands: trial b of every band's raster [B][rows][C]; rows outside [0, f1) are zero; the LDS regions are sized for NKmax
template <class Emit>
__device__ __forceinline__ void track_bands_ws_walk(unsigned char *smem, const TrackBandsArgs &a, int F, int NKmax, int b, int C, int rows, int f0,
                                                    int f1, int abs0, int G, int cg, double a_rise, double i_rise, double a_fall, double &state,
                                                    const Emit &emit)
{
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    const int lc = l & 15;
    const int q = l >> 4;
    double *Y = reinterpret_cast<double *>(smem);  // [TRK_CH][TRK_LD]
    double *ntab = Y + TRK_CH * TRK_LD;
    double *S = ntab + 4 * NKmax + 16;

    for (int cs = f0; cs < f1; cs += TRK_CH) {
        for (int f = 0; f < F; ++f) {
            const int NK = a.NK[f];
            if (f > 0) __syncthreads();  // every wave is done with the previous band's table and rows
            double Wf[4][4];
            track_ws_weights(Wf, a.Wp[f], a.GT[f], cg, lc, q);
            track_ws_table(ntab, a.tab[f], NK, tid);
            track_ws_stage(S, static_cast<const int8_t *>(a.src[f]) + (size_t)b * rows * C, C, cs, f1, NK, tid);
            __syncthreads();  // (f == 0 also: the previous chunk's row reduction is done with Y)
            track_ws_tile(S, ntab, NK, cs, f1, wv, lc, q, Wf, TrackBandPut{Y, f == 0});
        }
        __syncthreads();
        const int nrow = f1 - cs < TRK_CH ? f1 - cs : TRK_CH;
        track_chain_reduce(Y, wv, l, tid, cs, abs0 + cs == 0, nrow, G, cg, a_rise, i_rise, a_fall, state, emit);
    }
}

// complex bands: trial b of every band's planar rows [B][C][stride]
template <int KM, int KV, class Emit>
__device__ __forceinline__ void track_bands_wsc_walk(unsigned char *smem, const TrackBandsArgs &a, int F, int b, int C, int stride, int f0, int f1,
                                                     int abs0, int G, int cg, double a_rise, double i_rise, double a_fall, double &state,
                                                     const Emit &emit)
{
    constexpr int KF = KM + (KV > 0 ? 1 : 0);
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    const int lc = l & 15;
    const int q = l >> 4;
    double *Y = reinterpret_cast<double *>(smem);
    double *tail = Y + TRK_CH * TRK_LD + wv * 64;

    for (int cs = f0; cs < f1; cs += TRK_CH) {
        for (int f = 0; f < F; ++f) {
            double V[KF];
            TrackCW<KM, KV> w;
            track_wsc_weights<KM, KV>(w, a.Wp[f], a.GT[f], cg, lc, q);
            if (f > 0) __syncthreads();  // the reads of the previous band's tail fragment are done
            track_wsc_frags<KM, KV>(V, tail, static_cast<const double *>(a.src[f]) + (size_t)b * C * stride, C, stride, cs, f1, wv, l);
            __syncthreads();  // (f == 0 also: the previous chunk's row reduction is done with Y)
            track_wsc_tile<KM, KV>(V, tail, w, wv, lc, q, TrackBandPut{Y, f == 0});
        }
        __syncthreads();
        const int nrow = f1 - cs < TRK_CH ? f1 - cs : TRK_CH;
        track_chain_reduce(Y, wv, l, tid, cs, abs0 + cs == 0, nrow, G, cg, a_rise, i_rise, a_fall, state, emit);
    }
}

}  // namespace micloc
