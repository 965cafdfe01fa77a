// Internal declarations of the MUSIC stream (stream_music.hip), shared with its C-ABI entries (api_stream.hip).
#pragma once
#include "micloc_internal.h"

namespace micloc {

// ---- streaming, MUSIC (stream_music.hip) ------------------------------------------------------------------------------------------
struct MusicStreamDims {
    int B, M;         // trials, microphones
    int L, hop;       // slice length and advance (slice s: [s hop, s hop + L))
    int N, Np, F;     // FFT length, frame row stride (N rounded up to 64), frames of a full slice
    int nbin, Cp;     // in-band bins, W / X columns (2 nbin rounded up to 16)
    int G, ksel;      // DoAs, selected bins per slice
    int slots;        // K = ceil(L / hop) + 1 slots per trial, slice s in slot s % K
    int max_slices;   // rows of the caller's result ring, slice s in row s % max_slices
};
// state: [clock: 4 ints per trial][DF2T words: word i of chain q at i nl + q, nl = B K M][sum_s P^2 [B][G]][slot spectra [B][K][G]]
// [frame rows xf [Rp][Np]][DFT rows X [Rp][Cp]], row ((b K + slot) M + m) F + f, Rp = B K M F rounded up to 64
struct MusicStreamLayout {
    size_t clk, z, sum, spec, xf, X, total;
    long long R, Rp;
};
// false: a shape the stream does not serve (k > nbin, hop > L, N > L, nbin > 4096, ...)
bool music_stream_dims(int B, int M, int L, int hop, int N, int nbin, int G, int k, int max_slices, MusicStreamDims *d);
MusicStreamLayout music_stream_layout(const MusicStreamDims &d);
// x [B][n][M]; every output may be NULL
hipError_t launch_music_stream_tile(const MusicStreamDims &d, const IirCoef &co, const double *x, int n, int final_tile, void *state,
                                    const double *W, const double *sre, const double *sim, double *power, int32_t *argmax,
                                    double *latest_spec, int32_t *latest_argmax, double *slice_spec, int32_t *slice_sel, int32_t *slice_argmax,
                                    hipStream_t st);

}  // namespace micloc
