// Wideband streaming form of the complex Beamformer's chain (micloc_stream_complex_bands_*): the band-pass tile of ALL bands' chains in
// ONE launch.  The rule is stated in include/micloc_hip.h ("wideband streaming, complex Beamformer"); DESIGN 4.18 has the footprint and
// the measurement.
//
// The complex chain has no encoder state and no horizon, so a stream of F bands x B recordings is one complex stream (stream_complex.hip)
// of F * B rows: its state layout, its staging array, its control words and every kernel behind the band-pass are that file's, unchanged.
// What differs is the band-pass tile:
//
// stream_bands_bandpass_tile_kernel<N, CH>: stream_bandpass_tile (bandpass_rows.h), the tile of stream_bandpass_tile_kernel<N>
// (stream_complex.hip), with the two changes of bands_bandpass_kernel<N, CH> (bands_complex.hip) --
//   * chain g of the F * B * 2M chains belongs to band g / (B 2M) and filters with that row of the coefficient table, which travels by
//     value as FilterbankCoef does (the plans' own band-pass coefficients, already divided by a[0]);
//   * CH, the chains per workgroup -- the lanes of wave 0 that run a recurrence --, is a template parameter: the step is latency bound
//     whatever the number of live lanes, so at large F * B more SIMDs carry a recurrence and the movers' share of a tile shrinks.
// Everything else -- the tile pipeline, the DF2T step, carry, state words, chunk padding and the pending control words -- is the shared
// code of bandpass_rows.h.
#include "bandpass_rows.h"

namespace micloc {

namespace {

// nl = F * band_chains chains, band_chains = B * 2M; the other arguments are stream_bandpass_tile's
template <int N, int CH>
__global__ __launch_bounds__(BR_THREADS) void stream_bands_bandpass_tile_kernel(const FilterbankCoef co, const double *__restrict__ h, int nl,
                                                                                 int band_chains, int n, size_t row_stride,
                                                                                 double *__restrict__ stg, int S, int chunk,
                                                                                 const double *__restrict__ carry, double *__restrict__ zst,
                                                                                 int *__restrict__ ctl)
{
    stream_bandpass_tile<N, CH>([&](Df2tChain<N> &chn, bool chain, int g) { chn.init(co, chain ? g / band_chains : 0); }, h, nl, n,
                                row_stride, stg, S, chunk, carry, zst, ctl);
}

}  // namespace

// Ring depth of the bands' windows: how many windows ONE tile can complete, plus the one cut at the end of the recording.  A tile
// contracts at most Ks chunk rows (stream_complex_chunks: its own max_tile frames and a carry of fewer than `chunk`).  With `done` chunks
// contracted before the tile and `ready` = done + r after it, stream_window_kernel has emitted e(c) = c < w ? 0 : (c - w) / h + 1 windows
// (w, h: window and hop in chunks) at c = done and at c = ready: e(ready) - e(done) <= ceil(r / h) <= ceil(Ks / h).  On the final tile the
// windows of micloc_window_count(T) are emitted, of which at most ONE is not complete by chunks: a window that starts at n h frames is cut
// only if T - window < n hop < T - window + hop, an open interval of one hop.  All bands emit the same windows in the same tile, so the
// band sum finds count - emitted <= this depth and never gives a window up.
int stream_bands_ring_depth(int Ks, int hop_chunks) { return (Ks + hop_chunks - 1) / hop_chunks + 1; }

hipError_t launch_stream_bands_bandpass(const FilterbankCoef &co, const double *h, int F, int band_chains, int n, size_t row_stride,
                                        double *staging, int S, int chunk, void *state, const StreamComplexLayout &L, int chains,
                                        hipStream_t stream)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || band_chains < 1 || n < 1 || chunk < 1 || S < chunk || S % chunk != 0 || n > S - (chunk - 1))
        return hipErrorInvalidValue;
    const long long nll = (long long)F * band_chains;
    if (nll > 0x7fffffffll) return hipErrorInvalidValue;
    const int nl = (int)nll;
    if (chains == 0) chains = bands_bandpass_chains(nl);
    unsigned char *base = reinterpret_cast<unsigned char *>(state);
    int *ctl = reinterpret_cast<int *>(base);
    double *zst = reinterpret_cast<double *>(base + L.z);
    const double *carry = reinterpret_cast<const double *>(base + L.carry);
    return dispatch_iir_order(co.n, [&](auto N) {
        return dispatch_bandpass_chains(chains, [&](auto CH) {
            constexpr int ch = decltype(CH)::value;
            hipLaunchKernelGGL((stream_bands_bandpass_tile_kernel<decltype(N)::value, ch>), dim3((nl + ch - 1) / ch), dim3(BR_THREADS), 0, stream,
                               co, h, nl, band_chains, n, row_stride, staging, S, chunk, carry, zst, ctl);
            return hipGetLastError();
        });
    });
}

}  // namespace micloc
