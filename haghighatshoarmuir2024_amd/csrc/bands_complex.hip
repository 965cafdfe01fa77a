// Wideband form of the complex Beamformer's front end (micloc_beamformer_pipeline_bands_f64): the band-pass of the analytic signal for
// ALL bands of a batch in ONE launch.  The rule is stated in include/micloc_hip.h ("wideband localisation, complex Beamformer"); DESIGN
// 4.17 has the footprint and the measurement.
//
// bands_bandpass_kernel<N, CH>: chain g of the F * B * 2M chains is (band f, trial b, channel c) = (g / (B 2M), (g / 2M) % B, g % 2M).
//   * in-phase channels c < M read the filterbank's output xf [F][B][T][M] through the roll's index map, x[(t - L/2) mod T][c] (the
//     map of rzcc.hip's loaders, which the one-shot complex front end reads `x` with); quadrature channels read the planar STHT rows
//     h [F B][2M][Ts] (rows c >= M; the in-phase rows of h are never written and never read);
//   * band f filters with row f of the coefficient table, which travels by value as FilterbankCoef does (the plans' own band-pass
//     coefficients, already divided by a[0]);
//   * the arithmetic is the project's DF2T contract from zero state, Df2tChain<N> (bandpass_rows.h): the same fmas in the same order,
//     every term computed;
//   * output: the planar rows pre [F B][2M][Ts] launch_planar_beamform reads, frames [T, Ts) zero.
// One lane per chain; the frames go through bandpass_rows_tiles (bandpass_rows.h), the one-barrier LDS tile pipeline of the stream's
// band-pass kernels.  The step is latency bound whatever the number of live lanes, so CH -- chains per workgroup, the lanes of wave 0
// that run a recurrence -- is a template parameter: the launcher takes the smallest of {16, 32, 64} that keeps the launch at one resident
// round (bands_bandpass_chains), so that as many SIMDs as possible carry a recurrence and the movers' share of a tile stays small.
#include "bandpass_rows.h"

namespace micloc {

namespace {

// nl = F * band_chains chains, band_chains = B * C, C = 2M; sh = (L / 2) % T, the roll.  All indices into xf, h and pre are size_t.
template <int N, int CH>
__global__ __launch_bounds__(BR_THREADS) void bands_bandpass_kernel(const FilterbankCoef co, const double *__restrict__ xf,
                                                                     const double *__restrict__ h, int nl, int band_chains, int C, int M, int T,
                                                                     int Ts, int sh, double *__restrict__ pre)
{
    constexpr int SHARE = CH * BR_TT / BR_THREADS;  // elements of a tile per thread
    const int tid = threadIdx.x;
    const int g0 = blockIdx.x * CH;
    const int rows = nl - g0 < CH ? nl - g0 : CH;  // chains of this workgroup

    // The row of a thread's r-th element does not depend on the tile, so its source and sink are resolved once, behind the chain's start.
    const double *src[SHARE];
    bool rolled[SHARE], live[SHARE];
    double *dst[SHARE];

    // (Ts <= ntiles * BR_TT: Ts is T rounded up to 8)
    bandpass_rows_tiles<N, CH>(
        rows, T,
        [&](Df2tChain<N> &chn, bool chain) {
            chn.init(co, chain ? (g0 + tid) / band_chains : 0);
#pragma unroll
            for (int r = 0; r < SHARE; ++r) {
                const int row = (tid + r * BR_THREADS) / BR_TT;
                live[r] = row < rows;
                const int g = live[r] ? g0 + row : g0;
                const int trial = g / C, c = g - trial * C;  // trial counts over bands: f * B + b
                rolled[r] = c < M;
                src[r] = rolled[r] ? xf + (size_t)trial * T * M + c : h + (size_t)g * Ts;
                dst[r] = pre + (size_t)g * Ts;
            }
        },
        [&](int k, int r, int, int tl) {
            const int nt = T - k * BR_TT < BR_TT ? T - k * BR_TT : BR_TT;
            const int t = k * BR_TT + tl;
            int tr = t - sh;
            tr = tr < 0 ? tr + T : tr;
            return (live[r] && tl < nt) ? (rolled[r] ? src[r][(size_t)tr * M] : src[r][t]) : 0.0;  // frames past T: the zeros of pre's padding
        },
        [&](int k, int r, int, int tl, const double &y) {
            const int ns = Ts - k * BR_TT < BR_TT ? Ts - k * BR_TT : BR_TT;  // (stores reach the padded end of the row: frames [T, Ts) are zero)
            if (live[r] && tl < ns) dst[r][(size_t)k * BR_TT + tl] = y;
        },
        [](const Df2tChain<N> &, bool) {});
}

}  // namespace

hipError_t launch_bands_bandpass(const FilterbankCoef &co, const double *xf, const double *h, int F, int B, int T, int M, int Ts, int shift,
                                 double *pre, hipStream_t stream)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || B < 1 || T < 1 || M < 1 || Ts < T || Ts > ((T + BR_TT - 1) / BR_TT) * BR_TT || shift < 0)
        return hipErrorInvalidValue;
    const long long nll = (long long)F * B * 2 * M;
    if (nll > 0x7fffffffll) return hipErrorInvalidValue;
    const int nl = (int)nll, C = 2 * M, sh = shift % T;
    return dispatch_iir_order(co.n, [&](auto N) {
        return dispatch_bandpass_chains(bands_bandpass_chains(nl), [&](auto CH) {
            constexpr int ch = decltype(CH)::value;
            hipLaunchKernelGGL((bands_bandpass_kernel<decltype(N)::value, ch>), dim3((nl + ch - 1) / ch), dim3(BR_THREADS), 0, stream, co, xf, h,
                               nl, B * C, C, M, T, Ts, sh, pre);
            return hipGetLastError();
        });
    });
}

}  // namespace micloc
