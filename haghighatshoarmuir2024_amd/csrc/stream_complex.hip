// Streaming form of the complex Beamformer's chain (micloc_stream_complex_*): band-pass with state carry, the one-shot time reduction
// cut at the stream's chunk borders, the running and the windowed read-out.  The rule is stated in full in include/micloc_hip.h
// ("streaming, complex Beamformer"); DESIGN 4.16 has the state layout and the footprint.
//
// No spikes, no open clusters, no horizon: a frame is final once its tile has been band-passed.  A tile of n frames is
//   stream_bandpass_tile_kernel<N>      carry -> staging [0, fill); DF2T steps of the tile -> staging [fill, fill + n); zeros up to the
//                                       next chunk border (what the one-shot kernels put behind a ragged last chunk)
//   launch_planar_beamform              (beamform.hip, unchanged) on staging [B][2M][Ks CH] as a recording of Ks whole chunks: the launch
//                                       shape depends on max_tile only; rows past the valid ones are computed and never read
//   stream_complex_accumulate_kernel    the new chunk rows onto {total, open-block sum} in the one-shot order, Re | Im folded
//   stream_window_kernel<1>             (windowed; stream_windows.hip) the streaming read-out's one kernel, instantiated for folded rows
//   stream_complex_slide_kernel         frames behind the last whole chunk -> carry; the one-thread clock commit
// all on one stream, one after the other.
//
// CONTROL WORDS (the first 64 ints of the state).  A launch with more than one workgroup must never read a word that one of its own
// threads writes, so the words come in two sets: the COMMITTED ones {[0] chunks contracted, [2] carry fill, [8] frames contracted,
// [STREAM_CLK_T] frames pushed} are written by the slide kernel's commit only, and the PENDING ones are written by one thread of the
// kernel in front of their readers: the band-pass kernel leaves {[STREAM_CLK_TEND] frames pushed after this tile, [SC_N] the tile's
// length}, the accumulate kernel {[4] = 0, [5] new chunk rows, [6] chunks contracted after this tile -- the words stream_window_kernel
// reads --, [SC_SRC] first staging column behind the rows, [SC_REM] frames that stay, [SC_FRAMES] frames contracted after this tile}.
#include "bandpass_rows.h"
#include "readout_rows.h"

namespace micloc {

namespace {

constexpr int SC_SRC = 21, SC_REM = 22, SC_FRAMES = 23;  // (SC_N, the band-pass kernel's word, is bandpass_rows.h's)

constexpr int SB_CHAINS = 64;  // chains per workgroup: wave 0 runs the recurrences, all four waves move the tiles

// The tile of a single-band stream: stream_bandpass_tile (bandpass_rows.h) with every chain on the uniform coefficients `co`, which
// stay in scalar registers.  CH: frames per chunk of the contraction kernels.
template <int N>
__global__ __launch_bounds__(BR_THREADS) void stream_bandpass_tile_kernel(const IirCoef co, const double *__restrict__ h, int nl, int n,
                                                                          size_t row_stride, double *__restrict__ stg, int S, int CH,
                                                                          const double *__restrict__ carry, double *__restrict__ zst,
                                                                          int *__restrict__ ctl)
{
    stream_bandpass_tile<N, SB_CHAINS>([&](Df2tChain<N> &chn, bool, int) { chn.init(co); }, h, nl, n, row_stride, stg, S, CH, carry, zst, ctl);
}

constexpr int SA_COLS = 256;

// partial [B][Ks][Gp]: rows 0 .. nrows - 1 are the chunks [done, done + nrows) of the stream, columns [0, Ghp) Re and [Ghp, Gp) Im.  The
// additions are power_argmax_kernel's with complex_pairs = 1 (beamform.hip), chunks counted from chunk 0: BlockedSum of readout_rows.h,
// s += Re; s += Im per chunk.  The arg-max is its block_first_max.
__global__ __launch_bounds__(SA_COLS) void stream_complex_accumulate_kernel(const double *__restrict__ partial, int Ks, int Gp, int G, int Ghp,
                                                                             int CH, int final_tile, int *__restrict__ ctl,
                                                                             double *__restrict__ acc, double *__restrict__ power,
                                                                             int32_t *__restrict__ argmax)
{
    __shared__ double sv[SA_COLS];
    __shared__ int si[SA_COLS];
    const int b = blockIdx.x, col = threadIdx.x;
    const int done = ctl[0], fill = ctl[2], frames0 = ctl[8], n = ctl[SC_N];
    const int avail = fill + n;
    const int whole = avail / CH;
    int nrows = final_tile ? (avail + CH - 1) / CH : whole;
    if (nrows > Ks) nrows = Ks;  // (never: Ks covers max_tile + CH - 1 frames)
    const int taken = final_tile ? avail : whole * CH;
    const double frames = (double)(frames0 + taken);
    const double *pb = partial + (size_t)b * Ks * Gp;
    double *tot = acc + (size_t)b * 2 * G, *blk = tot + G;
    double best = -1.0;
    int bi = RO_NONE;
    for (int g = col; g < G; g += SA_COLS) {
        BlockedSum sum{tot[g], blk[g], done % STREAM_BLOCK_CHUNKS};
        for (int ch = 0; ch < nrows; ++ch) sum.add(pb[(size_t)ch * Gp + g], pb[(size_t)ch * Gp + Ghp + g]);
        tot[g] = sum.total;
        blk[g] = sum.s;
        const double p = frames > 0.0 ? sum.close() / frames : 0.0;
        if (power) power[(size_t)b * G + g] = p;
        if (p > best) {  // ascending g per thread: its first maximum; a NaN never wins
            best = p;
            bi = g;
        }
    }
    const int a = block_first_max<SA_COLS>(best, bi, sv, si, col);
    if (col == 0 && argmax) argmax[b] = a;
    if (b == 0 && col == 0) {  // pending words: no thread of this launch reads them
        ctl[4] = 0;
        ctl[5] = nrows;
        ctl[6] = done + nrows;
        ctl[SC_SRC] = whole * CH;
        ctl[SC_REM] = final_tile ? 0 : avail - whole * CH;
        ctl[SC_FRAMES] = frames0 + taken;
    }
}

// One workgroup per (trial, channel) row: the frames behind the last contracted chunk go to the row's carry.  Source (staging, the
// workspace) and destination (carry, the state) are different arrays: they never overlap, so there is no scratch pass.  Thread 0 of
// workgroup 0 commits the clock; the words it writes are read by no thread of this launch.
__global__ __launch_bounds__(256) void stream_complex_slide_kernel(const double *__restrict__ stg, int S, int CH, double *__restrict__ carry,
                                                                    int *__restrict__ ctl)
{
    const int row = blockIdx.x;
    const int src0 = ctl[SC_SRC], rem = ctl[SC_REM];
    if (rem > 0 && rem < CH && src0 >= 0 && (long long)src0 + rem <= S) {
        const double *src = stg + (size_t)row * S + src0;
        double *dst = carry + (size_t)row * CH;
        for (int i = threadIdx.x; i < rem; i += 256) dst[i] = src[i];
    }
    if (row == 0 && threadIdx.x == 0) {
        ctl[0] = ctl[6];
        ctl[2] = rem;
        ctl[8] = ctl[SC_FRAMES];
        ctl[STREAM_CLK_T] = ctl[STREAM_CLK_TEND];
    }
}

}  // namespace

int stream_complex_chunks(int max_tile, int CH) { return (int)(((long long)max_tile + 2 * (long long)CH - 2) / CH); }

StreamComplexLayout stream_complex_layout(int B, int C, int G, int iir_n, int CH)
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    StreamComplexLayout L{};
    size_t off = 256;  // control words
    L.z = off;
    off += al((size_t)(iir_n > 1 ? iir_n - 1 : 1) * B * C * sizeof(double));
    L.carry = off;
    off += al((size_t)B * C * CH * sizeof(double));
    L.acc = off;
    off += al((size_t)B * 2 * G * sizeof(double));
    L.total = off;
    return L;
}

hipError_t launch_stream_complex_bandpass(const IirCoef &co, const double *h, int nl, int n, size_t row_stride, double *staging, int S,
                                          int CH, void *state, const StreamComplexLayout &L, hipStream_t stream)
{
    if (nl < 1 || n < 1 || CH < 1 || S < CH || S % CH != 0 || n > S - (CH - 1)) return hipErrorInvalidValue;
    unsigned char *base = reinterpret_cast<unsigned char *>(state);
    int *ctl = reinterpret_cast<int *>(base);
    double *zst = reinterpret_cast<double *>(base + L.z);
    const double *carry = reinterpret_cast<const double *>(base + L.carry);
    return dispatch_iir_order(co.n, [&](auto N) {
        hipLaunchKernelGGL(stream_bandpass_tile_kernel<decltype(N)::value>, dim3((nl + SB_CHAINS - 1) / SB_CHAINS), dim3(BR_THREADS), 0, stream,
                           co, h, nl, n, row_stride, staging, S, CH, carry, zst, ctl);
        return hipGetLastError();
    });
}

hipError_t launch_stream_complex_accumulate(const double *partial, int B, int Ks, int Gp, int G, int CH, int final_tile, void *state,
                                            const StreamComplexLayout &L, double *power, int32_t *argmax, hipStream_t stream)
{
    unsigned char *base = reinterpret_cast<unsigned char *>(state);
    hipLaunchKernelGGL(stream_complex_accumulate_kernel, dim3(B), dim3(SA_COLS), 0, stream, partial, Ks, Gp, G, Gp / 2, CH, final_tile ? 1 : 0,
                       reinterpret_cast<int *>(base), reinterpret_cast<double *>(base + L.acc), power, argmax);
    return hipGetLastError();
}

hipError_t launch_stream_complex_slide(const double *staging, int nl, int S, int CH, void *state, const StreamComplexLayout &L,
                                       hipStream_t stream)
{
    unsigned char *base = reinterpret_cast<unsigned char *>(state);
    hipLaunchKernelGGL(stream_complex_slide_kernel, dim3(nl), dim3(256), 0, stream, staging, S, CH, reinterpret_cast<double *>(base + L.carry),
                       reinterpret_cast<int *>(base));
    return hipGetLastError();
}

}  // namespace micloc
