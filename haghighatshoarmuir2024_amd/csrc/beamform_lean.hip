// The fixed-shape form of beamform_ws_kernel<3, 2, false, 3, 2> (beamform.hip): 14 channels, three DoA tiles per wave, power only --
// the sweep's launch.  Same algorithm, same operands in the same order (the per-chunk partial sums are the general kernel's to the last
// bit), same launch geometry (grid nchunks x B, 512 threads, 256-frame chunks, xcd_chunk_order, 37.9 KB of LDS, three workgroups per CU).
// What differs is only what the general kernel spends on being general -- vector instructions that are no arithmetic of the result, and
// on a gfx950 SIMD a vector instruction is never hidden behind a v_mfma_f64 (DESIGN.md 4.3 holds the instruction census of both):
//   * NK (k-steps of the LIF product) is a template parameter: the LIF is straight-line code, every LDS read an immediate offset from one
//     base, the first matrix instruction of a chain takes a literal zero C (no accumulator clears, no pointer updates, no loop);
//     -- and at 35 taps, the sweep's neuron kernel, the LIF leaves the matrix cores altogether: a sliding-window FIR on the vector ALU
//     without the product's padding (the kernel's own header, below; 32.9 KB of LDS);
//   * LDS is a static array: the parked fragments and the nir table sit at compile-time addresses;
//   * an interior chunk's (240 + 4 NK) x 14 raster bytes are ONE contiguous range: 8 bytes per lane, one coalesced load per wave, every
//     lane converts its 8 values and writes them as four 16-byte pairs (a pair never straddles a row: 14 is even); the two padding
//     columns of a row are one 16-byte store of zeros.  (The general kernel: one byte per load, 64-bit pointer updates, and the
//     padding lanes of every wave walk all rows in a divergent branch of their own.)  First / last chunks keep the element-wise path;
//   * stage 2's loop over the time tiles is the general kernel's (3 matrix instructions and 12 FMAs per DoA tile, 2 address updates
//     per time tile): the compiler had already given it immediate offsets, a literal zero C and no clamp;
//   * the row sums of the first two DoA tiles share their exchanges (row_sum4_pair's pairing: the additions of row_sum4).
// Everything else -- other channel counts, G > 384, y stored, streaming's device-side chunk range, windows, tracking -- is
// beamform_ws_kernel's.  launch_lif_beamform_lean() says whether a launch is this kernel's; the callers fall through to the general one.
#include "micloc_internal.h"

namespace micloc {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef unsigned uint2_t __attribute__((ext_vector_type(2)));

constexpr int LEAN_THREADS = BF_WAVES * 64;
constexpr int LEAN_NT = 2;                           // 16-frame tiles per wave
constexpr int LEAN_CH = BF_WAVES * LEAN_NT * 16;     // frames per workgroup (256)
constexpr int LEAN_TILES = LEAN_CH / 16;
constexpr int LEAN_C = 14;                           // channels: 3 k-steps on the matrix cores + 2 on the vector ALU
constexpr int LEAN_KM = 3, LEAN_KV = 2;

// beamform.hip's xcd_chunk_order: an XCD walks the chunks of one trial, the LIF halo is an L2 hit
__device__ __forceinline__ void lean_chunk_order(int &chunk, int &b)
{
    const int nchunks = gridDim.x, nb = gridDim.y;
    const int L = chunk + nchunks * b;
    const int full = (nb >> 3) << 3;
    if (L < full * nchunks) {
        const int j = L >> 3;
        const int bq = j / nchunks;
        chunk = j - bq * nchunks;
        b = 8 * bq + (L & 7);
    }
}

// beamform.hip's row_sum4 / row_sum4_pair: (r0 + r1) + (r2 + r3) over the four 16-lane rows, in the VALU
__device__ __forceinline__ double lean_row_sum4(double x)
{
    unsigned lo = __double2loint(x), hi = __double2hiint(x);
    uint2_t a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    uint2_t b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const double s = __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
    lo = __double2loint(s);
    hi = __double2hiint(s);
    a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
}

// rows 0 / 1 of the result hold the row sums of a / of b
__device__ __forceinline__ double lean_row_sum4_pair(double a, double b)
{
    uint2_t lo = __builtin_amdgcn_permlane16_swap(__double2loint(a), __double2loint(b), false, false);
    uint2_t hi = __builtin_amdgcn_permlane16_swap(__double2hiint(a), __double2hiint(b), false, false);
    const double s = __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
    const unsigned sl = __double2loint(s), sh = __double2hiint(s);
    lo = __builtin_amdgcn_permlane32_swap(sl, sl, false, false);
    hi = __builtin_amdgcn_permlane32_swap(sh, sh, false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}

// Stage 2 of ws_stage2_kv<NG, 16, 3, 2, true>: per time tile 3 NG matrix instructions (the first of each chain on a literal zero), the
// two tail channels one at a time as 4 NG FMAs each, 4 NG squares.
template <int NG>
__device__ __forceinline__ void lean_stage2(const double *Vl, const double *__restrict__ Wp, int Gp, int wv, int l, int ntile,
                                            double *__restrict__ pout)
{
    const int lc = l & 15;
    const int q = l >> 4;
    // bf_mat fragments of this wave's DoA tiles, straight from L2, once: wave-uniform row bases + one 32-bit lane offset
    double Wf[NG][LEAN_KM], Wv[NG][LEAN_KV];
    const unsigned of = (unsigned)(q * Gp + lc), ov = (unsigned)lc;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const double *wp = Wp + 16 * (wv + BF_WAVES * j);
#pragma unroll
        for (int k = 0; k < LEAN_KM; ++k) Wf[j][k] = (wp + (size_t)(4 * k) * Gp)[of];
#pragma unroll
        for (int i = 0; i < LEAN_KV; ++i) Wv[j][i] = (wp + (size_t)(4 * LEAN_KM + i) * Gp)[ov];
    }
    double sq[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) sq[j] = 0.0;
    const double *pf = Vl + l;                  // matrix fragments of tile t: pf[256 t + 64 k]
    const double *pt = Vl + 64 * LEAN_KM + q;   // channel 12 + i at the lane's accumulator rows q + 4 r: pt[256 t + 16 i + 4 r]
    auto tile_step = [&](const int tile) {
        double V[LEAN_KM];
#pragma unroll
        for (int k = 0; k < LEAN_KM; ++k) V[k] = pf[256 * tile + 64 * k];
        double4_t acc[NG];
#pragma unroll
        for (int k = 0; k < LEAN_KM; ++k)
#pragma unroll
            for (int j = 0; j < NG; ++j)
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(V[k], Wf[j][k], k == 0 ? double4_t{0.0, 0.0, 0.0, 0.0} : acc[j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < LEAN_KV; ++i) {
            double Vv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) Vv[r] = pt[256 * tile + 16 * i + 4 * r];
#pragma unroll
            for (int j = 0; j < NG; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[j][r] = __builtin_fma(Vv[r], Wv[j][i], acc[j][r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < NG; ++j) sq[j] = __builtin_fma(acc[j][r], acc[j][r], sq[j]);
    };
    // (unrolling the walk -- all 16 tiles, or 4 or 2 per address update -- was built: 1460 / 16 / 16 B of scratch at 80 registers; the
    //  loop keeps 2 address updates per tile and no scratch)
#pragma unroll 1
    for (int t = 0; t < ntile; ++t) tile_step(t);
    if constexpr (NG >= 2) {
        const double s = lean_row_sum4_pair(sq[0], sq[1]);
        if (l < 32) pout[16 * (wv + BF_WAVES * q) + lc] = s;
    } else {
        const double s = lean_row_sum4(sq[0]);
        if (l < 16) pout[16 * wv + l] = s;
    }
    if constexpr (NG == 3) {
        const double s = lean_row_sum4(sq[2]);
        if (l < 16) pout[16 * (wv + BF_WAVES * 2) + l] = s;
    }
}

}  // namespace

// NTAPS == 0: stage 1 on the matrix cores (any tap count of NK k-steps).  NTAPS > 0: stage 1 as a sliding-window FIR of exactly NTAPS taps
// on the vector ALU.  The Toeplitz product pads: 16 rows for 14 channels, 4 NK lags for NTAPS, two triangles of zeros -- 41 % of its matrix
// cycles at 35 taps; the FIR issues only the NTAPS x 14 useful multiply-adds per frame, at the same peak rate.  Lane = (channel, 8 consecutive
// frames of the wave's 32): 56 lanes, 8 independent chains per lane, each chain lag NTAPS - 1 down to 0 -- past samples in chronological
// order, one fma per sample from +0, which is what the matrix core does with the same operands; the lags it also multiplies (zero taps, zero
// rows) leave a +0-started chain as it is.  Same membrane bits, same fragments in LDS, same stage 2.
//   * the spike tile is channel-major, [14][FP] doubles: a lane's 8 + NTAPS - 1 values are contiguous and 16-byte aligned, each is read once
//     (21 ds_read_b128 per lane at 35 taps); FP = 2 (mod 4) doubles keeps the four 16-lane groups of a b128 read on distinct banks
//     (lane = 4 c + block: slot (FP / 2) c + 4 block mod 16);
//   * the window lives in registers: with the loop unrolled its advance by one value per lag is register renaming;
//   * the taps are wave-uniform: scalar loads of the global table (tap k at tab[15 + k], see micloc_plan_set_neuron_kernel), the scalar
//     operand of every fma; no table in LDS.  They are requested where they are used, not at the kernel's start: 70 SGPRs live across
//     staging made 105 in all, one wave per SIMD fewer than the 100 that eight waves allow, and the three-stream step LOST 0.03 ms to
//     it while the launch alone won (96 now; profiles/ws_lean_fir/RECORD.json);
//   * the wave runs its fmas at raised priority: on a SIMD whose other waves issue fp64 matrix instructions a vector instruction between
//     two of them pays the switch, a run of 280 of them must not be dealt out one at a time (step 1.42 -> 1.39 ms);
//   * staging keeps its one 8-byte load and one conversion per element; the stores go to [channel][row], there are no padding columns.
template <int NK, int NGW, int NTAPS>
__global__ __launch_bounds__(LEAN_THREADS, 6) void beamform_ws_kernel_lean(const int8_t *__restrict__ spikes, const double *__restrict__ ntab_g,
                                                                            const double *__restrict__ Wp, int GT, int T,
                                                                            double *__restrict__ partial)
{
    constexpr bool FIR = NTAPS > 0;
    constexpr int R = LEAN_CH + 4 * NK - 16;    // spike rows of a chunk: its frames and the LIF halo in front of them
    constexpr int FP = R + 2;                   // FIR: doubles per channel row of the spike tile
    constexpr int FOFF = 4 * NK - 16 - (NTAPS - 1);  // FIR: the row of frame 0's oldest sample
    constexpr int NTAB = FIR ? 0 : 4 * NK + 16;
    constexpr int NSPK = FIR ? LEAN_C * FP : R * 16;
    constexpr int NB8 = R * LEAN_C / 8;         // 8-byte words of an interior chunk's raster bytes
    static_assert(FIR || R * 16 >= LEAN_TILES * 256, "the parked fragments alias the spike tile");
    static_assert(!FIR || (FOFF >= 0 && FOFF % 2 == 0 && FP % 4 == 2 && (NTAPS + 7) % 2 == 0), "FIR: 16-byte window reads, conflict-free pitch");
    static_assert((R * LEAN_C) % 8 == 0 && 4 * NB8 < 13000, "wide staging: whole 8-byte words, and the division by 7 below");
    // [ union{ spike tile as fp64 [R][16] (FIR: [14][FP]) , V fragments [16 tiles][4][64 lanes] } ][ nir table (matrix form only) ]
    __shared__ __attribute__((aligned(16))) double smem[(NSPK > LEAN_TILES * 256 ? NSPK : LEAN_TILES * 256) + NTAB];
    double *S = smem;
    double *Vl = smem;
    double *ntab = smem + (NSPK > LEAN_TILES * 256 ? NSPK : LEAN_TILES * 256);
    const int Gp = 16 * GT;
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    const int lc = l & 15;
    const int q = l >> 4;
    int chunk = blockIdx.x, b = blockIdx.y;
    lean_chunk_order(chunk, b);
    const int nchunks = gridDim.x;
    const int cs = chunk * LEAN_CH;

    if constexpr (!FIR)
        for (int e = tid; e < NTAB; e += LEAN_THREADS) ntab[e] = ntab_g[e];
    {
        const int8_t *sb = spikes + (size_t)b * T * LEAN_C;
        const int tau0 = cs + 16 - 4 * NK;
        if (tau0 >= 0 && tau0 + R <= T) {
            // interior chunk (workgroup-uniform): rows tau0 .. tau0 + R - 1 are R x 14 contiguous bytes
            const int8_t *src = sb + (size_t)tau0 * LEAN_C;
            for (int i = tid; i < NB8; i += LEAN_THREADS) {
                uint2_t w;
                __builtin_memcpy(&w, src + 8 * i, 8);  // (2-byte aligned)
                const int row0 = (4 * i * 9363) >> 16;   // (8 i) / 14, exact below 13107
                const int col0 = 8 * i - LEAN_C * row0;  // even
                const int k = (LEAN_C - col0) >> 1;      // pairs in front of the row's end
                if constexpr (FIR) {
                    double *d = S + col0 * FP + row0;
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const unsigned h = w[p >> 1] >> (16 * (p & 1));
                        // behind the row's end: channel 0 of the next row (k >= 1: never the first pair)
                        double *dp = (p > 0 && p >= k) ? d + (1 - LEAN_C * FP) : d;
                        dp[(2 * p) * FP] = (double)(int)(int8_t)(h & 0xff);
                        dp[(2 * p + 1) * FP] = (double)(int)(int8_t)((h >> 8) & 0xff);
                    }
                } else {
                    double *d = S + row0 * 16 + col0;
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const unsigned h = w[p >> 1] >> (16 * (p & 1));
                        double2_t v;
                        v[0] = (double)(int)(int8_t)(h & 0xff);
                        v[1] = (double)(int)(int8_t)((h >> 8) & 0xff);
                        // behind the row's end: over the two padding columns, into the next row.  k >= 1, so never the first pair: `p > 0` says so at compile time and spares that pair's compare and select
                        double *dp = (p > 0 && p >= k) ? d + 2 : d;
                        *reinterpret_cast<double2_t *>(dp + 2 * p) = v;
                    }
                }
            }
            if constexpr (!FIR)
                for (int rho = tid; rho < R; rho += LEAN_THREADS) *reinterpret_cast<double2_t *>(S + rho * 16 + LEAN_C) = double2_t{0.0, 0.0};
        } else {
            // first / last chunk of a trial: rows outside [0, T) are zero (element-wise, as in beamform_ws_kernel)
            const int c = tid & 15;
            constexpr int RP = LEAN_THREADS / 16;
            const int rr = tid >> 4;
            if (c >= LEAN_C) {
                if constexpr (!FIR)
                    for (int rho = rr; rho < R; rho += RP) S[rho * 16 + c] = 0.0;
            } else {
                for (int r0 = rr; r0 < R; r0 += RP * 6) {
                    int8_t v[6];
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        int tau = tau0 + r0 + RP * i;
                        tau = tau < 0 ? 0 : (tau >= T ? T - 1 : tau);
                        v[i] = sb[(size_t)tau * LEAN_C + c];
                    }
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        const int rho = r0 + RP * i;
                        const int tau = tau0 + rho;
                        if (rho < R) S[FIR ? c * FP + rho : rho * 16 + c] = (tau >= 0 && tau < T) ? (double)v[i] : 0.0;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- stage 1: membrane fragments of this wave's 2 time tiles; past samples in chronological order ------------------------------
    const int tb0 = cs + wv * LEAN_NT * 16;
    const bool active = tb0 < T;  // wave-uniform
    if constexpr (FIR) {
        constexpr int NW = NTAPS + 7;            // the lane's window: 8 frames and NTAPS - 1 samples in front of them
        const int fc = l >> 2, fb = l & 3;       // channel, block of 8 frames
        const bool mine = active && fc < LEAN_C;
        double facc[8];
        // one unbroken run of fmas, ahead of the other waves' matrix instructions
        if (active) __builtin_amdgcn_s_setprio(3);
        if (mine) {
            double tap[NTAPS];
#pragma unroll
            for (int k = 0; k < NTAPS; ++k) tap[k] = ntab_g[15 + k];
            const double2_t *sp = reinterpret_cast<const double2_t *>(S + fc * FP + wv * LEAN_NT * 16 + 8 * fb + FOFF);
            double wnd[NW];
#pragma unroll
            for (int m = 0; m < NW / 2; ++m) {
                const double2_t v = sp[m];
                wnd[2 * m] = v[0];
                wnd[2 * m + 1] = v[1];
            }
#pragma unroll
            for (int s = 0; s < NTAPS; ++s)      // lag NTAPS - 1 - s: frame i takes the sample s + i of the window
#pragma unroll
                for (int i = 0; i < 8; ++i) facc[i] = __builtin_fma(tap[NTAPS - 1 - s], wnd[s + i], s == 0 ? 0.0 : facc[i]);
        }
        if (active) __builtin_amdgcn_s_setprio(0);
        __syncthreads();  // every wave is done with the spike tile: the V fragments may overwrite it
        if (mine) {
            if (tb0 + LEAN_NT * 16 > T) {  // only the wave that straddles the end of the trial masks
#pragma unroll
                for (int i = 0; i < 8; ++i) facc[i] = (tb0 + 8 * fb + i) < T ? facc[i] : 0.0;
            }
            // frame 8 fb + i of channel fc, where the matrix form's accumulator rows lie: tile [c][t]
            double2_t *vp = reinterpret_cast<double2_t *>(Vl + (wv * LEAN_NT + (fb >> 1)) * 256 + 16 * fc + 8 * (fb & 1));
#pragma unroll
            for (int i = 0; i < 4; ++i) vp[i] = double2_t{facc[2 * i], facc[2 * i + 1]};
        }
    } else {
        double4_t vacc[LEAN_NT];
        if (active) {
            const double *sp = S + (wv * LEAN_NT * 16 + q) * 16 + lc;
            const double *np_ = ntab + (lc - q + 3);  // the tap row of the LAST k-step: non-negative immediate offsets only
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                const double bn = np_[4 * (NK - 1 - ks)];
                double a[LEAN_NT];
#pragma unroll
                for (int tt = 0; tt < LEAN_NT; ++tt) a[tt] = sp[(16 * tt + 4 * ks) * 16];
#pragma unroll
                for (int tt = 0; tt < LEAN_NT; ++tt)
                    vacc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[tt], bn, ks == 0 ? double4_t{0.0, 0.0, 0.0, 0.0} : vacc[tt], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave is done with the spike tile: the V fragments may overwrite it
        if (active) {
            if (tb0 + LEAN_NT * 16 > T) {  // only the wave that straddles the end of the trial masks
#pragma unroll
                for (int tt = 0; tt < LEAN_NT; ++tt) {
                    const bool tvalid = (tb0 + 16 * tt + lc) < T;
#pragma unroll
                    for (int r = 0; r < 4; ++r) vacc[tt][r] = tvalid ? vacc[tt][r] : 0.0;
                }
            }
#pragma unroll
            for (int tt = 0; tt < LEAN_NT; ++tt) {
                double *vp = Vl + (wv * LEAN_NT + tt) * 256 + l;
#pragma unroll
                for (int r = 0; r < 4; ++r) vp[64 * r] = vacc[tt][r];
            }
        }
    }
    __syncthreads();

    // ---- stage 2: this wave's DoA tiles (wv, wv + 8, wv + 16) against every time tile of the chunk -------------------------------
    int ntile = (T - cs + 15) >> 4;  // (>= 1: the chunk exists)
    ntile = ntile > LEAN_TILES ? LEAN_TILES : ntile;
    double *pout = partial + ((size_t)b * nchunks + chunk) * Gp;
    const bool owns_all = wv + BF_WAVES * (NGW - 1) < GT;  // wave-uniform
    if (owns_all)
        lean_stage2<NGW>(Vl, Wp, Gp, wv, l, ntile, pout);
    else
        lean_stage2<NGW - 1>(Vl, Wp, Gp, wv, l, ntile, pout);
}

bool launch_lif_beamform_lean(const BeamformW &W, const NeuronTab &nt, const int8_t *spikes, int B, int T, double *y, double *partial,
                              hipStream_t stream, int *nchunks, hipError_t *err)
{
    if (VARIANT_WS_GENERAL_ONLY) return false;  // a variant build of beamform.hip measures ITS kernel at this shape
    if (y || !partial || W.chunk_range || W.complex_pairs || W.CT != 1 || W.C != LEAN_C) return false;
    if ((W.GT + BF_WAVES - 1) / BF_WAVES != 3) return false;  // three DoA tiles per wave: 257 .. 384 DoAs
    const int nch = (T + LEAN_CH - 1) / LEAN_CH;
    const dim3 grid(nch, B), block(LEAN_THREADS);
    switch (nt.NK) {
        case 13:
            if (nt.n == 35)  // the neuron kernel of the 48 kHz sweeps (BASELINE configs 2 and 3): stage 1 as a vector FIR
                hipLaunchKernelGGL((beamform_ws_kernel_lean<13, 3, 35>), grid, block, 0, stream, spikes, nt.tab, W.Wp, W.GT, T, partial);
            else  // 34 .. 37 taps: stage 1 on the matrix cores
                hipLaunchKernelGGL((beamform_ws_kernel_lean<13, 3, 0>), grid, block, 0, stream, spikes, nt.tab, W.Wp, W.GT, T, partial);
            break;
        default: return false;
    }
    *nchunks = nch;
    *err = hipGetLastError();
    return true;
}

}  // namespace micloc
