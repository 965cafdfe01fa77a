// Internal declarations shared by the HIP translation units of libmicloc_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/micloc_hip.h"

namespace micloc {

// ---- measurement variants -------------------------------------------------------------------------------------------
// The shipped library is built with both `false`: what runs never depends on the environment.  tools/dev/make_variant.py builds
// tools/_variants/libmicloc_hip_<name>.so from a copy of this header with ONE of them flipped (A/B runs on one box and
// tests/test_hip_parity.py::test_stht_vector_form_still_exact); results are identical in every variant.
constexpr bool VARIANT_WS_FOUR_KSTEPS = false;    // ws_k4: beamform_ws_kernel multiplies four k-steps whatever the channel count
constexpr bool VARIANT_STHT_VECTOR_FORM = false;  // stht_valu: stride-2 STHT kernels on the vector ALU instead of the matrix cores
constexpr bool VARIANT_STHT_WIDE_TWO_TILES = false;  // stht_wide2: the 480-tap walking STHT (96 kHz) with two time tiles per wave and ONE workgroup per CU (98 KB) instead of one tile / two workgroups
constexpr bool VARIANT_STHT_ONE_TILE = false;     // stht_one_tile: the matrix-core STHT with one time tile per workgroup (round 3's form) instead of the walk
constexpr bool VARIANT_WS_GENERAL_ONLY = false;  // set in EVERY variant of the `beamform` unit (ws_k4, ws_sparse_lif): beamform_lean.hip's fixed-shape kernel declines, so the variant's beamform_ws_kernel serves the sweep's shape too
constexpr bool VARIANT_RZ_TWO_SLOTS = false;  // rz_two_slots: rzcc_sweep.hip's three-slot encoder declines, so the sweep's encoder launch is rzcc.hip's 64-entry ring form (two workgroups per CU)

// ---- XCD-aware workgroup order (speed only, never correctness) -------------------------------------------------------
// Workgroup L of a launch runs on XCD L % 8, and every XCD has its own L2.  Kernels whose NEIGHBOURING work items read the same
// cache lines (stream groups that end in the middle of a trial: a frame row [t][0..M) is shorter than a line; time tiles that
// share a halo) walk the items so that XCD x gets the contiguous range [x n/8, (x + 1) n/8) in ascending order; the n % 8
// items at the end keep their place.  A bijection of [0, n).
__device__ __forceinline__ int xcd_walk(int L, int n)
{
    const int per = n >> 3;
    return L < 8 * per ? (L & 7) * per + (L >> 3) : L;
}

// ---- STHT ---------------------------------------------------------------------------------------
constexpr int STHT_R = 8;                // consecutive output samples per lane (register window; groups of STHT_R delays)
constexpr int STHT_TILE = 64 * STHT_R;   // outputs per wave-task
constexpr int STHT_MAX_MB = 8;           // mics per block (one wave each)

struct SthtTaps {
    // compact tap table on device: taps[j] = ker[klo + j * kstep], zero padded to a multiple of 8/kstep
    const double *taps;
    int ngroups;  // number of groups of (STHT_R / kstep) taps
    int klo;      // delay of the first tap
    int kstep;    // 1 or 2
    int halo;     // Hh: samples staged before the tile; Hh == klo (mod STHT_R), Hh >= largest delay
    int shift;    // L / 2 (np.roll amount)
};

hipError_t launch_stht(const SthtTaps &tp, const double *x, double *h, int B, int T, int M, int Ts,
                       hipStream_t stream, bool write_re = true);
size_t stht_lds_bytes(const SthtTaps &tp, int M);

// ---- band-pass + RZCC ---------------------------------------------------------------------------
struct IirCoef {
    double b[MICLOC_MAX_IIR];
    double a[MICLOC_MAX_IIR];
    int n;
};

// Scratch of the encoder: flagged-unit list, chunk checkpoints, fallback candidate lists (rzcc.hip "Time chunking").
// chunk_frames: 0 = automatic, < 0 = never chunk, > 0 = owned frames per chunk.
size_t rzcc_scratch_bytes(int nlanes, int T, int robust_width, int chunk_frames);
int rzcc_chunks(int nlanes, int T, int robust_width, int chunk_frames);  // chunks per stream the launcher will use
// phases: the serial scan of a chunked launch (RZ_PHASE_SCAN: checkpoints into the scratch; nothing when the launch is not chunked)
// and everything else (RZ_PHASE_ENCODE) may be enqueued by separate calls, scan first, with the same arguments
constexpr int RZ_PHASE_SCAN = 1, RZ_PHASE_ENCODE = 2, RZ_PHASE_ALL = 3;
hipError_t launch_bandpass_rzcc(const IirCoef &coef, const double *h, int nlanes, int C, int T, int Ts,
                                int robust_width, int bipolar, double *pre, int8_t *spikes, void *scratch,
                                hipStream_t stream, const double *xin = nullptr, int M = 0, int shift = 0,
                                int chunk_frames = 0, int phases = RZ_PHASE_ALL);
// rzcc_sweep.hip, the three-workgroups-per-CU form of the sweep's launch (spikes only, one chunk, five filter coefficients): true = this
// launch was its to serve (*err: the status; same spikes, same scratch layout), false = nothing was enqueued and the caller launches
// launch_bandpass_rzcc
bool launch_bandpass_rzcc_sweep(const IirCoef &coef, const double *h, int nlanes, int C, int T, int Ts, int robust_width, int bipolar,
                                int8_t *spikes, void *scratch, hipStream_t stream, const double *xin, int M, int shift, int chunk_frames,
                                int phases, hipError_t *err);
// streaming: one tile per launch, exact state hand-off (rzcc.hip "streaming")
size_t rzcc_stream_state_bytes(int nlanes);
hipError_t launch_stream_encode(const IirCoef &coef, const double *h, int nlanes, int C, int T, int Ts, int robust_width,
                                int bipolar, int8_t *spikes, int Ttot, long long t_base, int first_tile, int final_tile,
                                void *state, hipStream_t stream, int pos_lo = 0, const int *clk = nullptr);
// streaming localisation (rzcc.hip "which frames of the spike raster are final"); ctl: 64 device ints
hipError_t launch_stream_horizon(const void *enc_state, int nlanes, int bipolar, int t_end, int final_, int chunk_frames, int base_chunk,
                                 int nwin, int *ctl, hipStream_t stream, int clocked = 0);
// the device clock of a stream: control words of loc_state (ints).  [0] chunks done, [1] chunks of the open block, [4..7] + [10] chunk
// range / window length of the beamforming launch, [8] frames beamformed, [12..15] status -- and the clock:
constexpr int STREAM_CLK_T = 16;      // frames pushed so far (absolute time of the next tile's first frame)
constexpr int STREAM_CLK_BASE = 17;   // absolute frame of the raster window's row 0
constexpr int STREAM_CLK_SHIFT = 18;  // frames the window slides in front of the current tile
constexpr int STREAM_CLK_TEND = 19;   // t + n of the current tile
hipError_t launch_stream_begin_tile(int *ctl, int8_t *win, int8_t *tmp, int B, size_t row_bytes, int C, int n, int cap, int chunk_frames,
                                    hipStream_t stream);
hipError_t launch_stream_tick(int *ctl, hipStream_t stream);
hipError_t launch_stht_wrap_rows(double *h, const double *wrap, int B, int M, int Ts, int col0, int n, int half, const int *ctl,
                                 hipStream_t stream);
hipError_t launch_stream_commit(int *ctl, int block_chunks, hipStream_t stream);
hipError_t launch_stream_accumulate(const double *partial, int B, int nwin, int Gp, int G, const int *range, const int *ctl,
                                    double *acc, const int *frames_ptr, double *power, int32_t *argmax, hipStream_t stream);
constexpr int STREAM_BLOCK_CHUNKS = 32;  // == PA_BLOCK of the one-shot time reduction (beamform.hip)
hipError_t launch_zero_fill(void *ptr, size_t bytes, hipStream_t stream);
// row-major [B][T][C] <-> planar [B][C][Ts]
hipError_t launch_pack_planar(const double *src, double *dst, int B, int T, int C, int Ts, hipStream_t stream);
hipError_t launch_unpack_planar(const double *src, double *dst, int B, int T, int C, int Ts, hipStream_t stream);

// ---- LIF + beamforming --------------------------------------------------------------------------
constexpr int BF_WAVES = 8;                         // waves per block
constexpr int BF_NT = 4;                            // 16-frame tiles per wave
constexpr int BF_CHUNK = BF_WAVES * BF_NT * 16;     // frames per block (512)

struct BeamformW {
    const double *Wp;  // device, zero padded [Kp][Gp] row-major; Kp = 16 * CT, Gp = 16 * GT
    int CT, GT;
    int C, G;          // logical sizes (G counts real columns: 2 * G_complex for the complex variant)
    int complex_pairs; // 0: real bf_mat; 1: columns [0,G/2) are Re, [Gp/2 ...) see api
    // device {lo, hi, -, trial stride in frames} or nullptr: only the chunks lo <= chunk < hi of every trial are computed (the
    // others leave their row of `partial` untouched), trial b starts at spikes + b * stride * C -- the streaming path beamforms the chunks whose spikes have become final, the range is decided on
    // the device and the launch stays sync-free
    const int *chunk_range = nullptr;
};

struct NeuronTab {
    const double *tab;  // device: zero padded Toeplitz lookup, see beamform.hip
    int n;              // taps
    int NK;             // k-steps of 4 past samples: 4 * NK >= n + 15
};

// partial sums: [B][nchunks][Gp] doubles
size_t beamform_partial_bytes(int B, int T, int Gp);
// *nchunks: number of partial-sum rows per trial the chosen kernel wrote (input of launch_power_argmax)
hipError_t launch_lif_beamform(const BeamformW &W, const NeuronTab &nt, const int8_t *spikes, int B, int T,
                               double *y, double *partial, hipStream_t stream, int *nchunks);
// beamform_lean.hip, the fixed-shape form of the sweep's launch (real bf_mat, 14 channels, three DoA tiles per wave, an instantiated NK,
// power only, no device-side chunk range): true = this launch was its to serve (*err, *nchunks as above, same bits in `partial`),
// false = nothing was enqueued and the caller launches launch_lif_beamform
bool launch_lif_beamform_lean(const BeamformW &W, const NeuronTab &nt, const int8_t *spikes, int B, int T, double *y, double *partial,
                              hipStream_t stream, int *nchunks, hipError_t *err);
// *nchunks: partial-sum rows per trial the chosen kernel wrote
hipError_t launch_planar_beamform(const BeamformW &W, const double *pre, int B, int T, int Ts, double *y,
                                  int y_complex, double *partial, hipStream_t stream, int *nchunks);
hipError_t launch_power_argmax(const double *partial, int B, int T, int nchunks, int Gp, int G, int complex_pairs,
                               int Ghalf_pad, double *power, int32_t *argmax, hipStream_t stream);
int beamform_nchunks(int T);
int beamform_nchunks_ct(int T, int CT);  // chunking of the kernel family that serves CT channel tiles
int lif_beamform_chunk_frames(const BeamformW &W, const NeuronTab &nt);  // frames per chunk of the kernel launch_lif_beamform picks (power only)

// ---- windowed read-out of the partial sums (windows.hip) -----------------------------------------------------------
// windows of the rule in include/micloc_hip.h: 1 if T <= window, else 1 + ceil((T - window) / hop)
long long window_count(int T, int window, int hop);
// partial [B][nchunks][Gp] with chunk_frames frames per row -> power_w [B][nW][G], argmax_w [B][nW] (either may be NULL);
// window and hop must be multiples of chunk_frames (hipErrorInvalidValue otherwise: the API checks first)
hipError_t launch_window_power(const double *partial, int B, int T, int nchunks, int Gp, int G, int complex_pairs, int Ghalf_pad,
                               int chunk_frames, int window, int hop, double *power_w, int32_t *argmax_w, hipStream_t stream);

// ---- the same read-out while the recording arrives (stream_windows.hip) -------------------------------------------------
// win_state: [256 B: int windows emitted][B][K][2][G] doubles, K = stream_window_slots = ceil(window / hop) open windows per trial
int stream_window_slots(int window, int hop);
size_t stream_window_state_bytes(int B, int G, int window, int hop);
// between launch_stream_accumulate and launch_stream_commit of a tile: ctl is the head of loc_state (chunks done, the chunk range of
// this call, the clock); window n goes to row n % max_windows of power_w [B][max_windows][G] / argmax_w [B][max_windows], the newest
// one also to latest_power [B][G] / latest_argmax [B] (each may be NULL).  hop <= window, both multiples of chunk_frames.
// complex_pairs: the rows are folded, columns [0, Ghp) Re and [Ghp, Gp) Im (the complex stream, whose control words are its ctl,
// between its accumulate and its slide); 0: real rows, Ghp is not read.
hipError_t launch_stream_windows(const double *partial, int B, int nwin, int Gp, int G, int complex_pairs, int Ghp, int chunk_frames,
                                 const int *ctl, int final_tile, int window, int hop, int max_windows, void *win_state, double *power_w,
                                 int32_t *argmax_w, double *latest_power, int32_t *latest_argmax, hipStream_t stream);

// ---- streaming, complex Beamformer (stream_complex.hip) -------------------------------------------------------------------------
// state: [256 B: 64 control ints][z: (n - 1) x nl DF2T words, word i of chain g at i nl + g][carry [nl][CH]][acc [B][2][G]], nl = B C
struct StreamComplexLayout {
    size_t z, carry, acc, total;
};
StreamComplexLayout stream_complex_layout(int B, int C, int G, int iir_n, int CH);
int stream_complex_chunks(int max_tile, int CH);  // Ks: chunk rows of the staging array, ceil((max_tile + CH - 1) / CH)
// h: the tile's first column of planar rows (row stride row_stride) -> staging [nl][S] columns [fill, fill + n), S = Ks CH
hipError_t launch_stream_complex_bandpass(const IirCoef &co, const double *h, int nl, int n, size_t row_stride, double *staging, int S,
                                          int CH, void *state, const StreamComplexLayout &L, hipStream_t stream);
// partial [B][Ks][Gp] of launch_planar_beamform on the staging array: the new chunk rows onto the accumulators, running power / argmax
hipError_t launch_stream_complex_accumulate(const double *partial, int B, int Ks, int Gp, int G, int CH, int final_tile, void *state,
                                            const StreamComplexLayout &L, double *power, int32_t *argmax, hipStream_t stream);
// the frames behind the last contracted chunk -> carry, then the clock commit
hipError_t launch_stream_complex_slide(const double *staging, int nl, int S, int CH, void *state, const StreamComplexLayout &L,
                                       hipStream_t stream);

// fp32-MFMA variant of LIF + beamforming + power (up to 64 channels, bf_mat must fit in LDS)
hipError_t launch_lif_beamform_f32(const BeamformW &W, const NeuronTab &nt, const int8_t *spikes, int B, int T,
                                   double *partial, hipStream_t stream, int *nchunks);

// ---- covariance-form power / membrane covariance ------------------------------------------------------------
size_t cov_partial_bytes(int B, int T, int CT);
hipError_t launch_lif_cov(const NeuronTab &nt, const int8_t *spikes, int B, int T, int C, int CT, int t_start,
                          double *partial, hipStream_t stream);
hipError_t launch_cov_power(const double *partial, int B, int T, int CT, int C, int Tn, const double *Wp, int Gp, int G,
                            double *cov_out, double *power, int32_t *argmax, hipStream_t stream);

// Gram matrix of a planar signal [B][C][Ts] over frames t >= t_start (complex covariance of Beamformer.design_from_template)
size_t planar_gram_partial_bytes(int B, int T, int C, int t_start);
hipError_t launch_planar_gram(const double *x, int B, int C, int T, int Ts, int t_start, int normalise, double *gram, double *partial,
                              hipStream_t stream);

// ---- Xylo integer LIF (parity unpinned) ------------------------------------------------------------------
size_t xylo_ws_bytes(int Cin, int N);
hipError_t launch_xylo(const uint8_t *spikes_in, int B, int T, int Cin, const int8_t *W_in_host, int N, int w_rec,
                       const uint8_t *dash_syn_host, const uint8_t *dash_mem_host, const int16_t *thr_host,
                       int max_spikes, uint8_t *spikes_out, int32_t *rate, void *ws, hipStream_t stream);

hipError_t xylo_upload(int Cin, const int8_t *W_in_host, int N, const uint8_t *dash_syn_host, const uint8_t *dash_mem_host,
                       const int16_t *thr_host, void *ws, hipStream_t stream);
hipError_t launch_xylo_resident(const void *spikes_in, int ternary_C, int B, int T, int Cin, int N, int w_rec, int max_spikes,
                                uint8_t *spikes_out, int32_t *rate, void *ws, hipStream_t stream);

// counts-only sweep form (ternary raster, no recurrence): persistent workgroups on a (trial, time chunk) ticket queue
size_t xylo_sweep_scratch_bytes(int B);
hipError_t launch_xylo_sweep(const int8_t *raster, int ternary_C, int B, int T, int Cin, int N, int max_spikes, int32_t *rate, void *ws,
                             void *scratch, int workers_per_cu, hipStream_t stream);

// ---- array-signal synthesis ---------------------------------------------------------------------------------
hipError_t launch_synth(const double *xp, const double *fp, const double *slopes, int T, const double *delays, int B,
                        int M, double inv_step, double *out, hipStream_t stream);
struct SynthArgs {
    const double *time, *sig, *slopes;  // template on the fs grid
    int T, B, K, M;
    const double *delays;               // [B][K][Td][M] or nullptr
    const double *doa;                  // [B][K][Td] (delays == nullptr)
    int moving;                         // Td = moving ? T : 1
    const double *r_vec, *theta_vec;    // [M] geometry (delays == nullptr)
    double speed;
    const double *shift;                // [B] or nullptr
    const double *gain;                 // [B][K][T] or nullptr
    int mode;                           // 0: t - (d - shift), clamped at t0;  1: t + d
    double inv_step;
    double *x;                          // [B][T][M]
};
hipError_t launch_synth_targets(const SynthArgs &a, hipStream_t stream);
hipError_t launch_delay_min(const double *doa, int B, int K, int Td, const double *r_vec, const double *theta_vec, int M,
                            double speed, double *shift, hipStream_t stream);

// ---- counter-based random numbers (Philox-4x32-10) ---------------------------------------------------------------
hipError_t launch_uniform(double *out, size_t n, uint64_t seed, uint32_t substream, const uint32_t *epoch, double lo, double hi,
                          hipStream_t stream);
hipError_t launch_counter_add(uint32_t *counter, uint32_t inc, hipStream_t stream);
size_t awgn_ws_bytes(int B, size_t n);
hipError_t launch_awgn(double *x, int B, size_t n, int M, const double *snr_db, const double *sigma, uint64_t seed, uint32_t substream,
                       const uint32_t *epoch, uint32_t trial0, void *ws, hipStream_t stream);

// fused: x = synth(args) + sigma N(0, 1) without ever storing the noise-free signal (same bits as synth_targets + awgn)
size_t synth_awgn_ws_bytes(int B, size_t n, int K, int M);
hipError_t launch_synth_awgn(const SynthArgs &a, const double *snr_db, uint64_t seed, uint32_t substream, const uint32_t *epoch,
                             uint32_t trial0, void *ws, hipStream_t stream);

// ---- sweep results ---------------------------------------------------------------------------------------------
hipError_t launch_doa_error(const int32_t *argmax, const double *doa_list, int G, const double *doa_true, int B, int groups,
                            double *err, double *mae, hipStream_t stream);

hipError_t launch_design_vec(const double *cov, int n_doa, int C, int bipolar, double rel_prec, double *bf, int G, int g0,
                             hipStream_t stream);
hipError_t launch_pack_events(const int8_t *raster, size_t rows, int C, uint8_t *out, int stride, int pos_off, int neg_off, int mode,
                              hipStream_t stream);
hipError_t launch_rate_from_counts(const int32_t *counts, int B, int G, int F, int T, double fs, double *rate, hipStream_t stream);
hipError_t launch_envelope_track(const void *y, int kind, int B, int T, int G, double a_rise, double i_rise, double a_fall, double *env,
                                 int32_t *index, hipStream_t stream);
hipError_t launch_peak_location(const int32_t *rate, int B, int G, int F, int win, int32_t *index, hipStream_t stream);
hipError_t launch_doa_peaks(const double *power, int B, int G, const double *doa, int kind, int K, double min_sep, double rel, int32_t *index,
                            double *value, hipStream_t stream);

// ---- fused moving-target tracking (track.hip) ---------------------------------------------------------------------
// true: the fused kernels serve this plan (<= 16 channels, the shapes of the bf_mat-stationary beamforming kernels); false: the two-step route
bool track_fused_eligible(const BeamformW &W, const NeuronTab &nt, int is_complex);
int track_col_groups(int G);
size_t track_pairs_bytes(int B, int T, int G);  // (value, index) pairs [B][T][ceil(G / 64)]
hipError_t launch_track_fused(const BeamformW &W, const NeuronTab &nt, int is_complex, const void *src, int B, int T, int Ts, int G,
                              double a_rise, double i_rise, double a_fall, int32_t *index, double *peak, double *env_last, void *pairs,
                              hipStream_t stream);
// the read-out of a stored envelope [B][T][G]: first maximum and its value per row, the last row (peak / env_last may be NULL)
hipError_t launch_track_rows(const double *env, int B, int T, int G, int32_t *index, double *peak, double *env_last, hipStream_t stream);

// ---- wideband: filterbank and band sum (filterbank.hip) ------------------------------------------------------------------------
// coefficients of F bands, already divided by a[0]; they travel by value as a kernel argument (2.3 KB: no device table)
struct FilterbankCoef {
    double b[MICLOC_MAX_BANDS][MICLOC_MAX_IIR];
    double a[MICLOC_MAX_BANDS][MICLOC_MAX_IIR];
    int n;
};
// x [B][T][M] -> xf [F][B][T][M], every band from zero state (DF2T, the arithmetic of launch_bandpass_rzcc's `pre`)
hipError_t launch_filterbank(const FilterbankCoef &co, const double *x, int F, int B, int T, int M, double *xf, hipStream_t stream);
// band_power [F][R][G] -> power [R][G] (ascending band order, from p_0), argmax [R] (first maximum; either may be NULL)
hipError_t launch_band_sum(const double *band_power, int F, long long R, int G, double *power, int32_t *argmax, hipStream_t stream);

// ---- wideband, complex Beamformer: the band-pass of all bands' analytic signals in one launch (bands_complex.hip) ---------------------
// xf [F][B][T][M] (in-phase rows, through the roll by `shift`) and h [F B][2M][Ts] (quadrature rows c >= M) -> pre [F B][2M][Ts]; band f
// filters with row f of `co` (the plans' band-pass coefficients, divided by a[0]); the bits of launch_bandpass_rzcc's `pre` band by band
hipError_t launch_bands_bandpass(const FilterbankCoef &co, const double *xf, const double *h, int F, int B, int T, int M, int Ts, int shift,
                                 double *pre, hipStream_t stream);
// Chains per workgroup the band-pass launchers of the complex bands (batch and stream) take for nl chains.  256 CUs; a workgroup is four
// waves, one per SIMD, and 8.4 KB (16 chains) or 16.9 KB (32) of LDS; every instantiation with <= 32 chains runs at least four waves per
// SIMD (DESIGN 4.17 and 4.18 have the registers), so four workgroups are resident per CU: up to 1024 workgroups run as one round.  Past
// that the 64-chain form (33.8 KB) keeps the number of rounds down.
inline int bands_bandpass_chains(int nl)
{
    constexpr int ROUND = 1024;
    if (nl <= 16 * ROUND) return 16;
    if (nl <= 32 * ROUND) return 32;
    return 64;
}

// ---- wideband streaming: the resumable filterbank (filterbank.hip) and the band sum of a stream (stream_bands.hip) ----------------
// fb_state: [B][n - 1][F][M] doubles (at least 256 B), zero-filled once; one tile x [B][T][M] -> xf [F][B][T][M]
size_t filterbank_stream_state_bytes(int F, int n, int B, int M);
hipError_t launch_filterbank_tile(const FilterbankCoef &co, const double *x, int F, int B, int T, int M, double *xf, double *state,
                                  hipStream_t stream);
// per band: running power [B][G], window ring [B][Kb][G], the device word that counts the band's windows -- by value, no device table
struct StreamBandsArgs {
    const double *power[MICLOC_MAX_BANDS];
    const double *rows[MICLOC_MAX_BANDS];
    const int32_t *count[MICLOC_MAX_BANDS];
};
constexpr size_t STREAM_BANDS_STATE_BYTES = 256;  // int words {emitted, given up, pending emitted, pending given up}
// the running band sum and (windowed) the emission of the wideband windows every band has emitted, then the one-thread commit
hipError_t launch_stream_band_sum(const StreamBandsArgs &args, int F, int B, int G, int windowed, int Kb, int max_windows, void *state,
                                  double *power, int32_t *argmax, double *power_w, int32_t *argmax_w, double *latest_power,
                                  int32_t *latest_argmax, hipStream_t stream);

// ---- wideband streaming, complex Beamformer: the band-pass tile of all bands' chains in one launch (stream_bands_complex.hip) --------
// the complex stream's band-pass tile (launch_stream_complex_bandpass) over F * band_chains chains, band_chains = B 2M, state and staging
// laid out by stream_complex_layout for F * B rows; band f filters with row f of `co`; chains: 0 (bands_bandpass_chains) or 16 / 32 / 64
hipError_t launch_stream_bands_bandpass(const FilterbankCoef &co, const double *h, int F, int band_chains, int n, size_t row_stride,
                                        double *staging, int S, int chunk, void *state, const StreamComplexLayout &L, int chains,
                                        hipStream_t stream);
int stream_bands_ring_depth(int Ks, int hop_chunks);         // windows one tile of Ks chunk rows can complete, plus the one cut at the end

// ---- MUSIC (music.hip) ------------------------------------------------------------------------------------------------
struct MusicDims {
    int B, T, M;     // trials, samples per trial, microphones
    int S, L, hop;   // slices per trial, slice length, slice advance (slice s: [s hop, min(s hop + L, T)))
    int N, Np, Fmax; // FFT length, frame row stride (N rounded up to 64), frames of the longest slice
    int nbin, Cp;    // in-band bins, W / X columns (2 nbin rounded up to 16)
    int G, ksel;     // DoAs, selected bins per slice
};
struct MusicBuffers {
    long long R, Rp;  // frame rows, padded to a multiple of 64
    size_t xf_bytes, X_bytes, sel_bytes, spec_bytes;
};
MusicBuffers music_layout(const MusicDims &d);
hipError_t launch_music(const MusicDims &d, const IirCoef &co, const double *x, const double *W, const double *sre, const double *sim,
                        double *xf, double *X, int32_t *sel, double *spec, double *power, int32_t *argmax, hipStream_t st);

}  // namespace micloc
