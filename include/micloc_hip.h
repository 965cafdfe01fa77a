/*
 * micloc_hip.h -- C-ABI of libmicloc_hip.so, the MI355X (gfx950) implementation of the micloc
 * hot path (STHT -> band-pass -> RZCC spike encoding -> alpha-kernel "LIF" filter -> beamforming ->
 * power / arg-max) of synsense/HaghighatshoarMuir2024.
 *
 * The reference has no FFI: its boundary is the Python class surface in micloc/.  Each entry point
 * below therefore names the reference *method lines* it replaces (paths relative to the reference
 * repository root); INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / HIP types in the signatures (`stream` is a
 *     hipStream_t passed as void*; NULL = the default stream).
 *   - Pointers documented "host" are read synchronously during the call; everything else is a
 *     caller-owned DEVICE buffer on the plan's device.  No allocation happens in the stage calls:
 *     scratch comes from the caller (`ws`, sized by micloc_workspace_bytes).
 *   - All stage calls are asynchronous on `stream`, re-entrant per plan+stream, and safe to capture
 *     in a hipGraph.  Return value: MICLOC_OK (0) or a negative micloc_status.
 *   - A plan's calls launch on the plan's device; the entry points without a plan (synthesis, random
 *     numbers, DoA error, design vectors, peak location, Xylo LIF, stand-alone operators) launch on the
 *     device that OWNS their output / workspace buffer -- in both cases whatever the caller's current
 *     device is (the previous current device is restored before the call returns).
 *   - All arithmetic is IEEE binary64 unless a name says otherwise (float32 before the
 *     encoder flips spikes).
 *   - PRECONDITION: recordings are FINITE (no Inf / NaN samples).  The bit-exactness contract (time chunking,
 *     streaming and the one-shot call give the same spikes) rests on it: the checkpoint scan of a chunked encoder
 *     skips the products with a band-pass numerator coefficient that is exactly zero (fma(0, x, z) == z for finite
 *     x, up to the sign of a zero that no comparison, sum or spike sees), which the one-pass encoder multiplies --
 *     0 * Inf would be NaN there.  The reference's own chain is NaN-poisoned from the first non-finite sample on
 *     (lfilter -> cumsum -> find_peaks), so there is no result to reproduce; signed zeros and subnormals are fine.
 *
 * Device layouts
 *   x        [B][T][M]      row-major: trial b is the reference's `sig_in_vec` (T x num_mic).
 *   planar   [B][C][Ts]     C = 2M channels ordered re_0..re_{M-1}, im_0..im_{M-1}
 *                           (np.hstack([real, imag]), snn_beamformer.py:335); Ts = micloc_padded_T(T).
 *   spikes   [B][T][C]      int8 in {-1,0,+1}: trial b is the reference's spikes_vec (T x 2M).
 *   y        [B][T][G]      trial b is the reference's return value of apply_to_signal (T x num_grid);
 *                           complex variant: [B][T][G][2] (re, im) == numpy complex128.
 *   power    [B][G]         mean_t |y|^2  (target_snn_localization.py:462);  argmax [B] int32.
 */
#ifndef MICLOC_HIP_H
#define MICLOC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MICLOC_ABI_VERSION 1
#define MICLOC_MAX_IIR 9 /* len(b) = len(a) <= 9, i.e. band-pass order <= 4 */

typedef enum {
    MICLOC_OK = 0,
    MICLOC_ERR_INVALID = -1,     /* bad argument (NULL, non-positive size, unsupported length) */
    MICLOC_ERR_SHAPE = -2,       /* channel count / matrix shape mismatch (the reference's ValueError) */
    MICLOC_ERR_WORKSPACE = -3,   /* ws too small or misaligned */
    MICLOC_ERR_NOT_SET = -4,     /* neuron kernel / bf_mat not set on the plan */
    MICLOC_ERR_HIP = -5,         /* a HIP runtime call failed; see micloc_last_hip_error */
    MICLOC_ERR_NO_DEVICE = -6    /* device ordinal out of range, or the device is not a gfx950 (checked in plan_create) */
} micloc_status;

typedef struct micloc_plan micloc_plan;

/* Parameters fixed at construction time of SNNBeamformer / Beamformer (host pointers, copied). */
typedef struct {
    int device;                 /* HIP device ordinal */
    int num_mic;                /* M */
    int stht_len;               /* L = int(fs * kernel_duration)            snn_beamformer.py:50 */
    const double *stht_kernel;  /* host [L] fftshift(imag(hilbert(delta)))  snn_beamformer.py:51-53 */
    int iir_len;                /* n = len(b) = len(a) (zero-padded), 1..MICLOC_MAX_IIR */
    const double *iir_b;        /* host [n]  scipy.signal.butter(...)[0]    snn_beamformer.py:68-72 */
    const double *iir_a;        /* host [n]  a[0] != 0 (normalised inside) */
    int robust_width;           /* find_peaks(distance=...)                 snn_beamformer.py:75-80 */
    int bipolar;                /* 0: +1 spikes only, 1: +1 / -1            spike_encoder.py:131-135 */
} micloc_config;

/* ---- plan life cycle -------------------------------------------------------------------------- */
int micloc_plan_create(const micloc_config *cfg, micloc_plan **out);
void micloc_plan_destroy(micloc_plan *plan);

/* neuron impulse response (host [n]); replaces the kernel built in snn_beamformer.py:342-361 */
int micloc_plan_set_neuron_kernel(micloc_plan *plan, const double *nir, int n);
/* real beamforming matrix (host, row-major [C][G], C must equal 2M); SNNBeamformer bf_mat */
int micloc_plan_set_bf_mat(micloc_plan *plan, const double *W, int C, int G);
/* complex beamforming matrix (host, row-major [M][G] re and im); Beamformer bf_mat, applied as
 * sig @ bf_mat.conj() (beamformer.py:290) */
int micloc_plan_set_bf_mat_c128(micloc_plan *plan, const double *Wre, const double *Wim, int M, int G);

/* Counter that changes whenever a hipGraph captured from this plan's stage calls has become stale: a device table was
 * RE-ALLOCATED (set_neuron_kernel / set_bf_mat with a table larger than any before: the graph holds the raw pointer) or
 * replaced by a table of ANOTHER SHAPE (other channel / DoA count, real vs complex, other neuron-kernel length: the graph
 * holds those dimensions by value).  Re-capture (or refuse to replay) when the value differs from the one read at capture
 * time.  A table of the same shape is overwritten in place after a device synchronisation and leaves the counter -- and
 * captured graphs -- valid. */
int micloc_plan_generation(const micloc_plan *plan);

/* Time chunking of the band-pass / RZCC stage.  The stage is serial in time per (trial, channel) stream; with few, long
 * streams it is cut into chunks of `chunk_frames` owned frames that run side by side, each restarted from the exact
 * state a serial scan stored at its boundary -- results are bit-identical for every setting.  0 (default): automatic
 * (chunks only when the launch would not fill the chip); < 0: never; > 0: this many frames per chunk.  Changes the
 * workspace size: query micloc_workspace_bytes again.  micloc_plan_encoder_chunks reports the chunks per stream a
 * (B, T) launch will use. */
int micloc_plan_set_encoder_chunk(micloc_plan *plan, int chunk_frames);
int micloc_plan_encoder_chunks(const micloc_plan *plan, int B, int T);

/* A HIP stream whose kernels run only on compute units [cu_lo, cu_hi) of EVERY XCD of `device` (MI355X: 8 XCDs of 32 compute
 * units; hipExtStreamCreateWithCUMask with the mask layout of gfx950).  For callers that keep several batches in flight: the serial
 * scan of a chunked encoder (MICLOC_STAGE_ENCODE_SCAN below) is a latency chain of few workgroups that runs at a fraction of its
 * pace when its SIMD also issues another kernel's matrix instructions; on a stream of its own with e.g. [0, 4), beside work streams
 * restricted to [4, 32), consecutive batches' scans run one after the other at full pace while the other stages overlap them
 * (runtime.StreamPipeline(scan_lane=...)).  Scheduling only: results never depend on where a kernel runs.  The reference has no
 * counterpart (one NumPy process per trial, target_snn_localization.py:447-467). */
int micloc_stream_create_cu_range(int device, int cu_lo, int cu_hi, void **stream);
int micloc_stream_destroy(void *stream);

/* padded time stride of planar buffers (multiple of 8 samples) */
int micloc_padded_T(int T);
/* bytes of scratch needed by any stage / pipeline call with this (B, T) */
size_t micloc_workspace_bytes(const micloc_plan *plan, int B, int T);

/* ---- stages (device pointers) ----------------------------------------------------------------- */
/* STHT: roll by L/2 + 1j * FIR.  Replaces snn_beamformer.py:325-327 / :158-160,
 * beamformer.py:281-283, xylo_snn_localization.py:329-331.   x [B][T][M] -> h planar [B][2M][Ts].
 * The FIR is the chain acc = fma(ker[k], x[t - k], acc) over the non-zero taps in ascending k, from +0.  When every second tap
 * is zero (every even-length Hilbert kernel) it runs as a Toeplitz product on the fp64 matrix cores -- the same chain, the same
 * bits -- otherwise (or with MICLOC_STHT_VALU=1 in the environment, for A/B timing) on the vector ALU. */
int micloc_stht_f64(const micloc_plan *plan, const double *x, int B, int T, double *h, int Ts, void *stream);

/* Band-pass (DF2T, lfilter(b,a,.)) + RZCC encoder.  Replaces snn_beamformer.py:330-338 and
 * spike_encoder.py:115-137.  h planar in; `pre` (planar, post-filter signal) and `spikes` may each be
 * NULL.  spikes must not alias anything; it is fully overwritten. */
int micloc_bandpass_rzcc_f64(const micloc_plan *plan, const double *h, int B, int T, int Ts, double *pre,
                             int8_t *spikes, void *ws, size_t ws_bytes, void *stream);

/* alpha-kernel FIR ("LIF") + real beamforming + power/argmax.  Replaces snn_beamformer.py:364-368 and
 * target_snn_localization.py:462-464.  y, power, argmax may each be NULL. */
int micloc_lif_beamform_f64(const micloc_plan *plan, const int8_t *spikes, int B, int T, double *y,
                            double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);

/* complex beamforming of the band-passed analytic signal: pre (planar) @ conj(W).
 * Replaces beamformer.py:290.  y is [B][T][G][2]. */
int micloc_beamform_c128_f64(const micloc_plan *plan, const double *pre, int B, int T, int Ts, double *y,
                             double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);

/* ---- fused pipelines -------------------------------------------------------------------------- */
/* SNNBeamformer.apply_to_signal (snn_beamformer.py:283-370) + power/argmax for B trials.
 * spikes / y / power / argmax may each be NULL (at least one must be given). */
int micloc_snn_pipeline_f64(const micloc_plan *plan, const double *x, int B, int T, int8_t *spikes, double *y,
                            double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);
/* The same pipeline, launched in parts: `stages` selects which of its three kernel groups this call enqueues.  The
 * intermediate results live in the workspace (and in `spikes` when given), so the parts of one batch must use the same
 * workspace, in order; a caller may enqueue them on different streams with its own event dependencies -- e.g. the STHT
 * of batch i+1 next to the latency-bound band-pass/RZCC of batch i. */
#define MICLOC_STAGE_STHT 1     /* snn_beamformer.py:325-327 (quadrature FIR)                    */
#define MICLOC_STAGE_ENCODE 2   /* snn_beamformer.py:330-338 (band-pass, re/im stack, RZCC)      */
#define MICLOC_STAGE_BEAMFORM 4 /* snn_beamformer.py:342-368 (LIF, beamforming) + power/arg-max  */
#define MICLOC_STAGE_ALL 7
/* MICLOC_STAGE_ENCODE in two parts.  Long recordings are encoded in time chunks that restart from checkpoints a serial scan of
 * every stream stores first (micloc_plan_set_encoder_chunk): few workgroups, one dependent chain each -- latency, not throughput,
 * and a chain that shares its SIMD with another kernel's waves runs at a fraction of its pace.  A caller with several batches in
 * flight can give the scans a stream (and compute units) of their own: _SCAN enqueues only the scan (nothing when the launch is not
 * chunked), _REST everything else of the stage; same workspace, scan first.  MICLOC_STAGE_ENCODE == both. */
#define MICLOC_STAGE_ENCODE_SCAN 8
#define MICLOC_STAGE_ENCODE_REST 16
int micloc_snn_pipeline_stages_f64(const micloc_plan *plan, const double *x, int B, int T, int8_t *spikes, double *y,
                                   double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream, int stages);
/* Beamformer.apply_to_signal (beamformer.py:260-292) + power/argmax for B trials. */
int micloc_beamformer_pipeline_f64(const micloc_plan *plan, const double *x, int B, int T, double *y,
                                   double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);

/* ---- stand-alone operators (no plan) ---------------------------------------------------------- */
/* ZeroCrossingSpikeEncoder.evolve (spike_encoder.py:115-137) on row-major sig [B][T][C]. */
size_t micloc_rzcc_workspace_bytes(int B, int T, int C);
int micloc_rzcc_encode_f64(const double *sig, int B, int T, int C, int robust_width, int bipolar, int8_t *spikes,
                           void *ws, size_t ws_bytes, void *stream);
/* the same with an explicit time-chunking choice (see micloc_plan_set_encoder_chunk) */
size_t micloc_rzcc_workspace_bytes_ex(int B, int T, int C, int robust_width, int chunk_frames);
int micloc_rzcc_encode_ex_f64(const double *sig, int B, int T, int C, int robust_width, int bipolar, int chunk_frames,
                              int8_t *spikes, void *ws, size_t ws_bytes, void *stream);
/* scipy.signal.lfilter(b, a, x, axis=0) on row-major x [B][T][C] (Filterbank.evolve,
 * filterbank.py:25-46); b, a are host [n], zero-padded to the same length n <= MICLOC_MAX_IIR. */
size_t micloc_lfilter_workspace_bytes(int B, int T, int C);
int micloc_lfilter_f64(const double *b, const double *a, int n, const double *x, int B, int T, int C, double *y,
                       void *ws, size_t ws_bytes, void *stream);

/* ---- fp32-MFMA variant of the beamforming tail ------------------------------------------------------ */
/* Same contract as micloc_lif_beamform_f64 (power / arg-max only, real bf_mat, up to 64 channels) with the LIF filter
 * and the contraction on v_mfma_f32_16x16x4_f32: the spikes are exact in fp32, the power agrees with the fp64 path to
 * ~1e-6 relative (BASELINE's north star allows 1e-5 float32 for this stage).  A VARIANT, reported separately. */
int micloc_lif_beamform_f32(const micloc_plan *plan, const int8_t *spikes, int B, int T, double *power, int32_t *argmax,
                            void *ws, size_t ws_bytes, void *stream);

/* ---- covariance form ------------------------------------------------------------------ */
/* cov[b] = V^T V / (T - t_start) over frames t >= t_start of the membrane signal V = lfilter(nir,[1],spikes)
 * (the matrix design_from_template needs, snn_beamformer.py:176-191, with t_start = T // 4), and
 * power[b][g] = w_g^T (V^T V / T') w_g  ==  mean_t (V @ bf_mat)^2  without forming T x G.  An algebraically
 * identical VARIANT of micloc_lif_beamform_f64's power (2 C^2 instead of 2 C G flops per frame); it agrees to
 * ~1e-15 relative but is reported separately.  cov [B][C][C], power [B][G], argmax [B] may each be NULL.
 * Supports C <= 128 channels (lif_cov_kernel up to 64, lif_cov_wide_kernel beyond). */
int micloc_lif_covariance_f64(const micloc_plan *plan, const int8_t *spikes, int B, int T, int t_start, double *cov,
                              double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);
/* Gram matrix of a planar signal: gram[b] = sum_{t >= t_start} x[b][:, t] x[b][:, t]^T (divided by T - t_start when `normalise`),
 * x planar [B][C][Ts] (C <= 128), gram [B][C][C].  Beamformer.design_from_template (beamformer.py:142-150) takes the complex
 * covariance conj(h)^T h / T' of the STHT output over the stable part of each delayed template; with the planar rows
 * [re_0..re_{M-1}, im_0..im_{M-1}] it is the fold (R_rr + R_ii) + j (R_ri - R_ir) of this real 2M x 2M matrix.  fp64 MFMA,
 * deterministic (fixed-order chunk sums).  ws from micloc_planar_gram_workspace_bytes. */
size_t micloc_planar_gram_workspace_bytes(int B, int T, int C, int t_start);
int micloc_planar_gram_f64(const double *planar, int B, int C, int T, int Ts, int t_start, int normalise, double *gram, void *ws,
                           size_t ws_bytes, void *stream);
/* whole chain (STHT, band-pass, RZCC, LIF) with the covariance-form tail */
int micloc_snn_pipeline_cov_f64(const micloc_plan *plan, const double *x, int B, int T, int t_start, int8_t *spikes,
                                double *cov, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);

/* ---- streaming: a recording delivered tile by tile, localised while it arrives ----------------------------------- */
/* apply_to_signal (micloc/snn_beamformer.py:283-370) treats a recording as ONE stream; the reference's live loop restarts the chain
 * on every 0.25 s frame instead (micloc/localization_demo_snn.py:125-193).  Here the recording is one stream that arrives in tiles:
 *   - the band-pass / RZCC stage is a resumable machine: a tile of T_tile frames per call, the complete state of every stream (DF2T
 *     registers, running sum, detector state, the candidate ring with its open clusters and selection cursors) kept in `enc_state`
 *     (micloc_stream_state_bytes, 256-B aligned), so that the tiles together perform exactly the operations of one call on the whole
 *     recording: the spikes are bit-identical for any tiling (spike_encoder.py:115-137); tile lengths are multiples of 16 except the
 *     last, final_tile closes the clusters still open.  A stream whose candidate ring overflows (> 63 pending candidates: out-of-band
 *     input) cannot be redone from its start; micloc_stream_overflow returns how many were lost (synchronises) -- a non-zero count
 *     is an error;
 *   - the spikes go into a sliding WINDOW of the int8 raster ([B][window_frames][2M] over the absolute frames [base, base +
 *     window_frames), multiples of micloc_stream_chunk_frames), and after every tile the DEVICE decides which frames can no longer
 *     receive a spike (the earliest position an open cluster or an incomplete candidate of any stream can still emit), runs LIF +
 *     beamforming on the chunks that became final and adds their sums of y^2 to an accumulator in `loc_state` in the order of the
 *     one-shot time reduction: power / argmax (may be NULL) are the running estimate over the frames beamformed so far and, after
 *     the last tile, the one-shot result bit for bit;
 *   - the CLOCK of the stream (frames pushed, base of the window) lives in the control words of `loc_state`, on the device: no call
 *     takes an absolute time, every launch of a tile of n frames has the same arguments, so a tile is ONE capturable hipGraph.
 * One tile of n frames =
 *   micloc_stream_begin_tile        clock: t_end = t + n; the window slides forward by whole chunks when it must (through
 *                                   scratch_window; a slide past rows the next chunk still needs is counted as a lag failure)
 *   micloc_stht_f64                 on [history | tile] (the last L - 1 frames of the previous tile in front), by the caller
 *   micloc_stream_wrap_rows_f64     np.roll's wrap-around rows of the in-phase channels while t < L/2 (wrap_tail [B][L/2][M] or NULL:
 *                                   zeros -- a live source cannot know them; the tile's frame i sits at column first_col + i of
 *                                   h [B][2M][Ts])
 *   micloc_stream_encode_tile_f64   h = the tile's first column (row stride row_stride), spikes into the window
 *   micloc_stream_localize_tile_f64 horizon, LIF + beamforming of the final chunks, accumulation; ends with the clock's tick
 * micloc_stream_reset zero-fills the clock, both states and the window (once, before the first tile).  The last tile of a recording
 * is issued with final_tile = 1 (both calls).  micloc_stream_localize_status: {chunks beamformed, frames beamformed, lag failures,
 * open block fill}; synchronises the stream.  ws: micloc_stream_localize_workspace_bytes(B, window_frames). */
size_t micloc_lif_beamform_workspace_bytes(const micloc_plan *plan, int B, int T); /* ws of micloc_lif_beamform_f64 / micloc_beamform_c128_f64 alone (bf_mat set) */
size_t micloc_stream_state_bytes(const micloc_plan *plan, int B);
size_t micloc_stream_localize_state_bytes(const micloc_plan *plan, int B);
size_t micloc_stream_localize_workspace_bytes(const micloc_plan *plan, int B, int window_frames);
int micloc_stream_chunk_frames(const micloc_plan *plan);
int micloc_stream_reset(const micloc_plan *plan, int B, void *enc_state, size_t enc_bytes, void *loc_state, size_t loc_bytes, int8_t *window,
                        int window_frames, void *stream);
int micloc_stream_begin_tile(const micloc_plan *plan, void *loc_state, int8_t *window, int8_t *scratch_window, int B, int n, int window_frames,
                             void *stream);
int micloc_stream_wrap_rows_f64(const micloc_plan *plan, const void *loc_state, double *h, int B, int Ts, int first_col, int n,
                                const double *wrap_tail, void *stream);
int micloc_stream_encode_tile_f64(const micloc_plan *plan, const double *h, int B, int T_tile, int row_stride, int final_tile, int8_t *window,
                                  int window_frames, void *enc_state, size_t enc_bytes, const void *loc_state, void *stream);
int micloc_stream_localize_tile_f64(const micloc_plan *plan, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window, int B,
                                    int window_frames, int final_tile, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);
int micloc_stream_overflow(const void *state, int *count, void *stream);
int micloc_stream_localize_status(const void *loc_state, int *status4, void *stream);

/* ---- streaming windows: a DoA per time window while the recording arrives ------------------------------------------ */
/* The running power above is the mean over every frame since the stream began: right for a stationary source, all but frozen
 * for one that moves after a minute of audio.  micloc_stream_localize_tile_windows_f64 is micloc_stream_localize_tile_f64 plus
 * the time-resolved read-out ("time-resolved DoA" below) of the same per-chunk rows of sum y^2, emitted window by window as
 * soon as a window's last chunk is final, with the bits of the one-shot call and no T-sized buffer.  The rule:
 *   Window bounds.
 *   - The window rule of the time-resolved read-out holds unchanged, with the extra condition 1 <= hop <= window.
 *   - window and hop are multiples of CH = micloc_stream_chunk_frames(plan), the plan's window quantum (256 frames up to 64
 *     channels, 512 beyond).
 *   - Window n covers the frames [n hop, min(n hop + window, T)).
 *   When a window is emitted.
 *   - Before the final tile: window n is emitted by the first call after which chunk n hop / CH + window / CH - 1 has been
 *     beamformed, in ascending n.  With F frames beamformed that is F < window ? 0 : (F - window) / hop + 1 windows.
 *   - On the final tile (final_tile = 1): every window of micloc_window_count(T, window, hop, CH) not emitted yet is emitted,
 *     with T taken from the device clock; its frame count is min(window, T - n hop).
 *   - Windows that start before T but are not in that count are not emitted: window = 1024, hop = 256, T = 1100 has 2
 *     windows, not 5.
 *   Values.
 *   - The value of window n is bit for bit what micloc_snn_pipeline_windows_f64 returns for the whole recording.  The order of
 *     the additions is that read-out's: total = 0; the chunk rows are added in ascending order inside blocks of 32 chunks
 *     counted from the window's first chunk; each block sum is added onto the total in ascending order; the result is divided
 *     by the window's frame count.  The arg-max is the first maximum; a NaN never wins.
 *   - A row that has been emitted never changes afterwards (until window n + max_windows takes its place in the ring).
 * State: win_state (micloc_stream_window_state_bytes, 256-B aligned; zero-filled once by micloc_stream_window_reset) holds the
 * count of windows emitted and, per trial, the K = ceil(window / hop) windows that can be open at a time, window n in slot n % K,
 * each as {total, open-block sum} rows of G doubles: 256 + B K 2 G 8 bytes, whatever the length of the stream.
 * Outputs (device): window n goes to row n % max_windows of window_power [B][max_windows][G] (may be NULL) and window_argmax
 * [B][max_windows] int32; latest_power [B][G] / latest_argmax [B] (may be NULL) take the most recently emitted window and are
 * untouched until the first one exists.  power / argmax / loc_state end with exactly the bits of micloc_stream_localize_tile_f64:
 * the launches are horizon -> LIF + beamforming -> accumulate -> window read-out -> commit -> tick, the read-out being one
 * workgroup per trial whose grid depends on B only -- no atomics, no host synchronisation, no argument that depends on time, so a
 * tile is still ONE capturable hipGraph.  micloc_stream_window_count: windows emitted so far; synchronises the stream.
 * Status, before any launch: MICLOC_ERR_INVALID for NULL or non-positive arguments; MICLOC_ERR_NOT_SET without neuron kernel or
 * bf_mat; MICLOC_ERR_SHAPE for a window or hop that is not a multiple of CH, hop > window, or a complex bf_mat;
 * MICLOC_ERR_WORKSPACE for a short or misaligned loc_state, ws or win_state. */
size_t micloc_stream_window_state_bytes(const micloc_plan *plan, int B, int window, int hop, int max_windows); /* 0 on bad arguments */
int micloc_stream_window_reset(const micloc_plan *plan, int B, void *win_state, size_t win_bytes, int window, int hop, int max_windows,
                               void *stream);
int micloc_stream_localize_tile_windows_f64(const micloc_plan *plan, const void *enc_state, void *loc_state, size_t loc_bytes,
                                            const int8_t *window_raster, int B, int window_frames, int final_tile, double *power,
                                            int32_t *argmax, void *ws, size_t ws_bytes, void *win_state, size_t win_bytes, int window,
                                            int hop, int max_windows, double *window_power, int32_t *window_argmax, double *latest_power,
                                            int32_t *latest_argmax, void *stream);
int micloc_stream_window_count(const void *win_state, int *count, void *stream);
/* device address of the int32 word micloc_stream_window_count reads (a kernel that follows a band's windows takes it: "wideband
 * streaming" below); valid as long as win_state is */
const int32_t *micloc_stream_window_count_ptr(const void *win_state);

/* ---- streaming, complex Beamformer: tiles in, the one-shot bits out ------------------------------------------------- */
/* The non-spiking complex Beamformer (micloc/beamformer.py; deployed live, restarting on every 0.25 s pack, by
 * micloc/localization_demo.py) as ONE stream that arrives in tiles.  The entries above ("streaming", "streaming windows") keep
 * returning MICLOC_ERR_SHAPE for a complex bf_mat; these are the complex chain's own.  The rule, for a plan with a complex bf_mat,
 * any recording x [B][T][M] and any cut of T into tiles of n_1, n_2, ... frames (each n_i >= 1, no multiple of anything):
 *   Results.
 *   - After the final tile (final_tile = 1) power [B][G] and argmax [B] equal micloc_beamformer_pipeline_f64 on the whole recording
 *     bit for bit.
 *   - Before it they are the mean over the frames contracted so far: whole chunks of CH = micloc_window_quantum(plan) frames (256
 *     up to 64 channels, 512 beyond).  power is 0 and argmax is 0 while no chunk is complete.  (Mid-stream values are those of the
 *     one-shot call on the prefix only up to the prefix's own np.roll rows: see wrap_tail.)
 *   - With window / hop (multiples of CH, 1 <= hop <= window) window n is emitted as soon as its last chunk has been contracted, in
 *     ascending n; on the final tile every remaining window of micloc_window_count(T, window, hop, CH) is emitted, with T taken
 *     from the device clock.  Each window has the bits of micloc_beamformer_pipeline_windows_f64 on the whole recording.  Bounds,
 *     emission times, ring row n % max_windows, latest_* and "an emitted row never changes" are those of "streaming windows" above,
 *     word for word; win_state has that section's layout and micloc_stream_window_count reads its count.
 *   - Nothing allocates, synchronises with the host, uses atomics or takes an absolute time: the clock (frames pushed, chunks
 *     contracted, carry fill) lives in device control words, every launch of a tile of n frames has the same arguments, and the
 *     launches of a tile form ONE chain on the caller's stream with no parallel branches -- a tile is one capturable hipGraph.
 *   How the bits follow.
 *   - STHT: micloc_stht_f64 on [last L - 1 frames | tile] by the caller, then micloc_stream_wrap_rows_f64 with `state` as its
 *     loc_state (it reads the frames-pushed word only, which sits at the same place): in-phase[t] = wrap_tail[t] for t < L/2, the rows
 *     np.roll wraps around -- np.roll(x, L/2, axis = time)[: L/2], i.e. the last L/2 frames of a recording of at least L/2 frames.
 *   - Band-pass: the DF2T steps of the one-shot launch in the same order on the planar rows, the n_coef - 1 state
 *     words of every (trial, channel) chain loaded before the tile and stored after it; the ragged end of a tile is stepped frame by
 *     frame, so a carried state never advances over padding.  Against the one-shot rows only the sign of a zero may differ.
 *   - Contraction: the one-shot time reduction is per chunk of CH frames, the chunk rows added in ascending order inside blocks of
 *     32 chunks and the blocks in ascending order onto the total, each chunk as s += Re; s += Im.  Tile borders fall anywhere, so
 *     the band-passed frames behind the last whole chunk (fewer than CH) wait in a per-trial CARRY.  The band-pass writes carry and
 *     tile into a chunk-aligned staging array [B][2M][Ks CH], Ks = ceil((max_tile + CH - 1) / CH), and zeros up to the next chunk
 *     border; the one-shot contraction kernel runs on it unchanged as a recording of Ks whole chunks (its launch shape depends on
 *     max_tile only; rows past the valid ones are computed and never read); the accumulate kernel adds the new whole chunk rows in
 *     the order above; the slide kernel moves the frames behind them to the carry and commits the clock.  On the final tile the
 *     ragged last chunk is contracted too: the one-shot kernels feed zeros for the frames past T - 1 of a ragged chunk and skip
 *     nothing that would change a sum, so the zero-padded chunk row has the bits of the one-shot call's last row.
 *   State and footprint.  state (micloc_stream_complex_state_bytes, 256-B aligned, zero-filled once by micloc_stream_complex_reset):
 *     256 B of control words | (n_coef - 1) x B 2M DF2T words, word i of chain g = b 2M + c at i B 2M + g (the lanes of a wave touch
 *     consecutive doubles per word) | carry [B][2M][CH] | accumulators [B][2][G] {total, open-block sum}, each part rounded up to
 *     256 B.  Per trial: 2M (n_coef - 1 + CH) + 2G doubles -- 36 KB at M = 7, CH = 256, G = 449, n_coef = 5; 57 KB of carry at CH = 512.
 *     ws (micloc_stream_complex_workspace_bytes; pure scratch, nothing in it survives a tile): the staging array and the chunk rows
 *     partial [B][Ks][Gp].  The state does not grow with the stream.
 *   One tile of n <= max_tile frames =
 *     micloc_stht_f64, micloc_stream_wrap_rows_f64              by the caller, as above; the tile's frame i at column first_col + i
 *     micloc_stream_complex_bandpass_tile_f64                   h [B][2M][row_stride] -> staging
 *     micloc_stream_complex_localize_tile[_windows]_f64         contraction, accumulation, (windows,) slide and clock commit
 *   with the same max_tile, state and ws in both calls.  power / argmax may be NULL.  micloc_stream_complex_status: {chunks contracted,
 *   frames contracted, carry fill, frames pushed}; it synchronises the stream.  A stream is at most 2^31 - 1 frames.
 *   Status, before any launch: MICLOC_ERR_INVALID for NULL or non-positive arguments; MICLOC_ERR_NOT_SET without a bf_mat;
 *   MICLOC_ERR_SHAPE for a real bf_mat, a window or hop that is not a multiple of CH, hop > window, n > max_tile or
 *   first_col + n > row_stride; MICLOC_ERR_WORKSPACE for a short or misaligned state, ws or win_state.  The size functions return 0
 *   for such arguments. */
size_t micloc_stream_complex_state_bytes(const micloc_plan *plan, int B);
size_t micloc_stream_complex_workspace_bytes(const micloc_plan *plan, int B, int max_tile);
int micloc_stream_complex_reset(const micloc_plan *plan, int B, void *state, size_t state_bytes, void *stream);
int micloc_stream_complex_bandpass_tile_f64(const micloc_plan *plan, const double *h, int B, int n, int row_stride, int first_col,
                                            int max_tile, void *state, size_t state_bytes, void *ws, size_t ws_bytes, void *stream);
int micloc_stream_complex_localize_tile_f64(const micloc_plan *plan, void *state, size_t state_bytes, int B, int max_tile, int final_tile,
                                            double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);
size_t micloc_stream_complex_window_state_bytes(const micloc_plan *plan, int B, int window, int hop, int max_windows);
int micloc_stream_complex_window_reset(const micloc_plan *plan, int B, void *win_state, size_t win_bytes, int window, int hop,
                                       int max_windows, void *stream);
int micloc_stream_complex_localize_tile_windows_f64(const micloc_plan *plan, void *state, size_t state_bytes, int B, int max_tile,
                                                    int final_tile, double *power, int32_t *argmax, void *ws, size_t ws_bytes,
                                                    void *win_state, size_t win_bytes, int window, int hop, int max_windows,
                                                    double *window_power, int32_t *window_argmax, double *latest_power,
                                                    int32_t *latest_argmax, void *stream);
int micloc_stream_complex_status(const void *state, int *status4, void *stream);

/* ---- beamforming vectors from membrane covariances (design_from_template's decomposition step) ------ */
/* Replaces the per-DoA np.linalg.svd calls of SNNBeamformer.design_from_template (snn_beamformer.py:183-203) and
 * _find_dc_removed_sing_vec (:372-422) by one batched kernel: column g0 + i of bf_mat [C][G] from cov[i] [C][C]
 * (micloc_lif_covariance_f64's output).  bipolar = 0: the DC-removed conditional singular vector (secular equation solved by
 * the reference's bisection to rel_prec; the result does not depend on the signs of the singular vectors).  bipolar = 1: the
 * leading left singular vector of the folded complex covariance, stacked [Re; Im]; its unit phase -- arbitrary by
 * definition -- is fixed by making the FIRST component real and negative (what LAPACK's zgesdd leaves on these matrices, to
 * ~2e-4 of the component's modulus; a convention that is continuous along the DoA grid), so columns agree with the reference's
 * up to that residual phase and |W^H W| agrees.  C <= 32: cyclic two-sided Jacobi in LDS, one wave per DoA; 32 < C <= 128
 * (C even): one-sided (Hestenes) Jacobi on the matrix / the real embedding of the complex fold, one workgroup per DoA.
 * MICLOC_ERR_SHAPE beyond that.  Device buffers. */
int micloc_design_vectors_f64(const double *cov, int n_doa, int C, int bipolar, double rel_prec, double *bf_mat, int G, int g0,
                              void *stream);

/* ---- array-signal synthesis ------------------------------------------------------------------- */
/* Noise-free part of SNNBeamformer.apply_to_template for a constant DoA per trial (snn_beamformer.py:246-267):
 * x[b][t][m] = np.interp(max(time[t] - delays[b][m], time[0]), time, sig), bit-exact with NumPy.  All pointers are
 * DEVICE buffers: time [T] (the resampled grid, np.arange(t.min(), t.max(), 1/fs)), sig [T], slopes [T-1] =
 * diff(sig)/diff(time), delays [B][M] (already shifted so that their minimum is 0), x [B][T][M]. */
int micloc_synth_delay_f64(const double *time, const double *sig, const double *slopes, int T, const double *delays,
                           int B, int M, double fs, double *x, void *stream);

/* General form: every noise-free signal generator of the reference (all pointers are DEVICE buffers).
 *   x[b][t][m] = sum_k gain[b][k][t] * np.interp(arg, time, sig),   arg = max(time[t] - (d - shift[b]), time[0])   (mode 0)
 *                                                                   arg = time[t] + d                             (mode 1)
 *   d = delay of microphone m for target k of trial b at time t (geometry.delays(doa, normalized=False))
 * mode MICLOC_SYNTH_APPLY_TO_TEMPLATE   = SNNBeamformer / Beamformer.apply_to_template (snn_beamformer.py:239-267,
 *      beamformer.py:220-245; `shift` = delays.min() of :257), also with a moving DoA (`moving` = 1);
 * mode MICLOC_SYNTH_SIGNAL_FROM_TEMPLATE = signal_from_template (xylo_snn_localization.py:44-71: no shift, no clamp, np.interp
 *      saturates) and, with K > 1 and `gain`, signal_multiple_targets (paper_plots/multiple_targets_snn.py:87-160).
 * Delay source: `delays` [B][K][Td][M] (Td = T if moving else 1) computed by the caller (NumPy cos: bit-exact parity with
 * the reference), or, with delays == NULL, computed on the device from `doa` [B][K][Td] and the geometry r_vec / theta_vec
 * [M], `speed` (-r cos(theta_m - doa) / speed; device cos, within an ulp of NumPy's: throughput runs, nothing of size
 * B x T x M crosses PCIe).  `shift` [B] and `gain` [B][K][T] may be NULL.  time / sig [T], slopes [T-1], x [B][T][M]. */
#define MICLOC_SYNTH_APPLY_TO_TEMPLATE 0
#define MICLOC_SYNTH_SIGNAL_FROM_TEMPLATE 1
typedef struct micloc_synth_args {
    const double *time, *sig, *slopes;
    int T, B, K, M;
    const double *delays;
    const double *doa;
    int moving;
    const double *r_vec, *theta_vec;
    double speed;
    const double *shift;
    const double *gain;
    int mode;
    double fs;
    double *x;
} micloc_synth_args;
int micloc_synth_targets_f64(const micloc_synth_args *args, void *stream);
/* shift[b] = min over targets, time steps and microphones of -r cos(theta_m - doa) / speed  (snn_beamformer.py:257's
 * `delays.min()`), from doa [B][K][moving_T]; device buffers. */
int micloc_delay_min_f64(const double *doa, int B, int K, int moving_T, const double *r_vec, const double *theta_vec, int M,
                         double speed, double *shift, void *stream);

/* ---- counter-based random numbers (throughput-mode sweeps) --------------------------------------- */
/* Philox-4x32-10 keyed by `seed`; counter = (pair index, epoch, trial, substream); the uniforms use the reserved trial word
 * 0xFFFFFFFF, so for one seed no two draws of any (generator, trial, substream, epoch) share a block.  The reference draws from NumPy's sequential
 * global MT19937 stream (target_snn_localization.py:452, snn_beamformer.py:273); parity runs replay that on the host,
 * throughput runs use these: out[i] = lo + (hi - lo) * u_i, u in [0, 1) with 53 bits (np.random.rand's range), and
 * x[b] += sigma_b * N(0, 1) (Box-Muller, fp64) with sigma_b = sqrt(mean(x[b]^2)) / sqrt(10^(snr_db[b] / 10))
 * (snn_beamformer.py:270-275) computed on the device from snr_db [B], or taken from `sigma` [B] when it is not NULL.
 * Trial b of the call uses counter word `first_trial + b`, so a sweep sharded over ranks draws the same noise for a
 * given global trial whatever the world size (first_trial + B <= 0xFFFFFFFF).  `epoch` (device uint32, may be NULL: 0) is read when
 * the kernel runs and is a counter word of its own: a HIP graph that contains the generators draws fresh numbers on every replay once micloc_counter_add_u32 (also in
 * the graph) advances it.  Device buffers; ws from micloc_awgn_workspace_bytes (256-B aligned). */
int micloc_uniform_f64(double *out, size_t n, uint64_t seed, uint32_t substream, const uint32_t *epoch, double lo, double hi,
                       void *stream);
size_t micloc_awgn_workspace_bytes(int B, int T, int M);
int micloc_awgn_f64(double *x, int B, int T, int M, const double *snr_db, const double *sigma, uint64_t seed, uint32_t substream,
                    const uint32_t *epoch, uint32_t first_trial, void *ws, size_t ws_bytes, void *stream);
/* micloc_synth_targets_f64 followed by micloc_awgn_f64 (sigma from snr_db) WITHOUT storing the noise-free signal: pass 1 recomputes
 * the synthesis and reduces its squares (the unfused order: sigma is bit-identical), pass 2 recomputes it, adds the normals of
 * micloc_awgn_f64 (same counters) and stores x once -- one trip through HBM instead of four; same bits as the two calls.
 * ws from micloc_synth_awgn_workspace_bytes(B, T, M, K). */
size_t micloc_synth_awgn_workspace_bytes(int B, int T, int M, int K);
int micloc_synth_awgn_f64(const micloc_synth_args *args, const double *snr_db, uint64_t seed, uint32_t substream, const uint32_t *epoch,
                          uint32_t first_trial, void *ws, size_t ws_bytes, void *stream);
int micloc_counter_add_u32(uint32_t *counter, uint32_t inc, void *stream); /* *counter += inc (device word) */

/* ---- Monte-Carlo results ---------------------------------------------------------------------- */
/* err[b] = arcsin|sin(doa_list[argmax[b]] - doa_true[b])| (target_snn_localization.py:464-466; pi-periodic) and
 * mae[s] = mean of err over the `B / groups` consecutive trials of SNR group s (:520).  All pointers are DEVICE buffers
 * (doa_list [G], doa_true [B], err [B], mae [groups]); err or mae may be NULL; B must be a multiple of groups. */
int micloc_doa_error_f64(const int32_t *argmax, const double *doa_list, int G, const double *doa_true, int B, int groups,
                         double *err, double *mae, void *stream);

/* ---- Xylo-A2 hidden-layer integer LIF (BASELINE config 4) -------------------------------------- */
/* Replaces XyloSim.evolve as called by Demo.xylo_process (xylo_snn_localization.py:358-377) with the network built at
 * :173-290: bit-shift decay, int8 weights, saturating int16 state, subtractive reset, one shared recurrent weight.
 * PARITY UNPINNED: the reference's arithmetic is rockpool/xylosim (third party, unpinned, absent); this follows the
 * published update rule (oracle/micloc_oracle.c oracle_xylo_lif).  spikes_in [B][T][Cin] uint8 (device),
 * W_in [Cin][N] / dash_syn [N] / dash_mem [N] / thr [N] host arrays; spikes_out [B][T][N] uint8 and rate [B][N]
 * int32 (device) may each be NULL.  Synchronises the stream once (coefficient upload). */
size_t micloc_xylo_workspace_bytes(int Cin, int N);
int micloc_xylo_lif_i16(const uint8_t *spikes_in, int B, int T, int Cin, const int8_t *W_in, int N, int w_rec,
                        const uint8_t *dash_syn, const uint8_t *dash_mem, const int16_t *thr, int max_spikes,
                        uint8_t *spikes_out, int32_t *rate, void *ws, size_t ws_bytes, void *stream);

/* The same network in two phases: micloc_xylo_upload places the packed weights / constants in `ws` (synchronises once);
 * micloc_xylo_lif_resident_i16 then runs any number of batches without touching host memory or synchronising, so it can
 * be captured into a HIP graph.  ternary_channels > 0: `spikes_in` is the encoder's int8 raster [B][T][ternary_channels]
 * in {-1, 0, +1} and Cin = 2 * ternary_channels: input channel c carries the +1 events of raster channel c, channel
 * ternary_channels + c its -1 events -- Demo.spike_encoding's split (xylo_snn_localization.py:350-354) folded into the
 * kernel's staging loop.  ternary_channels == 0: spikes_in is uint8 [B][T][Cin] as above.
 * With a ternary raster, w_rec == 0 and a 16-byte aligned `spikes_in` the launch takes the sweep kernel (two neurons per
 * lane in packed 16-bit arithmetic, input currents on the int8 matrix cores); anything else the general one.  Same results. */
int micloc_xylo_upload(int Cin, const int8_t *W_in, int N, const uint8_t *dash_syn, const uint8_t *dash_mem, const int16_t *thr,
                       void *ws, size_t ws_bytes, void *stream);
int micloc_xylo_lif_resident_i16(const void *spikes_in, int ternary_channels, int B, int T, int Cin, int N, int w_rec,
                                 int max_spikes, uint8_t *spikes_out, int32_t *rate, void *ws, size_t ws_bytes, void *stream);
/* The sweep's form of the same call (paper_plots/target_xylo_localization.py:590-594 needs only rec["Spikes"].mean(0): the spike
 * COUNTS): ternary raster [B][T][ternary_channels] in, rate [B][N] out, w_rec == 0.  The launch is a set of persistent workgroups
 * that take (trial, time chunk) tickets from a device counter and hand a trial's integer state on through `scratch`
 * (micloc_xylo_sweep_scratch_bytes(B) bytes, 256-byte aligned, contents irrelevant on entry; one buffer per concurrent call) --
 * every SIMD carries the same number of chains from start to end.  Same counts as micloc_xylo_lif_resident_i16; shapes the queue does
 * not serve (N > 512, Cin > 64, unaligned raster) take that call's kernels.  workers_per_cu: persistent workgroups per CU, 0 = 4 (three
 * waves each: three per SIMD); fewer leave room for the kernels of other streams.  No host access, no synchronisation (graph-capturable). */
size_t micloc_xylo_sweep_scratch_bytes(int B);
/* status2 = {tickets handed out (>= chunks x trials once the launch has drained), workers that gave up waiting for a predecessor
 * (must be 0: the wait is bounded at ~half a minute only to keep a broken launch from hanging the device)} of the last
 * micloc_xylo_lif_sweep_i16 call on `scratch`; synchronises the stream. */
int micloc_xylo_sweep_status(const void *scratch, int *status2, void *stream);
int micloc_xylo_lif_sweep_i16(const int8_t *raster, int ternary_channels, int B, int T, int Cin, int N, int max_spikes, int32_t *rate,
                              void *ws, size_t ws_bytes, void *scratch, size_t scratch_bytes, int workers_per_cu, void *stream);
/* Demo.spike_encoding's channel bookkeeping (micloc/xylo_snn_localization.py:339-354: the per-band rasters side by side,
 * astype(int64), then [spikes > 0 | spikes < 0]) for ONE band of `bands`: raster int8 [B][T][C] in {-1, 0, +1} -> its channel block
 * of out [B][T][bands * C * (2 if BIPOLAR else 1)].  TERNARY: the value itself at channel band*C + c (the concatenated raster the
 * sweep kernel reads); UNIPOLAR: (s > 0) there; BIPOLAR: (s > 0) there and (s < 0) at bands*C + band*C + c. */
#define MICLOC_PACK_TERNARY 0
#define MICLOC_PACK_UNIPOLAR 1
#define MICLOC_PACK_BIPOLAR 2
int micloc_pack_events_u8(const int8_t *raster, int B, int T, int C, int band, int bands, int mode, uint8_t *out, void *stream);
/* Demo.extract_rate (micloc/xylo_snn_localization.py:379-398) from the spike COUNTS of the hidden layer: rate[b][g] = mean over bands of
 * (counts[b][f * G + g] / T) * fs.  counts int32 [B][bands * G], rate double [B][G] (device). */
int micloc_rate_from_counts_f64(const int32_t *counts, int B, int G, int bands, int T, double fs, double *rate, void *stream);
/* index[b] = find_peak_location(power_b, win_size) (micloc/utils.py:84-121; paper_plots/target_xylo_localization.py:594-604)
 * with power_b[g] = sum over `bands` of rate[b][f * G + g] (the per-DoA spike counts; the reference's positive scale
 * factors T / fs and 1 / max do not move the arg-max): box-car of win_size samples, FULL non-circular convolution, first
 * maximum, minus win_size // 2, modulo G.  Exact integer window sums.  rate [B][bands * G] int32, index [B] (device). */
int micloc_peak_location_i32(const int32_t *rate, int B, int G, int bands, int win_size, int32_t *index, void *stream);
/* Multi-source read-out: the K strongest peaks of every row power [B][G] (fp64) over the DoA grid doa_list [G].
 * Grid kinds: LINEAR (no wrap: the end points have one neighbour); CIRCULAR (the G points cover one period without a duplicate:
 * point G-1 neighbours point 0); CIRCULAR_CLOSED (np.linspace(-pi, pi, G): points 0 and G-1 are one direction and are merged
 * into one ring point whose value is max(p[0], p[G-1]), whose reported index is 0 if p[0] >= p[G-1] (or p[G-1] is NaN) and
 * G-1 otherwise, and whose ring neighbours are 1 and G-2; G = 1 is taken as CIRCULAR).
 * A (ring) point is a local maximum when its value is >= each neighbour's; a NaN neighbour counts as lower, a NaN point is
 * never a peak.  Selection: visit the local maxima in order of value, largest first, ties to the lower reported index; accept
 * one if (rel_threshold > 0 only) its value is >= rel_threshold * max(row) (the maximum over the non-NaN values) and its
 * distance to every accepted peak is >= min_separation; stop at K accepted peaks.  Distance in fp64, exactly:
 * r = |doa[i] - doa[j]| on a linear grid, min(r, 2 pi - r) on a circular one.  For K = 1 and a row without NaN, index[b][0] is
 * the first maximum (np.argmax) on every grid kind.
 * Outputs index [B][K] int32 and value [B][K] (may be NULL): the accepted peaks in selection order, unfilled slots -1 and NaN.
 * Supported: 1 <= G <= 4096, 1 <= K <= 16, min_separation >= 0, rel_threshold >= 0 (MICLOC_ERR_INVALID otherwise, checked
 * before any device work).  Device buffers; one wave per row, no atomics, no host synchronisation (graph-capturable). */
#define MICLOC_GRID_LINEAR 0
#define MICLOC_GRID_CIRCULAR 1
#define MICLOC_GRID_CIRCULAR_CLOSED 2
int micloc_doa_peaks_f64(const double *power, int B, int G, const double *doa_list, int grid_kind, int K, double min_separation,
                         double rel_threshold, int32_t *index, double *value, void *stream);

/* Moving-target tracking: Envelope.evolve (micloc/utils.py:36-81) on the beamformer output and the per-time-step arg-max over the DoA
 * grid, `doa_index = np.argmax(sig_bf_env, axis=1)` (paper_plots/target_snn_localization.py:599-622), without the T x G array ever
 * leaving the device.  y [B][T][G] (apply_to_signal's result, real);  env [B][T][G]: env[t] = the envelope state after sample t,
 * state_0 = |y_0|, state_t = (1 - 1/w) state_{t-1} + 1/w |y_t| [|y_t| >= state_{t-1}] with w = the rise window when the bracket holds,
 * the fall window otherwise -- NumPy's order of operations, nothing fused: bit-identical to the reference class.  The caller passes
 * a_rise = 1 - 1/w_rise, i_rise = 1/w_rise, a_fall = 1 - 1/w_fall as NumPy computes them (w = int(fs * time) >= 1).  env is always
 * written (a caller that only wants the indices passes scratch); index [B][T] int32 (may be NULL) = first maximum of every row. */
int micloc_envelope_track_f64(const double *y, int B, int T, int G, double a_rise, double i_rise, double a_fall, double *env, int32_t *index,
                              void *stream);
/* The same for the other arrays the reference's scripts hand to Envelope.evolve: the complex Beamformer's output
 * (paper_plots/target_localization.py:597-600; y [B][T][G][2] = numpy complex128, |z| = hypot(re, im) -- the device library's, < 1 ulp) and
 * integer spike rasters (paper_plots/target_xylo_localization.py:757-768: `sig_bf = spikes_out`; exact).  env stays double [B][T][G]. */
#define MICLOC_ENV_F64 0
#define MICLOC_ENV_C128 1
#define MICLOC_ENV_U8 2
#define MICLOC_ENV_I32 3
#define MICLOC_ENV_I64 4
int micloc_envelope_track_any(const void *y, int kind, int B, int T, int G, double a_rise, double i_rise, double a_fall, double *env, int32_t *index,
                              void *stream);

/* ---- time-resolved DoA: power and arg-max per window ------------------------------------------ */
/* The read-outs above reduce a whole recording to one power row per trial.  These entries keep the time axis: power and
 * arg-max per WINDOW of frames, read from the per-chunk partial sums the beamforming kernels already write -- no T x G array.
 * The window rule:
 *   - `window` and `hop` are in frames, both >= 1, and both multiples of the plan's window QUANTUM: the chunk length (frames
 *     per row of partial sums) of the beamforming kernel that serves this plan and bf_mat (micloc_window_quantum; 256 up to 64
 *     channels, 512 beyond);
 *   - window n starts at s_n = n hop; there are nW = 1 windows if T <= window, else nW = 1 + ceil((T - window) / hop);
 *   - window n covers the frames [s_n, min(s_n + window, T));
 *   - power_w[b][n][g] is `power` restricted to those frames and divided by the window's own frame count: sum y^2 for the real
 *     (SNN) bf_mat, sum |y|^2 = sum re^2 + sum im^2 for the complex Beamformer;
 *   - argmax_w[b][n] is the first maximum of the row; a NaN never wins (a row of NaNs gives 0).
 * With hop > window the last window of the formula can start at or after T; it holds no frame, its power is NaN and its
 * arg-max 0.  With hop <= window every window holds at least one frame.
 * Order of the additions (fixed): the chunk rows of a window are added in ascending order inside blocks of 32 chunks counted
 * from the window's first chunk, the block sums in ascending order onto the total -- the one-shot reduction's order re-based at
 * the window start.  A single window with window >= T therefore returns the bits of `power` and `argmax`.
 * power_w [B][nW][G], argmax_w [B][nW] int32, power [B][G], argmax [B] are device buffers and may each be NULL (at least one of
 * power_w / argmax_w must be given); power / argmax are the ordinary whole-recording results from the SAME partial sums: the
 * beamforming kernel runs once.  Status: MICLOC_ERR_SHAPE for a window or hop that is not a multiple of the quantum, a hop or
 * window < 1, or B nW > INT32_MAX; MICLOC_ERR_WORKSPACE for a short or misaligned ws.  One workgroup per (window, trial), no
 * atomics, no host synchronisation: re-entrant per stream and graph-capturable like the entries they extend. */
int micloc_window_quantum(const micloc_plan *plan); /* frames (> 0), or MICLOC_ERR_INVALID / MICLOC_ERR_NOT_SET (neuron kernel of a real bf_mat, bf_mat) */
/* nW of the rule for a given quantum (pure function): > 0, or MICLOC_ERR_INVALID (T or quantum < 1) / MICLOC_ERR_SHAPE */
int micloc_window_count(int T, int window, int hop, int quantum);
/* ws bytes of the stage-level (pipeline == 0) or pipeline-level (pipeline != 0) windowed entries; 0 on bad arguments.  The
 * read-out needs no scratch of its own: these are the sizes of the unwindowed calls (partial sums: B x ceil(T / 256) x Gp doubles). */
size_t micloc_window_workspace_bytes(const micloc_plan *plan, int B, int T, int window, int hop, int pipeline);
/* micloc_lif_beamform_f64 / micloc_beamform_c128_f64 with the windowed read-out (no y) */
int micloc_lif_beamform_windows_f64(const micloc_plan *plan, const int8_t *spikes, int B, int T, int window, int hop, double *power_w,
                                    int32_t *argmax_w, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);
int micloc_beamform_c128_windows_f64(const micloc_plan *plan, const double *pre, int B, int T, int Ts, int window, int hop, double *power_w,
                                     int32_t *argmax_w, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);
/* micloc_snn_pipeline_f64 (spikes may be NULL) / micloc_beamformer_pipeline_f64 with the windowed read-out (no y) */
int micloc_snn_pipeline_windows_f64(const micloc_plan *plan, const double *x, int B, int T, int window, int hop, int8_t *spikes,
                                    double *power_w, int32_t *argmax_w, double *power, int32_t *argmax, void *ws, size_t ws_bytes,
                                    void *stream);
int micloc_beamformer_pipeline_windows_f64(const micloc_plan *plan, const double *x, int B, int T, int window, int hop, double *power_w,
                                           int32_t *argmax_w, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);

/* ---- moving-target tracking: the DoA per time step, without the T x G arrays -------------------- */
/* paper_plots/target_snn_localization.py:595-622: `np.argmax(Envelope.evolve(sig_bf), axis=1)` for a batch, as ONE read-out of the
 * beamforming stage.  The rule, for every trial b and DoA column g independently:
 *   y[t][g]   the beamformer output of frame t: exactly the value micloc_lif_beamform_f64 / micloc_beamform_c128_f64 store in `y`
 *             (same instruction sequence, same bits);
 *   m[t][g]   = |y[t][g]|  (real: fabs; complex: hypot(re, im), the device library's, as MICLOC_ENV_C128);
 *   e[0][g]   = m[0][g];   for t >= 1:  rise = m[t][g] >= e[t-1][g];
 *   e[t][g]   = rise ? a_rise * e[t-1][g] + i_rise * m[t][g] : a_fall * e[t-1][g]      -- two rounded products, one rounded sum,
 *             nothing fused: micloc_envelope_track_f64's recurrence; a_rise = 1 - 1/w_rise, i_rise = 1/w_rise, a_fall = 1 - 1/w_fall as
 *             NumPy computes them (w = int(fs * time) >= 1);
 *   index[b][t]    = the FIRST g with e[t][g] = max_g e[t][g]; a NaN never wins; a row of NaN only gives 0  (np.argmax without NaN);
 *   peak_env[b][t] = e[t][index[b][t]]  (NaN for a row of NaN only; may be NULL);
 *   env_last[b][g] = e[T-1][g]  (may be NULL).
 * index / peak_env / env_last equal, bit for bit, what micloc_envelope_track_any computes from the stored y.
 * Plans with up to 16 channels whose y the bf_mat-stationary kernels produce (micloc_track_is_fused() == 1) run the fused kernels of
 * csrc/track.hip: neither y nor e is stored, the scratch is one (value, index) pair per frame and 64 DoA columns.  Other plans run
 * the two-step route inside the call -- beamforming with y stored, the envelope kernel, a row read-out -- over sub-batches of
 * trials: the minimum workspace holds y and e of ONE trial, and a caller that passes more has as many trials per sub-batch as fit
 * (the results do not depend on it).
 * Status codes before any launch: MICLOC_ERR_SHAPE for T < 1 or B * T > 2^31 - 1 (and a plan of the other kind, a Ts that is not
 * micloc_padded_T(T)), MICLOC_ERR_WORKSPACE for a missing, misaligned or short workspace, MICLOC_ERR_INVALID / MICLOC_ERR_NOT_SET as
 * everywhere.  No atomics on results, no host synchronisation, no allocation: re-entrant per stream with workspaces of their own. */
/* ws bytes of all four calls below (what the pipeline's first two stages need + the tracking region); 0 on bad arguments or a plan
 * without bf_mat */
size_t micloc_track_workspace_bytes(const micloc_plan *plan, int B, int T);
/* 1: the fused kernels serve this plan and its bf_mat, 0: the two-step route; < 0: a status code */
int micloc_track_is_fused(const micloc_plan *plan);
int micloc_lif_beamform_track_f64(const micloc_plan *plan, const int8_t *spikes, int B, int T, double a_rise, double i_rise, double a_fall,
                                  int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream);
int micloc_beamform_c128_track_f64(const micloc_plan *plan, const double *pre, int B, int T, int Ts, double a_rise, double i_rise,
                                   double a_fall, int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes,
                                   void *stream);
/* STHT + band-pass (+ RZCC) + the above, x [B][T][M] */
int micloc_snn_pipeline_track_f64(const micloc_plan *plan, const double *x, int B, int T, double a_rise, double i_rise, double a_fall,
                                  int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes, void *stream);
int micloc_beamformer_pipeline_track_f64(const micloc_plan *plan, const double *x, int B, int T, double a_rise, double i_rise,
                                         double a_fall, int32_t *index, double *peak_env, double *env_last, void *ws, size_t ws_bytes,
                                         void *stream);

/* ---- Xylo moving-target tracking: the DoA per time step from the hidden layer's spikes ----------- */
/* paper_plots/target_xylo_localization.py:672-789 (`test_moving_target`, and its `_unipolar` twin): `sig_bf = spikes_out`, then
 * `Envelope.evolve`, then `np.argmax(axis=1)` -- for a batch, as ONE read-out of the integer LIF ("Xylo-A2 hidden-layer integer LIF"
 * above; PARITY UNPINNED like every Xylo entry).  The rule, for every trial b and neuron n independently:
 *   c[t][n]   the spike count of step t: exactly the value micloc_xylo_lif_resident_i16 stores in spikes_out (the second spike within a
 *             step and the max_spikes cap included);
 *   m[t][n]   = (double)c[t][n];
 *   e[0][n]   = m[0][n];   for t >= 1:  rise = m[t][n] >= e[t-1][n];
 *   e[t][n]   = rise ? a_rise * e[t-1][n] + i_rise * m[t][n] : a_fall * e[t-1][n]      -- two rounded products, one rounded sum,
 *             nothing fused: micloc_envelope_track_f64's recurrence, with a_rise = 1 - 1/w_rise, i_rise = 1/w_rise, a_fall = 1 - 1/w_fall
 *             as NumPy computes them (w = int(fs * time) >= 1);
 *   index[b][t]    = the FIRST n in [0, N) with e[t][n] = max_n e[t][n]  (np.argmax; counts are integers, so a row always has a winner);
 *   peak_env[b][t] = that value  (may be NULL);
 *   env_last[b][n] = e[T-1][n]  (may be NULL);
 *   rate[b][n]     = sum_t c[t][n], the counts of micloc_xylo_lif_resident_i16  (may be NULL).
 * All four equal, bit for bit, what micloc_xylo_lif_resident_i16 with spikes_out followed by micloc_envelope_track_any (MICLOC_ENV_U8)
 * and a row arg-max compute from the stored raster.
 * Arguments as micloc_xylo_lif_resident_i16: spikes_in is the encoder's int8 raster [B][T][ternary_channels] (ternary_channels > 0,
 * Cin = 2 * ternary_channels) or uint8 event counts [B][T][Cin] (ternary_channels == 0); net_ws / net_ws_bytes: micloc_xylo_upload's.
 * Networks the packed kernel serves -- w_rec == 0, the ternary raster, Cin <= 64, max_spikes >= 1 (micloc_xylo_track_is_fused() == 1)
 * and a 16-byte aligned raster -- run the tracking form of the packed LIF walk (csrc/stream_xylo.hip): one workgroup per 512-neuron block and
 * trial, neither the spikes nor the envelope is stored; up to 512 neurons the workgroup writes index and peak_env itself, beyond that
 * the scratch is one (value, index) pair per frame and block and a small launch combines the blocks in ascending order.  Every other
 * network (a recurrent weight, event counts, the unipolar input) runs the two-step route inside the call over sub-batches of trials:
 * the minimum workspace holds the raster and the envelope of ONE trial (9 T N bytes), and a caller that passes more has as many trials
 * per sub-batch as fit (the results do not depend on it).
 * Status codes before any launch: MICLOC_ERR_SHAPE for T < 1, N < 1, B * T > 2^31 - 1 (and Cin > 64, Cin != 2 * ternary_channels,
 * w_rec != 0 with N > 1024, as micloc_xylo_lif_resident_i16); MICLOC_ERR_WORKSPACE for a missing, misaligned (256 bytes) or short net_ws
 * or ws; MICLOC_ERR_INVALID for a NULL index or input, a bad B or max_spikes < 1.  No atomics on results, no host synchronisation, no
 * allocation: re-entrant per stream with workspaces of their own, and graph-capturable. */
/* 1: the fused kernel serves this network and input, 0: it does not (the two-step route; also Cin > 64, which no Xylo kernel takes:
 * the call itself then answers MICLOC_ERR_SHAPE); < 0: a status code */
int micloc_xylo_track_is_fused(int ternary_channels, int Cin, int N, int w_rec, int max_spikes);
/* minimum ws bytes of the call below (never 0 for valid arguments; fused: at most 16 B T ceil(N / 512) + 4096); 0 on bad arguments */
size_t micloc_xylo_track_workspace_bytes(int ternary_channels, int Cin, int N, int w_rec, int B, int T);
int micloc_xylo_lif_track_i16(const void *spikes_in, int ternary_channels, int B, int T, int Cin, int N, int w_rec, int max_spikes,
                              double a_rise, double i_rise, double a_fall, int32_t *index, double *peak_env, double *env_last,
                              int32_t *rate, void *net_ws, size_t net_ws_bytes, void *ws, size_t ws_bytes, void *stream);

/* ---- time-resolved DoA, Xylo: counts, rate and peak per window of a batch ------------------------ */
/* The windows of "streaming, Xylo" below (micloc_stream_xylo_tile_windows_i16 / micloc_stream_xylo_readout) for recordings that are
 * complete: one call for a batch, for EVERY network micloc_xylo_lif_resident_i16 serves (unipolar input, uint8 event counts, a recurrent
 * weight with N <= 1024).  PARITY UNPINNED like every Xylo entry: the LIF equals oracle_xylo_lif bit for bit, the oracle is not checked
 * against XyloSim.  The rule:
 *   - the quantum is 256 frames (micloc_xylo_window_quantum); window and hop are positive multiples of it, hop <= window;
 *     nW = micloc_window_count(T, window, hop, 256); window n covers the frames [n hop, min(n hop + window, T));
 *   - window_counts[b][n][j] = the sum over the window's frames of the spike count of neuron j, the value micloc_xylo_lif_resident_i16
 *     stores in spikes_out -- exact integers.  The network is NOT reset between windows: a trial is one continuous run.  With
 *     hop == window the windows of a trial add up to counts[b]; a single window >= T IS counts[b];
 *   - counts[b][j] (may be NULL) = micloc_xylo_lif_resident_i16's rate, from the same walk: the LIF runs once;
 *   - window_rate[b][n][g] = micloc_rate_from_counts_f64's expression and band order on the row window_counts[b][n] with the window's
 *     own frame count in place of T; window_peak[b][n] = what micloc_peak_location_i32 returns for that row and win_size.
 * All of them equal, bit for bit, what the stream has emitted after the last tile wherever the stream serves the network.
 * micloc_xylo_lif_windows_i16: arguments as micloc_xylo_lif_resident_i16 (net_ws: micloc_xylo_upload's); ws
 * (micloc_xylo_windows_workspace_bytes, 256-B aligned) holds the counts per chunk of 256 frames, 4 B ceil(T / 256) N bytes -- nothing of
 * size T x N is stored.  The routing is micloc_xylo_lif_resident_i16's: w_rec == 0, the ternary raster, Cin <= 64 and a 16-byte aligned
 * raster run the chunk-count form of the packed kernel (one workgroup per trial and 512 neurons; the ticket queue of
 * micloc_xylo_lif_sweep_i16 has no such form), everything else the chunk-count form of the general kernel; then one launch adds the chunk
 * rows of every window.  micloc_xylo_window_readout: one launch; either output may be NULL, not both.
 * Status codes, all before any launch: MICLOC_ERR_SHAPE for a window or hop off the quantum, hop > window, B nW > 2^31 - 1 and the
 * shapes micloc_xylo_lif_resident_i16 refuses; MICLOC_ERR_INVALID for NULL or out-of-range arguments, a win_size
 * micloc_peak_location_i32 refuses (with window_peak) and both read-out outputs NULL; MICLOC_ERR_WORKSPACE for a missing, misaligned or
 * short net_ws or ws.  Two launches and one, whatever B and nW; no atomics, no host synchronisation, no allocation: re-entrant per
 * stream with workspaces of their own, and graph-capturable. */
int micloc_xylo_window_quantum(void);                            /* 256 */
size_t micloc_xylo_windows_workspace_bytes(int B, int T, int N); /* the chunk rows; 0 on bad arguments */
int micloc_xylo_lif_windows_i16(const void *spikes_in, int ternary_channels, int B, int T, int Cin, int N, int w_rec, int max_spikes,
                                int window, int hop, int32_t *window_counts /*[B][nW][N]*/, int32_t *counts /*[B][N], may be NULL*/,
                                void *net_ws, size_t net_ws_bytes, void *ws, size_t ws_bytes, void *stream);
int micloc_xylo_window_readout(const int32_t *window_counts, int B, int T, int window, int hop, int G, int bands, double fs, int win_size,
                               double *window_rate /*[B][nW][G], may be NULL*/, int32_t *window_peak /*[B][nW], may be NULL*/, void *stream);

/* ---- streaming, tracking: a DoA per frame while the recording arrives ---------------------------- */
/* The tracking rule above for a recording that arrives tile by tile ("streaming" and "streaming, complex Beamformer"): every frame is
 * EMITTED -- its index and its peak envelope written -- by the localize call of the tile that makes it final, and the emitted rows equal,
 * bit for bit, index / peak_env of the one-shot tracking call on the whole recording, whatever the tiling; after the last tile the first
 * G columns of every trial's row of track_state equal env_last.
 *   - When a frame is final.  SNN stream: when the chunk of the stream that holds it is beamformed (the chunk range the horizon leaves;
 *     micloc_stream_localize_status' frames count the emitted frames).  Complex stream: when its tile is band-passed (the frames pushed).
 *   - Where it goes.  Frame t of trial b goes to row t % max_track of track_index [B][max_track] int32 / track_peak [B][max_track] double;
 *     the newest emitted frame also to latest_index [B] / latest_peak [B].  All four are required device buffers.  max_track must be at
 *     least what one tile can make final: window_frames (SNN), max_tile (complex).
 *   - State.  track_state holds e[t-1][g] in front of the next frame: [B][ceil(G / 64) * 64] doubles (micloc_stream_track_state_bytes),
 *     zero-filled once by micloc_stream_track_reset; e[0] = m[0] is taken where the stream's clock says frame 0.  Nothing grows with the
 *     stream.  track_ws is scratch of micloc_stream_track_workspace_bytes (one (value, index) pair per window frame and 64 DoA columns;
 *     for a complex plan its third argument is max_tile).
 * The entries are micloc_stream_localize_tile_f64 / micloc_stream_complex_localize_tile_f64 with the tracking launch (and its combine
 * launch when G > 64) in front of the commit / the slide, where the window read-out sits; they take the window arguments too: with
 * win_state == NULL (the other window arguments are then not read) there is no window read-out, otherwise it is that of the *_windows
 * entry.  power, argmax and the window rows have the bits of the entries without tracking.  No launch argument depends on time: a tile
 * stays one capturable sequence.
 * Status codes before any launch: MICLOC_ERR_SHAPE for a plan the fused kernels do not serve (micloc_track_is_fused() != 1), a plan of
 * the other kind, max_track below what one tile can make final, or (SNN) a neuron kernel whose LIF history 4 NK - 16 is longer than a
 * chunk of the stream; MICLOC_ERR_WORKSPACE for a missing, misaligned or short state / scratch; MICLOC_ERR_INVALID (a NULL track_state
 * or result buffer among them) / MICLOC_ERR_NOT_SET as everywhere. */
size_t micloc_stream_track_state_bytes(const micloc_plan *plan, int B); /* 0 on bad arguments or a plan the fused kernels do not serve */
size_t micloc_stream_track_workspace_bytes(const micloc_plan *plan, int B, int window_frames); /* likewise */
int micloc_stream_track_reset(const micloc_plan *plan, int B, void *track_state, size_t track_bytes, void *stream);
int micloc_stream_localize_tile_track_f64(const micloc_plan *plan, const void *enc_state, void *loc_state, size_t loc_bytes,
                                          const int8_t *window_raster, int B, int window_frames, int final_tile, double *power, int32_t *argmax,
                                          void *ws, size_t ws_bytes, void *win_state, size_t win_bytes, int window, int hop, int max_windows,
                                          double *window_power, int32_t *window_argmax, double *latest_power, int32_t *latest_argmax,
                                          void *track_state, size_t track_bytes, double a_rise, double i_rise, double a_fall, int max_track,
                                          int32_t *track_index, double *track_peak, int32_t *latest_index, double *latest_peak, void *track_ws,
                                          size_t track_ws_bytes, void *stream);
int micloc_stream_complex_localize_tile_track_f64(const micloc_plan *plan, void *state, size_t state_bytes, int B, int max_tile, int final_tile,
                                                  double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *win_state, size_t win_bytes,
                                                  int window, int hop, int max_windows, double *window_power, int32_t *window_argmax,
                                                  double *latest_power, int32_t *latest_argmax, void *track_state, size_t track_bytes,
                                                  double a_rise, double i_rise, double a_fall, int max_track, int32_t *track_index,
                                                  double *track_peak, int32_t *latest_index, double *latest_peak, void *track_ws,
                                                  size_t track_ws_bytes, void *stream);

/* ---- wideband localisation: filterbank, one SNN chain per band, band sum ------------------------ */
/* The deployed form of the method (micloc/localization_demo_snn.py:125-193): a filterbank splits the recording into F bands
 * (:160-164, micloc/filterbank.py:25-46), every band runs its own SNNBeamformer.apply_to_signal with its own band-pass, neuron
 * kernel and bf_mat, the angular power patterns are added and ONE arg-max is taken (:166-190).  The rule:
 *   Filterbank.
 *   - xf[f][b] = scipy.signal.lfilter(b_f, a_f, x[b], axis=0) from zero state, f < F <= MICLOC_MAX_BANDS, in the DF2T arithmetic of
 *     micloc_lfilter_f64 (coefficients divided by a_f[0] on the host): the same numbers, band by band.  b, a are HOST arrays
 *     [F][n], zero-padded to one length n <= MICLOC_MAX_IIR; they travel as kernel arguments: no device table, no allocation, no
 *     host synchronisation.  x [B][T][M] -> xf [F][B][T][M], ONE launch for all bands (the input is read from memory once).
 *   - Time is serial per (band, trial, microphone) chain and is not chunked: a lone long recording runs at one chain's pace.
 *   Band sum.
 *   - power[r][g] = ((p_0[r][g] + p_1[r][g]) + p_2[r][g]) + ... in ascending band order, starting FROM p_0 (not from zero), every
 *     addition rounded to nearest: band_power [F][R][G] -> power [R][G].
 *   - argmax[r] is the first maximum of the row; a NaN never wins; a row of NaN only gives 0.  power or argmax may be NULL.
 *   - R = B for whole recordings, B * nW for windows (row r = b * nW + n).
 *   Pipeline (micloc_snn_pipeline_bands_f64), all on the one stream, in this order: the filterbank; per band f in ascending order
 *   micloc_snn_pipeline_f64 (window == 0) or micloc_snn_pipeline_windows_f64 (window > 0, the window rule of "time-resolved DoA"
 *   above) of plans[f] on xf[f], power only; the band sum.  band_power [F][R][G] receives every band's rows (NULL: they stay in
 *   the workspace).  Each band's rows are bit for bit what that band's own pipeline call returns for xf[f].
 *   Workspace (micloc_snn_bands_workspace_bytes, 256-B aligned): xf, band_power when the caller passes NULL, and ONE pipeline
 *   workspace -- the largest micloc_workspace_bytes(plans[f], B, T): the bands run one after the other and share it.
 *   Status, before any launch: MICLOC_ERR_INVALID for NULL (plans, a plan, coefficients, x, both of power / argmax), F outside
 *   1..MICLOC_MAX_BANDS, fb_n outside 1..MICLOC_MAX_IIR, a_f[0] == 0, B outside 1..65535, T < 1, window or hop < 0;
 *   MICLOC_ERR_NOT_SET for a plan without neuron kernel or bf_mat; MICLOC_ERR_SHAPE for plans on different devices, with
 *   different M or G, with a complex bf_mat, or (window > 0) a window or hop that is not a positive multiple of EVERY plan's
 *   window quantum (micloc_window_quantum: the common quantum is their least common multiple) or B * nW > INT32_MAX;
 *   MICLOC_ERR_WORKSPACE for a short or misaligned ws.  hop == 0 means hop = window.
 * No atomics, no host synchronisation, no allocation: re-entrant per stream with workspaces of their own and capturable in a
 * hipGraph (on ONE stream: nothing runs side by side).  The stand-alone entries launch on the device that owns their output. */
#define MICLOC_MAX_BANDS 16
int micloc_filterbank_f64(const double *b, const double *a, int F, int n, /* host [F][n] each */
                          const double *x, int B, int T, int M, double *xf, void *stream);
int micloc_band_sum_f64(const double *band_power, int F, int R, int G, double *power, int32_t *argmax, void *stream);
size_t micloc_snn_bands_workspace_bytes(const micloc_plan *const *plans, int F, int B, int T, int window, int hop); /* 0 on bad arguments */
int micloc_snn_pipeline_bands_f64(const micloc_plan *const *plans, int F, const double *fb_b, const double *fb_a, int fb_n,
                                  const double *x, int B, int T, int window, int hop, /* window 0: whole recording */
                                  double *band_power /* [F][R][G] or NULL */, double *power, int32_t *argmax, void *ws, size_t ws_bytes,
                                  void *stream);

/* ---- wideband localisation, complex Beamformer: every band's chain in one batch ------------------ */
/* The non-spiking form the reference deploys (micloc/localization_demo.py:43-89,158-182): a filterbank, one complex Beamformer per
 * band (own band-pass, own complex bf_mat), mean_t |y|^2 per band, the patterns added, ONE arg-max.  The chains have no encoder
 * state, so the band dimension folds into the batch dimension.  The rule:
 *   - xf = the filterbank of "wideband localisation" above: x [B][T][M] -> xf [F][B][T][M], one launch.
 *   - Band f's rows of band_power [F][R][G] are bit for bit the `power` of micloc_beamformer_pipeline_f64(plans[f], xf[f], B, T)
 *     (window == 0) or the power_w of micloc_beamformer_pipeline_windows_f64(plans[f], xf[f], B, T, window, hop) (window > 0, the
 *     window rule of "time-resolved DoA" above; R = B * nW, row r = b * nW + n).  band_power may be NULL: the rows stay in the workspace.
 *   - power[r][g] = ((p_0[r][g] + p_1[r][g]) + p_2[r][g]) + ... in ascending band order, starting FROM p_0, every addition rounded
 *     to nearest.  argmax[r] is the first maximum of the row; a NaN never wins; a row of NaN only gives 0.  power or argmax may be NULL.
 *   Launches, all on the one stream, in this order: (1) the filterbank; (2) ONE STHT launch over the F * B trials of xf (the plans
 *   share the Hilbert kernel); (3) ONE band-pass launch over the F * B * 2M chains of the analytic signal, band f with plans[f]'s
 *   coefficients -- in-phase rows from xf through the roll by L / 2, quadrature rows from the STHT, the DF2T arithmetic of
 *   micloc_lfilter_f64 from zero state, every term computed: against the rows the one-shot pipeline of band f forms only the sign of a
 *   zero may differ; (4) per band in ascending order the contraction of that band's own pipeline call (its bf_mat) on its B
 *   trials, into one array of chunk sums [F * B][chunks][Gp]; (5) ONE time reduction (window == 0) or window read-out (window > 0)
 *   over the F * B trials; (6) the band sum.  5 + F launches; no atomics, no host synchronisation, no allocation: re-entrant per
 *   stream with workspaces of their own and capturable in a hipGraph (a straight chain: nothing runs side by side).
 *   Workspace (micloc_beamformer_bands_workspace_bytes, 256-B aligned): xf, the STHT rows and the band-passed rows [F * B][2M][Ts]
 *   each, the chunk sums, and band_power when the caller passes NULL.
 *   Status, before any launch and in this order: MICLOC_ERR_INVALID for NULL (plans, a plan, coefficients, x, both of power /
 *   argmax), F outside 1..MICLOC_MAX_BANDS, fb_n outside 1..MICLOC_MAX_IIR, a_f[0] == 0, B or F * B outside 1..65535, T < 1, window
 *   or hop < 0; MICLOC_ERR_NOT_SET for a plan without bf_mat; MICLOC_ERR_SHAPE for a real bf_mat, plans on different devices, with
 *   different M or G, a different Hilbert kernel or band-pass length, T * M >= 2^32, or (window > 0) a window or hop that is not a
 *   positive multiple of EVERY plan's micloc_window_quantum, or F * B * nW > INT32_MAX; MICLOC_ERR_WORKSPACE for a short or
 *   misaligned ws.  hop == 0 means hop = window.
 * micloc_beamformer_bands_bandpass_f64 is stages (2) and (3) alone, for tests and measurements: xf [F][B][T][M] -> h, pre
 * [F * B][2M][Ts] (Ts = micloc_padded_T(T); the in-phase rows of h are not written; frames [T, Ts) of pre are zero with
 * one_launch != 0 and unspecified with one_launch == 0, which takes the one-shot band-pass launch per band instead of (3)).
 * with_stht == 0 skips (2): the quadrature rows of h are the caller's.  The plans need no bf_mat; the checks are those above that
 * do not concern it. */
size_t micloc_beamformer_bands_workspace_bytes(const micloc_plan *const *plans, int F, int B, int T, int window, int hop); /* 0 on bad arguments */
int micloc_beamformer_pipeline_bands_f64(const micloc_plan *const *plans, int F, const double *fb_b, const double *fb_a, int fb_n,
                                         const double *x, int B, int T, int window, int hop, /* window 0: whole recording */
                                         double *band_power /* [F][R][G] or NULL */, double *power, int32_t *argmax, void *ws, size_t ws_bytes,
                                         void *stream);
int micloc_beamformer_bands_bandpass_f64(const micloc_plan *const *plans, int F, const double *xf, int B, int T, double *h, double *pre, int Ts,
                                         int with_stht, int one_launch, void *stream);

/* ---- wideband moving-target tracking: a DoA per frame over all bands ---------------------------- */
/* "moving-target tracking" above for the wideband localizers: the per-frame read-out of F bands (1 <= F <= MICLOC_MAX_BANDS) whose
 * plans agree in device, M and G, all with a real bf_mat and a neuron kernel (the snn / lif entries) or all with a complex bf_mat (the
 * beamformer / c128 entries).  The rule, for trial b, bands f = 0 .. F-1 in ascending order, frame t, DoA column g:
 *   y_f[t][g]  the beamformer output of band f: exactly the value band f's own chain stores for its filterbank output xf[f] when y is
 *              kept (micloc_lif_beamform_f64 / micloc_beamform_c128_f64 with plans[f]: same instruction sequence, same bits);
 *   a_f[t][g]  = |y_f[t][g]|  (real: fabs; complex: hypot(re, im), the device library's, as MICLOC_ENV_C128);
 *   m[t][g]    = a_0[t][g], then m = m + a_f for f = 1 .. F-1: one addition per band, rounded to nearest, nothing fused, ascending
 *              band order.  Magnitudes are added, not powers: with F = 1 the call IS the single-plan tracking entry on xf[0];
 *   e, index, peak_env, env_last: the rule of "moving-target tracking" on m, unchanged -- e[0] = m[0]; rise when m[t] >= e[t-1]; two
 *              rounded products and one rounded sum; the first maximum over g; a NaN never wins; a row of NaN only gives index 0 and
 *              peak NaN.
 * Sets in which every plan is one the fused kernels serve (micloc_track_is_fused() == 1) and whose workgroup, sized for the largest
 * neuron kernel, fits in 160 KB of LDS (micloc_*_bands_track_is_fused() == 1) run ONE kernel of csrc/track.hip over all bands (and the
 * combine launch when G > 64): no y, m or e is stored, and the workspace -- xf, the front end's arrays, every band's raster or planar
 * rows, one (value, index) pair per frame and 64 DoA columns -- depends on G through the pairs alone.  Other sets run the two-step
 * route inside the call over sub-batches of trials: per band y stored, m formed by the rule above, the envelope kernel on m, a row
 * read-out; the minimum workspace holds y, m and e of ONE trial, and a caller that passes more has as many trials per sub-batch as fit.
 * The results do not depend on the route or the sub-batches.
 *   micloc_snn_pipeline_bands_track_f64: the filterbank of "wideband localisation", per band the first two launches of
 *   micloc_snn_pipeline_f64 on xf[f] (the bands share the STHT rows and the encoder scratch: they run one after the other), the read-out.
 *   micloc_beamformer_pipeline_bands_track_f64: launches (1) to (3) of micloc_beamformer_pipeline_bands_f64, the read-out.
 *   micloc_lif_beamform_bands_track_f64 / micloc_beamform_c128_bands_track_f64: the read-out alone, of the caller's rasters
 *   [F][B][T][2M] int8 / planar band-passed rows [F * B][2M][Ts], Ts = micloc_padded_T(T).
 * Status, before any launch: MICLOC_ERR_INVALID for NULL (plans, a plan, coefficients, the input, index), F outside
 * 1..MICLOC_MAX_BANDS, fb_n outside 1..MICLOC_MAX_IIR, a_f[0] == 0, B or F * B outside 1..65535; MICLOC_ERR_SHAPE for T < 1 or
 * B * T > 2^31 - 1 (both without reading a plan); MICLOC_ERR_NOT_SET for a plan without bf_mat or (real) neuron kernel;
 * MICLOC_ERR_SHAPE for plans on different devices, with different M or G, a bf_mat of the other kind, (complex) a different Hilbert
 * kernel or band-pass length or T * M >= 2^32, a Ts that is not micloc_padded_T(T); MICLOC_ERR_WORKSPACE for a missing, misaligned or
 * short ws.  The size functions return 0 for arguments the calls refuse; the is_fused functions return 1, 0 or a status code < 0.
 * No atomics, no host synchronisation, no allocation: re-entrant per stream with workspaces of their own and capturable in a
 * hipGraph (a straight chain on ONE stream). */
size_t micloc_snn_bands_track_workspace_bytes(const micloc_plan *const *plans, int F, int B, int T);
size_t micloc_beamformer_bands_track_workspace_bytes(const micloc_plan *const *plans, int F, int B, int T);
int micloc_snn_bands_track_is_fused(const micloc_plan *const *plans, int F);
int micloc_beamformer_bands_track_is_fused(const micloc_plan *const *plans, int F);
int micloc_lif_beamform_bands_track_f64(const micloc_plan *const *plans, int F, const int8_t *spikes, int B, int T, double a_rise,
                                        double i_rise, double a_fall, int32_t *index, double *peak_env, double *env_last, void *ws,
                                        size_t ws_bytes, void *stream);
int micloc_beamform_c128_bands_track_f64(const micloc_plan *const *plans, int F, const double *pre, int B, int T, int Ts, double a_rise,
                                         double i_rise, double a_fall, int32_t *index, double *peak_env, double *env_last, void *ws,
                                         size_t ws_bytes, void *stream);
int micloc_snn_pipeline_bands_track_f64(const micloc_plan *const *plans, int F, const double *fb_b, const double *fb_a, int fb_n,
                                        const double *x, int B, int T, double a_rise, double i_rise, double a_fall, int32_t *index,
                                        double *peak_env /* [B][T] or NULL */, double *env_last /* [B][G] or NULL */, void *ws,
                                        size_t ws_bytes, void *stream);
int micloc_beamformer_pipeline_bands_track_f64(const micloc_plan *const *plans, int F, const double *fb_b, const double *fb_a, int fb_n,
                                               const double *x, int B, int T, double a_rise, double i_rise, double a_fall, int32_t *index,
                                               double *peak_env /* [B][T] or NULL */, double *env_last /* [B][G] or NULL */, void *ws,
                                               size_t ws_bytes, void *stream);

/* ---- wideband streaming: filterbank state carry, band sum per tile ------------------------------ */
/* The wideband chain above for ONE stream that arrives in tiles: the results after the last tile are bit for bit those of
 * micloc_snn_pipeline_bands_f64 on the whole recording, for any tiling.  One tile of n frames, every launch on the caller's one
 * stream in this order (nothing side by side: a captured tile is a chain of nodes), no allocation, no host synchronisation, no
 * atomics, no argument that depends on absolute time:
 *   micloc_filterbank_tile_f64      x_tile [B][n][M] -> xf_tile [F][B][n][M], n >= 1 of any length
 *   per band f in ascending order   the tile sequence of "streaming" above (begin_tile .. localize_tile[_windows]) of plans[f] on
 *                                   xf_tile[f], with that band's own states, raster window, running power and window ring
 *   micloc_stream_band_sum_f64      the running band sum and the wideband windows every band has emitted
 *   Filterbank tile.
 *   - The arithmetic is the filterbank's DF2T step unchanged; the state of every (band, trial, microphone) chain is read from and
 *     written back to fb_state, so a stream cut into tiles at any frames performs exactly the operations of one
 *     micloc_filterbank_f64 call on the whole recording: xf is bit-identical.
 *   - fb_state: micloc_filterbank_stream_state_bytes(F, n_coef, B, M) bytes, 256-B aligned, zero-filled once by
 *     micloc_filterbank_stream_reset: F B M (n_coef - 1) doubles rounded up to 256 B (at least 256 B), laid out
 *     [B][n_coef - 1][F][M] -- word i of chain (f, b, m) at ((b (n_coef - 1) + i) F + f) M + m -- so that the chain lanes of a
 *     workgroup (band-major over the trial's microphones) touch consecutive addresses for every i.  Loaded once before the tile's
 *     first frame, stored once after its last.
 *   - Status, before any launch: as micloc_filterbank_f64 (MICLOC_ERR_INVALID for NULL, F outside 1..MICLOC_MAX_BANDS, n outside
 *     1..MICLOC_MAX_IIR, a_f[0] == 0, B, n_frames or M < 1); MICLOC_ERR_WORKSPACE for a short or misaligned fb_state.
 *   Band sum, running read-out.
 *   - power[b][g] = ((p_0[b][g] + p_1[b][g]) + p_2[b][g]) + ... over the bands' running power [B][G] (band_power: a HOST array of F
 *     device pointers; they travel by value in the kernel argument), ascending band order from p_0, every addition rounded to
 *     nearest; argmax by micloc_band_sum_f64's rule.  Before the last tile this is the running estimate -- each band's power is
 *     over the frames THAT band has beamformed so far, which can differ between bands; after the last tile it is bit for bit the
 *     one-shot power / argmax.  power or argmax may be NULL, not both.
 *   Band sum, windows (window > 0; window == 0: the running read-out only and the window arguments are ignored).
 *   - Every band emits its own windows into a ring band_window_power[f] [B][Kb][G] (its micloc_stream_localize_tile_windows_f64
 *     called with max_windows = Kb: window n in row n % Kb) and counts them in the device word band_window_count[f]
 *     (micloc_stream_window_count_ptr of its win_state); both are HOST arrays of F device pointers.  Bands finish a window at
 *     different calls: their horizons depend on their own open clusters.
 *   - Wideband window n is emitted by the first band-sum launch after which every band has emitted window n: after a launch,
 *     min_f count_f windows have been emitted, in ascending n, window n into row n % max_windows of window_power
 *     [B][max_windows][G] (may be NULL) and window_argmax [B][max_windows]; latest_power [B][G] / latest_argmax [B] (may be NULL)
 *     take the most recently emitted window and are untouched until the first one exists.
 *   - The value is the ascending band sum of the bands' rows: bit for bit the one-shot window_power / window_argmax.  An emitted row
 *     never changes until window n + max_windows takes its place.
 *   - Ring depth: the windows [emitted, count_f) must still be in band f's ring.  Where count_f - emitted > Kb for some band, the
 *     windows n < max_f count_f - Kb not emitted yet are GIVEN UP: nothing is written for them, they are added to the failure count
 *     and to the emitted count (emission goes on behind them); a row that holds a later window is never summed.
 *   - window and hop are multiples of every band's micloc_stream_chunk_frames (checked by the bands' own calls).
 *   State: bands_state (micloc_stream_bands_state_bytes, 256-B aligned, zero-filled once by micloc_stream_bands_reset): the count of
 *   windows emitted or given up and the count given up.  The launch is followed by a one-thread commit launch that makes the new
 *   counts visible, so every workgroup of a launch reads the same count.  micloc_stream_bands_status: {emitted or given up, given
 *   up}; synchronises the stream.
 *   Status, before any launch: MICLOC_ERR_INVALID for NULL (band_power, an entry of it, bands_state, both of power / argmax; with
 *   window > 0 the two window tables, an entry of them, window_argmax), F outside 1..MICLOC_MAX_BANDS, B outside 1..65535, G < 1,
 *   window < 0, and with window > 0 max_windows < 1 or Kb < 1; MICLOC_ERR_WORKSPACE for a short or misaligned bands_state. */
size_t micloc_filterbank_stream_state_bytes(int F, int n, int B, int M); /* 0 on bad arguments */
int micloc_filterbank_stream_reset(void *fb_state, size_t bytes, void *stream);
int micloc_filterbank_tile_f64(const double *b, const double *a, int F, int n, /* host [F][n] each */
                               const double *x_tile, int B, int n_frames, int M, void *fb_state, size_t fb_bytes, double *xf_tile,
                               void *stream);
size_t micloc_stream_bands_state_bytes(void);
int micloc_stream_bands_reset(void *bands_state, size_t bytes, void *stream);
int micloc_stream_band_sum_f64(int F, int B, int G, const double *const *band_power, int window /* 0: running read-out only */, int Kb,
                               int max_windows, const double *const *band_window_power, const int32_t *const *band_window_count,
                               void *bands_state, size_t bands_bytes, double *power, int32_t *argmax, double *window_power,
                               int32_t *window_argmax, double *latest_power, int32_t *latest_argmax, void *stream);
int micloc_stream_bands_status(const void *bands_state, int *status2, void *stream);
/* device address of the int32 word [0] of micloc_stream_bands_status, the wideband windows emitted or given up (a kernel that follows the
 * wideband windows takes it: "streaming, multi-source" below); valid as long as bands_state is */
const int32_t *micloc_stream_bands_window_count_ptr(const void *bands_state);

/* ---- wideband streaming, complex Beamformer: all bands' tiles in one batch ----------------------- */
/* The chain of "wideband localisation, complex Beamformer" for ONE stream that arrives in tiles.  The complex chain has no encoder
 * state and no horizon, so all bands advance in lock step: a stream of F bands x B recordings is one complex stream ("streaming, complex
 * Beamformer" above) of F * B rows -- row f B + b is band f of recording b -- with per-band band-pass coefficients and per-band bf_mat.
 * The rule, for F plans (1 <= F <= MICLOC_MAX_BANDS) with complex bf_mats that agree in device, M, G, Hilbert kernel and band-pass length,
 * filterbank coefficients [F][n], a recording x [B][T][M] and any cut of T into tiles of any lengths >= 1:
 *   Results.
 *   - After the final tile band_power [F][B][G], power [B][G] and argmax [B] equal micloc_beamformer_pipeline_bands_f64 on the whole
 *     recording bit for bit.
 *   - With window / hop (multiples of CH = micloc_window_quantum, 1 <= hop <= window) every emitted wideband window has the bits of that
 *     entry's windows form.  Emission time, ring row n % max_windows, latest_* and "an emitted row never changes" are those of "streaming
 *     windows" above.  power = ((p_0 + p_1) + p_2) + ... in ascending band order from p_0, every addition rounded to nearest; the
 *     arg-max is the first maximum, a NaN never wins, a row of NaN gives 0.
 *   - Before the final tile band f's power is the running read-out of "streaming, complex Beamformer" (the mean over the whole chunks
 *     contracted so far; the same frames for every band) and power is their band sum.
 *   - Nothing allocates, synchronises with the host, uses atomics or takes an absolute time.  A tile of n frames is ONE chain of launches
 *     on the caller's stream with no parallel branches: one capturable hipGraph per tile length.
 *   One tile of n <= max_tile frames, in this order:
 *     micloc_filterbank_tile_f64                         x_tile [B][n][M] -> xf_tile [F][B][n][M] ("wideband streaming" above)
 *     micloc_stht_f64, micloc_stream_wrap_rows_f64       by the caller with plans[0] over the F * B trials of [last L - 1 FILTERED frames |
 *                                                        xf_tile]; the wrap rows are those of every band's filtered recording,
 *                                                        [F][B][L/2][M]; `state` serves as loc_state
 *     micloc_stream_complex_bands_bandpass_tile_f64      h [F B][2M][row_stride] -> staging: ONE launch over the F * B * 2M chains, band
 *                                                        g / (B 2M) of chain g with plans[f]'s coefficients; the DF2T steps, the state
 *                                                        words (word i of chain g at i F B 2M + g), the carry and the zero padding of
 *                                                        micloc_stream_complex_bandpass_tile_f64.  Against the rows of
 *                                                        micloc_beamformer_bands_bandpass_f64 on the whole recording only the sign of a
 *                                                        zero may differ.  chains_per_workgroup: 0 (the launcher's choice by chain
 *                                                        count) or 16 / 32 / 64 (tests, measurements): the bits do not depend on it
 *     micloc_stream_complex_bands_localize_tile[_windows]_f64
 *                                                        per band in ascending order the contraction of that band's bf_mat on its B rows
 *                                                        of the staging array into one array of chunk rows [F B][Ks][Gp]; then ONE
 *                                                        accumulate, (ONE window read-out,) ONE slide + clock commit over the F * B rows
 *                                                        -- the kernels of the complex stream, unchanged; then the band sum of "wideband
 *                                                        streaming" (followed, with windows, by its one-thread commit)
 *   with the same max_tile, state and ws in both calls: 6 + F launches, 8 + F with windows.  band_power, power and argmax may be NULL.
 *   Windows.  The bands complete every window in the same tile.  Band f's windows go to a ring [B][Kb][G] inside win_state, window n in row
 *   n % Kb, all bands counted by the one count word of the window state; the band sum then emits the windows [emitted, count).  Kb =
 *   ceil(Ks / (hop / CH)) + 1: a tile contracts at most Ks = ceil((max_tile + CH - 1) / CH) chunk rows, r chunk rows complete at most
 *   ceil(r / (hop / CH)) windows, and on the final tile at most ONE more window is cut at the end of the recording.  So count - emitted
 *   <= Kb always and no window is ever given up.  micloc_stream_window_count(win_state) is the number of wideband windows emitted.
 *   State and footprint.  state (micloc_stream_complex_bands_state_bytes; zero-filled once by _reset): the complex stream's layout for
 *   F * B rows.  ws (_workspace_bytes; pure scratch): staging [F B][2M][Ks CH], chunk rows [F B][Ks][Gp], running band power [F B][G].
 *   win_state (_window_state_bytes; zero-filled once by _window_reset): the window state of F * B rows, whose 256-B head also holds the
 *   band sum's counts, and the band ring [F B][Kb][G].  All 256-B aligned; none grows with the stream.  The filterbank state is the
 *   caller's (micloc_filterbank_stream_state_bytes).
 *   micloc_stream_complex_bands_status: {chunks contracted, frames contracted, carry fill, frames pushed, wideband windows emitted or
 *   given up, windows given up}; win_state may be NULL (the last two are then 0); it synchronises the stream.
 *   Status, before any launch and in this order: MICLOC_ERR_INVALID for NULL (plans, a plan, h, state, ws, win_state, window_argmax),
 *   F outside 1..MICLOC_MAX_BANDS, B or F * B outside 1..65535, n, max_tile or row_stride < 1, first_col < 0, a chains_per_workgroup other
 *   than 0, 16, 32, 64, window, hop or max_windows < 1; MICLOC_ERR_NOT_SET for a plan without bf_mat; MICLOC_ERR_SHAPE for a real bf_mat,
 *   plans on different devices, with different M or G, a different Hilbert kernel or band-pass length, a window or hop that is not a
 *   multiple of CH, hop > window, n > max_tile or first_col + n > row_stride; MICLOC_ERR_WORKSPACE for a short or misaligned state, ws
 *   or win_state.  The size functions return 0 for such arguments. */
size_t micloc_stream_complex_bands_state_bytes(const micloc_plan *const *plans, int F, int B);
size_t micloc_stream_complex_bands_workspace_bytes(const micloc_plan *const *plans, int F, int B, int max_tile);
int micloc_stream_complex_bands_reset(const micloc_plan *const *plans, int F, int B, void *state, size_t state_bytes, void *stream);
int micloc_stream_complex_bands_bandpass_tile_f64(const micloc_plan *const *plans, int F, const double *h, int B, int n, int row_stride,
                                                  int first_col, int max_tile, int chains_per_workgroup, void *state, size_t state_bytes,
                                                  void *ws, size_t ws_bytes, void *stream);
int micloc_stream_complex_bands_localize_tile_f64(const micloc_plan *const *plans, int F, void *state, size_t state_bytes, int B,
                                                  int max_tile, int final_tile, double *band_power, double *power, int32_t *argmax,
                                                  void *ws, size_t ws_bytes, void *stream);
size_t micloc_stream_complex_bands_window_state_bytes(const micloc_plan *const *plans, int F, int B, int max_tile, int window, int hop,
                                                      int max_windows);
int micloc_stream_complex_bands_window_reset(const micloc_plan *const *plans, int F, int B, int max_tile, void *win_state, size_t win_bytes,
                                             int window, int hop, int max_windows, void *stream);
int micloc_stream_complex_bands_localize_tile_windows_f64(const micloc_plan *const *plans, int F, void *state, size_t state_bytes, int B,
                                                          int max_tile, int final_tile, double *band_power, double *power,
                                                          int32_t *argmax, void *ws, size_t ws_bytes, void *win_state, size_t win_bytes,
                                                          int window, int hop, int max_windows, double *window_power,
                                                          int32_t *window_argmax, double *latest_power, int32_t *latest_argmax,
                                                          void *stream);
int micloc_stream_complex_bands_status(const void *state, const void *win_state, int *status6, void *stream);
/* device address of the int32 word [4] of micloc_stream_complex_bands_status, the wideband windows emitted or given up ("streaming,
 * multi-source" below); NULL for a NULL win_state; valid as long as win_state is */
const int32_t *micloc_stream_complex_bands_window_count_ptr(const void *win_state);

/* ---- wideband streaming, tracking: a DoA per frame over all bands while the recording arrives ---- */
/* The rule of "wideband moving-target tracking" for a recording that arrives tile by tile through one of the two wideband streams above.
 *   Values.  The rows emitted for frame t of trial b are index[b][t] and peak_envelope[b][t] of "wideband moving-target tracking": the
 *   bands' magnitudes |y_f| added with one rounded add per band in ascending band order, the envelope, the first maximum and the NaN rule
 *   of "moving-target tracking".  The stream is that call on the whole recording, bit for bit, for any tiling; after the last tile the
 *   first G columns of every trial's state row equal env_last.
 *   When a frame is final.
 *   - Complex bands advance in lock step as ONE complex stream of F * B rows: a frame is final when its tile has been band-passed, as in
 *     "streaming, tracking".  The range of a tile comes from that stream's control words (carry fill, tile length, clock).
 *   - SNN bands have a horizon each and finish chunks at different pushes: a frame is final when the chunk that holds it has been
 *     beamformed by EVERY band.  The tracked frontier after a tile is min(min_f done_f * CH, t_end), done_f = band f's committed chunk
 *     count, CH the bands' one chunk length, t_end the frames pushed; a tile tracks the frames from the previous frontier to the new one.
 *     The frontier is a word of the tracked state of its own, in absolute frames -- not derived from any one band's range words.  The
 *     words are written by one thread of a small launch in front of the tracking launch; no launch argument depends on time.
 *   Why the rows are still there (SNN).  The bands share window_frames and CH, so their raster windows share the base schedule (the
 *   stream's clock depends on the tile sizes only).  A band without a lag failure keeps chunk done_f - 1 in its window (the slide's
 *   check).  The frontier is at most done_f * CH for every f, hence the chunk in front of the frontier is in every band's window, and the
 *   LIF history 4 NK_f - 16 <= CH of every band with it.  A band's lag failure stops that band's done_f and with it the frontier: no
 *   wrong row is emitted, and micloc_stream_localize_status reports the failure as it does without tracking.
 *   Ring, latest words, scratch: as in "streaming, tracking".  max_track is at least what a tile can make final: window_frames (SNN),
 *   max_tile (complex).  track_state (micloc_stream_bands_track_state_bytes, zero-filled once by micloc_stream_bands_track_reset) is a
 *   256-byte head that holds the frontier words, then [B][ceil(G / 64) * 64] doubles; track_ws is scratch of
 *   micloc_stream_bands_track_workspace_bytes (its last argument: window_frames for SNN bands, max_tile for complex ones).  Nothing grows
 *   with the stream and nothing of size T x G exists.
 *   Who is served.  A set that is fused by micloc_snn_bands_track_is_fused / micloc_beamformer_bands_track_is_fused (the kind is that of
 *   plans[0]'s bf_mat); SNN sets also need one chunk length and 4 NK_f - 16 <= CH in every band, complex sets what "wideband streaming,
 *   complex Beamformer" asks of a set.  The two-step route has no streaming form.
 *   Entries.  micloc_stream_bands_track_tile_f64 (SNN) is called once per tile BEHIND the last band's micloc_stream_localize_tile[_windows]_f64
 *   (its commit and tick included) and in front of or behind micloc_stream_band_sum_f64, with which it shares no word; loc_states[f] /
 *   windows[f] are band f's loc_state and raster window.  It launches the frontier kernel, the tracking kernel and (G > 64) the combine.
 *   micloc_stream_complex_bands_localize_tile_track_f64 is micloc_stream_complex_bands_localize_tile[_windows]_f64 with the tracking
 *   launch (and its combine) in front of the slide; it takes the window arguments as micloc_stream_complex_localize_tile_track_f64 does:
 *   with win_state == NULL there is no window read-out.  band_power, power, argmax and the window rows keep the bits of the entries
 *   without tracking.  micloc_stream_bands_track_status gives the SNN frontier in frames (it synchronises the stream); the complex
 *   frontier is the frames pushed of micloc_stream_complex_bands_status.
 *   Status, before any launch and in this order: MICLOC_ERR_INVALID (NULL plans, a NULL plan, loc_state, window, track_state or result
 *   buffer, F, B, window_frames / max_tile or max_track out of range) / MICLOC_ERR_NOT_SET as everywhere; MICLOC_ERR_SHAPE for a set that
 *   is not served, a set of the other kind, window_frames that is no multiple of CH, or max_track below what a tile can make final;
 *   MICLOC_ERR_WORKSPACE for a missing, misaligned or short state / scratch.  The size functions return 0 for a set that is not served. */
size_t micloc_stream_bands_track_state_bytes(const micloc_plan *const *plans, int F, int B);
size_t micloc_stream_bands_track_workspace_bytes(const micloc_plan *const *plans, int F, int B, int frames);
int micloc_stream_bands_track_reset(const micloc_plan *const *plans, int F, int B, void *track_state, size_t track_bytes, void *stream);
int micloc_stream_bands_track_tile_f64(const micloc_plan *const *plans, int F, const void *const *loc_states, const int8_t *const *windows,
                                       int B, int window_frames, void *track_state, size_t track_bytes, double a_rise, double i_rise,
                                       double a_fall, int max_track, int32_t *track_index, double *track_peak, int32_t *latest_index,
                                       double *latest_peak, void *track_ws, size_t track_ws_bytes, void *stream);
int micloc_stream_complex_bands_localize_tile_track_f64(const micloc_plan *const *plans, int F, void *state, size_t state_bytes, int B,
                                                        int max_tile, int final_tile, double *band_power, double *power, int32_t *argmax,
                                                        void *ws, size_t ws_bytes, void *win_state, size_t win_bytes, int window, int hop,
                                                        int max_windows, double *window_power, int32_t *window_argmax,
                                                        double *latest_power, int32_t *latest_argmax, void *track_state,
                                                        size_t track_bytes, double a_rise, double i_rise, double a_fall, int max_track,
                                                        int32_t *track_index, double *track_peak, int32_t *latest_index,
                                                        double *latest_peak, void *track_ws, size_t track_ws_bytes, void *stream);
int micloc_stream_bands_track_status(const void *track_state, int *frontier, void *stream);

/* ---- MUSIC baseline beamformer (micloc/music_beamformer.py) ----------------------------------- */
/* MUSIC.apply_to_signal for a batch of trials: x [B][T][M] (device) is cut into S slices, slice s = samples
 * [s hop, min(s hop + L, T)) (the reference's full slices and its leftover one); each slice is band-passed from zero state
 * (lfilter(b, a) with the host coefficients b, a of length n, DF2T as micloc_lfilter_f64), cut into F_s = len_s / N frames and
 * transformed at the in-band bins only: W (device) is [Np][Cp] with Np = N rounded up to 64, Cp = 2 nbin rounded up to 16,
 * W[n][2j] = cos(2 pi ((k_j n) mod N) / N), W[n][2j + 1] = -sin(...) for bin k_j, zero elsewhere.  Bin power = mean over
 * (mic, frame) of |X|^2; the k strongest bins are taken in np.argsort order (ascending power, exact ties: the later bin sorts
 * later; a NaN power sorts behind every number, NaNs among themselves by bin as well -- a total order, so sel always holds ksel
 * distinct bins in [0, nbin), also for a slice with a NaN or Inf sample, whose bin powers and spectrum row are NaN while the
 * other slices and trials keep their bits); k == 0 or k > nbin takes all.  spec[b][s][g] = sum over those bins of mean_f |a^H X[:, f, bin]|^2 with the steering
 * table steer_re / steer_im [nbin][M][G] (device; a = exp(-1j 2 pi freq delays), conjugated here).  Outputs (device, each may be
 * NULL): sel [B][S][ksel] int32 (the selected in-band bin indices, in order), spec [B][S][G], power [B][G] = mean_s spec^2 and
 * argmax [B] (first maximum).  MICLOC_ERR_SHAPE: a slice shorter than N (the reference's broadcast ValueError) or a slice start
 * outside the signal.  ws from micloc_music_workspace_bytes (256-B aligned); no host synchronisation. */
size_t micloc_music_workspace_bytes(int B, int T, int M, int L, int hop, int S, int N, int nbin, int G, int k);
int micloc_music_f64(const double *x, int B, int T, int M, const double *b, const double *a, int n, int L, int hop, int S, int N,
                     const double *W, int nbin, const double *steer_re, const double *steer_im, int G, int k, int32_t *sel, double *spec,
                     double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream);

/* ---- streaming, MUSIC ---------------------------------------------------------------------------- */
/* "MUSIC baseline beamformer" above for ONE stream of B recordings that arrive in tiles x_tile [B][n][M] of any lengths n >= 1.  A stream
 * is fixed at reset by B, M, L, hop (1 <= hop <= L), N (2 <= N <= L), nbin (<= 4096), G, k (0 or 1 .. nbin) and max_slices; W, the steering
 * table and the filter are those of micloc_music_f64 and are passed with every tile.
 *   Results.  Full slice s = samples [s hop, s hop + L) is emitted by the tile that delivers sample s hop + L - 1; the final tile
 *   (final_tile != 0) also emits the reference's leftover slice, start = (number of full slices) hop, when T - start > L / 2, with its
 *   (T - start) / N frames.  An emitted slice writes its spectrum row [G], its selected bins [ksel] and its first arg-max into row
 *   s % max_slices of slice_spec [B][max_slices][G], slice_sel [B][max_slices][ksel], slice_argmax [B][max_slices], and the newest one of
 *   a tile into latest_spec [B][G], latest_argmax [B]; power [B][G] = (sum over the emitted slices, in ascending order, of spec^2) / their
 *   number and argmax [B] its first maximum, after every tile that emits a slice.  All of them equal micloc_music_f64 on the samples
 *   pushed so far, bit for bit, for every cut into tiles: the band-pass of a slice runs from zero state as the samples arrive, a frame
 *   of N samples is transformed by the tile that completes it, the read-out is a left-to-right sum.  Every output may be NULL.
 *   A leftover slice shorter than N (micloc_music_f64: MICLOC_ERR_SHAPE) is not emitted; status[3] reports it.
 *   Launches.  A tile is cut into pieces of at most hop samples; a piece is four launches (filter, DFT of the completed frames, slice,
 *   read-out + clock) on the caller's stream with no parallel branches.  The sequence depends on n only -- the clock is a device word --
 *   so a tile length is ONE capturable hipGraph (not the final tile: final_tile is an argument).  Nothing allocates, synchronises with
 *   the host or uses atomics; two streams with their own state may run on two HIP streams at once.
 *   State (micloc_stream_music_state_bytes, 256-B aligned, zero-filled by _reset): the clock, 8 DF2T words per (trial, slot, mic), the
 *   frame rows [.. ][Np] and DFT rows [..][Cp] of K = ceil(L / hop) + 1 slots per trial (slice s in slot s % K; one slot more than
 *   slices can be open, so that a slot rests while the kernels behind the filter still read it), sum_s spec^2 [B][G], the slots' spectra
 *   [B][K][G].  It does not grow with the stream.
 *   micloc_stream_music_status: {samples pushed, slices emitted, slices open, 1 after a leftover slice shorter than N}; it synchronises.
 *   Status, before any launch: MICLOC_ERR_INVALID for NULL (state, x_tile, b, a, W, steer_re, steer_im, status), B outside 1..65535, M, L,
 *   hop, nbin, G, max_slices or n < 1, N < 2, k < 0, ncoef outside 1..MICLOC_MAX_IIR, a[0] == 0; MICLOC_ERR_SHAPE for hop > L, N > L,
 *   k > nbin, nbin > N or > 4096, L > 2^28 or more than 2^31 frame rows; MICLOC_ERR_WORKSPACE for a short or misaligned state.  The size
 *   function returns 0 for such arguments. */
size_t micloc_stream_music_state_bytes(int B, int M, int L, int hop, int N, int nbin, int G, int k, int max_slices);
int micloc_stream_music_reset(void *state, size_t state_bytes, int B, int M, int L, int hop, int N, int nbin, int G, int k, int max_slices,
                              void *stream);
int micloc_stream_music_tile_f64(void *state, size_t state_bytes, const double *x_tile, int B, int n, int M, int final_tile, const double *b,
                                 const double *a, int ncoef, int L, int hop, int N, const double *W, int nbin, const double *steer_re,
                                 const double *steer_im, int G, int k, int max_slices, double *power, int32_t *argmax, double *latest_spec,
                                 int32_t *latest_argmax, double *slice_spec, int32_t *slice_sel, int32_t *slice_argmax, void *stream);
int micloc_stream_music_status(const void *state, int *status4, void *stream);
/* device address of the int32 word [1] of micloc_stream_music_status, the slices emitted ("streaming, multi-source" below); NULL for a
 * NULL state; valid as long as state is */
const int32_t *micloc_stream_music_slice_count_ptr(const void *state);

/* ---- streaming, Xylo ----------------------------------------------------------------------------- */
/* The Xylo chain ("Xylo-A2 hidden-layer integer LIF" above: RZCC spikes into the integer LIF layer, rate, peak) for ONE stream of B
 * recordings that arrive in tiles -- the reference's live loop micloc/xylo_snn_localization.py:446-542 without restarting the chain on
 * every pack.  PARITY UNPINNED like every Xylo entry: the LIF equals oracle_xylo_lif bit for bit, the oracle is not checked against XyloSim.
 *   Limits.  The stream is the w_rec == 0 packed form: no recurrent weight (it would couple all bands per step), a bipolar encoder
 *   (ternary raster, Cin = 2 x ternary_channels), Cin <= 64 (at most 16 microphones), any N.
 *   The resumable LIF by value.  state (micloc_xylo_stream_state_bytes, 256-B aligned) holds {isyn, vmem, count0, count1} of every lane
 *   pair, 16 bytes per two neurons, [B][N rounded up to 512 / 2]; micloc_xylo_stream_reset zero-fills it -- zero state and zero counts come
 *   from there, never from the kernel.  micloc_xylo_lif_resume_i16 integrates the frames [t0, t0 + n) of raster int8
 *   [B][trial_stride_frames][ternary_channels] (16-byte aligned) from the state and leaves the state behind them: the counts accumulate
 *   in the state and counts [B][N] is rewritten by every call; n == 0 returns MICLOC_OK and rewrites nothing.  t0 is a multiple of 16,
 *   t0 + n <= trial_stride_frames.  spikes_out (may be NULL) uint8 [B][T_out][N] receives the rows t0 .. t0 + n - 1 (t0 + n <= T_out).
 *   ws / ws_bytes: micloc_xylo_upload's.  Calls over consecutive ranges from a reset state equal micloc_xylo_lif_resident_i16 on the whole
 *   raster bit for bit, for every cut.  No host access, no synchronisation.
 *   One band's stream.  Per band: the plan of its band-pass (no bf_mat, no neuron kernel), the encoder state (micloc_stream_state_bytes),
 *   loc_state (micloc_stream_xylo_state_bytes: the control words and the clock), the raster window int8 [B][window_frames][2M]
 *   (window_frames a multiple of 256), the network (micloc_xylo_upload), lif_state and counts [B][N]; micloc_stream_xylo_reset zeroes all
 *   but the network.  One tile = micloc_stream_xylo_begin_tile (clock, window slide) -> micloc_stht_f64 of [history | tile] ->
 *   micloc_stream_wrap_rows_f64 -> micloc_stream_encode_tile_f64 -> micloc_stream_xylo_tile_i16: the horizon in chunks of 256 frames, the
 *   resumable LIF over the chunks that became final (everything up to the end on the final tile), (the window read-out,) the commit, the
 *   clock's tick.  No call carries an absolute time: a tile length is ONE capturable hipGraph.
 *   micloc_stream_xylo_status: {chunks integrated, frames integrated, window-lag failures, frames pushed}; it synchronises.
 *   Windows (micloc_stream_xylo_tile_windows_i16): window and hop are multiples of 256 frames, hop <= window; the rule of "streaming
 *   windows" above -- window n = frames [n hop, n hop + window), emitted when its last chunk is integrated, on the final tile also the
 *   windows of micloc_window_count that the end of the recording cuts.  The band's emitted windows (per-neuron counts, exact integers) go
 *   to row n % ring_depth of a ring inside win_state (micloc_stream_xylo_window_state_bytes; _window_reset zero-fills it); ws
 *   (micloc_stream_xylo_workspace_bytes) holds the per-chunk counts of a tile and may be shared by bands that run one after the other.  The
 *   network state is NOT reset between windows: one stream is one continuous run of the network.
 *   Read-out over the bands (micloc_stream_xylo_readout, behind the tiles of all F bands): counts [B][F G] (band f's neurons at f G ..),
 *   rate[b][g] = mean over the bands of counts_f[b][g] / frames_f * fs -- micloc_rate_from_counts_f64's expression and band order, frames_f
 *   the frames band f has integrated so far -- and peak[b] as micloc_peak_location_i32 computes it (win_size odd, <= G / 2).  Mid-stream
 *   each band is read over the frames IT has integrated; after the final tile every frames_f is T and rate / peak equal the one-shot
 *   calls on the one-shot counts bit for bit.  window > 0: a window is emitted once every band has emitted it, from the bands' rings:
 *   window n in row n % max_windows of window_counts [B][max_windows][F G], window_rate [B][max_windows][G] (over the frames the window
 *   holds) and window_peak [B][max_windows], the newest one also in latest_* (each may be NULL); a window that a band's ring has
 *   overwritten by then is counted as given up instead.  micloc_stream_xylo_readout_status: {windows emitted or given up, given up}.
 *   Status, before any launch: MICLOC_ERR_INVALID for NULL or out-of-range arguments (B outside 1..65535, N, n, window_frames, max_spikes,
 *   ring_depth, max_windows < 1, t0 or n < 0, F outside 1..MICLOC_MAX_BANDS, fs <= 0, a win_size micloc_peak_location_i32 refuses);
 *   MICLOC_ERR_SHAPE for t0 % 16 != 0, Cin != 2 * ternary_channels, Cin > 64, a range past trial_stride_frames or T_out, a raster that is
 *   not 16-byte aligned, a unipolar plan, window_frames, window or hop that is no multiple of 256, hop > window, n > window_frames, G > 4096
 *   in the read-out; MICLOC_ERR_WORKSPACE for a short or misaligned buffer.  The size functions return 0 for such arguments. */
size_t micloc_xylo_stream_state_bytes(int B, int N);
int micloc_xylo_stream_reset(void *state, size_t state_bytes, void *stream);
int micloc_xylo_lif_resume_i16(const int8_t *raster, int ternary_channels, int trial_stride_frames, int B, int t0, int n, int Cin, int N,
                               int max_spikes, uint8_t *spikes_out, int T_out, int32_t *counts, void *state, size_t state_bytes, void *ws,
                               size_t ws_bytes, void *stream);
size_t micloc_stream_xylo_state_bytes(void);
size_t micloc_stream_xylo_workspace_bytes(int B, int N, int window_frames);
int micloc_stream_xylo_reset(const micloc_plan *p, int B, void *enc_state, size_t enc_bytes, void *loc_state, size_t loc_bytes, int8_t *window,
                             int window_frames, int N, void *lif_state, size_t lif_bytes, int32_t *counts, void *stream);
int micloc_stream_xylo_begin_tile(const micloc_plan *p, void *loc_state, int8_t *window, int8_t *scratch_window, int B, int n, int window_frames,
                                  void *stream);
int micloc_stream_xylo_tile_i16(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window, int B,
                                int window_frames, int final_tile, int N, int max_spikes, int32_t *counts, void *lif_state, size_t lif_bytes,
                                void *net_ws, size_t net_ws_bytes, void *stream);
size_t micloc_stream_xylo_window_state_bytes(int B, int N, int window, int hop, int ring_depth);
int micloc_stream_xylo_window_reset(void *win_state, size_t win_bytes, int B, int N, int window, int hop, int ring_depth, void *stream);
int micloc_stream_xylo_tile_windows_i16(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window_raster,
                                        int B, int window_frames, int final_tile, int N, int max_spikes, int32_t *counts, void *lif_state,
                                        size_t lif_bytes, void *net_ws, size_t net_ws_bytes, void *ws, size_t ws_bytes, void *win_state,
                                        size_t win_bytes, int window, int hop, int ring_depth, void *stream);
int micloc_stream_xylo_status(const void *loc_state, int *status4, void *stream);
size_t micloc_stream_xylo_readout_state_bytes(void);
int micloc_stream_xylo_readout_reset(void *ro_state, size_t ro_bytes, void *stream);
int micloc_stream_xylo_readout(int F, int B, int G, double fs, int win_size, const int32_t *const *band_counts, const void *const *band_loc_state,
                               int window, int hop, int ring_depth, int max_windows, void *const *band_win_state, void *ro_state, size_t ro_bytes,
                               int32_t *counts, double *rate, int32_t *peak, int32_t *window_counts, double *window_rate, int32_t *window_peak,
                               int32_t *latest_counts, double *latest_rate, int32_t *latest_peak, void *stream);
int micloc_stream_xylo_readout_status(const void *ro_state, int *status2, void *stream);

/* ---- streaming, Xylo tracking: a DoA per frame from the Xylo chain while the recording arrives --- */
/* "Xylo moving-target tracking" above for a recording that arrives tile by tile ("streaming, Xylo"): every frame the integer LIF
 * integrates in a call is EMITTED by that call -- its neuron (DoA) index and its peak envelope written -- and the emitted rows equal, bit
 * for bit, index / peak_env of micloc_xylo_lif_track_i16 on the whole raster, whatever the cuts; behind the last frame env_last and counts
 * equal its env_last and rate.  PARITY UNPINNED like every Xylo entry: the LIF equals oracle_xylo_lif bit for bit, the oracle is not
 * checked against XyloSim.  The rule, in full, for every trial b and neuron n independently, t the ABSOLUTE frame of the recording:
 *   c[t][n]   the spike count of step t, exactly the value micloc_xylo_lif_resident_i16 stores in spikes_out (the second spike within a
 *             step and the max_spikes cap included);   m[t][n] = (double)c[t][n];
 *   e[0][n]   = m[0][n];   for t >= 1:  rise = m[t][n] >= e[t-1][n];
 *   e[t][n]   = rise ? a_rise * e[t-1][n] + i_rise * m[t][n] : a_fall * e[t-1][n]      -- two rounded products, one rounded sum,
 *             nothing fused; a_rise = 1 - 1/w_rise, i_rise = 1/w_rise, a_fall = 1 - 1/w_fall as NumPy computes them (w >= 1);
 *   index of frame t    = the FIRST n in [0, N) with e[t][n] = max_n e[t][n]  (counts are integers, so a row always has a winner);
 *   peak of frame t     = that value.
 *   - Frame 0.  e[0] = m[0] is taken where the ABSOLUTE frame is 0: t0 == 0 by value; in a band's stream where the clock words of
 *     loc_state say so (the base of the raster window, written by micloc_stream_xylo_begin_tile, plus the position in the window).
 *     Position 0 of a raster window that has slid is NOT frame 0.  No flag that the kernel writes for itself is read.
 *   - State.  lif_state is "streaming, Xylo"'s, unchanged (micloc_xylo_stream_state_bytes).  track_state holds e[t-1] in front of the
 *     next frame, two doubles per lane pair in lif_state's order: [B][N rounded up to 512 / 2] x {e of the pair's neurons}
 *     (micloc_xylo_stream_track_state_bytes), zero-filled by micloc_xylo_stream_track_reset -- never by the kernel.  Nothing of size
 *     T x N is stored and nothing grows with the stream.
 *   - Where a frame goes.  Frame t of trial b goes to row t % max_track of track_index [B][max_track] int32 / track_peak [B][max_track]
 *     double, the newest frame of the call also to latest_index [B] / latest_peak [B]; env_last [B][N] (e of the newest frame) and counts
 *     [B][N] are rewritten by every call that integrates a frame.  All are required device buffers.  A call that integrates nothing (n ==
 *     0; a tile that makes no chunk final) rewrites nothing.  max_track must be at least what one call can make final: n by value,
 *     window_frames in a stream.
 *   - Scratch.  track_ws (micloc_xylo_stream_track_workspace_bytes(B, N, frames), frames = n by value, window_frames in a stream; 256-B
 *     aligned): 256 bytes up to 512 neurons, where the workgroup of a trial writes the ring itself; beyond that one (value, index) pair
 *     per frame and 512-neuron block, which a second launch combines in ascending block order (a strictly larger value takes over).
 *   micloc_xylo_lif_track_resume_i16: the by-value form beside micloc_xylo_lif_resume_i16 -- the frames [t0, t0 + n) of raster
 *   [B][trial_stride_frames][ternary_channels], t0 a multiple of 16, from lif_state and track_state, which it leaves behind them.
 *   micloc_stream_xylo_tile_track_i16: micloc_stream_xylo_tile_i16's launch sequence with the tracking LIF (and the combine launch) in place
 *   of the counting one -- horizon, tracking LIF, (windows,) commit, tick -- with the window arguments of micloc_stream_xylo_tile_windows_i16:
 *   win_state == NULL (the other window arguments are then not read) means no window read-out.  counts, the window rows and lif_state have
 *   the bits of the entries without tracking.  No launch argument depends on time: a tile stays one capturable sequence; no workgroup waits
 *   for another, no atomics.  micloc_stream_xylo_status' frames integrated count the emitted frames.
 *   Status, before any launch: as the entries without tracking, and MICLOC_ERR_INVALID for a NULL track_state, result buffer or track_ws or
 *   max_track < 1; MICLOC_ERR_SHAPE for max_track below what the call can make final; MICLOC_ERR_WORKSPACE for a short or misaligned
 *   track_state / track_ws.  The size functions return 0 for bad arguments and never for valid ones. */
size_t micloc_xylo_stream_track_state_bytes(int B, int N);
size_t micloc_xylo_stream_track_workspace_bytes(int B, int N, int frames);
int micloc_xylo_stream_track_reset(void *track_state, size_t track_bytes, int B, int N, void *stream);
int micloc_xylo_lif_track_resume_i16(const int8_t *raster, int ternary_channels, int trial_stride_frames, int B, int t0, int n, int Cin, int N,
                                     int max_spikes, void *lif_state, size_t lif_bytes, void *track_state, size_t track_bytes, double a_rise,
                                     double i_rise, double a_fall, int max_track, int32_t *track_index, double *track_peak, int32_t *latest_index,
                                     double *latest_peak, double *env_last, int32_t *counts, void *ws, size_t ws_bytes, void *track_ws,
                                     size_t track_ws_bytes, void *stream);
int micloc_stream_xylo_tile_track_i16(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window_raster,
                                      int B, int window_frames, int final_tile, int N, int max_spikes, int32_t *counts, void *lif_state,
                                      size_t lif_bytes, void *net_ws, size_t net_ws_bytes, void *ws, size_t ws_bytes, void *win_state,
                                      size_t win_bytes, int window, int hop, int ring_depth, void *track_state, size_t track_bytes, double a_rise,
                                      double i_rise, double a_fall, int max_track, int32_t *track_index, double *track_peak, int32_t *latest_index,
                                      double *latest_peak, double *env_last, void *track_ws, size_t track_ws_bytes, void *stream);

/* ---- streaming, multi-source: the K strongest peaks per window while the recording arrives -------- */
/* Every stream above ends in ONE arg-max per running row and one per window.  micloc_stream_peaks_tile_f64 is the multi-source read-out
 * ("Multi-source read-out" above: micloc_doa_peaks_f64's rule, grid kinds, limits and outputs, unchanged) as a read-out that FOLLOWS a
 * stream: it is called behind a tile's own read-out entry, on the same stream, and belongs to the tile's graph.  It serves every stream
 * that keeps its windows in a ring window_power [B][max_windows][G] (window n in row n % max_windows) and counts the windows it has
 * emitted in a device word: the SNN and the complex stream (micloc_stream_window_count_ptr), the two wideband streams
 * (micloc_stream_bands_window_count_ptr, micloc_stream_complex_bands_window_count_ptr), the MUSIC stream, whose windows are its slices
 * (micloc_stream_music_slice_count_ptr).  The rule:
 *   Running estimate.
 *   - power [B][G] (may be NULL: skipped) is the stream's running power as it stands after the tile.  On EVERY call peaks [B][K] int32
 *     and peak_power [B][K] (may be NULL) are the multi-source rule applied to its rows.
 *   Windows (window_power != NULL and max_windows > 0; otherwise the running read-out only).
 *   - c = *window_count, the count word after this tile's window read-out.  r = "windows whose peaks are read", word 0 of pk_state.
 *   - For every n in [max(r, c - max_windows), c): row n % max_windows of window_peaks [B][max_windows][K] int32 and of
 *     window_peak_power [B][max_windows][K] (may be NULL) is the multi-source rule applied to row n % max_windows of window_power.
 *   - If c > r, latest_peaks [B][K] and latest_peak_power [B][K] (each may be NULL) take window c - 1; they are untouched otherwise.
 *   - Then r = c, and word 1 of pk_state grows by max(0, c - max_windows - r): the windows whose rows were overwritten before they
 *     were read ("skipped").  A read-out that runs behind every tile of a stream whose ring holds what one tile can emit skips none.
 *   - Rows of windows outside [max(r, c - max_windows), c) are not written.
 *   - Row r of the peak rings is always the rule applied to the bits of row r of window_power as they stand when the read-out runs:
 *     the read-out never looks at anything but the stored row, so a window's peaks are bit for bit micloc_doa_peaks_f64 of its row.
 * The call works for ANY number of new windows -- none, one, more than MICLOC_STREAM_PEAKS_SLOTS, more than max_windows (the final tile
 * of a stream may emit ceil(window / hop) at once): one wave per (trial, window), grid (B, MICLOC_STREAM_PEAKS_SLOTS), a workgroup walks
 * the windows n_lo + slot, n_lo + slot + SLOTS, ...; the running rows ride on the last slot.  No argument depends on time or on the tile.
 * No atomics, no host synchronisation; no workgroup reads a word that another workgroup of the same launch writes -- r and the skipped
 * count are committed by a one-thread launch of their own behind the read-out.  A tile is still ONE capturable hipGraph.
 * State: pk_state, micloc_stream_peaks_state_bytes() = 256 bytes, 256-B aligned, zero-filled once by micloc_stream_peaks_reset.
 * micloc_stream_peaks_status: {windows read, windows skipped}; it synchronises the stream.
 * Status, before any device work: MICLOC_ERR_INVALID for a NULL doa_list, G outside 1 .. 4096, K outside 1 .. 16, a negative (or NaN)
 * min_separation or rel_threshold, an unknown grid kind, max_windows < 0, a bad B, neither a running row nor windows to read, or a
 * missing peaks / window_count / window_peaks for the part selected; MICLOC_ERR_WORKSPACE for a NULL, short or misaligned pk_state. */
#define MICLOC_STREAM_PEAKS_SLOTS 8
size_t micloc_stream_peaks_state_bytes(void); /* 256 */
int micloc_stream_peaks_reset(void *pk_state, size_t pk_bytes, void *stream);
int micloc_stream_peaks_tile_f64(const double *power, const double *window_power, const int32_t *window_count, int B, int G,
                                 int max_windows, const double *doa_list, int grid_kind, int K, double min_separation,
                                 double rel_threshold, void *pk_state, size_t pk_bytes, int32_t *peaks, double *peak_power,
                                 int32_t *window_peaks, double *window_peak_power, int32_t *latest_peaks,
                                 double *latest_peak_power, void *stream);
int micloc_stream_peaks_status(const void *pk_state, int *status2, void *stream); /* {windows read, windows skipped}; synchronises */

/* ---- misc ------------------------------------------------------------------------------------- */
int micloc_abi_version(void);
const char *micloc_status_string(int status);
int micloc_last_hip_error(void); /* last hipError_t seen by this thread (0 if none) */

#ifdef __cplusplus
}
#endif
#endif /* MICLOC_HIP_H */
