// C-ABI of libmicloc_hip.so (see include/micloc_hip.h for the contract and reference citations): the stand-alone operators, which take
// no plan -- their launches belong to the device of their buffers.
#include "api_internal.h"

using namespace micloc;

extern "C" {

size_t micloc_rzcc_workspace_bytes(int B, int T, int C) { return micloc_rzcc_workspace_bytes_ex(B, T, C, 1, 0); }

size_t micloc_rzcc_workspace_bytes_ex(int B, int T, int C, int robust_width, int chunk_frames)
{
    if (B < 1 || T < 1 || C < 1 || robust_width < 1) return 0;
    const size_t planar = align256((size_t)B * C * micloc_padded_T(T) * sizeof(double));
    return planar + rzcc_scratch_bytes(B * C, T, robust_width, chunk_frames);
}

int micloc_rzcc_encode_f64(const double *sig, int B, int T, int C, int robust_width, int bipolar, int8_t *spikes,
                           void *ws, size_t ws_bytes, void *stream)
{
    return micloc_rzcc_encode_ex_f64(sig, B, T, C, robust_width, bipolar, 0, spikes, ws, ws_bytes, stream);
}

int micloc_rzcc_encode_ex_f64(const double *sig, int B, int T, int C, int robust_width, int bipolar, int chunk_frames,
                              int8_t *spikes, void *ws, size_t ws_bytes, void *stream)
{
    if (!sig || !spikes || bad_batch(B) || T < 1 || C < 1 || robust_width < 1) return MICLOC_ERR_INVALID;
    // (the automatic choice does not depend on robust_width: micloc_rzcc_workspace_bytes(B, T, C) covers chunk_frames 0)
    if (bad_ws(ws, ws_bytes, micloc_rzcc_workspace_bytes_ex(B, T, C, robust_width, chunk_frames))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(spikes));
    const int Ts = micloc_padded_T(T);
    unsigned char *base = reinterpret_cast<unsigned char *>(ws);
    double *planar = reinterpret_cast<double *>(base);
    void *scratch = base + align256((size_t)B * C * Ts * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_pack_planar(sig, planar, B, T, C, Ts, st));
    IirCoef id{};
    id.n = 1;
    id.b[0] = 1.0;  // fma(1, x, +0) == x: the identity filter keeps the stream bit-exact
    id.a[0] = 1.0;
    HIP_TRY(launch_bandpass_rzcc(id, planar, B * C, C, T, Ts, robust_width, bipolar ? 1 : 0, nullptr, spikes, scratch,
                                 st, nullptr, 0, 0, chunk_frames));
    return MICLOC_OK;
}

size_t micloc_lfilter_workspace_bytes(int B, int T, int C)
{
    if (B < 1 || T < 1 || C < 1) return 0;
    return 2 * align256((size_t)B * C * micloc_padded_T(T) * sizeof(double));
}

int micloc_lfilter_f64(const double *b, const double *a, int n, const double *x, int B, int T, int C, double *y,
                       void *ws, size_t ws_bytes, void *stream)
{
    if (!b || !a || !x || !y || n < 1 || n > MICLOC_MAX_IIR || bad_batch(B) || T < 1 || C < 1 || a[0] == 0.0)
        return MICLOC_ERR_INVALID;
    if (bad_ws(ws, ws_bytes, micloc_lfilter_workspace_bytes(B, T, C))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(y));
    const int Ts = micloc_padded_T(T);
    const size_t planar_bytes = align256((size_t)B * C * Ts * sizeof(double));
    unsigned char *base = reinterpret_cast<unsigned char *>(ws);
    double *pin = reinterpret_cast<double *>(base);
    double *pout = reinterpret_cast<double *>(base + planar_bytes);
    IirCoef co{};
    co.n = n;
    for (int i = 0; i < n; ++i) {
        co.b[i] = b[i] / a[0];
        co.a[i] = a[i] / a[0];
    }
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_pack_planar(x, pin, B, T, C, Ts, st));
    HIP_TRY(launch_bandpass_rzcc(co, pin, B * C, C, T, Ts, 1, 0, pout, nullptr, nullptr, st));
    HIP_TRY(launch_unpack_planar(pout, y, B, T, C, Ts, st));
    return MICLOC_OK;
}

// ---- Gram matrix of a planar signal (complex covariance of Beamformer.design_from_template) ------------------------------
size_t micloc_planar_gram_workspace_bytes(int B, int T, int C, int t_start)
{
    if (B < 1 || T < 1 || C < 1 || t_start < 0 || t_start >= T) return 0;
    return align256(planar_gram_partial_bytes(B, T, C, t_start));
}

int micloc_planar_gram_f64(const double *planar, int B, int C, int T, int Ts, int t_start, int normalise, double *gram, void *ws,
                           size_t ws_bytes, void *stream)
{
    if (!planar || !gram || bad_batch(B) || C < 1 || C > 128 || T < 1 || t_start < 0 || t_start >= T) return MICLOC_ERR_INVALID;
    if (Ts < T) return MICLOC_ERR_SHAPE;
    if (bad_ws(ws, ws_bytes, planar_gram_partial_bytes(B, T, C, t_start))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(gram));
    HIP_TRY(launch_planar_gram(planar, B, C, T, Ts, t_start, normalise, gram, reinterpret_cast<double *>(ws), (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- array-signal synthesis (noise-free part of apply_to_template) -------------------------------------------
int micloc_synth_delay_f64(const double *time, const double *sig, const double *slopes, int T, const double *delays,
                           int B, int M, double fs, double *x, void *stream)
{
    if (!time || !sig || !slopes || !delays || !x || T < 2 || bad_batch(B) || M < 1 || !(fs > 0.0)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(x));
    HIP_TRY(launch_synth(time, sig, slopes, T, delays, B, M, fs, x, (hipStream_t)stream));
    return MICLOC_OK;
}

static int synth_args_from_abi(const micloc_synth_args *a, SynthArgs *out)
{
    if (!a || !a->time || !a->sig || !a->slopes || !a->x || a->T < 2 || bad_batch(a->B) || a->K < 1 || a->M < 1 || !(a->fs > 0.0))
        return MICLOC_ERR_INVALID;
    if (a->mode != MICLOC_SYNTH_APPLY_TO_TEMPLATE && a->mode != MICLOC_SYNTH_SIGNAL_FROM_TEMPLATE) return MICLOC_ERR_INVALID;
    if (!a->delays && (!a->doa || !a->r_vec || !a->theta_vec || !(a->speed > 0.0))) return MICLOC_ERR_INVALID;
    SynthArgs k{};
    k.time = a->time;
    k.sig = a->sig;
    k.slopes = a->slopes;
    k.T = a->T;
    k.B = a->B;
    k.K = a->K;
    k.M = a->M;
    k.delays = a->delays;
    k.doa = a->doa;
    k.moving = a->moving ? 1 : 0;
    k.r_vec = a->r_vec;
    k.theta_vec = a->theta_vec;
    k.speed = a->speed;
    k.shift = a->shift;
    k.gain = a->gain;
    k.mode = a->mode;
    k.inv_step = a->fs;
    k.x = a->x;
    *out = k;
    return MICLOC_OK;
}

int micloc_synth_targets_f64(const micloc_synth_args *a, void *stream)
{
    SynthArgs k{};
    const int rc = synth_args_from_abi(a, &k);
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(device_of(a->x));
    HIP_TRY(launch_synth_targets(k, (hipStream_t)stream));
    return MICLOC_OK;
}

size_t micloc_synth_awgn_workspace_bytes(int B, int T, int M, int K)
{
    if (B < 1 || T < 1 || M < 1 || K < 1) return 0;
    return synth_awgn_ws_bytes(B, (size_t)T * M, K, M);
}

int micloc_synth_awgn_f64(const micloc_synth_args *a, const double *snr_db, uint64_t seed, uint32_t substream, const uint32_t *epoch,
                          uint32_t first_trial, void *ws, size_t ws_bytes, void *stream)
{
    SynthArgs k{};
    const int rc = synth_args_from_abi(a, &k);
    if (rc != MICLOC_OK) return rc;
    if (!snr_db) return MICLOC_ERR_INVALID;
    if (((size_t)k.T * k.M + 1) / 2 > 0xFFFFFFFFull || (uint64_t)first_trial + (uint64_t)k.B > 0xFFFFFFFFull) return MICLOC_ERR_INVALID;
    if (bad_ws(ws, ws_bytes, synth_awgn_ws_bytes(k.B, (size_t)k.T * k.M, k.K, k.M))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(a->x));
    HIP_TRY(launch_synth_awgn(k, snr_db, seed, substream, epoch, first_trial, ws, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_delay_min_f64(const double *doa, int B, int K, int moving_T, const double *r_vec, const double *theta_vec, int M,
                         double speed, double *shift, void *stream)
{
    if (!doa || !r_vec || !theta_vec || !shift || bad_batch(B) || K < 1 || moving_T < 1 || M < 1 || !(speed > 0.0)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(shift));
    HIP_TRY(launch_delay_min(doa, B, K, moving_T, r_vec, theta_vec, M, speed, shift, (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- counter-based random numbers ----------------------------------------------------------------------------
int micloc_uniform_f64(double *out, size_t n, uint64_t seed, uint32_t substream, const uint32_t *epoch, double lo, double hi,
                       void *stream)
{
    if (!out || n < 1 || (n + 1) / 2 > 0xFFFFFFFFull) return MICLOC_ERR_INVALID;  // the pair index is one counter word
    DeviceGuard guard(device_of(out));
    HIP_TRY(launch_uniform(out, n, seed, substream, epoch, lo, hi, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_counter_add_u32(uint32_t *counter, uint32_t inc, void *stream)
{
    if (!counter) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(counter));
    HIP_TRY(launch_counter_add(counter, inc, (hipStream_t)stream));
    return MICLOC_OK;
}

size_t micloc_awgn_workspace_bytes(int B, int T, int M)
{
    if (B < 1 || T < 1 || M < 1) return 0;
    return awgn_ws_bytes(B, (size_t)T * M);
}

int micloc_awgn_f64(double *x, int B, int T, int M, const double *snr_db, const double *sigma, uint64_t seed, uint32_t substream,
                    const uint32_t *epoch, uint32_t first_trial, void *ws, size_t ws_bytes, void *stream)
{
    if (!x || bad_batch(B) || T < 1 || M < 1 || (!snr_db && !sigma)) return MICLOC_ERR_INVALID;
    // counter words: pair index < 2^32; trial ids stay below the uniform generator's reserved word 0xFFFFFFFF
    if (((size_t)T * M + 1) / 2 > 0xFFFFFFFFull || (uint64_t)first_trial + (uint64_t)B > 0xFFFFFFFFull) return MICLOC_ERR_INVALID;
    if (!sigma && bad_ws(ws, ws_bytes, awgn_ws_bytes(B, (size_t)T * M))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(x));
    HIP_TRY(launch_awgn(x, B, (size_t)T * M, M, snr_db, sigma, seed, substream, epoch, first_trial, ws, (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- per-trial DoA error and per-SNR mean absolute error ------------------------------------------------------
int micloc_doa_error_f64(const int32_t *argmax, const double *doa_list, int G, const double *doa_true, int B, int groups,
                         double *err, double *mae, void *stream)
{
    if (!argmax || !doa_list || !doa_true || G < 1 || bad_batch(B) || groups < 1 || B % groups != 0 || (!err && !mae))
        return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(argmax));
    HIP_TRY(launch_doa_error(argmax, doa_list, G, doa_true, B, groups, err, mae, (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- Xylo integer LIF (BASELINE config 4; parity unpinned, see xylo.hip) ------------------------------------
size_t micloc_xylo_workspace_bytes(int Cin, int N)
{
    if (Cin < 1 || N < 1) return 0;
    return xylo_ws_bytes(Cin, N);
}

int micloc_xylo_lif_i16(const uint8_t *spikes_in, int B, int T, int Cin, const int8_t *W_in, int N, int w_rec,
                        const uint8_t *dash_syn, const uint8_t *dash_mem, const int16_t *thr, int max_spikes,
                        uint8_t *spikes_out, int32_t *rate, void *ws, size_t ws_bytes, void *stream)
{
    if (!spikes_in || !W_in || !dash_syn || !dash_mem || !thr || bad_batch(B) || T < 1 || Cin < 1 || N < 1 || max_spikes < 1 ||
        (!spikes_out && !rate))
        return MICLOC_ERR_INVALID;
    if (Cin > 64 || (w_rec != 0 && N > 1024)) return MICLOC_ERR_SHAPE;
    for (int g = 0; g < N; ++g)
        if (thr[g] <= 0 || dash_syn[g] > 15 || dash_mem[g] > 15) return MICLOC_ERR_INVALID;
    if (bad_ws(ws, ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ws));
    HIP_TRY(launch_xylo(spikes_in, B, T, Cin, W_in, N, w_rec, dash_syn, dash_mem, thr, max_spikes, spikes_out, rate, ws,
                        (hipStream_t)stream));
    return MICLOC_OK;
}

// Two-phase form of the same network: constants uploaded once, then any number of launches that touch no host memory
// and never synchronise (capturable into a HIP graph).  `ternary_channels` > 0: the input is the encoder's int8 raster.
int micloc_xylo_upload(int Cin, const int8_t *W_in, int N, const uint8_t *dash_syn, const uint8_t *dash_mem, const int16_t *thr,
                       void *ws, size_t ws_bytes, void *stream)
{
    if (!W_in || !dash_syn || !dash_mem || !thr || Cin < 1 || N < 1) return MICLOC_ERR_INVALID;
    if (Cin > 64) return MICLOC_ERR_SHAPE;
    for (int g = 0; g < N; ++g)
        if (thr[g] <= 0 || dash_syn[g] > 15 || dash_mem[g] > 15) return MICLOC_ERR_INVALID;
    if (bad_ws(ws, ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ws));
    HIP_TRY(xylo_upload(Cin, W_in, N, dash_syn, dash_mem, thr, ws, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_xylo_lif_resident_i16(const void *spikes_in, int ternary_channels, int B, int T, int Cin, int N, int w_rec,
                                 int max_spikes, uint8_t *spikes_out, int32_t *rate, void *ws, size_t ws_bytes, void *stream)
{
    if (!spikes_in || bad_batch(B) || T < 1 || Cin < 1 || N < 1 || max_spikes < 1 || (!spikes_out && !rate)) return MICLOC_ERR_INVALID;
    if (Cin > 64 || (w_rec != 0 && N > 1024)) return MICLOC_ERR_SHAPE;
    if (ternary_channels < 0 || (ternary_channels > 0 && Cin != 2 * ternary_channels)) return MICLOC_ERR_SHAPE;
    if (bad_ws(ws, ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ws));
    HIP_TRY(launch_xylo_resident(spikes_in, ternary_channels, B, T, Cin, N, w_rec, max_spikes, spikes_out, rate, ws, (hipStream_t)stream));
    return MICLOC_OK;
}

size_t micloc_xylo_sweep_scratch_bytes(int B)
{
    if (bad_batch(B)) return 0;
    return xylo_sweep_scratch_bytes(B);
}

int micloc_xylo_lif_sweep_i16(const int8_t *raster, int ternary_channels, int B, int T, int Cin, int N, int max_spikes, int32_t *rate,
                              void *ws, size_t ws_bytes, void *scratch, size_t scratch_bytes, int workers_per_cu, void *stream)
{
    if (!raster || !rate || bad_batch(B) || T < 1 || Cin < 1 || N < 1 || max_spikes < 1 || workers_per_cu < 0 || workers_per_cu > 8) return MICLOC_ERR_INVALID;
    if (Cin > 64 || ternary_channels < 1 || Cin != 2 * ternary_channels) return MICLOC_ERR_SHAPE;
    if (bad_ws(ws, ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(scratch, scratch_bytes, xylo_sweep_scratch_bytes(B))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ws));
    HIP_TRY(launch_xylo_sweep(raster, ternary_channels, B, T, Cin, N, max_spikes, rate, ws, scratch, workers_per_cu, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_xylo_sweep_status(const void *scratch, int *status2, void *stream)
{
    if (!scratch || !status2) return MICLOC_ERR_INVALID;
    int ctl[2];
    HIP_TRY(hipMemcpyAsync(ctl, scratch, sizeof(ctl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status2[0] = ctl[0];
    status2[1] = ctl[1];
    return MICLOC_OK;
}

int micloc_design_vectors_f64(const double *cov, int n_doa, int C, int bipolar, double rel_prec, double *bf_mat, int G, int g0,
                              void *stream)
{
    if (!cov || !bf_mat || n_doa < 1 || C < 2 || G < 1 || g0 < 0 || g0 + n_doa > G || !(rel_prec > 0.0)) return MICLOC_ERR_INVALID;
    if (C > 128 || (C > 32 && (C & 1)) || (bipolar && (C & 1))) return MICLOC_ERR_SHAPE;  // (the one-sided kernel pairs all columns: even C)
    DeviceGuard guard(device_of(bf_mat));
    HIP_TRY(launch_design_vec(cov, n_doa, C, bipolar ? 1 : 0, rel_prec, bf_mat, G, g0, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_pack_events_u8(const int8_t *raster, int B, int T, int C, int band, int bands, int mode, uint8_t *out, void *stream)
{
    if (!raster || !out || bad_batch(B) || T < 1 || C < 1 || bands < 1 || band < 0 || band >= bands) return MICLOC_ERR_INVALID;
    if (mode != MICLOC_PACK_TERNARY && mode != MICLOC_PACK_UNIPOLAR && mode != MICLOC_PACK_BIPOLAR) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(out));
    const int stride = bands * C * (mode == MICLOC_PACK_BIPOLAR ? 2 : 1);
    HIP_TRY(launch_pack_events(raster, (size_t)B * T, C, out, stride, band * C, bands * C + band * C, mode, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_rate_from_counts_f64(const int32_t *counts, int B, int G, int bands, int T, double fs, double *rate, void *stream)
{
    if (!counts || !rate || bad_batch(B) || G < 1 || bands < 1 || T < 1 || !(fs > 0.0) || (long long)B * G > 0x7fffffffll) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(rate));
    HIP_TRY(launch_rate_from_counts(counts, B, G, bands, T, fs, rate, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_envelope_track_f64(const double *y, int B, int T, int G, double a_rise, double i_rise, double a_fall, double *env, int32_t *index,
                              void *stream)
{
    if (!y || !env || bad_batch(B) || T < 1 || G < 1 || (long long)B * T > 0x7fffffffll * 4) return MICLOC_ERR_INVALID;
    // 1 - 1/w and 1/w of window lengths w >= 1 (utils.py:34): finite, in [0, 1]
    if (!(a_rise >= 0.0 && a_rise <= 1.0 && i_rise >= 0.0 && i_rise <= 1.0 && a_fall >= 0.0 && a_fall <= 1.0)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(env));
    HIP_TRY(launch_envelope_track(y, MICLOC_ENV_F64, B, T, G, a_rise, i_rise, a_fall, env, index, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_envelope_track_any(const void *y, int kind, int B, int T, int G, double a_rise, double i_rise, double a_fall, double *env, int32_t *index,
                              void *stream)
{
    if (!y || !env || bad_batch(B) || T < 1 || G < 1 || (long long)B * T > 0x7fffffffll * 4) return MICLOC_ERR_INVALID;
    if (kind < MICLOC_ENV_F64 || kind > MICLOC_ENV_I64) return MICLOC_ERR_INVALID;
    if (!(a_rise >= 0.0 && a_rise <= 1.0 && i_rise >= 0.0 && i_rise <= 1.0 && a_fall >= 0.0 && a_fall <= 1.0)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(env));
    HIP_TRY(launch_envelope_track(y, kind, B, T, G, a_rise, i_rise, a_fall, env, index, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_peak_location_i32(const int32_t *rate, int B, int G, int bands, int win_size, int32_t *index, void *stream)
{
    if (!rate || !index || bad_batch(B) || G < 1 || bands < 1) return MICLOC_ERR_INVALID;
    if (win_size < 1 || win_size % 2 != 1 || win_size > G / 2 || G > 16384) return MICLOC_ERR_INVALID;  // utils.py:96-107
    DeviceGuard guard(device_of(index));
    HIP_TRY(launch_peak_location(rate, B, G, bands, win_size, index, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_doa_peaks_f64(const double *power, int B, int G, const double *doa_list, int grid_kind, int K, double min_separation,
                         double rel_threshold, int32_t *index, double *value, void *stream)
{
    if (!power || !doa_list || !index || bad_batch(B) || G < 1 || G > 4096 || K < 1 || K > 16) return MICLOC_ERR_INVALID;
    if (grid_kind < MICLOC_GRID_LINEAR || grid_kind > MICLOC_GRID_CIRCULAR_CLOSED) return MICLOC_ERR_INVALID;
    if (!(min_separation >= 0.0) || !(rel_threshold >= 0.0) || isinf(rel_threshold)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(device_of(index));
    HIP_TRY(launch_doa_peaks(power, B, G, doa_list, grid_kind, K, min_separation, rel_threshold, index, value, (hipStream_t)stream));
    return MICLOC_OK;
}

}  // extern "C"

namespace {

bool music_dims(int B, int T, int M, int L, int hop, int S, int N, int nbin, int G, int k, MusicDims *d)
{
    if (bad_batch(B) || T < 1 || M < 1 || L < 1 || hop < 1 || S < 1 || N < 2 || nbin < 1 || nbin > N || nbin > 8192 || G < 1 || k < 0)
        return false;
    d->B = B, d->T = T, d->M = M, d->S = S, d->L = L, d->hop = hop, d->N = N;
    d->Np = (N + 63) / 64 * 64;
    d->Fmax = (L < T ? L : T) / N;
    d->nbin = nbin;
    d->Cp = (2 * nbin + 15) / 16 * 16;
    d->G = G;
    d->ksel = (k == 0 || k > nbin) ? nbin : k;
    return true;
}

// every slice starts inside the signal and holds at least one frame (the last slice is the shortest)
bool music_slices_ok(const MusicDims &d)
{
    const long long last = (long long)(d.S - 1) * d.hop;
    if (last >= d.T) return false;
    const long long len = d.T - last < d.L ? d.T - last : d.L;
    return len >= d.N && d.Fmax >= 1;
}

size_t music_ws(const MusicDims &d)
{
    const MusicBuffers L = music_layout(d);
    return align256(L.xf_bytes) + align256(L.X_bytes) + align256(L.sel_bytes) + align256(L.spec_bytes);
}

}  // namespace

extern "C" {

size_t micloc_music_workspace_bytes(int B, int T, int M, int L, int hop, int S, int N, int nbin, int G, int k)
{
    MusicDims d{};
    if (!music_dims(B, T, M, L, hop, S, N, nbin, G, k, &d)) return 0;
    return music_ws(d);
}

int micloc_music_f64(const double *x, int B, int T, int M, const double *b, const double *a, int n, int L, int hop, int S, int N,
                     const double *W, int nbin, const double *steer_re, const double *steer_im, int G, int k, int32_t *sel, double *spec,
                     double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    MusicDims d{};
    if (!x || !b || !a || !W || !steer_re || !steer_im || n < 1 || n > MICLOC_MAX_IIR || a[0] == 0.0 ||
        !music_dims(B, T, M, L, hop, S, N, nbin, G, k, &d))
        return MICLOC_ERR_INVALID;
    if (!music_slices_ok(d)) return MICLOC_ERR_SHAPE;
    if (bad_ws(ws, ws_bytes, music_ws(d))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(x));
    IirCoef co{};
    co.n = n;
    for (int i = 0; i < n; ++i) {
        co.b[i] = b[i] / a[0];
        co.a[i] = a[i] / a[0];
    }
    const MusicBuffers Lb = music_layout(d);
    unsigned char *base = reinterpret_cast<unsigned char *>(ws);
    double *xf = reinterpret_cast<double *>(base);
    base += align256(Lb.xf_bytes);
    double *X = reinterpret_cast<double *>(base);
    base += align256(Lb.X_bytes);
    int32_t *sel_ws = reinterpret_cast<int32_t *>(base);
    base += align256(Lb.sel_bytes);
    double *spec_ws = reinterpret_cast<double *>(base);
    HIP_TRY(launch_music(d, co, x, W, steer_re, steer_im, xf, X, sel ? sel : sel_ws, spec ? spec : spec_ws, power, argmax, (hipStream_t)stream));
    return MICLOC_OK;
}

}  // extern "C"
