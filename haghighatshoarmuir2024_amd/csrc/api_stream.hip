// C-ABI of libmicloc_hip.so (see include/micloc_hip.h for the contract and reference citations): recordings that arrive tile by tile --
// the filterbank's state carry and the band sum per tile, the SNN stream, the complex stream (each with or without the window read-out and the tracked read-out), the complex stream of F bands, and
// the MUSIC stream; the tracked read-out of the two wideband streams.
#include "api_sets.h"
#include "stream_music.h"
#include "stream_track.h"
#include "stream_track_bands.h"

using namespace micloc;

extern "C" {

// ---- wideband streaming: filterbank state carry (filterbank.hip), band sum per tile (stream_bands.hip) ------------------------------
size_t micloc_filterbank_stream_state_bytes(int F, int n, int B, int M)
{
    if (F < 1 || F > MICLOC_MAX_BANDS || n < 1 || n > MICLOC_MAX_IIR || B < 1 || M < 1) return 0;
    return filterbank_stream_state_bytes(F, n, B, M);
}

int micloc_filterbank_stream_reset(void *fb_state, size_t bytes, void *stream)
{
    if (!fb_state) return MICLOC_ERR_INVALID;
    if (bad_ws(fb_state, bytes, 256)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(fb_state));
    HIP_TRY(launch_zero_fill(fb_state, bytes, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_filterbank_tile_f64(const double *b, const double *a, int F, int n, const double *x_tile, int B, int n_frames, int M, void *fb_state,
                               size_t fb_bytes, double *xf_tile, void *stream)
{
    FilterbankCoef co;
    const int rc = filterbank_coef(b, a, F, n, &co);
    if (rc != MICLOC_OK) return rc;
    if (!x_tile || !xf_tile || !fb_state || B < 1 || n_frames < 1 || M < 1) return MICLOC_ERR_INVALID;
    if (bad_ws(fb_state, fb_bytes, filterbank_stream_state_bytes(F, n, B, M))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(xf_tile));
    HIP_TRY(launch_filterbank_tile(co, x_tile, F, B, n_frames, M, xf_tile, reinterpret_cast<double *>(fb_state), (hipStream_t)stream));
    return MICLOC_OK;
}

size_t micloc_stream_bands_state_bytes(void) { return STREAM_BANDS_STATE_BYTES; }

int micloc_stream_bands_reset(void *bands_state, size_t bytes, void *stream)
{
    if (!bands_state) return MICLOC_ERR_INVALID;
    if (bad_ws(bands_state, bytes, STREAM_BANDS_STATE_BYTES)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(bands_state));
    HIP_TRY(launch_zero_fill(bands_state, STREAM_BANDS_STATE_BYTES, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_band_sum_f64(int F, int B, int G, const double *const *band_power, int window, int Kb, int max_windows,
                               const double *const *band_window_power, const int32_t *const *band_window_count, void *bands_state,
                               size_t bands_bytes, double *power, int32_t *argmax, double *window_power, int32_t *window_argmax,
                               double *latest_power, int32_t *latest_argmax, void *stream)
{
    if (!band_power || !bands_state || (!power && !argmax) || F < 1 || F > MICLOC_MAX_BANDS || bad_batch(B) || G < 1 || window < 0)
        return MICLOC_ERR_INVALID;
    if (window > 0 && (!band_window_power || !band_window_count || !window_argmax || max_windows < 1 || Kb < 1)) return MICLOC_ERR_INVALID;
    StreamBandsArgs args{};
    for (int f = 0; f < F; ++f) {
        if (!band_power[f]) return MICLOC_ERR_INVALID;
        args.power[f] = band_power[f];
        if (window > 0) {
            if (!band_window_power[f] || !band_window_count[f]) return MICLOC_ERR_INVALID;
            args.rows[f] = band_window_power[f];
            args.count[f] = band_window_count[f];
        }
    }
    if (bad_ws(bands_state, bands_bytes, STREAM_BANDS_STATE_BYTES)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(bands_state));
    HIP_TRY(launch_stream_band_sum(args, F, B, G, window > 0, Kb, max_windows, bands_state, power, argmax, window_power, window_argmax, latest_power,
                                   latest_argmax, (hipStream_t)stream));
    return MICLOC_OK;
}

/* status[0] = wideband windows emitted (or given up) so far, [1] = windows given up because a band's ring had overwritten them
 * (synchronises the stream) */
int micloc_stream_bands_status(const void *bands_state, int *status2, void *stream)
{
    if (!bands_state || !status2) return MICLOC_ERR_INVALID;
    int w[2];
    HIP_TRY(hipMemcpyAsync(w, bands_state, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status2[0] = w[0];
    status2[1] = w[1];
    return MICLOC_OK;
}

/* device address of word [0] of micloc_stream_bands_status (for kernels that follow the wideband windows: stream_peaks.hip) */
const int32_t *micloc_stream_bands_window_count_ptr(const void *bands_state) { return reinterpret_cast<const int32_t *>(bands_state); }

// ---- streaming: the band-pass / RZCC stage tile by tile, exact state hand-off -----------------------------------
size_t micloc_stream_state_bytes(const micloc_plan *p, int B)
{
    if (!p || bad_batch(B)) return 0;
    return rzcc_stream_state_bytes(B * p->C);
}

int micloc_stream_overflow(const void *state, int *count, void *stream)
{
    if (!state || !count) return MICLOC_ERR_INVALID;
    HIP_TRY(hipMemcpyAsync(count, state, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return MICLOC_OK;
}

// ---- streaming localisation: LIF + beamforming + power as the spikes become final ---------------------------------------------
// loc_state: [256 B: 64 control ints][acc: B x 2 x G doubles]
size_t micloc_stream_localize_state_bytes(const micloc_plan *p, int B)
{
    if (!p || bad_batch(B) || p->G_out < 1) return 0;
    return 256 + align256((size_t)B * 2 * p->G_out * sizeof(double));
}

int micloc_stream_chunk_frames(const micloc_plan *p)
{
    if (!p || !p->d_ntab || !p->d_W) return MICLOC_ERR_NOT_SET;
    return lif_beamform_chunk_frames(p->W, p->ntab);
}

size_t micloc_stream_localize_workspace_bytes(const micloc_plan *p, int B, int window_frames)
{
    if (!p || bad_batch(B) || window_frames < 1 || p->W.GT < 1) return 0;
    return align256(beamform_partial_bytes(B, window_frames, 16 * p->W.GT));
}

// ---- clocked streaming: the same stages with the absolute time in a device word ----------------------------------------------
// One tile = begin_tile (clock + window slide) -> STHT of [history | tile] (micloc_stht_f64) -> wrap_rows -> encode_tile ->
// localize_tile (which ends with the clock's tick).  No call takes an absolute time: every launch of a tile of n frames has the
// same arguments, so the sequence can be captured into ONE hipGraph and replayed per tile (StreamingLocalizer.capture).
int micloc_stream_reset(const micloc_plan *p, int B, void *enc_state, size_t enc_bytes, void *loc_state, size_t loc_bytes, int8_t *window,
                        int window_frames, void *stream)
{
    if (!p || !enc_state || !loc_state || !window || bad_batch(B) || window_frames < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    if (bad_ws(enc_state, enc_bytes, rzcc_stream_state_bytes(B * p->C))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(loc_state, loc_bytes, micloc_stream_localize_state_bytes(p, B))) return MICLOC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_zero_fill(enc_state, 256, st));  // overflow counter (the encoder's own state is written by the first tile)
    HIP_TRY(launch_zero_fill(loc_state, micloc_stream_localize_state_bytes(p, B), st));  // control words, clock, accumulators
    HIP_TRY(launch_zero_fill(window, (size_t)B * window_frames * p->C, st));
    return MICLOC_OK;
}

int micloc_stream_begin_tile(const micloc_plan *p, void *loc_state, int8_t *window, int8_t *scratch_window, int B, int n, int window_frames,
                             void *stream)
{
    if (!p || !loc_state || !window || !scratch_window || window == scratch_window || bad_batch(B) || n < 1 || window_frames < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    if (!p->d_ntab || !p->d_W) return MICLOC_ERR_NOT_SET;
    const int CH = lif_beamform_chunk_frames(p->W, p->ntab);
    if (window_frames % CH != 0 || n > window_frames) return MICLOC_ERR_SHAPE;
    HIP_TRY(launch_stream_begin_tile(reinterpret_cast<int *>(loc_state), window, scratch_window, B, (size_t)window_frames * p->C, p->C, n, window_frames,
                                     CH, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_wrap_rows_f64(const micloc_plan *p, const void *loc_state, double *h, int B, int Ts, int first_col, int n, const double *wrap_tail,
                                void *stream)
{
    if (!p || !loc_state || !h || bad_batch(B) || n < 1 || first_col < 0 || first_col + n > Ts) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    HIP_TRY(launch_stht_wrap_rows(h, wrap_tail, B, p->M, Ts, first_col, n, p->L / 2, reinterpret_cast<const int *>(loc_state), (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_encode_tile_f64(const micloc_plan *p, const double *h, int B, int T_tile, int row_stride, int final_tile, int8_t *window,
                                  int window_frames, void *enc_state, size_t enc_bytes, const void *loc_state, void *stream)
{
    if (!p || !h || !window || !loc_state || bad_batch(B) || T_tile < 1 || window_frames < T_tile || row_stride < T_tile) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    if (!final_tile && T_tile % 16 != 0) return MICLOC_ERR_SHAPE;
    if (bad_ws(enc_state, enc_bytes, rzcc_stream_state_bytes(B * p->C))) return MICLOC_ERR_WORKSPACE;
    HIP_TRY(launch_stream_encode(p->iir, h, B * p->C, p->C, T_tile, row_stride, p->robust_width, p->bipolar, window, window_frames, 0, 0,
                                 final_tile, enc_state, (hipStream_t)stream, 0, reinterpret_cast<const int *>(loc_state)));
    return MICLOC_OK;
}

// ---- the localize step of a tile, with or without the streaming windows: the time-resolved read-out of the same chunk rows, emitted
// while the recording arrives ----------------------------------------------------------------------------------------------------
// win_state: [256 B: int windows emitted][B][ceil(window / hop)][2][G] doubles (stream_windows.hip), for the SNN stream and the complex one
namespace {

// MICLOC_OK and *CH, or the status of a plan that cannot serve the SNN stream's localize step (p non-NULL)
int stream_plan_args(const micloc_plan *p, int *CH)
{
    *CH = 0;
    if (!p->d_ntab || !p->d_W) return MICLOC_ERR_NOT_SET;
    if (p->W_is_complex) return MICLOC_ERR_SHAPE;
    *CH = lif_beamform_chunk_frames(p->W, p->ntab);
    return MICLOC_OK;
}

// the window-argument rule of both streams; rc: the status of the stream's own plan check, which gave the chunk length *CH (read only
// behind rc == MICLOC_OK, so the check may be an argument of the same call)
int stream_window_args(int rc, int window, int hop, int max_windows, const int *CH)
{
    if (window < 1 || hop < 1 || max_windows < 1) return MICLOC_ERR_INVALID;
    if (rc != MICLOC_OK) return rc;
    if (window % *CH != 0 || hop % *CH != 0 || hop > window) return MICLOC_ERR_SHAPE;
    return MICLOC_OK;
}

// the tail of both *_window_reset entries; rc: stream_window_args' status
int stream_window_zero(int rc, const micloc_plan *p, int B, void *win_state, size_t win_bytes, int window, int hop, void *stream)
{
    if (rc != MICLOC_OK) return rc;
    const size_t need = stream_window_state_bytes(B, p->G_out, window, hop);
    if (bad_ws(win_state, win_bytes, need)) return MICLOC_ERR_WORKSPACE;
    HIP_TRY(launch_zero_fill(win_state, need, (hipStream_t)stream));
    return MICLOC_OK;
}

// the tracked read-out of a tile ("streaming, tracking"): the envelope state, the rule's constants, the ring and the pair scratch
struct TrackArgs {
    void *state;
    size_t state_bytes;
    double a_rise, i_rise, a_fall;
    int R;
    int32_t *index;
    double *peak;
    int32_t *latest_index;
    double *latest_peak;
    void *ws;
    size_t ws_bytes;
};

// the argument rule of both tracked entries behind the stream's own plan check: `most` frames can become final in one tile
int stream_track_args(const micloc_plan *p, const TrackArgs &t, int B, int most, int cap)
{
    if (!t.state || !t.index || !t.peak || !t.latest_index || !t.latest_peak || t.R < 1) return MICLOC_ERR_INVALID;
    if (!track_fused_eligible(p->W, p->ntab, p->W_is_complex) || t.R < most) return MICLOC_ERR_SHAPE;
    if (bad_ws(t.state, t.state_bytes, stream_track_state_bytes(B, p->G_out))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(t.ws, t.ws_bytes, stream_track_pairs_bytes(B, cap, p->G_out))) return MICLOC_ERR_WORKSPACE;
    return MICLOC_OK;
}

int stream_track_launch(const micloc_plan *p, const TrackArgs &t, const void *src, const int *ctl, int B, int cap, int CH, hipStream_t st)
{
    HIP_TRY(launch_stream_track(p->W, p->ntab, p->W_is_complex, src, ctl, B, cap, CH, p->G_out, t.a_rise, t.i_rise, t.a_fall,
                                reinterpret_cast<double *>(t.state), t.R, t.index, t.peak, t.latest_index, t.latest_peak, t.ws, st));
    return MICLOC_OK;
}

// the launches of a tile behind the encoder: horizon, LIF + beamforming of the chunks that became final, accumulation, (the window
// read-out in front of the commit,) (the tracked read-out, there as well,) commit, tick.  win_state == nullptr / trk == nullptr: no such
// read-out; loc_state, power and argmax end with the same bits either way.
int stream_localize(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *raster, int B, int window_frames,
                    int final_tile, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *win_state, size_t win_bytes, int window,
                    int hop, int max_windows, double *window_power, int32_t *window_argmax, double *latest_power, int32_t *latest_argmax,
                    void *stream, const TrackArgs *trk = nullptr)
{
    if (!p || !enc_state || !loc_state || !raster || bad_batch(B) || window_frames < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    int CH;
    int rc = stream_plan_args(p, &CH);
    if (win_state) rc = stream_window_args(rc, window, hop, max_windows, &CH);
    if (rc != MICLOC_OK) return rc;
    if (window_frames % CH != 0) return MICLOC_ERR_SHAPE;
    if (trk) {  // a tile can make every frame of the window final; the LIF history of a chunk is the one chunk in front of it
        rc = stream_track_args(p, *trk, B, window_frames, window_frames);
        if (rc != MICLOC_OK) return rc;
        if (stream_track_halo(p->ntab) > CH) return MICLOC_ERR_SHAPE;
    }
    const int G = p->G_out, Gp = 16 * p->W.GT;
    if (bad_ws(loc_state, loc_bytes, micloc_stream_localize_state_bytes(p, B))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, beamform_partial_bytes(B, window_frames, Gp))) return MICLOC_ERR_WORKSPACE;
    if (win_state && bad_ws(win_state, win_bytes, stream_window_state_bytes(B, G, window, hop))) return MICLOC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int *ctl = reinterpret_cast<int *>(loc_state);
    double *acc = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(loc_state) + 256);
    const int nwin = window_frames / CH;
    HIP_TRY(launch_stream_horizon(enc_state, B * p->C, p->bipolar, 0, final_tile ? 1 : 0, CH, 0, nwin, ctl, st, 1));
    BeamformW W = p->W;
    W.chunk_range = ctl + 4;
    double *partial = reinterpret_cast<double *>(ws);
    int nch = 0;
    // the whole window as the launch shape; the kernel takes the frames that exist from the control words
    HIP_TRY(launch_lif_beamform(W, p->ntab, raster, B, window_frames, nullptr, partial, st, &nch));
    HIP_TRY(launch_stream_accumulate(partial, B, nch, Gp, G, ctl + 4, ctl, acc, ctl + 8, power, argmax, st));
    if (win_state)
        HIP_TRY(launch_stream_windows(partial, B, nch, Gp, G, 0, 0, CH, ctl, final_tile ? 1 : 0, window, hop, max_windows, win_state, window_power,
                                      window_argmax, latest_power, latest_argmax, st));
    if (trk) {  // in front of the commit as well: the range and ctl[0] as the horizon left them
        rc = stream_track_launch(p, *trk, raster, ctl, B, window_frames, CH, st);
        if (rc != MICLOC_OK) return rc;
    }
    HIP_TRY(launch_stream_commit(ctl, STREAM_BLOCK_CHUNKS, st));
    HIP_TRY(launch_stream_tick(ctl, st));
    return MICLOC_OK;
}

}  // namespace

int micloc_stream_localize_tile_f64(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window, int B,
                                    int window_frames, int final_tile, double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    return stream_localize(p, enc_state, loc_state, loc_bytes, window, B, window_frames, final_tile, power, argmax, ws, ws_bytes, nullptr, 0, 0, 0, 0,
                           nullptr, nullptr, nullptr, nullptr, stream);
}

size_t micloc_stream_window_state_bytes(const micloc_plan *p, int B, int window, int hop, int max_windows)
{
    int CH;
    if (!p || bad_batch(B) || p->G_out < 1 || stream_window_args(stream_plan_args(p, &CH), window, hop, max_windows, &CH) != MICLOC_OK) return 0;
    return stream_window_state_bytes(B, p->G_out, window, hop);
}

int micloc_stream_window_reset(const micloc_plan *p, int B, void *win_state, size_t win_bytes, int window, int hop, int max_windows, void *stream)
{
    if (!p || !win_state || bad_batch(B)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    int CH;
    const int rc = stream_plan_args(p, &CH);
    return stream_window_zero(stream_window_args(rc, window, hop, max_windows, &CH), p, B, win_state, win_bytes, window, hop, stream);
}

int micloc_stream_localize_tile_windows_f64(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window_raster,
                                            int B, int window_frames, int final_tile, double *power, int32_t *argmax, void *ws, size_t ws_bytes,
                                            void *win_state, size_t win_bytes, int window, int hop, int max_windows, double *window_power,
                                            int32_t *window_argmax, double *latest_power, int32_t *latest_argmax, void *stream)
{
    if (!win_state || !window_argmax) return MICLOC_ERR_INVALID;
    return stream_localize(p, enc_state, loc_state, loc_bytes, window_raster, B, window_frames, final_tile, power, argmax, ws, ws_bytes, win_state,
                           win_bytes, window, hop, max_windows, window_power, window_argmax, latest_power, latest_argmax, stream);
}

/* windows emitted so far (synchronises the stream) */
int micloc_stream_window_count(const void *win_state, int *count, void *stream)
{
    if (!win_state || !count) return MICLOC_ERR_INVALID;
    HIP_TRY(hipMemcpyAsync(count, win_state, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return MICLOC_OK;
}

/* device address of the count word micloc_stream_window_count reads (for kernels that follow a band's windows: stream_bands.hip) */
const int32_t *micloc_stream_window_count_ptr(const void *win_state) { return reinterpret_cast<const int32_t *>(win_state); }

/* status[0] = chunks beamformed, [1] = frames beamformed, [2] = window-lag failures, [3] = chunks in the open reduction block
 * (synchronises the stream) */
int micloc_stream_localize_status(const void *loc_state, int *status4, void *stream)
{
    if (!loc_state || !status4) return MICLOC_ERR_INVALID;
    int ctl[16];
    HIP_TRY(hipMemcpyAsync(ctl, loc_state, sizeof(ctl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status4[0] = ctl[0];
    status4[1] = ctl[8];
    status4[2] = ctl[13];
    status4[3] = ctl[1];
    return MICLOC_OK;
}

// ---- streaming, complex Beamformer (stream_complex.hip; the rule: include/micloc_hip.h) ------------------------------------------------
// state: [256 B control words][DF2T words][carry][acc] (stream_complex_layout); ws: [staging [B][2M][Ks CH]][partial [B][Ks][Gp]]
namespace {

struct ScArgs {
    int CH, Ks, S, Gp;
    StreamComplexLayout L;
    size_t ws_partial, ws_total;
};

// MICLOC_OK and *a, or the status of the rule's argument errors (p non-NULL, B checked)
int sc_args(const micloc_plan *p, int B, int max_tile, ScArgs *a)
{
    *a = ScArgs{};
    if (!p->d_W) return MICLOC_ERR_NOT_SET;
    if (!p->W_is_complex) return MICLOC_ERR_SHAPE;
    const int CH = window_quantum(p);
    if (CH < 1) return MICLOC_ERR_INVALID;
    a->CH = CH;
    a->Gp = 16 * p->W.GT;
    a->L = stream_complex_layout(B, p->C, p->G_out, p->iir.n, CH);
    if (max_tile > 0) {
        if ((long long)max_tile + 2ll * CH > 0x7fffffffll) return MICLOC_ERR_SHAPE;
        a->Ks = stream_complex_chunks(max_tile, CH);
        a->S = a->Ks * CH;
        a->ws_partial = align256((size_t)B * p->C * a->S * sizeof(double));
        a->ws_total = a->ws_partial + align256(beamform_partial_bytes(B, a->S, a->Gp));
    }
    return MICLOC_OK;
}

// the launches behind the band-pass of a tile: contraction, accumulation, (windows,) slide + commit -- one chain on one stream
int sc_localize(const micloc_plan *p, const ScArgs &a, void *state, int B, int final_tile, double *power, int32_t *argmax, void *ws,
                void *win_state, int window, int hop, int max_windows, double *window_power, int32_t *window_argmax, double *latest_power,
                int32_t *latest_argmax, hipStream_t st, const TrackArgs *trk = nullptr)
{
    double *staging = reinterpret_cast<double *>(ws);
    double *partial = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(ws) + a.ws_partial);
    int nch = 0;
    // the staging array as a recording of Ks whole chunks: the launch shape depends on max_tile only; the rows past the valid ones are never read
    HIP_TRY(launch_planar_beamform(p->W, staging, B, a.S, a.S, nullptr, 1, partial, st, &nch));
    if (nch != a.Ks) return MICLOC_ERR_INVALID;  // the launch chose a kernel window_quantum() does not describe
    HIP_TRY(launch_stream_complex_accumulate(partial, B, a.Ks, a.Gp, p->G_out, a.CH, final_tile, state, a.L, power, argmax, st));
    if (win_state)
        HIP_TRY(launch_stream_windows(partial, B, a.Ks, a.Gp, p->G_out, 1, a.Gp / 2, a.CH, reinterpret_cast<const int *>(state), final_tile ? 1 : 0,
                                      window, hop, max_windows, win_state, window_power, window_argmax, latest_power, latest_argmax, st));
    if (trk) {  // in front of the slide: the carry fill and the clock as they were before the tile
        const int rc = stream_track_launch(p, *trk, staging, reinterpret_cast<const int *>(state), B, a.S, a.CH, st);
        if (rc != MICLOC_OK) return rc;
    }
    HIP_TRY(launch_stream_complex_slide(staging, B * p->C, a.S, a.CH, state, a.L, st));
    return MICLOC_OK;
}

}  // namespace

size_t micloc_stream_complex_state_bytes(const micloc_plan *p, int B)
{
    ScArgs a;
    if (!p || bad_batch(B) || sc_args(p, B, 0, &a) != MICLOC_OK) return 0;
    return a.L.total;
}

size_t micloc_stream_complex_workspace_bytes(const micloc_plan *p, int B, int max_tile)
{
    ScArgs a;
    if (!p || bad_batch(B) || max_tile < 1 || sc_args(p, B, max_tile, &a) != MICLOC_OK) return 0;
    return a.ws_total;
}

int micloc_stream_complex_reset(const micloc_plan *p, int B, void *state, size_t state_bytes, void *stream)
{
    if (!p || !state || bad_batch(B)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    const int rc = sc_args(p, B, 0, &a);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, a.L.total)) return MICLOC_ERR_WORKSPACE;
    HIP_TRY(launch_zero_fill(state, a.L.total, (hipStream_t)stream));  // clock, zero DF2T state (lfilter's), empty carry, accumulators
    return MICLOC_OK;
}

int micloc_stream_complex_bandpass_tile_f64(const micloc_plan *p, const double *h, int B, int n, int row_stride, int first_col, int max_tile,
                                            void *state, size_t state_bytes, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !h || !state || !ws || bad_batch(B) || n < 1 || max_tile < 1 || first_col < 0 || row_stride < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    const int rc = sc_args(p, B, max_tile, &a);
    if (rc != MICLOC_OK) return rc;
    if (n > max_tile || (long long)first_col + n > row_stride) return MICLOC_ERR_SHAPE;
    if (bad_ws(state, state_bytes, a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, a.ws_total)) return MICLOC_ERR_WORKSPACE;
    HIP_TRY(launch_stream_complex_bandpass(p->iir, h + first_col, B * p->C, n, (size_t)row_stride, reinterpret_cast<double *>(ws), a.S, a.CH,
                                           state, a.L, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_complex_localize_tile_f64(const micloc_plan *p, void *state, size_t state_bytes, int B, int max_tile, int final_tile,
                                            double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *stream)
{
    if (!p || !state || !ws || bad_batch(B) || max_tile < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    const int rc = sc_args(p, B, max_tile, &a);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, a.ws_total)) return MICLOC_ERR_WORKSPACE;
    return sc_localize(p, a, state, B, final_tile, power, argmax, ws, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

size_t micloc_stream_complex_window_state_bytes(const micloc_plan *p, int B, int window, int hop, int max_windows)
{
    ScArgs a;
    if (!p || bad_batch(B) || stream_window_args(sc_args(p, B, 0, &a), window, hop, max_windows, &a.CH) != MICLOC_OK) return 0;
    return stream_window_state_bytes(B, p->G_out, window, hop);
}

int micloc_stream_complex_window_reset(const micloc_plan *p, int B, void *win_state, size_t win_bytes, int window, int hop, int max_windows,
                                       void *stream)
{
    if (!p || !win_state || bad_batch(B)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    const int rc = sc_args(p, B, 0, &a);
    return stream_window_zero(stream_window_args(rc, window, hop, max_windows, &a.CH), p, B, win_state, win_bytes, window, hop, stream);
}

int micloc_stream_complex_localize_tile_windows_f64(const micloc_plan *p, void *state, size_t state_bytes, int B, int max_tile, int final_tile,
                                                    double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *win_state, size_t win_bytes,
                                                    int window, int hop, int max_windows, double *window_power, int32_t *window_argmax,
                                                    double *latest_power, int32_t *latest_argmax, void *stream)
{
    if (!p || !state || !ws || !win_state || !window_argmax || bad_batch(B) || max_tile < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    const int rc = stream_window_args(sc_args(p, B, max_tile, &a), window, hop, max_windows, &a.CH);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, a.ws_total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(win_state, win_bytes, stream_window_state_bytes(B, p->G_out, window, hop))) return MICLOC_ERR_WORKSPACE;
    return sc_localize(p, a, state, B, final_tile, power, argmax, ws, win_state, window, hop, max_windows, window_power, window_argmax,
                       latest_power, latest_argmax, (hipStream_t)stream);
}

// ---- streaming, tracking (stream_track.hip; the rule: include/micloc_hip.h) --------------------------------------------------------------
size_t micloc_stream_track_state_bytes(const micloc_plan *p, int B)
{
    if (!p || bad_batch(B) || p->G_out < 1 || micloc_track_is_fused(p) != 1) return 0;
    return stream_track_state_bytes(B, p->G_out);
}

size_t micloc_stream_track_workspace_bytes(const micloc_plan *p, int B, int window_frames)
{
    if (!p || bad_batch(B) || window_frames < 1 || p->G_out < 1 || micloc_track_is_fused(p) != 1) return 0;
    int cap = window_frames;
    if (p->W_is_complex) {  // the staging array of a complex stream whose longest tile has window_frames frames
        ScArgs a;
        if (sc_args(p, B, window_frames, &a) != MICLOC_OK) return 0;
        cap = a.S;
    }
    return stream_track_pairs_bytes(B, cap, p->G_out);
}

int micloc_stream_track_reset(const micloc_plan *p, int B, void *track_state, size_t track_bytes, void *stream)
{
    if (!p || !track_state || bad_batch(B)) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    const int fused = micloc_track_is_fused(p);
    if (fused < 0) return fused;
    if (fused != 1) return MICLOC_ERR_SHAPE;
    const size_t need = stream_track_state_bytes(B, p->G_out);
    if (bad_ws(track_state, track_bytes, need)) return MICLOC_ERR_WORKSPACE;
    HIP_TRY(launch_zero_fill(track_state, need, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_localize_tile_track_f64(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window_raster,
                                          int B, int window_frames, int final_tile, double *power, int32_t *argmax, void *ws, size_t ws_bytes,
                                          void *win_state, size_t win_bytes, int window, int hop, int max_windows, double *window_power,
                                          int32_t *window_argmax, double *latest_power, int32_t *latest_argmax, void *track_state,
                                          size_t track_bytes, double a_rise, double i_rise, double a_fall, int max_track, int32_t *track_index,
                                          double *track_peak, int32_t *latest_index, double *latest_peak, void *track_ws, size_t track_ws_bytes,
                                          void *stream)
{
    if (win_state && !window_argmax) return MICLOC_ERR_INVALID;
    const TrackArgs trk{track_state, track_bytes, a_rise, i_rise, a_fall, max_track, track_index, track_peak, latest_index, latest_peak, track_ws,
                        track_ws_bytes};
    return stream_localize(p, enc_state, loc_state, loc_bytes, window_raster, B, window_frames, final_tile, power, argmax, ws, ws_bytes, win_state,
                           win_bytes, window, hop, max_windows, window_power, window_argmax, latest_power, latest_argmax, stream, &trk);
}

int micloc_stream_complex_localize_tile_track_f64(const micloc_plan *p, void *state, size_t state_bytes, int B, int max_tile, int final_tile,
                                                  double *power, int32_t *argmax, void *ws, size_t ws_bytes, void *win_state, size_t win_bytes,
                                                  int window, int hop, int max_windows, double *window_power, int32_t *window_argmax,
                                                  double *latest_power, int32_t *latest_argmax, void *track_state, size_t track_bytes,
                                                  double a_rise, double i_rise, double a_fall, int max_track, int32_t *track_index,
                                                  double *track_peak, int32_t *latest_index, double *latest_peak, void *track_ws,
                                                  size_t track_ws_bytes, void *stream)
{
    if (!p || !state || !ws || (win_state && !window_argmax) || bad_batch(B) || max_tile < 1) return MICLOC_ERR_INVALID;
    DeviceGuard guard(p->device);
    ScArgs a;
    int rc = sc_args(p, B, max_tile, &a);
    if (win_state) rc = stream_window_args(rc, window, hop, max_windows, &a.CH);
    if (rc != MICLOC_OK) return rc;
    const TrackArgs trk{track_state, track_bytes, a_rise, i_rise, a_fall, max_track, track_index, track_peak, latest_index, latest_peak, track_ws,
                        track_ws_bytes};
    rc = stream_track_args(p, trk, B, max_tile, a.S);  // a tile makes its own frames final, no more
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, a.ws_total)) return MICLOC_ERR_WORKSPACE;
    if (win_state && bad_ws(win_state, win_bytes, stream_window_state_bytes(B, p->G_out, window, hop))) return MICLOC_ERR_WORKSPACE;
    return sc_localize(p, a, state, B, final_tile, power, argmax, ws, win_state, window, hop, max_windows, window_power, window_argmax,
                       latest_power, latest_argmax, (hipStream_t)stream, &trk);
}

/* status[0] = chunks contracted, [1] = frames contracted, [2] = carry fill, [3] = frames pushed (synchronises the stream) */
int micloc_stream_complex_status(const void *state, int *status4, void *stream)
{
    if (!state || !status4) return MICLOC_ERR_INVALID;
    int ctl[STREAM_CLK_T + 1];
    HIP_TRY(hipMemcpyAsync(ctl, state, sizeof(ctl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status4[0] = ctl[0];
    status4[1] = ctl[8];
    status4[2] = ctl[2];
    status4[3] = ctl[STREAM_CLK_T];
    return MICLOC_OK;
}

// ---- wideband streaming, complex Beamformer (stream_bands_complex.hip; the rule: include/micloc_hip.h) ----------------------------------
// The complex stream above for F * B rows.  state: stream_complex_layout(F * B); ws: [staging [F B][2M][Ks CH]][partial [F B][Ks][Gp]]
// [running band power [F B][G]]; win_state: [the window state of F * B rows, the band sum's words at byte SCB_BANDS_WORDS of its 256-B head][band ring [F B][Kb][G]]
}  // extern "C"

namespace {

struct ScbArgs {
    ScArgs a;  // the complex stream's arguments for F * B rows
    int FB;
    size_t ws_band_power, ws_total;
    // windows (scb_window_args)
    int Kb;
    size_t win_ring, win_total;
};

// the window kernel keeps its count in int word 0 of win_state's 256-B head and touches no other word of it: the band sum's four words
// {emitted, given up, pending emitted, pending given up} live further on in the same head, zero-filled with it
constexpr size_t SCB_BANDS_WORDS = 64;

// argument checks of the wideband complex stream in the header's order (max_tile == 0: the state's layout only)
int scb_args(const micloc_plan *const *plans, int F, int B, int max_tile, ScbArgs *s)
{
    *s = ScbArgs{};
    if (set_pointers(plans, F) != MICLOC_OK || bad_batch(B) || bad_batch(F * B) || max_tile < 0) return MICLOC_ERR_INVALID;
    if (set_tables(plans, F, true, false) != MICLOC_OK) return MICLOC_ERR_NOT_SET;
    if (set_shares(plans, F, SET_GRID | SET_COMPLEX | SET_CHAIN) != MICLOC_OK) return MICLOC_ERR_SHAPE;
    const micloc_plan *p0 = plans[0];
    s->FB = F * B;
    const int rc = sc_args(p0, s->FB, max_tile, &s->a);  // (one chunk length: it depends on CT and GT only, which the plans share)
    if (rc != MICLOC_OK) return rc;
    s->ws_band_power = s->a.ws_total;
    s->ws_total = s->a.ws_total + align256((size_t)s->FB * p0->G_out * sizeof(double));
    return MICLOC_OK;
}

// the window rule of the streams, then the layout of win_state; rc: scb_args' status with max_tile >= 1
int scb_window_args(int rc, const micloc_plan *const *plans, int window, int hop, int max_windows, ScbArgs *s)
{
    rc = stream_window_args(rc, window, hop, max_windows, &s->a.CH);
    if (rc != MICLOC_OK) return rc;
    s->Kb = stream_bands_ring_depth(s->a.Ks, hop / s->a.CH);
    s->win_ring = stream_window_state_bytes(s->FB, plans[0]->G_out, window, hop);
    s->win_total = s->win_ring + align256((size_t)s->FB * s->Kb * plans[0]->G_out * sizeof(double));
    return MICLOC_OK;
}

// the launches behind the band-pass of a tile: contraction per band, accumulation, (windows,) slide + commit over the F * B rows, band sum
int scb_localize(const micloc_plan *const *plans, int F, int B, const ScbArgs &s, void *state, int final_tile, double *band_power, double *power,
                 int32_t *argmax, void *ws, void *win_state, int window, int hop, int max_windows, double *window_power, int32_t *window_argmax,
                 double *latest_power, int32_t *latest_argmax, hipStream_t st, const TrackArgs *trk = nullptr)
{
    const micloc_plan *p0 = plans[0];
    const ScArgs &a = s.a;
    const int G = p0->G_out;
    double *staging = ws_doubles(ws, 0), *partial = ws_doubles(ws, a.ws_partial);
    double *bp = band_power ? band_power : ws_doubles(ws, s.ws_band_power);
    // per band the contraction of 4.16's tile (that band's bf_mat) on its B rows of the one staging array, into one array of chunk rows
    const size_t band_rows = (size_t)B * p0->C * a.S, band_partial = (size_t)B * a.Ks * a.Gp;
    for (int f = 0; f < F; ++f) {
        int nch = 0;
        HIP_TRY(launch_planar_beamform(plans[f]->W, staging + f * band_rows, B, a.S, a.S, nullptr, 1, partial + f * band_partial, st, &nch));
        if (nch != a.Ks) return MICLOC_ERR_INVALID;  // the launch chose a kernel window_quantum() does not describe
    }
    HIP_TRY(launch_stream_complex_accumulate(partial, s.FB, a.Ks, a.Gp, G, a.CH, final_tile, state, a.L, bp, nullptr, st));
    unsigned char *wbase = reinterpret_cast<unsigned char *>(win_state);
    double *ring = win_state ? reinterpret_cast<double *>(wbase + s.win_ring) : nullptr;
    if (win_state)  // every band's windows into its rows of the ring, window n in row n % Kb; the one count word serves all bands
        HIP_TRY(launch_stream_windows(partial, s.FB, a.Ks, a.Gp, G, 1, a.Gp / 2, a.CH, reinterpret_cast<const int *>(state), final_tile ? 1 : 0, window,
                                      hop, s.Kb, win_state, ring, nullptr, nullptr, nullptr, st));
    if (trk) {  // in front of the slide: the carry fill and the clock as they were before the tile; band f's rows of the staging array
        TrackBandsArgs ta{};
        for (int f = 0; f < F; ++f) {
            ta.src[f] = staging + f * band_rows;
            ta.Wp[f] = plans[f]->W.Wp;
            ta.GT[f] = plans[f]->W.GT;
        }
        HIP_TRY(launch_stream_track_bands_complex(ta, F, reinterpret_cast<const int *>(state), p0->C, B, a.S, G, trk->a_rise, trk->i_rise, trk->a_fall,
                                                  trk->state, trk->R, trk->index, trk->peak, trk->latest_index, trk->latest_peak, trk->ws, st));
    }
    HIP_TRY(launch_stream_complex_slide(staging, s.FB * p0->C, a.S, a.CH, state, a.L, st));
    StreamBandsArgs args{};
    for (int f = 0; f < F; ++f) {
        args.power[f] = bp + (size_t)f * B * G;
        if (win_state) {
            args.rows[f] = ring + (size_t)f * B * s.Kb * G;
            args.count[f] = reinterpret_cast<const int32_t *>(win_state);
        }
    }
    // (without windows the band sum reads no word of its state: the stream's own stands in for the non-NULL pointer the launcher wants)
    HIP_TRY(launch_stream_band_sum(args, F, B, G, win_state != nullptr, s.Kb, max_windows, win_state ? (void *)(wbase + SCB_BANDS_WORDS) : state, power,
                                   argmax, window_power, window_argmax, latest_power, latest_argmax, st));
    return MICLOC_OK;
}

}  // namespace

extern "C" {

size_t micloc_stream_complex_bands_state_bytes(const micloc_plan *const *plans, int F, int B)
{
    ScbArgs s;
    return scb_args(plans, F, B, 0, &s) == MICLOC_OK ? s.a.L.total : 0;
}

size_t micloc_stream_complex_bands_workspace_bytes(const micloc_plan *const *plans, int F, int B, int max_tile)
{
    ScbArgs s;
    if (max_tile < 1 || scb_args(plans, F, B, max_tile, &s) != MICLOC_OK) return 0;
    return s.ws_total;
}

int micloc_stream_complex_bands_reset(const micloc_plan *const *plans, int F, int B, void *state, size_t state_bytes, void *stream)
{
    if (!plans || !state) return MICLOC_ERR_INVALID;
    ScbArgs s;
    const int rc = scb_args(plans, F, B, 0, &s);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, s.a.L.total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(plans[0]->device);
    HIP_TRY(launch_zero_fill(state, s.a.L.total, (hipStream_t)stream));  // clock, zero DF2T state, empty carry, accumulators
    return MICLOC_OK;
}

int micloc_stream_complex_bands_bandpass_tile_f64(const micloc_plan *const *plans, int F, const double *h, int B, int n, int row_stride,
                                                  int first_col, int max_tile, int chains_per_workgroup, void *state, size_t state_bytes, void *ws,
                                                  size_t ws_bytes, void *stream)
{
    if (!plans || !h || !state || !ws || n < 1 || max_tile < 1 || first_col < 0 || row_stride < 1) return MICLOC_ERR_INVALID;
    if (chains_per_workgroup != 0 && chains_per_workgroup != 16 && chains_per_workgroup != 32 && chains_per_workgroup != 64) return MICLOC_ERR_INVALID;
    ScbArgs s;
    const int rc = scb_args(plans, F, B, max_tile, &s);
    if (rc != MICLOC_OK) return rc;
    if (n > max_tile || (long long)first_col + n > row_stride) return MICLOC_ERR_SHAPE;
    if (bad_ws(state, state_bytes, s.a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, s.ws_total)) return MICLOC_ERR_WORKSPACE;
    const micloc_plan *p0 = plans[0];
    DeviceGuard guard(p0->device);
    FilterbankCoef pc;
    cbands_coef(plans, F, &pc);
    HIP_TRY(launch_stream_bands_bandpass(pc, h + first_col, F, B * p0->C, n, (size_t)row_stride, ws_doubles(ws, 0), s.a.S, s.a.CH, state, s.a.L,
                                         chains_per_workgroup, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_complex_bands_localize_tile_f64(const micloc_plan *const *plans, int F, void *state, size_t state_bytes, int B, int max_tile,
                                                  int final_tile, double *band_power, double *power, int32_t *argmax, void *ws, size_t ws_bytes,
                                                  void *stream)
{
    if (!plans || !state || !ws || max_tile < 1) return MICLOC_ERR_INVALID;
    ScbArgs s;
    const int rc = scb_args(plans, F, B, max_tile, &s);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, s.a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, s.ws_total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(plans[0]->device);
    return scb_localize(plans, F, B, s, state, final_tile, band_power, power, argmax, ws, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr,
                        (hipStream_t)stream);
}

size_t micloc_stream_complex_bands_window_state_bytes(const micloc_plan *const *plans, int F, int B, int max_tile, int window, int hop,
                                                      int max_windows)
{
    ScbArgs s;
    if (max_tile < 1 || scb_window_args(scb_args(plans, F, B, max_tile, &s), plans, window, hop, max_windows, &s) != MICLOC_OK) return 0;
    return s.win_total;
}

int micloc_stream_complex_bands_window_reset(const micloc_plan *const *plans, int F, int B, int max_tile, void *win_state, size_t win_bytes,
                                             int window, int hop, int max_windows, void *stream)
{
    if (!plans || !win_state || max_tile < 1) return MICLOC_ERR_INVALID;
    ScbArgs s;
    const int rc = scb_window_args(scb_args(plans, F, B, max_tile, &s), plans, window, hop, max_windows, &s);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(win_state, win_bytes, s.win_total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(plans[0]->device);
    HIP_TRY(launch_zero_fill(win_state, s.win_total, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_complex_bands_localize_tile_windows_f64(const micloc_plan *const *plans, int F, void *state, size_t state_bytes, int B,
                                                          int max_tile, int final_tile, double *band_power, double *power, int32_t *argmax,
                                                          void *ws, size_t ws_bytes, void *win_state, size_t win_bytes, int window, int hop,
                                                          int max_windows, double *window_power, int32_t *window_argmax, double *latest_power,
                                                          int32_t *latest_argmax, void *stream)
{
    if (!plans || !state || !ws || !win_state || !window_argmax || max_tile < 1) return MICLOC_ERR_INVALID;
    ScbArgs s;
    const int rc = scb_window_args(scb_args(plans, F, B, max_tile, &s), plans, window, hop, max_windows, &s);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, s.a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, s.ws_total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(win_state, win_bytes, s.win_total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(plans[0]->device);
    return scb_localize(plans, F, B, s, state, final_tile, band_power, power, argmax, ws, win_state, window, hop, max_windows, window_power,
                        window_argmax, latest_power, latest_argmax, (hipStream_t)stream);
}

/* status[0 .. 3] = micloc_stream_complex_status' words of the F * B rows; [4] = wideband windows emitted or given up, [5] = given up
 * (0 and 0 with win_state == NULL) (synchronises the stream) */
int micloc_stream_complex_bands_status(const void *state, const void *win_state, int *status6, void *stream)
{
    if (!state || !status6) return MICLOC_ERR_INVALID;
    int ctl[STREAM_CLK_T + 1], w[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(ctl, state, sizeof(ctl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (win_state)
        HIP_TRY(hipMemcpyAsync(w, reinterpret_cast<const unsigned char *>(win_state) + SCB_BANDS_WORDS, sizeof(w), hipMemcpyDeviceToHost,
                               (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status6[0] = ctl[0];
    status6[1] = ctl[8];
    status6[2] = ctl[2];
    status6[3] = ctl[STREAM_CLK_T];
    status6[4] = w[0];
    status6[5] = w[1];
    return MICLOC_OK;
}

/* device address of word [4] of micloc_stream_complex_bands_status (for kernels that follow the wideband windows: stream_peaks.hip) */
const int32_t *micloc_stream_complex_bands_window_count_ptr(const void *win_state)
{
    return win_state ? reinterpret_cast<const int32_t *>(reinterpret_cast<const unsigned char *>(win_state) + SCB_BANDS_WORDS) : nullptr;
}

}  // extern "C"

// ---- wideband streaming, tracking (stream_track_bands.hip; the rule: include/micloc_hip.h) --------------------------------------------------
namespace {

// what the stream serves of a set: MICLOC_OK, *cpx = the set's kind and (SNN) *CH = the bands' one chunk length -- or the status of the set
// rule (INVALID / NOT_SET from micloc_*_bands_track_is_fused), MICLOC_ERR_SHAPE for a set off the fused route, for SNN bands whose chunk
// lengths differ or whose LIF history 4 NK - 16 is longer than a chunk, and for complex bands that are not one chain
int stb_served(const micloc_plan *const *plans, int F, int B, bool *cpx, int *CH)
{
    *CH = 0;
    if (set_pointers(plans, F) != MICLOC_OK || bad_batch(B)) return MICLOC_ERR_INVALID;
    *cpx = plans[0]->W_is_complex != 0;
    const int fused = *cpx ? micloc_beamformer_bands_track_is_fused(plans, F) : micloc_snn_bands_track_is_fused(plans, F);
    if (fused < 0) return fused;
    if (fused != 1) return MICLOC_ERR_SHAPE;
    if (*cpx) {
        ScbArgs s;
        return scb_args(plans, F, B, 0, &s);
    }
    *CH = lif_beamform_chunk_frames(plans[0]->W, plans[0]->ntab);
    for (int f = 0; f < F; ++f)
        if (lif_beamform_chunk_frames(plans[f]->W, plans[f]->ntab) != *CH || stream_track_halo(plans[f]->ntab) > *CH) return MICLOC_ERR_SHAPE;
    return MICLOC_OK;
}

// the rule of the tracked arguments behind stb_served: `most` frames can become final in one tile, the pairs cover `cap` positions
int stb_track_args(const micloc_plan *p0, const TrackArgs &t, int B, int most, int cap)
{
    if (t.R < most) return MICLOC_ERR_SHAPE;
    if (bad_ws(t.state, t.state_bytes, stream_track_bands_state_bytes(B, p0->G_out))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(t.ws, t.ws_bytes, stream_track_pairs_bytes(B, cap, p0->G_out))) return MICLOC_ERR_WORKSPACE;
    return MICLOC_OK;
}

bool stb_missing(const TrackArgs &t) { return !t.state || !t.index || !t.peak || !t.latest_index || !t.latest_peak || t.R < 1; }

}  // namespace

extern "C" {

size_t micloc_stream_bands_track_state_bytes(const micloc_plan *const *plans, int F, int B)
{
    bool cpx;
    int CH;
    if (stb_served(plans, F, B, &cpx, &CH) != MICLOC_OK || plans[0]->G_out < 1) return 0;
    return stream_track_bands_state_bytes(B, plans[0]->G_out);
}

size_t micloc_stream_bands_track_workspace_bytes(const micloc_plan *const *plans, int F, int B, int frames)
{
    bool cpx;
    int CH;
    if (frames < 1 || stb_served(plans, F, B, &cpx, &CH) != MICLOC_OK || plans[0]->G_out < 1) return 0;
    int cap = frames;
    if (cpx) {  // the staging array of a complex stream whose longest tile has `frames` frames
        ScbArgs s;
        if (scb_args(plans, F, B, frames, &s) != MICLOC_OK) return 0;
        cap = s.a.S;
    } else if (frames % CH != 0) {
        return 0;
    }
    return stream_track_pairs_bytes(B, cap, plans[0]->G_out);
}

int micloc_stream_bands_track_reset(const micloc_plan *const *plans, int F, int B, void *track_state, size_t track_bytes, void *stream)
{
    if (!plans || !track_state) return MICLOC_ERR_INVALID;
    bool cpx;
    int CH;
    const int rc = stb_served(plans, F, B, &cpx, &CH);
    if (rc != MICLOC_OK) return rc;
    const size_t need = stream_track_bands_state_bytes(B, plans[0]->G_out);
    if (bad_ws(track_state, track_bytes, need)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(plans[0]->device);
    HIP_TRY(launch_zero_fill(track_state, need, (hipStream_t)stream));  // the frontier at frame 0, the envelope rows
    return MICLOC_OK;
}

int micloc_stream_bands_track_tile_f64(const micloc_plan *const *plans, int F, const void *const *loc_states, const int8_t *const *windows, int B,
                                       int window_frames, void *track_state, size_t track_bytes, double a_rise, double i_rise, double a_fall,
                                       int max_track, int32_t *track_index, double *track_peak, int32_t *latest_index, double *latest_peak,
                                       void *track_ws, size_t track_ws_bytes, void *stream)
{
    const TrackArgs trk{track_state, track_bytes, a_rise, i_rise, a_fall, max_track, track_index, track_peak, latest_index, latest_peak, track_ws,
                        track_ws_bytes};
    if (set_pointers(plans, F) != MICLOC_OK || !loc_states || !windows || bad_batch(B) || window_frames < 1 || stb_missing(trk)) return MICLOC_ERR_INVALID;
    for (int f = 0; f < F; ++f)
        if (!loc_states[f] || !windows[f]) return MICLOC_ERR_INVALID;
    bool cpx;
    int CH;
    int rc = stb_served(plans, F, B, &cpx, &CH);
    if (rc != MICLOC_OK) return rc;
    if (cpx || window_frames % CH != 0) return MICLOC_ERR_SHAPE;
    const micloc_plan *p0 = plans[0];
    rc = stb_track_args(p0, trk, B, window_frames, window_frames);  // a tile can make every frame of the windows final
    if (rc != MICLOC_OK) return rc;
    DeviceGuard guard(p0->device);
    TrackBandsArgs ta{};
    TrackBandsCtl tc{};
    int NKmax = 0;
    for (int f = 0; f < F; ++f) {
        ta.src[f] = windows[f];
        ta.tab[f] = plans[f]->ntab.tab;
        ta.Wp[f] = plans[f]->W.Wp;
        ta.NK[f] = plans[f]->ntab.NK;
        ta.GT[f] = plans[f]->W.GT;
        tc.ctl[f] = reinterpret_cast<const int *>(loc_states[f]);
        if (ta.NK[f] > NKmax) NKmax = ta.NK[f];
    }
    HIP_TRY(launch_stream_track_bands(ta, tc, F, NKmax, p0->C, B, window_frames, CH, p0->G_out, a_rise, i_rise, a_fall, track_state, max_track,
                                      track_index, track_peak, latest_index, latest_peak, track_ws, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_complex_bands_localize_tile_track_f64(const micloc_plan *const *plans, int F, void *state, size_t state_bytes, int B, int max_tile,
                                                        int final_tile, double *band_power, double *power, int32_t *argmax, void *ws,
                                                        size_t ws_bytes, void *win_state, size_t win_bytes, int window, int hop, int max_windows,
                                                        double *window_power, int32_t *window_argmax, double *latest_power,
                                                        int32_t *latest_argmax, void *track_state, size_t track_bytes, double a_rise,
                                                        double i_rise, double a_fall, int max_track, int32_t *track_index, double *track_peak,
                                                        int32_t *latest_index, double *latest_peak, void *track_ws, size_t track_ws_bytes,
                                                        void *stream)
{
    const TrackArgs trk{track_state, track_bytes, a_rise, i_rise, a_fall, max_track, track_index, track_peak, latest_index, latest_peak, track_ws,
                        track_ws_bytes};
    if (!plans || !state || !ws || (win_state && !window_argmax) || max_tile < 1 || stb_missing(trk)) return MICLOC_ERR_INVALID;
    ScbArgs s;
    int rc = scb_args(plans, F, B, max_tile, &s);
    if (win_state) rc = scb_window_args(rc, plans, window, hop, max_windows, &s);
    if (rc != MICLOC_OK) return rc;
    bool cpx;
    int CH;
    rc = stb_served(plans, F, B, &cpx, &CH);
    if (rc != MICLOC_OK) return rc;
    rc = stb_track_args(plans[0], trk, B, max_tile, s.a.S);  // a tile makes its own frames final, no more
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, s.a.L.total)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, s.ws_total)) return MICLOC_ERR_WORKSPACE;
    if (win_state && bad_ws(win_state, win_bytes, s.win_total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(plans[0]->device);
    return scb_localize(plans, F, B, s, state, final_tile, band_power, power, argmax, ws, win_state, window, hop, max_windows, window_power,
                        window_argmax, latest_power, latest_argmax, (hipStream_t)stream, &trk);
}

/* the tracked frontier of the SNN bands in absolute frames: every frame below it has been emitted (synchronises the stream) */
int micloc_stream_bands_track_status(const void *track_state, int *frontier, void *stream)
{
    if (!track_state || !frontier) return MICLOC_ERR_INVALID;
    HIP_TRY(hipMemcpyAsync(frontier, reinterpret_cast<const int *>(track_state) + STB_FRONT, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return MICLOC_OK;
}

}  // extern "C"

// ---- streaming, MUSIC (stream_music.hip; the rule: include/micloc_hip.h) ------------------------------------------------------------------
namespace {

// MICLOC_OK and *d, or the status of the rule's argument errors
int sm_args(int B, int M, int L, int hop, int N, int nbin, int G, int k, int max_slices, MusicStreamDims *d)
{
    if (bad_batch(B) || M < 1 || L < 1 || hop < 1 || N < 2 || nbin < 1 || G < 1 || k < 0 || max_slices < 1) return MICLOC_ERR_INVALID;
    return music_stream_dims(B, M, L, hop, N, nbin, G, k, max_slices, d) ? MICLOC_OK : MICLOC_ERR_SHAPE;
}

}  // namespace

extern "C" {

size_t micloc_stream_music_state_bytes(int B, int M, int L, int hop, int N, int nbin, int G, int k, int max_slices)
{
    MusicStreamDims d{};
    if (sm_args(B, M, L, hop, N, nbin, G, k, max_slices, &d) != MICLOC_OK) return 0;
    return music_stream_layout(d).total;
}

int micloc_stream_music_reset(void *state, size_t state_bytes, int B, int M, int L, int hop, int N, int nbin, int G, int k, int max_slices,
                              void *stream)
{
    if (!state) return MICLOC_ERR_INVALID;
    MusicStreamDims d{};
    const int rc = sm_args(B, M, L, hop, N, nbin, G, k, max_slices, &d);
    if (rc != MICLOC_OK) return rc;
    const size_t total = music_stream_layout(d).total;
    if (bad_ws(state, state_bytes, total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(state));
    // clock 0, lfilter's zero state, no slice emitted, sum 0, and the zero padding of the frame rows (columns N .. Np, rows R .. Rp)
    HIP_TRY(launch_zero_fill(state, total, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_music_tile_f64(void *state, size_t state_bytes, const double *x_tile, int B, int n, int M, int final_tile, const double *b,
                                 const double *a, int ncoef, int L, int hop, int N, const double *W, int nbin, const double *steer_re,
                                 const double *steer_im, int G, int k, int max_slices, double *power, int32_t *argmax, double *latest_spec,
                                 int32_t *latest_argmax, double *slice_spec, int32_t *slice_sel, int32_t *slice_argmax, void *stream)
{
    if (!state || !x_tile || !b || !a || !W || !steer_re || !steer_im || n < 1 || ncoef < 1 || ncoef > MICLOC_MAX_IIR || a[0] == 0.0)
        return MICLOC_ERR_INVALID;
    MusicStreamDims d{};
    const int rc = sm_args(B, M, L, hop, N, nbin, G, k, max_slices, &d);
    if (rc != MICLOC_OK) return rc;
    if (bad_ws(state, state_bytes, music_stream_layout(d).total)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(state));
    IirCoef co{};
    co.n = ncoef;
    for (int i = 0; i < ncoef; ++i) {
        co.b[i] = b[i] / a[0];
        co.a[i] = a[i] / a[0];
    }
    HIP_TRY(launch_music_stream_tile(d, co, x_tile, n, final_tile ? 1 : 0, state, W, steer_re, steer_im, power, argmax, latest_spec, latest_argmax,
                                     slice_spec, slice_sel, slice_argmax, (hipStream_t)stream));
    return MICLOC_OK;
}

/* status[0] = samples pushed, [1] = slices emitted, [2] = open slices, [3] = 1 when the final tile left a leftover slice shorter than N
 * (synchronises the stream) */
int micloc_stream_music_status(const void *state, int *status4, void *stream)
{
    if (!state || !status4) return MICLOC_ERR_INVALID;
    int clk[4];
    HIP_TRY(hipMemcpyAsync(clk, state, sizeof(clk), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status4[0] = clk[0];
    status4[1] = clk[1];
    status4[2] = clk[3];
    status4[3] = clk[2];
    return MICLOC_OK;
}

/* device address of word [1] of micloc_stream_music_status, the slices emitted (for kernels that follow the slices: stream_peaks.hip) */
const int32_t *micloc_stream_music_slice_count_ptr(const void *state)
{
    return state ? reinterpret_cast<const int32_t *>(state) + 1 : nullptr;
}

}  // extern "C"
