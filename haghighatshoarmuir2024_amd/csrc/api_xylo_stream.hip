// C-ABI of libmicloc_hip.so (see include/micloc_hip.h "streaming, Xylo" for the contract): the packed integer LIF resumable across
// launches, one tile of a band's Xylo stream behind micloc_stream_encode_tile_f64, the read-out over the bands, and the tracked form of the
// first two ("streaming, Xylo tracking": a DoA index and a peak envelope per frame).  PARITY UNPINNED
// like every Xylo entry (the oracle restates the published update rule; it is not checked against XyloSim).
#include "api_internal.h"
#include "stream_xylo.h"

using namespace micloc;

namespace {

constexpr int CH = XYLO_STREAM_CHUNK;
constexpr size_t XS_LOC_BYTES = 256;  // the control words of a band's stream (the STREAM_CLK_* clock among them)

// the network's shape rule of the stream: the w_rec == 0 packed form, Cin = 2 x ternary channels <= 64
int xs_net_args(int ternary_channels, int Cin, int N, int max_spikes)
{
    if (ternary_channels < 1 || Cin < 1 || N < 1 || max_spikes < 1) return MICLOC_ERR_INVALID;
    if (Cin != 2 * ternary_channels || Cin > 64) return MICLOC_ERR_SHAPE;
    return MICLOC_OK;
}

// the window rule of the Xylo stream: multiples of the 256-frame chunk, hop <= window, a ring of at least one row
int xs_window_args(int window, int hop, int ring_depth)
{
    if (window < 1 || hop < 1 || ring_depth < 1) return MICLOC_ERR_INVALID;
    if (window % CH != 0 || hop % CH != 0 || hop > window) return MICLOC_ERR_SHAPE;
    return MICLOC_OK;
}

// the tracked read-out of a call (track == NULL: the counting LIF): the envelope state, the rule's constants, the ring, the scratch
struct XsTrack {
    void *state;
    size_t state_bytes;
    double a_rise, i_rise, a_fall;
    int R;
    int32_t *index;
    double *peak;
    int32_t *latest_index;
    double *latest_peak;
    double *env_last;
    void *ws;
    size_t ws_bytes;
};

// its status, before any launch; cap: the positions of the pair scratch, most: the frames one call can make final
int xs_track_args(const XsTrack &t, int B, int N, int cap, int most)
{
    if (!t.state || !t.index || !t.peak || !t.latest_index || !t.latest_peak || !t.env_last || !t.ws || t.R < 1) return MICLOC_ERR_INVALID;
    if (t.R < most) return MICLOC_ERR_SHAPE;
    if (bad_ws(t.state, t.state_bytes, xylo_stream_track_state_bytes(B, N))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(t.ws, t.ws_bytes, xylo_stream_track_pairs_bytes(B, N, cap))) return MICLOC_ERR_WORKSPACE;
    return MICLOC_OK;
}

// the launches of a tile behind the encoder: horizon, the resumable LIF over the chunks that became final -- counting or (track) tracking --,
// (the window read-out,) commit, tick
int xs_tile(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *raster, int B, int window_frames,
            int final_tile, int N, int max_spikes, int32_t *counts, void *lif_state, size_t lif_bytes, void *net_ws, size_t net_bytes, void *ws,
            size_t ws_bytes, void *win_state, size_t win_bytes, int window, int hop, int ring_depth, void *stream, const XsTrack *track = nullptr)
{
    if (!p || !enc_state || !loc_state || !raster || !counts || !lif_state || !net_ws || bad_batch(B) || window_frames < 1) return MICLOC_ERR_INVALID;
    if (win_state && !ws) return MICLOC_ERR_INVALID;
    const int Cin = 2 * p->C;
    int rc = xs_net_args(p->C, Cin, N, max_spikes);
    if (rc == MICLOC_OK && win_state) rc = xs_window_args(window, hop, ring_depth);
    if (rc != MICLOC_OK) return rc;
    if (!p->bipolar || window_frames % CH != 0 || (reinterpret_cast<uintptr_t>(raster) & 15) != 0) return MICLOC_ERR_SHAPE;
    const int rows = window_frames / CH;
    if (bad_ws(loc_state, loc_bytes, XS_LOC_BYTES)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(lif_state, lif_bytes, xylo_stream_state_bytes(B, N))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(net_ws, net_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    if (ws && bad_ws(ws, ws_bytes, xylo_stream_chunk_bytes(B, N, rows))) return MICLOC_ERR_WORKSPACE;
    if (win_state && bad_ws(win_state, win_bytes, xylo_stream_window_state_bytes(B, N, window, hop, ring_depth))) return MICLOC_ERR_WORKSPACE;
    if (track && (rc = xs_track_args(*track, B, N, window_frames, window_frames)) != MICLOC_OK) return rc;
    DeviceGuard guard(p->device);
    hipStream_t st = (hipStream_t)stream;
    int *ctl = reinterpret_cast<int *>(loc_state);
    int32_t *chunk_counts = win_state ? reinterpret_cast<int32_t *>(ws) : nullptr;
    HIP_TRY(launch_stream_horizon(enc_state, B * p->C, p->bipolar, 0, final_tile ? 1 : 0, CH, 0, rows, ctl, st, 1));
    // the whole window as the launch shape; the kernel takes its frame range from the control words
    if (track)
        HIP_TRY(launch_xylo_track_resume(raster, p->C, window_frames, B, 0, 0, ctl, Cin, N, max_spikes, counts, lif_state, track->state, net_ws,
                                         chunk_counts, rows, track->a_rise, track->i_rise, track->a_fall, track->R, track->index, track->peak,
                                         track->latest_index, track->latest_peak, track->env_last, track->ws, window_frames, st));
    else
        HIP_TRY(launch_xylo_resume(raster, p->C, window_frames, B, 0, 0, ctl, Cin, N, max_spikes, nullptr, 0, counts, lif_state, net_ws, chunk_counts, rows,
                                   st));
    if (win_state) HIP_TRY(launch_xylo_stream_windows(chunk_counts, B, rows, N, ctl, final_tile, window, hop, ring_depth, win_state, st));
    HIP_TRY(launch_stream_commit(ctl, STREAM_BLOCK_CHUNKS, st));
    HIP_TRY(launch_stream_tick(ctl, st));
    return MICLOC_OK;
}

}  // namespace

extern "C" {

// ---- the resumable LIF by value ------------------------------------------------------------------------------------------------
size_t micloc_xylo_stream_state_bytes(int B, int N)
{
    if (bad_batch(B) || N < 1) return 0;
    return xylo_stream_state_bytes(B, N);
}

int micloc_xylo_stream_reset(void *state, size_t bytes, void *stream)
{
    if (!state || bytes < 1) return MICLOC_ERR_INVALID;
    if (bad_ws(state, bytes, 16)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(state));
    HIP_TRY(launch_zero_fill(state, bytes, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_xylo_lif_resume_i16(const int8_t *raster, int ternary_channels, int trial_stride_frames, int B, int t0, int n, int Cin, int N,
                               int max_spikes, uint8_t *spikes_out, int T_out, int32_t *counts, void *state, size_t state_bytes, void *ws,
                               size_t ws_bytes, void *stream)
{
    if (!raster || !counts || !state || !ws || bad_batch(B) || trial_stride_frames < 1 || t0 < 0 || n < 0) return MICLOC_ERR_INVALID;
    const int rc = xs_net_args(ternary_channels, Cin, N, max_spikes);
    if (rc != MICLOC_OK) return rc;
    if (t0 % 16 != 0 || (long long)t0 + n > trial_stride_frames || (reinterpret_cast<uintptr_t>(raster) & 15) != 0) return MICLOC_ERR_SHAPE;
    if (spikes_out && (long long)t0 + n > T_out) return MICLOC_ERR_SHAPE;
    if (bad_ws(state, state_bytes, xylo_stream_state_bytes(B, N))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ws));
    HIP_TRY(launch_xylo_resume(raster, ternary_channels, trial_stride_frames, B, t0, n, nullptr, Cin, N, max_spikes, spikes_out, T_out, counts, state, ws,
                               nullptr, 0, (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- the tracked read-out ("streaming, Xylo tracking") ---------------------------------------------------------------------------
size_t micloc_xylo_stream_track_state_bytes(int B, int N)
{
    if (bad_batch(B) || N < 1) return 0;
    return xylo_stream_track_state_bytes(B, N);
}

size_t micloc_xylo_stream_track_workspace_bytes(int B, int N, int window_frames)
{
    if (bad_batch(B) || N < 1 || window_frames < 1) return 0;
    return xylo_stream_track_pairs_bytes(B, N, window_frames);
}

int micloc_xylo_stream_track_reset(void *track_state, size_t track_bytes, int B, int N, void *stream)
{
    if (!track_state || bad_batch(B) || N < 1) return MICLOC_ERR_INVALID;
    const size_t need = xylo_stream_track_state_bytes(B, N);
    if (bad_ws(track_state, track_bytes, need)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(track_state));
    HIP_TRY(launch_zero_fill(track_state, need, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_xylo_lif_track_resume_i16(const int8_t *raster, int ternary_channels, int trial_stride_frames, int B, int t0, int n, int Cin, int N,
                                     int max_spikes, void *state, size_t state_bytes, void *track_state, size_t track_bytes, double a_rise,
                                     double i_rise, double a_fall, int max_track, int32_t *track_index, double *track_peak, int32_t *latest_index,
                                     double *latest_peak, double *env_last, int32_t *counts, void *ws, size_t ws_bytes, void *track_ws,
                                     size_t track_ws_bytes, void *stream)
{
    if (!raster || !counts || !state || !ws || bad_batch(B) || trial_stride_frames < 1 || t0 < 0 || n < 0) return MICLOC_ERR_INVALID;
    int rc = xs_net_args(ternary_channels, Cin, N, max_spikes);
    if (rc != MICLOC_OK) return rc;
    if (t0 % 16 != 0 || (long long)t0 + n > trial_stride_frames || (reinterpret_cast<uintptr_t>(raster) & 15) != 0) return MICLOC_ERR_SHAPE;
    if (bad_ws(state, state_bytes, xylo_stream_state_bytes(B, N))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(ws, ws_bytes, xylo_ws_bytes(Cin, N))) return MICLOC_ERR_WORKSPACE;
    const XsTrack t{track_state, track_bytes, a_rise, i_rise, a_fall, max_track, track_index, track_peak, latest_index, latest_peak, env_last,
                    track_ws, track_ws_bytes};
    const int cap = n > 0 ? n : 1;  // the pair scratch holds the frames of this call
    if ((rc = xs_track_args(t, B, N, cap, n)) != MICLOC_OK) return rc;
    DeviceGuard guard(device_of(ws));
    HIP_TRY(launch_xylo_track_resume(raster, ternary_channels, trial_stride_frames, B, t0, n, nullptr, Cin, N, max_spikes, counts, state, track_state, ws,
                                     nullptr, 0, a_rise, i_rise, a_fall, max_track, track_index, track_peak, latest_index, latest_peak, env_last, track_ws,
                                     cap, (hipStream_t)stream));
    return MICLOC_OK;
}

// ---- one band's stream -----------------------------------------------------------------------------------------------------------
size_t micloc_stream_xylo_state_bytes(void) { return XS_LOC_BYTES; }

size_t micloc_stream_xylo_workspace_bytes(int B, int N, int window_frames)
{
    if (bad_batch(B) || N < 1 || window_frames < 1 || window_frames % CH != 0) return 0;
    return xylo_stream_chunk_bytes(B, N, window_frames / CH);
}

int micloc_stream_xylo_reset(const micloc_plan *p, int B, void *enc_state, size_t enc_bytes, void *loc_state, size_t loc_bytes, int8_t *window,
                             int window_frames, int N, void *lif_state, size_t lif_bytes, int32_t *counts, void *stream)
{
    if (!p || !enc_state || !loc_state || !window || !lif_state || !counts || bad_batch(B) || window_frames < 1 || N < 1) return MICLOC_ERR_INVALID;
    if (window_frames % CH != 0) return MICLOC_ERR_SHAPE;
    if (bad_ws(enc_state, enc_bytes, rzcc_stream_state_bytes(B * p->C))) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(loc_state, loc_bytes, XS_LOC_BYTES)) return MICLOC_ERR_WORKSPACE;
    if (bad_ws(lif_state, lif_bytes, xylo_stream_state_bytes(B, N))) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(p->device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(launch_zero_fill(enc_state, 256, st));  // overflow counter (the encoder's own state is written by the first tile)
    HIP_TRY(launch_zero_fill(loc_state, XS_LOC_BYTES, st));  // control words, clock
    HIP_TRY(launch_zero_fill(window, (size_t)B * window_frames * p->C, st));
    HIP_TRY(launch_zero_fill(lif_state, xylo_stream_state_bytes(B, N), st));  // zero synaptic current, membrane and counts
    HIP_TRY(launch_zero_fill(counts, (size_t)B * N * sizeof(int32_t), st));
    return MICLOC_OK;
}

int micloc_stream_xylo_begin_tile(const micloc_plan *p, void *loc_state, int8_t *window, int8_t *scratch_window, int B, int n, int window_frames,
                                  void *stream)
{
    if (!p || !loc_state || !window || !scratch_window || window == scratch_window || bad_batch(B) || n < 1 || window_frames < 1) return MICLOC_ERR_INVALID;
    if (window_frames % CH != 0 || n > window_frames) return MICLOC_ERR_SHAPE;
    DeviceGuard guard(p->device);
    HIP_TRY(launch_stream_begin_tile(reinterpret_cast<int *>(loc_state), window, scratch_window, B, (size_t)window_frames * p->C, p->C, n, window_frames,
                                     CH, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_xylo_tile_i16(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window, int B,
                                int window_frames, int final_tile, int N, int max_spikes, int32_t *counts, void *lif_state, size_t lif_bytes,
                                void *net_ws, size_t net_ws_bytes, void *stream)
{
    return xs_tile(p, enc_state, loc_state, loc_bytes, window, B, window_frames, final_tile, N, max_spikes, counts, lif_state, lif_bytes, net_ws,
                   net_ws_bytes, nullptr, 0, nullptr, 0, 0, 0, 0, stream);
}

size_t micloc_stream_xylo_window_state_bytes(int B, int N, int window, int hop, int ring_depth)
{
    if (bad_batch(B) || N < 1 || xs_window_args(window, hop, ring_depth) != MICLOC_OK) return 0;
    return xylo_stream_window_state_bytes(B, N, window, hop, ring_depth);
}

int micloc_stream_xylo_window_reset(void *win_state, size_t win_bytes, int B, int N, int window, int hop, int ring_depth, void *stream)
{
    if (!win_state || bad_batch(B) || N < 1) return MICLOC_ERR_INVALID;
    const int rc = xs_window_args(window, hop, ring_depth);
    if (rc != MICLOC_OK) return rc;
    const size_t need = xylo_stream_window_state_bytes(B, N, window, hop, ring_depth);
    if (bad_ws(win_state, win_bytes, need)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(win_state));
    HIP_TRY(launch_zero_fill(win_state, need, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_xylo_tile_windows_i16(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window_raster,
                                        int B, int window_frames, int final_tile, int N, int max_spikes, int32_t *counts, void *lif_state,
                                        size_t lif_bytes, void *net_ws, size_t net_ws_bytes, void *ws, size_t ws_bytes, void *win_state,
                                        size_t win_bytes, int window, int hop, int ring_depth, void *stream)
{
    if (!win_state || !ws) return MICLOC_ERR_INVALID;
    return xs_tile(p, enc_state, loc_state, loc_bytes, window_raster, B, window_frames, final_tile, N, max_spikes, counts, lif_state, lif_bytes, net_ws,
                   net_ws_bytes, ws, ws_bytes, win_state, win_bytes, window, hop, ring_depth, stream);
}

// xs_tile with the tracking LIF (and its combine launch beyond 512 neurons) in place of the counting one; win_state == NULL: no windows
int micloc_stream_xylo_tile_track_i16(const micloc_plan *p, const void *enc_state, void *loc_state, size_t loc_bytes, const int8_t *window_raster,
                                      int B, int window_frames, int final_tile, int N, int max_spikes, int32_t *counts, void *lif_state,
                                      size_t lif_bytes, void *net_ws, size_t net_ws_bytes, void *ws, size_t ws_bytes, void *win_state,
                                      size_t win_bytes, int window, int hop, int ring_depth, void *track_state, size_t track_bytes, double a_rise,
                                      double i_rise, double a_fall, int max_track, int32_t *track_index, double *track_peak, int32_t *latest_index,
                                      double *latest_peak, double *env_last, void *track_ws, size_t track_ws_bytes, void *stream)
{
    const XsTrack t{track_state, track_bytes, a_rise, i_rise, a_fall, max_track, track_index, track_peak, latest_index, latest_peak, env_last,
                    track_ws, track_ws_bytes};
    if (!win_state) return xs_tile(p, enc_state, loc_state, loc_bytes, window_raster, B, window_frames, final_tile, N, max_spikes, counts, lif_state,
                                   lif_bytes, net_ws, net_ws_bytes, nullptr, 0, nullptr, 0, 0, 0, 0, stream, &t);
    if (!ws) return MICLOC_ERR_INVALID;
    return xs_tile(p, enc_state, loc_state, loc_bytes, window_raster, B, window_frames, final_tile, N, max_spikes, counts, lif_state, lif_bytes, net_ws,
                   net_ws_bytes, ws, ws_bytes, win_state, win_bytes, window, hop, ring_depth, stream, &t);
}

/* status[0] = chunks integrated, [1] = frames integrated, [2] = window-lag failures, [3] = frames pushed (synchronises the stream) */
int micloc_stream_xylo_status(const void *loc_state, int *status4, void *stream)
{
    if (!loc_state || !status4) return MICLOC_ERR_INVALID;
    int ctl[STREAM_CLK_T + 1];
    HIP_TRY(hipMemcpyAsync(ctl, loc_state, sizeof(ctl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status4[0] = ctl[0];
    status4[1] = ctl[8];
    status4[2] = ctl[13];
    status4[3] = ctl[STREAM_CLK_T];
    return MICLOC_OK;
}

// ---- the read-out over the bands -------------------------------------------------------------------------------------------------
size_t micloc_stream_xylo_readout_state_bytes(void) { return XYLO_STREAM_READOUT_STATE_BYTES; }

int micloc_stream_xylo_readout_reset(void *ro_state, size_t bytes, void *stream)
{
    if (!ro_state) return MICLOC_ERR_INVALID;
    if (bad_ws(ro_state, bytes, XYLO_STREAM_READOUT_STATE_BYTES)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ro_state));
    HIP_TRY(launch_zero_fill(ro_state, XYLO_STREAM_READOUT_STATE_BYTES, (hipStream_t)stream));
    return MICLOC_OK;
}

int micloc_stream_xylo_readout(int F, int B, int G, double fs, int win_size, const int32_t *const *band_counts, const void *const *band_loc_state,
                               int window, int hop, int ring_depth, int max_windows, void *const *band_win_state, void *ro_state, size_t ro_bytes,
                               int32_t *counts, double *rate, int32_t *peak, int32_t *window_counts, double *window_rate, int32_t *window_peak,
                               int32_t *latest_counts, double *latest_rate, int32_t *latest_peak, void *stream)
{
    if (!band_counts || !band_loc_state || !ro_state || !counts || !rate || !peak || F < 1 || F > MICLOC_MAX_BANDS || bad_batch(B) || G < 1 ||
        !(fs > 0.0) || window < 0)
        return MICLOC_ERR_INVALID;
    if (win_size < 1 || win_size % 2 != 1 || win_size > G / 2) return MICLOC_ERR_INVALID;  // micloc_peak_location_i32's rule
    if (window > 0 && (!band_win_state || !window_counts || !window_rate || !window_peak || max_windows < 1)) return MICLOC_ERR_INVALID;
    XyloReadoutArgs a{};
    for (int f = 0; f < F; ++f) {
        if (!band_counts[f] || !band_loc_state[f] || (window > 0 && !band_win_state[f])) return MICLOC_ERR_INVALID;
        a.counts[f] = band_counts[f];
        a.ctl[f] = reinterpret_cast<const int *>(band_loc_state[f]);
    }
    if (window > 0) {
        const int rc = xs_window_args(window, hop, ring_depth);
        if (rc != MICLOC_OK) return rc;
    }
    if (G > xylo_stream_readout_max_grid()) return MICLOC_ERR_SHAPE;
    if (bad_ws(ro_state, ro_bytes, XYLO_STREAM_READOUT_STATE_BYTES)) return MICLOC_ERR_WORKSPACE;
    DeviceGuard guard(device_of(ro_state));
    HIP_TRY(launch_xylo_stream_readout(a, band_win_state, F, B, G, fs, win_size, window, hop, ring_depth, max_windows, ro_state, counts, rate, peak,
                                       window_counts, window_rate, window_peak, latest_counts, latest_rate, latest_peak, (hipStream_t)stream));
    return MICLOC_OK;
}

/* status[0] = windows emitted or given up so far, [1] = windows given up because a band's ring had overwritten them (synchronises the stream) */
int micloc_stream_xylo_readout_status(const void *ro_state, int *status2, void *stream)
{
    if (!ro_state || !status2) return MICLOC_ERR_INVALID;
    int w[2];
    HIP_TRY(hipMemcpyAsync(w, ro_state, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    status2[0] = w[0];
    status2[1] = w[1];
    return MICLOC_OK;
}

}  // extern "C"
