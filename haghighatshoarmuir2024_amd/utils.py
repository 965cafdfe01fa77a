"""Host utilities with the reference's call surface (micloc/utils.py: Envelope :15-81,
find_peak_location :84-121), and the multi-source read-out `find_doa_peaks`.  Post-processing outside the hot path; the moving-target read-out (Envelope over the T x G beamformer
output + per-step arg-max, paper_plots/target_snn_localization.py:599-622) has a device form so that T x G never crosses PCIe."""
import warnings

import numpy as np


class Envelope:
    def __init__(self, rise_time, fall_time, fs):
        if rise_time > fall_time:
            raise ValueError("for proper functioning, an envelope estimator should have a larger fall time!")
        self.rise_time = rise_time
        self.fall_time = fall_time
        self.fs = fs
        # index 0: falling, index 1: rising
        self.win_lens = np.asarray([int(fs * fall_time), int(fs * rise_time)])

    def evolve(self, sig_in):
        """`T x num_chan` in, the envelope of every channel out (reference :36-81).  A float64 DEVICE tensor ([T, G] or a batch
        [B, T, G], e.g. `apply_to_signal(..., to_host=False)`) is processed by the device kernel (micloc_envelope_track_f64: the same
        recurrence in the same order of operations, bit-identical) and a device tensor comes back; a NumPy array takes the reference's
        host loop."""
        if _is_device_tensor(sig_in):
            from . import runtime

            T, channel = sig_in.shape[-2:]
            if T < channel:
                warnings.warn("number of channels in the input signal is larger than number of samples in each channel!")
            return runtime.envelope_track(sig_in, self.win_lens[0], self.win_lens[1], want_index=False)[0]
        T, channel = sig_in.shape
        if T < channel:
            warnings.warn("number of channels in the input signal is larger than number of samples in each channel!")
        # (float64 from the start: what the reference's list of rows becomes in `np.asarray` -- an integer raster, target_xylo_localization.py:
        #  757-768, stays exact; a complex array gives its modulus)
        mag = np.abs(sig_in).astype(np.float64)
        state = np.array(mag[0], copy=True)
        out = np.empty_like(mag)
        for t in range(1, T):
            out[t - 1] = state
            rising = (mag[t] >= state).astype(int)
            inv_len = 1 / self.win_lens[rising]
            state = (1 - inv_len) * state + inv_len * mag[t] * rising
        out[T - 1] = state
        return out

    def track(self, sig_in, want_envelope=False):
        """The moving-target read-out of paper_plots/target_snn_localization.py:599-622 in one call: `np.argmax(self.evolve(sig_bf), axis=1)`
        -- the DoA index per time step -- for a device tensor [T, G] / [B, T, G] without the T x G array leaving the device (17 MB per
        0.1 s at G = 449; the script's 5 s recording: 862 MB): returns int32 indices on the device (and the envelope if asked for).  A
        NumPy array takes the host class and returns NumPy."""
        if _is_device_tensor(sig_in):
            from . import runtime

            env, idx = runtime.envelope_track(sig_in, self.win_lens[0], self.win_lens[1], want_index=True)
            return (idx, env) if want_envelope else idx
        env = self.evolve(sig_in)
        idx = np.argmax(env, axis=1)
        return (idx, env) if want_envelope else idx


def _is_device_tensor(x):
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def find_peak_location(sig_in, win_size, periodic=True):
    """argmax of the box-car smoothed signal (full, NON-circular convolution as in the reference)."""
    sig_in = np.asarray(sig_in)
    if sig_in.ndim != 1:
        raise ValueError("input signal should be 1-dim!")
    if win_size % 2 != 1:
        raise ValueError("averaging window size should be odd to not create confusion in peak index!")
    if win_size > len(sig_in) // 2:
        raise ValueError("size of averaging window is larger than half the length of input signal!")
    smoothed = np.convolve(np.ones(win_size), sig_in, mode="full")
    index = int(np.argmax(smoothed)) - win_size // 2
    if periodic:
        index = index % len(sig_in)
    return index


def doa_grid_kind(doa_list, tol=1e-9):
    """The kind of a DoA grid for find_doa_peaks: "circular_closed" when it spans 2 pi end to end (np.linspace(-pi, pi, G): first
    and last point are one direction), "circular" when its G points cover one period without a duplicate (uniform step, span + step
    = 2 pi), "linear" otherwise; `tol` applies to the span."""
    doa = np.asarray(doa_list, dtype=np.float64)
    G = len(doa)
    if G < 2:
        return "linear"
    span = doa[-1] - doa[0]
    if abs(span - 2 * np.pi) <= tol:
        return "circular_closed"
    if abs(span * G / (G - 1) - 2 * np.pi) <= tol:
        return "circular"
    return "linear"


def doa_peaks_defaults(doa_list, num_sources, min_separation=None, grid=None):
    """The one rule for the arguments of the multi-source read-out, batch (find_doa_peaks) and stream (streaming._TileStream._set_peaks):
    -> (doa float64 [G] host array, K, grid, min_separation).  ValueError for a doa_list that is not 1-dim and for num_sources outside
    1 .. 16; the grid kind is doa_grid_kind(doa_list) unless `grid` names it; min_separation defaults to two grid steps (0 for one point).
    Host work only."""
    doa = np.asarray(doa_list.cpu().numpy() if _is_device_tensor(doa_list) else doa_list, dtype=np.float64)
    if doa.ndim != 1:
        raise ValueError("doa_list should be 1-dim!")
    K = int(num_sources)
    if not 1 <= K <= 16:
        raise ValueError("num_sources must be between 1 and 16")
    if grid is None:
        grid = doa_grid_kind(doa)
    if min_separation is None:
        min_separation = 2 * abs(doa[-1] - doa[0]) / (len(doa) - 1) if len(doa) > 1 else 0.0
    return doa, K, grid, min_separation


def find_doa_peaks(power, doa_list, num_sources, min_separation=None, rel_threshold=0.0, grid=None):
    """The `num_sources` strongest sources of a DoA power profile: power [G] or [B, G] (host array or device tensor) over doa_list
    [G] -> (index int32, value float64), [K] or [B, K], where the input was (device tensors for a device tensor, NumPy otherwise).

    Peaks are local maxima (>= each neighbour, a NaN neighbour counts as lower, a NaN point is never a peak), taken largest first
    (ties: lower index) if their value is >= rel_threshold * max(row) (when rel_threshold > 0) and they lie at least
    `min_separation` (radians; default: two grid steps, so a peak's immediate neighbours -- a plateau of two points included -- never give a second peak) from
    every peak already taken.  Unfilled slots hold -1 and NaN.  The grid kind ("linear", "circular", "circular_closed", see
    doa_grid_kind) is taken from doa_list unless `grid` names it.  For num_sources = 1 and a row without NaN the index is
    np.argmax.  Runs on the device only (micloc_doa_peaks_f64: include/micloc_hip.h states the rule in full)."""
    from . import runtime

    doa, K, grid, min_separation = doa_peaks_defaults(doa_list, num_sources, min_separation, grid)
    on_device = _is_device_tensor(power)
    if on_device:
        p = power
        if p.dtype != runtime._torch().float64:
            p = p.double()
    else:
        p = runtime._as_dev(np.asarray(power, dtype=np.float64), runtime.require_gpu())
    single = p.dim() == 1
    if single:
        p = p.reshape(1, -1)
    if p.dim() != 2 or p.shape[1] != len(doa):
        raise ValueError(f"power has shape {tuple(power.shape)}, the DoA grid {len(doa)} points")
    idx, val = runtime.doa_peaks(p, doa, grid, K, min_separation, rel_threshold)
    if single:
        idx, val = idx[0], val[0]
    if on_device:
        return idx, val
    return idx.cpu().numpy(), val.cpu().numpy()


def window_bounds(T, window, hop=None):
    """The window rule of the time-resolved read-out (include/micloc_hip.h), stated once for Python: frames `window` long starting
    every `hop` frames (default: `window`), window n = [n hop, min(n hop + window, T)); one window if T <= window, otherwise
    1 + ceil((T - window) / hop).  Returns (start, stop) int64 arrays [nW]: window n is the frames start[n] : stop[n].  With
    hop > window the last window of the formula can start at or after T; it is empty (stop == start).  The device additionally
    wants window and hop to be multiples of the plan's window quantum (runtime.Plan.window_quantum)."""
    T, window = int(T), int(window)
    hop = window if hop is None else int(hop)
    if T < 1 or window < 1 or hop < 1:
        raise ValueError("T, window and hop must be at least 1")
    nW = 1 if T <= window else 1 + -(-(T - window) // hop)
    start = np.arange(nW, dtype=np.int64) * hop
    stop = np.maximum(np.minimum(start + window, T), start)
    return start, stop


def windows_complete(frames_final, window, hop=None, T=None):
    """How many windows the STREAMING form of the rule (include/micloc_hip.h, "streaming windows") has emitted once `frames_final`
    frames are beamformed: window n is emitted when its last frame n hop + window - 1 is, so 0 while frames_final < window and
    (frames_final - window) // hop + 1 from then on.  With `T` (the length of the recording) and frames_final >= T the final tile
    has been beamformed and every window of the rule exists: len(window_bounds(T, window, hop)[0]) -- the leftover window
    included, the windows that start before T but are not in that count (window = 1024, hop = 256, T = 1100: 2, not 5) excluded.
    The streaming rule wants 1 <= hop <= window (the device additionally multiples of the plan's window quantum)."""
    frames_final, window = int(frames_final), int(window)
    hop = window if hop is None else int(hop)
    if window < 1 or hop < 1 or (T is not None and int(T) < 1):
        raise ValueError("T, window and hop must be at least 1")
    if hop > window:
        raise ValueError(f"the streaming read-out needs hop <= window (hop {hop}, window {window})")
    if frames_final < 0:
        raise ValueError("frames_final must not be negative")
    if T is not None and frames_final >= int(T):
        return len(window_bounds(T, window, hop)[0])
    return 0 if frames_final < window else (frames_final - window) // hop + 1


def _add_window_peaks(out, doa_list, num_sources, min_separation, rel_threshold):
    """localize_batch's multi-source read-out per window: window_peaks [B, nW, K] int32 and window_peak_power [B, nW, K] from the
    B nW rows of out["window_power"] (find_doa_peaks, at most 65535 rows per launch)."""
    if num_sources is None:
        return out
    if doa_list is None:
        raise ValueError("num_sources needs the DoA grid of bf_mat's columns (doa_list=)")
    from . import runtime

    torch = runtime._torch()
    wp = out["window_power"]
    B, nW, G = wp.shape
    rows = wp.reshape(B * nW, G)
    parts = [find_doa_peaks(rows[r : r + 65535], doa_list, num_sources, min_separation=min_separation, rel_threshold=rel_threshold)
             for r in range(0, B * nW, 65535)]
    out["window_peaks"] = torch.cat([p[0] for p in parts]).reshape(B, nW, -1)
    out["window_peak_power"] = torch.cat([p[1] for p in parts]).reshape(B, nW, -1)
    return out


def _add_peaks(out, doa_list, num_sources, min_separation, rel_threshold):
    """localize_batch's optional multi-source read-out: out["peaks"] [B, K] int32 and out["peak_power"] [B, K] from out["power"]."""
    if num_sources is None:
        return out
    if doa_list is None:
        raise ValueError("num_sources needs the DoA grid of bf_mat's columns (doa_list=)")
    out["peaks"], out["peak_power"] = find_doa_peaks(out["power"], doa_list, num_sources, min_separation=min_separation, rel_threshold=rel_threshold)
    return out


def active_packs(packs, rel_threshold):
    """The live demos' activity test (reference micloc/localization_demo.py:127-137, localization_demo_snn.py:141-150,
    localization_demo_MUSIC.py:142-165), pack by pack: packs [B, T, num_mic + 1], integer samples (full scale: the type's maximum) or float
    ones (full scale 1) -> (float signals [B, T, num_mic] without the devkit's empty last channel, active [B] bool: the pack's RMS is at
    least rel_threshold x full scale)."""
    packs = np.asarray(packs)
    max_value = np.iinfo(packs.dtype).max if np.issubdtype(packs.dtype, np.integer) else 1.0
    sig = np.asarray(packs[:, :, :-1], dtype=np.float64)
    return sig, np.asarray([np.sqrt(np.mean(s**2)) >= rel_threshold * max_value for s in sig], dtype=bool)
