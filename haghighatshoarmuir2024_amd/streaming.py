"""A recording delivered tile by tile: SNNBeamformer.apply_to_signal's chain with exact state hand-off across tiles, localised
INCREMENTALLY -- a running power spectrum / DoA after every tile, O(tile) memory, no host synchronisation in push().

The reference has two ways of consuming audio: `apply_to_signal` on a whole recording (micloc/snn_beamformer.py:283-370) and
the live demo, which restarts the chain on every 0.25 s frame (micloc/localization_demo_snn.py:125-193; here:
localization_demo_snn.Demo.process_frame).  This module adds the third, which the reference lacks: the recording is ONE
stream but arrives in tiles, and the result is bit-identical to the one-shot call whatever the tiling --

  STHT        the quadrature FIR sees the last L - 1 frames of the previous tile (kept here), the in-phase channel is the input
              delayed by L / 2 frames; its first L / 2 frames are np.roll's wrap-around, i.e. the LAST L / 2 frames of the
              recording (snn_beamformer.py:325-326), which a caller that knows them passes as `wrap_tail` (offline tiling of
              a long file); a live source does not, and gets zeros there like any causal implementation would;
  band-pass   DF2T state carried in the device-side stream state;
  RZCC        running sum, detector state, open clusters (candidate ring) and selection cursors carried as well
              (csrc/rzcc.hip "streaming"); spikes of a cluster are emitted when it closes, into a sliding WINDOW of the int8
              raster (micloc_stream_encode_tile_f64);
  LIF / beamforming / power   after every tile the device decides which frames can no longer receive a spike, filters and
              beamforms the 256-frame chunks that became final and adds their sum of y^2 to a persistent [B, G] accumulator in
              the order of the one-shot call's time reduction (micloc_stream_localize_tile_f64): power and arg-max after the last
              tile equal the one-shot call bit for bit; in between they are the running estimate the live loop wants.

The stream's CLOCK (frames pushed so far, base of the raster window) lives on the device as well: no launch of a tile carries an
absolute time, so a tile of a given length is one replayable hipGraph -- push_replay(), the reference's live loop
(micloc/localization_demo_snn.py:125-193) as one graph launch per 0.25 s frame.

Memory: the window (default: tile + 4096 frames, 14 B per frame and trial, twice), one tile of fp64 intermediates, 2 x G doubles per
trial.  push() allocates nothing and never synchronises (the ready range lives on the device); finish() / status() do.

TIME WINDOWS (window=, hop=): the running power is the mean over every frame since the stream began, which barely reacts to a source
that moves after a minute of audio.  With `window` the localizer also emits the time-resolved read-out of localize_batch(window=, hop=)
-- power and arg-max per window of the rule in include/micloc_hip.h ("streaming windows"), each window as soon as its last chunk is
final, bit for bit the one-shot rows -- into a ring of `max_windows` rows: latest_window() / windows() / finish().  The state is
2 x G doubles per trial and open window (ceil(window / hop) of them) whatever the length of the stream, and a tile is still one graph.

TRACKING (track=, max_track=; StreamingLocalizer and ComplexStreamingLocalizer): the read-out meant for a MOVING source, which neither the
running power nor a window of 256 frames follows -- `np.argmax(Envelope.evolve(y), axis=1)`, track_batch's rule (include/micloc_hip.h
"streaming, tracking").  With `track` (a utils.Envelope) every push also emits the DoA index and the peak envelope of every frame that became
final in it, bit for bit the rows of track_batch on the whole recording, into a ring of `max_track` frames: latest_track() / tracked() /
finish().  The state is the envelope in front of the next frame, 64 doubles per 64 DoAs and trial, whatever the length of the stream, and a
tile is still one graph.  track_setup is the host-side rule (which plans, which ring depths), ring_rows the arithmetic of a ring's rows.
XyloStreamingLocalizer (one band) takes track= too: Demo.track_batch's rows, from the tracking form of the packed integer LIF walk -- its
ring rule is track_ring, track_setup's without the limits of the fused kernels of csrc/track.hip (LIF parity unpinned).
The two wideband streams take track= as well (include/micloc_hip.h "wideband streaming, tracking"): the rows of the wideband localizers'
track_batch, one magnitude summed over the bands.  The complex bands advance in lock step; the SNN bands finish chunks at different pushes,
and a frame is tracked once EVERY band has beamformed its chunk -- bands_track_span is that frontier rule as host arithmetic.

SEVERAL SOURCES (num_sources=, doa_list=, min_separation=, rel_threshold=; every class but XyloStreamingLocalizer, whose read-out is the
box-car peak of an integer rate): the read-out of localize_batch(num_sources=) -- utils.find_doa_peaks' rule, the K strongest peaks -- of the
running power after every push and, with window=, of every window as soon as it is emitted, bit for bit the one-shot rows (include/micloc_hip.h
"streaming, multi-source").  The read-out follows the stream's count of emitted windows on the device and is the last launch of every tile,
inside the tile's graph: latest_peaks() / windows() / finish() / peaks_status().  _set_peaks holds the refusals, _alloc_peaks the device side,
_peaks_tile the launch; the defaults are utils.doa_peaks_defaults, the one rule batch and stream share.  May be given together with track=.

THE COMPLEX BEAMFORMER (ComplexStreamingLocalizer): the non-spiking baseline as the same kind of stream -- band-pass state, a carry of
the frames behind the last whole chunk and the accumulators on the device, tiles of any length, Beamformer.localize_batch's bits after
the last tile, with or without windows (include/micloc_hip.h "streaming, complex Beamformer").

THE CLASSES: StreamingLocalizer (one SNNBeamformer chain), WidebandStreamingLocalizer (a filterbank and one StreamingLocalizer per band),
ComplexStreamingLocalizer, WidebandComplexStreamingLocalizer (a filterbank and ONE complex stream of bands x batch rows),
MusicStreamingLocalizer and XyloStreamingLocalizer (one STHT, per band an encoder stream and the Xylo integer LIF resumed across tiles, the
rate / peak read-out over the bands; LIF parity unpinned) share one surface -- push, push_replay, status, latest_window, windows, finish -- and one tile protocol, which
_TileStream states once: what a window / hop / max_windows may be, which tiles are accepted, how a tile length becomes a captured graph, how
the ring of windows is read, what finish() refuses about it.  It also holds the pieces more than one class launches: the STHT front of a tile
for any number of rows (_stht_tile / _keep_history, with _set_stht, _alloc_stht and _set_wrap in the constructor), the read-out entry in its
plain or its windowed form (_localize_tile, with _reset_window_state), the host clock (_advance) and the refusals of finish() that the SNN
streams share (_need_spikes_final) and that the complex streams share (_need_clock).  _FilterbankFront is the filterbank of the two wideband
classes: the rules for the bands and wrap_tail, the state, the launch.  A class adds its own state and scratch, the launches of its tile
(_tile), what its clock mirrors beyond the frame count (StreamingLocalizer's window base), status() and its own refusals in finish().
"""
import ctypes

import numpy as np

from . import _lib, runtime, utils
from .snn_beamformer import neuron_impulse_response


def ring_rows(count, depth):
    """The rows of a ring of `depth` rows that holds items 0 .. count - 1, item n in row n % depth: -> (first, k, rows), the k = min(count,
    depth) newest items first .. count - 1 in ascending order and the ring rows they sit in.  Pure host arithmetic (windows(), tracked())."""
    k = min(int(count), int(depth))
    first = int(count) - k
    return first, k, [n % int(depth) for n in range(first, first + k)]


def track_setup(envelope, channels, num_doa, complex_bf, most, total_frames=None, max_track=None):
    """The host-side rule of a tracked stream (track=, max_track=), checked before any device work: -> (a_rise, i_rise, a_fall, R).
    envelope: utils.Envelope; channels: rows of the beamforming kernels' input (2 x microphones); num_doa: columns of bf_mat; most: the
    frames one tile can make final (SNN: the raster window's capacity, complex: max_tile).  ValueError for a plan off the fused route of
    csrc/track.hip (more than 16 channels, more than 512 DoAs with a real bf_mat), envelope windows below one sample, a ring shorter than
    `most`.  The constants are NumPy's own arithmetic, exactly as runtime.Plan.track builds them.  R defaults to total_frames when that is
    given (never below `most`), else to the smallest multiple of 64 that is >= 4 x most."""
    if int(channels) > 16 or (not complex_bf and int(num_doa) > 512):
        raise ValueError(f"a tracked stream runs the fused tracking kernels: up to 16 channels and, with a real bf_mat, up to 512 DoAs (got {channels} "
                         f"channels, {num_doa} DoAs); use track_batch on the whole recording")
    return track_ring(envelope, most, total_frames, max_track)


def track_ring(envelope, most, total_frames=None, max_track=None):
    """track_setup's constants-and-ring part, which does not depend on the kernels behind the stream (the Xylo stream's tracked read-out is
    the packed LIF walk, not csrc/track.hip): -> (a_rise, i_rise, a_fall, R), with track_setup's refusals of an envelope window below one
    sample and of a ring shorter than `most`, and its default for R."""
    consts = runtime.envelope_consts(envelope.win_lens[0], envelope.win_lens[1])
    most = int(most)
    if max_track is not None:
        R = int(max_track)
    elif total_frames is not None:
        R = max(int(total_frames), most)
    else:
        R = -(-4 * most // 64) * 64
    if R < most:
        raise ValueError(f"max_track must be at least the {most} frames one tile can make final (got {R})")
    return (*consts, R)


def bands_track_span(prev, done, chunk_frames, t_end):
    """The frontier rule of a tracked stream of SNN bands (include/micloc_hip.h "wideband streaming, tracking"), as the device's frontier
    kernel applies it after a tile: -> (first, last), the tile tracks the frames [first, last).  prev: the frontier before the tile (frames
    tracked so far); done: every band's committed chunk count (status()["chunks"] of the bands); chunk_frames: the bands' one chunk
    length; t_end: frames pushed so far.  A frame is final once the chunk that holds it has been beamformed by every band, the last
    chunk of a recording may be ragged, and the frontier never moves back.  Pure host arithmetic."""
    prev = int(prev)
    front = min(min(int(d) for d in done) * int(chunk_frames), int(t_end))
    return prev, max(front, prev)


class _TileStream:
    """The tile protocol of the localizers (module docstring, THE CLASSES).  A subclass supplies
      _tile(x, n, final)   the launches of one tile and nothing else: no allocation, no synchronisation, no absolute time by value (the clock
                           is a device word), so that a tile of a given length is ONE replayable hipGraph;
      _advance(n, final)   (optional) what the host mirrors of the device clock beyond the frame count and the end of the stream;
      _before_slide(n)     (optional) host work that must see the state in front of the tile's launches;
      _window_count()      (optional) windows emitted so far, where they are not counted in `wst`
    and sets plan, device, lib, B, M, G, T and max_tile before it uses the helpers of the constructor below."""

    TILE_MULTIPLE = 1  # a tile other than the last one holds a multiple of this many frames

    # ---- the constructor's shared parts -----------------------------------------------------------------------------------
    @staticmethod
    def _check_window_given(window, hop, max_windows):
        if window is None and (hop is not None or max_windows is not None):
            raise ValueError("hop and max_windows belong to the windowed read-out: give window as well")

    @staticmethod
    def _check_hop(hop, window):
        if hop > window:
            raise ValueError(f"the streaming read-out needs hop <= window (hop {hop}, window {window})")

    @staticmethod
    def _check_ring(max_windows):
        if max_windows < 1:
            raise ValueError("max_windows must be at least 1")

    def _set_windows(self, plan, window, hop, max_windows):
        """self.window / hop / max_windows (None without window=): ValueError, naming the quantum, for a window or hop that does not fit
        `plan`'s -- before any launch of the stream; the ring holds every window of the recording where total_frames is given, else 64."""
        self.window = self.hop = self.max_windows = None
        if window is not None:
            nW, self.window, self.hop = plan.window_count(self.T if self.T is not None else 1, window, hop)
            self._check_hop(self.hop, self.window)
            self.max_windows = int(max_windows) if max_windows is not None else (nW if self.T is not None else 64)
            self._check_ring(self.max_windows)

    def _alloc_results(self):
        """The running estimate and, with window=, the ring and the newest window; then the stream is at frame 0 with no graph."""
        torch = runtime._torch()
        dev = self.device
        self.power = torch.zeros((self.B, self.G), dtype=torch.float64, device=dev)
        self.argmax = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        self.window_power = self.window_argmax = self.latest_power = self.latest_argmax = None
        if self.window is not None:
            self.window_power = torch.zeros((self.B, self.max_windows, self.G), dtype=torch.float64, device=dev)
            self.window_argmax = torch.zeros((self.B, self.max_windows), dtype=torch.int32, device=dev)
            self.latest_power = torch.zeros((self.B, self.G), dtype=torch.float64, device=dev)
            self.latest_argmax = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        self.t = 0
        self.done = False
        self._seen, self._graphs = set(), {}

    track = None  # the tracked read-out is off unless _set_track has been called

    def _set_track(self, envelope, max_track, channels, num_doa, complex_bf, most, fused=True):
        """self.track (the rule's constants, None without track=), self.max_track and self.min_track (what one tile can make final):
        track_setup's refusals, before any device work.  fused=False: a stream whose tracked read-out is not csrc/track.hip's (the Xylo
        stream) -- track_ring's refusals alone."""
        self.track = self.max_track = None
        self.min_track = int(most)
        if envelope is None:
            if max_track is not None:
                raise ValueError("max_track belongs to the tracked read-out: give track as well")
            return
        if fused:
            *self.track, self.max_track = track_setup(envelope, channels, num_doa, complex_bf, most, self.T, max_track)
        else:
            *self.track, self.max_track = track_ring(envelope, most, self.T, max_track)

    _track_head = 0  # bytes in front of the envelope rows in `tst` (a set of plans: the frontier words)

    def _alloc_track(self, capacity, plans=None):
        """The device side of track=: the envelope state (zero-filled on the stream), the pair scratch for `capacity` (the raster window's
        frames / max_tile), the ring and the newest frame.  plans: (handles, F) of a wideband stream -- the state, the scratch and the
        reset of a set of plans (micloc_stream_bands_track_*), whose state has a 256-byte head; default: this stream's one plan."""
        if self.track is None:
            return
        torch = runtime._torch()
        dev, lib = self.device, self.lib
        lead, name = ((self.plan.handle,), "stream_track") if plans is None else (tuple(plans), "stream_bands_track")
        self._track_head = 0 if plans is None else 256
        self.ntst = int(getattr(lib, f"micloc_{name}_state_bytes")(*lead, self.B))
        self.ntws = int(getattr(lib, f"micloc_{name}_workspace_bytes")(*lead, self.B, int(capacity)))
        if self.ntst == 0 or self.ntws == 0:
            raise ValueError(f"micloc {name}_state_bytes: the fused tracking kernels do not serve " +
                             ("this plan and bf_mat" if plans is None else "this set of plans; use track_batch on the whole recording"))
        self.tst = torch.empty(self.ntst, dtype=torch.uint8, device=dev)
        self.tws = torch.empty(self.ntws, dtype=torch.uint8, device=dev)
        self.track_index = torch.zeros((self.B, self.max_track), dtype=torch.int32, device=dev)
        self.track_peak = torch.zeros((self.B, self.max_track), dtype=torch.float64, device=dev)
        self.latest_index = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        self.latest_peak = torch.zeros((self.B,), dtype=torch.float64, device=dev)
        _lib.check(getattr(lib, f"micloc_{name}_reset")(*lead, self.B, runtime._ptr(self.tst), self.ntst, runtime._stream(dev)), f"{name}_reset")

    num_sources = None  # the multi-source read-out is off unless _set_peaks has been given num_sources

    def _set_peaks(self, num_sources, doa_list, min_separation, rel_threshold, num_doa):
        """self.num_sources (K, None without num_sources=), self.doa_list (host float64 [G]), self.grid, self.min_separation and
        self.rel_threshold: the refusals of the multi-source read-out, before any device work -- num_sources without doa_list, K outside
        1 .. 16, a doa_list that does not have the `num_doa` columns of bf_mat, a negative separation or threshold.  The defaults are
        find_doa_peaks' (utils.doa_peaks_defaults)."""
        self.num_sources = None
        if num_sources is None:
            if min_separation is not None:
                raise ValueError("min_separation belongs to the multi-source read-out: give num_sources as well")
            return
        if doa_list is None:
            raise ValueError("num_sources needs the DoA grid of bf_mat's columns (doa_list=)")
        doa, K, grid, sep = utils.doa_peaks_defaults(doa_list, num_sources, min_separation)
        if len(doa) != int(num_doa):
            raise ValueError(f"doa_list has {len(doa)} entries for the {int(num_doa)} DoAs of bf_mat")
        if not 1 <= len(doa) <= 4096:
            raise ValueError(f"the multi-source read-out serves grids of 1 .. 4096 DoAs, got {len(doa)}")
        sep, rel = float(sep), float(rel_threshold)
        if not sep >= 0.0:
            raise ValueError(f"min_separation must not be negative (got {sep})")
        if not 0.0 <= rel < np.inf:
            raise ValueError(f"rel_threshold must be a finite number >= 0 (got {rel})")
        self.num_sources, self.doa_list, self.grid, self.min_separation, self.rel_threshold = K, doa, grid, sep, rel

    def _window_count_ptr(self):
        """Device address of the word that counts the windows this stream has emitted (what _peaks_tile follows)."""
        return self.lib.micloc_stream_window_count_ptr(runtime._ptr(self.wst))

    def _alloc_peaks(self):
        """The device side of num_sources=: the read-out's state (zero-filled on the stream), the device copy of doa_list, the running
        peaks and, with window=, the two rings and the newest window's peaks -- "no peak" (-1, NaN) until the read-out has written them."""
        if self.num_sources is None:
            return
        torch = runtime._torch()
        dev, lib, K = self.device, self.lib, self.num_sources

        def slots(*shape):
            return (torch.full(shape, -1, dtype=torch.int32, device=dev), torch.full(shape, float("nan"), dtype=torch.float64, device=dev))

        self.npk = int(lib.micloc_stream_peaks_state_bytes())
        self.pk_state = torch.empty(self.npk, dtype=torch.uint8, device=dev)
        self.doa_dev = runtime._as_dev(self.doa_list, dev)
        self.peaks, self.peak_power = slots(self.B, K)
        self.window_peaks = self.window_peak_power = self.latest_window_peaks = self.latest_window_peak_power = None
        self._pk_count = ctypes.c_void_p(0)
        if self.window is not None:
            self.window_peaks, self.window_peak_power = slots(self.B, self.max_windows, K)
            self.latest_window_peaks, self.latest_window_peak_power = slots(self.B, K)
            self._pk_count = ctypes.c_void_p(self._window_count_ptr())
        _lib.check(lib.micloc_stream_peaks_reset(runtime._ptr(self.pk_state), self.npk, runtime._stream(dev)), "stream_peaks_reset")

    def _peaks_tile(self):
        """The last launches of every tile with num_sources=: the multi-source read-out of the running row and of the windows the tile
        has emitted (micloc_stream_peaks_tile_f64, which follows the stream's count word on the device: nothing here depends on the tile)."""
        if self.num_sources is None:
            return
        win = self.window is not None
        _lib.check(self.lib.micloc_stream_peaks_tile_f64(runtime._ptr(self.power), runtime._ptr(self.window_power) if win else None, self._pk_count,
                                                         self.B, self.G, self.max_windows if win else 0, runtime._ptr(self.doa_dev),
                                                         runtime.GRID_KINDS[self.grid], self.num_sources, self.min_separation, self.rel_threshold,
                                                         runtime._ptr(self.pk_state), self.npk, runtime._ptr(self.peaks), runtime._ptr(self.peak_power),
                                                         runtime._ptr(self.window_peaks), runtime._ptr(self.window_peak_power),
                                                         runtime._ptr(self.latest_window_peaks), runtime._ptr(self.latest_window_peak_power),
                                                         runtime._stream(self.device)), "stream_peaks_tile")

    def _reset_window_state(self, name, lead=None, who="the plan", hint=""):
        """wst / nwst, the device state of the open windows (None / 0 without window=): sized by micloc_<name>_state_bytes, zero-filled by
        micloc_<name>_reset.  lead: the leading arguments of both entries (default: this stream's plan and batch)."""
        self.wst, self.nwst = None, 0
        if self.window is None:
            return
        lead = (self.plan.handle, self.B) if lead is None else lead
        wargs = (self.window, self.hop, self.max_windows)
        self.nwst = int(getattr(self.lib, f"micloc_{name}_state_bytes")(*lead, *wargs))
        if self.nwst == 0:
            raise _lib.MiclocError(f"micloc {name}_state_bytes: {who} cannot serve the windowed read-out{hint}")
        torch = runtime._torch()
        self.wst = torch.empty(self.nwst, dtype=torch.uint8, device=self.device)
        _lib.check(getattr(self.lib, f"micloc_{name}_reset")(*lead, runtime._ptr(self.wst), self.nwst, *wargs, runtime._stream(self.device)),
                   f"{name}_reset")

    def _set_stht(self, kernel):
        """L, halo and C of the STHT front: the taps, the frames of history in front of a tile (L - 1, rounded up to 8), the planar rows."""
        self.L = len(kernel)
        self.halo = -(-(self.L - 1) // 8) * 8
        self.C = 2 * self.M

    def _alloc_stht(self, rows):
        """The tile workspace of _stht_tile for `rows` trials, allocated once: the history (zero: the FIR's zero state), [history | tile]
        frames and their planar STHT output."""
        torch = runtime._torch()
        self.hist = torch.zeros((rows, self.halo, self.M), dtype=torch.float64, device=self.device)
        self.ext = torch.empty((rows * (self.halo + self.max_tile) * self.M,), dtype=torch.float64, device=self.device)
        self.h = torch.empty((rows * self.C * self.plan.padded_T(self.halo + self.max_tile),), dtype=torch.float64, device=self.device)

    def _set_wrap(self, wrap_tail, bands=False):
        """self.wrap: np.roll's wrap-around rows [batch, L // 2, M] on the device, or None (zeros).  bands: [F, batch, L // 2, M], already
        checked (_FilterbankFront), as the F * batch trials of one stream."""
        self.wrap = None
        if wrap_tail is not None:
            wrap_tail = self.plan.to_device(np.asarray(wrap_tail, dtype=np.float64) if isinstance(wrap_tail, np.ndarray) else wrap_tail)
            if not bands and tuple(wrap_tail.shape) != (self.B, self.L // 2, self.M):
                raise ValueError(f"wrap_tail must be [batch, {self.L // 2}, num_mic]")
            self.wrap = wrap_tail.reshape(-1, self.L // 2, self.M)

    # ---- one tile -------------------------------------------------------------------------------------------------------
    def _check_tile(self, B, n, M, final):
        if self.done:
            raise _lib.MiclocError("the stream has ended")
        if B != self.B or M != self.M:
            raise ValueError(f"number of channels in the input siganl {M} should be the same as the number of microphones {self.M}!")
        if final is None:
            final = self.T is not None and self.t + n == self.T
        if n < 1 or n > self.max_tile or (not final and n % self.TILE_MULTIPLE != 0) \
                or (self.T is not None and (self.t + n > self.T or (final and self.t + n != self.T))):
            raise ValueError("tiles must hold 1 .. max_tile frames and add up to total_frames" if self.TILE_MULTIPLE == 1 else
                             f"tiles must be multiples of {self.TILE_MULTIPLE} frames (except the last), at most max_tile long, and add up to total_frames")
        if self.t + n > 0x7FFFFFFF:
            raise ValueError("the stream's clock is a 32-bit frame counter")
        return bool(final)

    def _stht_tile(self, x, n, clock, rows=None, spare_rows=0):
        """The front of a tile of `rows` trials (default: the batch; a stream of bands: F * batch, ONE STHT launch for all of them):
        [history | tile] into `ext`, its STHT into the planar rows `h` (+ spare_rows rows), np.roll's wrap-around rows while the
        frames-pushed word of `clock` is below L / 2.  -> (ext, h, Ts)"""
        lib, plan, M = self.lib, self.plan, self.M
        R = self.B if rows is None else rows
        st = runtime._stream(self.device)
        Text = self.halo + n
        ext = self.ext[: R * Text * M].view(R, Text, M)  # contiguous [history | tile] of this tile length
        ext[:, : self.halo, :].copy_(self.hist)
        ext[:, self.halo :, :].copy_(x)
        Ts = plan.padded_T(Text)
        h = self.h[: (R * self.C + spare_rows) * Ts]
        _lib.check(lib.micloc_stht_f64(plan.handle, runtime._ptr(ext), R, Text, runtime._ptr(h), Ts, st), "stht")
        # in-phase[t] = x[T - L/2 + t] for t < L/2 (zeros if the caller could not know them); a no-op later
        _lib.check(lib.micloc_stream_wrap_rows_f64(plan.handle, runtime._ptr(clock), runtime._ptr(h), R, Ts, self.halo, n, runtime._ptr(self.wrap), st),
                   "stream_wrap_rows")
        return ext, h, Ts

    def _keep_history(self, ext):
        """The back of a tile: the last `halo` frames of [history | tile] for the next tile's quadrature FIR."""
        self.hist.copy_(ext[:, ext.shape[1] - self.halo :, :])

    def _localize_tile(self, name, *tile):
        """The read-out launches of a tile: micloc_<name>_f64(*tile, stream) or, with window=, micloc_<name>_windows_f64 -- the same
        launches with the window read-out in front of the commit -- which takes the window state, the rule and the ring behind `tile`."""
        st = runtime._stream(self.device)
        if self.track is not None:  # the same launches again with the tracked read-out behind the window read-out (NULL state: no windows)
            wargs = (None, 0, 0, 0, 0, None, None, None, None) if self.window is None else \
                (runtime._ptr(self.wst), self.nwst, self.window, self.hop, self.max_windows, runtime._ptr(self.window_power),
                 runtime._ptr(self.window_argmax), runtime._ptr(self.latest_power), runtime._ptr(self.latest_argmax))
            _lib.check(getattr(self.lib, f"micloc_{name}_track_f64")(*tile, *wargs, runtime._ptr(self.tst), self.ntst, *self.track, self.max_track,
                                                                     runtime._ptr(self.track_index), runtime._ptr(self.track_peak),
                                                                     runtime._ptr(self.latest_index), runtime._ptr(self.latest_peak),
                                                                     runtime._ptr(self.tws), self.ntws, st), f"{name}_track")
        elif self.window is None:
            _lib.check(getattr(self.lib, f"micloc_{name}_f64")(*tile, st), name)
        else:
            _lib.check(getattr(self.lib, f"micloc_{name}_windows_f64")(*tile, runtime._ptr(self.wst), self.nwst, self.window, self.hop, self.max_windows,
                                                                       runtime._ptr(self.window_power), runtime._ptr(self.window_argmax),
                                                                       runtime._ptr(self.latest_power), runtime._ptr(self.latest_argmax), st),
                       f"{name}_windows")

    def _before_slide(self, n):
        pass

    def _advance(self, n, final):
        self.t += n
        self.done = bool(final)

    def push(self, x_tile, final=None):
        """x_tile [batch, n, M] (numpy or device tensor); n <= max_tile and, except for the last tile, a multiple of TILE_MULTIPLE.
        final: this is the last tile (default: inferred from total_frames).  Returns the running (power, argmax) device tensors
        (overwritten by the next push; over the frames beamformed so far)."""
        x = self.plan.to_device(x_tile)
        B, n, M = x.shape
        final = self._check_tile(B, n, M, final)
        self._before_slide(n)
        self._tile(x, n, final)
        self._seen.add(n)
        self._advance(n, final)
        return self.power, self.argmax

    def push_replay(self, x_tile):
        """push() for the steady state of a live source (micloc/localization_demo_snn.py:125-193: one 0.25 s frame after the other):
        a non-final tile whose length has been pushed before is ONE hipGraph launch -- every launch of the tile, captured on the length's
        second occurrence, replayed from then on; the tile is copied into the graph's input buffer first.  Same results as push()."""
        torch = runtime._torch()
        x = self.plan.to_device(x_tile)
        B, n, M = x.shape
        if n not in self._seen or (self.T is not None and self.t + n == self.T):
            return self.push(x)  # first tile of this length (lazy kernel set-up must not happen inside a capture) / the final tile
        self._check_tile(B, n, M, False)
        g = self._graphs.get(n)
        if g is None:
            x_in = torch.empty((B, n, M), dtype=torch.float64, device=self.device)
            graph = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream(device=self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
                self._tile(x_in, n, False)
            torch.cuda.current_stream(self.device).wait_stream(s)
            g = self._graphs[n] = (graph, x_in)
        self._before_slide(n)
        g[1].copy_(x)
        g[0].replay()
        self._advance(n, False)
        return self.power, self.argmax

    # ---- results ----------------------------------------------------------------------------------------------------------
    def _need_windows(self):
        if self.window is None:
            raise ValueError("the localizer was built without window=")

    def _window_count(self):
        c = ctypes.c_int(0)
        _lib.check(self.lib.micloc_stream_window_count(runtime._ptr(self.wst), ctypes.byref(c), runtime._stream(self.device)), "stream_window_count")
        return int(c.value)

    def latest_window(self):
        """(power [B, G], argmax [B]) of the most recently emitted window: device tensors, overwritten when the next window is emitted,
        zeros until the first one exists.  Does not synchronise."""
        self._need_windows()
        return self.latest_power, self.latest_argmax

    def windows(self):
        """dict(count, first, window_power [B, k, G], window_argmax [B, k], window_start [k]): `count` windows have been emitted so far
        (utils.windows_complete of the frames beamformed); the k = min(count, max_windows) newest of them, windows first .. count - 1 in
        ascending order, as device tensors (copies: later pushes do not change them); window_start: their first frames, host int64.
        Synchronises the stream."""
        self._need_windows()
        torch = runtime._torch()
        count = self._window_count()
        first, _, rows = ring_rows(count, self.max_windows)
        rows = torch.tensor(rows, dtype=torch.int64, device=self.device)
        w = dict(count=count, first=first, window_power=self.window_power.index_select(1, rows), window_argmax=self.window_argmax.index_select(1, rows),
                 window_start=np.arange(first, count, dtype=np.int64) * self.hop)
        if self.num_sources is not None:  # the same k rows of the peak rings: [B, k, K]
            w.update(window_peaks=self.window_peaks.index_select(1, rows), window_peak_power=self.window_peak_power.index_select(1, rows))
        return w

    def _need_peaks(self):
        if self.num_sources is None:
            raise ValueError("the localizer was built without num_sources=")

    def latest_peaks(self):
        """(peaks [B, K] int32, peak_power [B, K]) of the running row -- the num_sources strongest sources of the running power after the
        last push, find_doa_peaks' rule, -1 / NaN in unfilled slots -- and, with window=, two more: (peaks, peak_power, window_peaks [B, K],
        window_peak_power [B, K]), the same of the most recently emitted window (-1 / NaN until the first one exists).  Device tensors,
        overwritten by the next push.  Does not synchronise."""
        self._need_peaks()
        if self.window is None:
            return self.peaks, self.peak_power
        return self.peaks, self.peak_power, self.latest_window_peaks, self.latest_window_peak_power

    def peaks_status(self):
        """(windows whose peaks have been read, windows skipped because their ring row was overwritten first): the read-out runs behind
        every tile, so the first equals windows()["count"] and the second stays 0.  Synchronises the stream."""
        self._need_peaks()
        st2 = (ctypes.c_int * 2)()
        _lib.check(self.lib.micloc_stream_peaks_status(runtime._ptr(self.pk_state), st2, runtime._stream(self.device)), "stream_peaks_status")
        return int(st2[0]), int(st2[1])

    def _finish_peaks(self, out):
        """finish()'s multi-source tail: `out` with peaks [B, K] int32 and peak_power [B, K], localize_batch's keys (the window rows come
        with _finish_windows)."""
        if self.num_sources is not None:
            out.update(peaks=self.peaks, peak_power=self.peak_power)
        return out

    def _need_track(self):
        if self.track is None:
            raise ValueError("the localizer was built without track=")

    def latest_track(self):
        """(index [B], peak_envelope [B]) of the newest tracked frame: device tensors, overwritten by the next push that makes a frame
        final, zeros until the first one exists.  Does not synchronise."""
        self._need_track()
        return self.latest_index, self.latest_peak

    def tracked(self):
        """dict(count, first, index [B, k], peak_envelope [B, k]): `count` frames have been tracked so far; the k = min(count, max_track)
        newest of them, frames first .. count - 1 in ascending order, as device tensors (copies: later pushes do not change them).
        Synchronises the stream."""
        self._need_track()
        torch = runtime._torch()
        count = self._track_count()
        first, _, rows = ring_rows(count, self.max_track)
        rows = torch.tensor(rows, dtype=torch.int64, device=self.device)
        return dict(count=count, first=first, index=self.track_index.index_select(1, rows), peak_envelope=self.track_peak.index_select(1, rows))

    def _finish_track(self, out, env_last=None):
        """finish()'s tracked tail: `out` with track_index [B, T], track_peak_envelope [B, T] and envelope_last [B, G] (a live source
        without total_frames: the max_track newest frames, see tracked()).  env_last: where the stream keeps envelope_last outside `tst`."""
        if self.track is not None:
            if self.T is not None and self.max_track < self.T:
                raise _lib.MiclocError(f"the recording has {self.T} frames and the ring keeps {self.max_track}: raise max_track (or read "
                                       "tracked() while the stream runs)")
            w = self.tracked()
            if env_last is None:
                env_last = self.tst[self._track_head :].view(runtime._torch().float64).view(self.B, -1)[:, : self.G]  # [B][column groups x 64]
            out.update(track_index=w["index"], track_peak_envelope=w["peak_envelope"], track_count=w["count"], envelope_last=env_last.clone())
        return out

    def _need_done(self):
        if not self.done:
            raise _lib.MiclocError(f"the stream is incomplete: {self.t} frames pushed and no final tile")

    def _need_spikes_final(self, s, cap, whose="the", by=""):
        """finish()'s refusals of the SNN streams, from status(): an overflowed encoder, frames the raster window (`cap` frames) left behind."""
        if s["overflow"]:
            raise _lib.MiclocError(f"{s['overflow']} stream(s) overflowed the candidate ring or the raster window (out-of-band input): use the "
                                   "one-shot call, which redoes such streams exactly")
        if s["lag_failures"] or s["frames"] != self.t:
            raise _lib.MiclocError(f"{whose} raster window ({cap} frames) slid past frames whose spikes were not final yet "
                                   f"({s['frames']} of {self.t} frames beamformed{by}): raise lag_frames")

    def _need_clock(self, s):
        """finish()'s refusal of the complex streams, from status(): every frame pushed has been contracted and none waits in the carry."""
        if s["frames"] != self.t or s["pushed"] != self.t or s["carry"] != 0:
            raise _lib.MiclocError(f"the device clock disagrees with the host's: {s} after {self.t} frames")

    def _finish_windows(self, out):
        """finish()'s windowed tail: `out` with window_power [B, nW, G], window_argmax [B, nW] and window_count = nW, every window of the
        recording (a live source without total_frames: the max_windows newest, see windows())."""
        if self.window is not None:
            if self.T is not None:
                nW = utils.windows_complete(self.T, self.window, self.hop, T=self.T)
                if self.max_windows < nW:
                    raise _lib.MiclocError(f"the recording has {nW} windows and the ring keeps {self.max_windows}: raise max_windows (or read "
                                           "windows() while the stream runs)")
            w = self.windows()
            out.update(window_power=w["window_power"], window_argmax=w["window_argmax"], window_count=w["count"])
            if "window_counts" in w:  # (XyloStreamingLocalizer)
                out["window_counts"] = w["window_counts"]
            if "window_peaks" in w:  # (num_sources=)
                out.update(window_peaks=w["window_peaks"], window_peak_power=w["window_peak_power"])
        return self._finish_peaks(out)


class _FilterbankFront:
    """The filterbank in front of a wideband stream (mixed into the two wideband classes): what the bands and `wrap_tail` must look like,
    the DF2T states of every band's section on the device, and the launch that filters a tile into xf [F][B][n][M]."""

    def _check_bands(self, loc, batch, wrap_tail):
        """F, B, M, G and the filterbank's host tables from `loc` (a wideband.WidebandSNNLocalizer / WidebandBeamformerLocalizer); ValueError
        for a band count, a wrap_tail shape or a section count that does not fit -- host work only, in front of any plan."""
        F = self.F = len(loc.beamfs)
        if not 1 <= F <= _lib.MICLOC_MAX_BANDS:
            raise ValueError(f"a wideband stream has 1 .. {_lib.MICLOC_MAX_BANDS} bands, got {F}")
        self.B, self.M, self.G = int(batch), loc.num_mic, loc.num_grid
        L2 = len(loc.beamfs[0].kernel) // 2
        if wrap_tail is not None and tuple(wrap_tail.shape) != (F, self.B, L2, self.M):
            raise ValueError(f"wrap_tail must be [bands, batch, {L2}, num_mic] = {(F, self.B, L2, self.M)}")
        if len(loc.filterbank.ba_list) != F:
            raise ValueError(f"{len(loc.filterbank.ba_list)} filterbank sections for {F} bands")
        self.bb, self.aa, self.ncoef = runtime.pad_ba_list(loc.filterbank.ba_list)

    def _alloc_filterbank(self):
        """fb_state (sized by the library, zeroed on the stream) and xf, the filtered tile; needs device, lib and max_tile."""
        torch = runtime._torch()
        self.nfb = int(self.lib.micloc_filterbank_stream_state_bytes(self.F, self.ncoef, self.B, self.M))
        if self.nfb == 0:
            raise ValueError("micloc filterbank_stream_state_bytes: the bands, the batch or the filters do not fit the filterbank's rule")
        self.fb_state = torch.empty(self.nfb, dtype=torch.uint8, device=self.device)
        self.xf = torch.empty(self.F * self.B * self.max_tile * self.M, dtype=torch.float64, device=self.device)  # the filtered tile [F][B][n][M]
        _lib.check(self.lib.micloc_filterbank_stream_reset(runtime._ptr(self.fb_state), self.nfb, runtime._stream(self.device)), "filterbank_stream_reset")

    def _filterbank_tile(self, x, n):
        """The first launch of a tile: every band's section over x [B, n, M] -> xf [F, B, n, M], the states carried in fb_state."""
        F, B, M = self.F, self.B, self.M
        xf = self.xf[: F * B * n * M].view(F, B, n, M)
        _lib.check(self.lib.micloc_filterbank_tile_f64(runtime._dptr(self.bb), runtime._dptr(self.aa), F, self.ncoef, runtime._ptr(x), B, n, M,
                                                       runtime._ptr(self.fb_state), self.nfb, runtime._ptr(xf), runtime._stream(self.device)),
                   "filterbank_tile")
        return xf


class StreamingLocalizer(_TileStream):
    TILE_MULTIPLE = 16  # the encoder takes its frames sixteen at a time

    def __init__(self, beamf, bf_mat, batch, total_frames=None, wrap_tail=None, max_tile=12_000, lag_frames=4096, keep_raster=False,
                 window=None, hop=None, max_windows=None, track=None, max_track=None, time_vec=None, num_sources=None, doa_list=None,
                 min_separation=None, rel_threshold=0.0, _share=None):
        """beamf: SNNBeamformer; bf_mat [2M, G]; `batch` recordings are streamed in lock step.
        total_frames  length of the recordings if known (the last tile is then recognised by itself, and the neuron kernel is
                      normalised over exactly that many samples like apply_to_signal does, snn_beamformer.py:342-361); None: a
                      live source -- pass final=True with the last tile; the kernel is normalised over 1 s (the sum has converged
                      to the last bit long before).
        wrap_tail     [batch, L // 2, M]: the last L // 2 frames of every recording (np.roll's wrap-around), or None (zeros).
        max_tile      longest tile push() will be given; lag_frames: how far spikes may trail the input (an open cluster holds
                      its frames back) before status() reports a lag failure.
        keep_raster   (tests) also assemble the full spike raster [batch, total_frames, 2M]; needs total_frames.
        window, hop   frames (hop defaults to window; 1 <= hop <= window, both multiples of the plan's window quantum): also emit power
                      and arg-max per window (module docstring); None: the running estimate only, with exactly the launches it always had.
        max_windows   rows of the ring the windows are kept in (window n in row n % max_windows); default: every window of the
                      recording when total_frames is given, else 64.
        track         a utils.Envelope: also emit the moving-target read-out of track_batch -- the DoA index and the peak envelope of every
                      frame, as soon as the frame is final, bit for bit the one-shot rows (latest_track() / tracked() / finish()); needs a
                      plan on the fused tracking route (up to 16 channels, up to 512 DoAs).  None: exactly the launches without it.
        max_track     rows of the ring the tracked frames are kept in (frame t in row t % max_track), at least min_track = the raster
                      window's capacity; default: total_frames when that is given (never below min_track), else the smallest multiple of 64 >= 4 x min_track.
        time_vec      the time axis the neuron kernel is normalised over, where the one-shot call to be matched was given one of its own
                      (track_batch(time_vec=)); default: total_frames (or 1 s of) samples on the fs grid, from 0.
        num_sources   K = 1 .. 16: also emit the multi-source read-out of localize_batch(num_sources=) -- the K strongest peaks of the running
                      power after every push and, with window=, of every window as soon as it is emitted, find_doa_peaks' rule bit for bit
                      (latest_peaks() / windows() / finish() / peaks_status()); needs doa_list.  None: exactly the launches without it.
        doa_list      [G]: the DoA grid of bf_mat's columns (radians); min_separation, rel_threshold: as find_doa_peaks' (default
                      separation: two grid steps).  May be given together with track=.
        _share        (WidebandStreamingLocalizer) another StreamingLocalizer whose tile-sized scratch (`ext`, `h`, `ws`, the slide's staging
                      copy) this one uses instead of allocating its own, where it is large enough: for localizers whose tiles run one
                      after the other on one stream.  None: nothing changes."""
        self._check_window_given(window, hop, max_windows)
        torch = runtime._torch()
        self.beamf = beamf
        self.B, self.M = int(batch), len(beamf.geometry)
        self.T = None if total_frames is None else int(total_frames)
        self.max_tile = -(-int(max_tile) // 16) * 16
        if track is not None:  # the refusals that need no plan, before any device work (the ring depth follows the chunk length, below)
            track_setup(track, 2 * self.M, np.shape(bf_mat)[1], False, 0)
        self._set_peaks(num_sources, doa_list, min_separation, rel_threshold, np.shape(bf_mat)[1])
        self.plan = beamf.new_plan()
        self.device = self.plan.device
        self._set_stht(beamf.kernel)
        nir_frames = self.T if self.T is not None else int(beamf.fs)
        self.plan.set_neuron_kernel(neuron_impulse_response(np.arange(nir_frames) / beamf.fs if time_vec is None else time_vec, beamf.tau_vec))
        self.plan.set_bf_mat(np.asarray(bf_mat, dtype=np.float64))
        self.lib = _lib.load()
        self.G = self.plan.G
        self.CH = self.lib.micloc_stream_chunk_frames(self.plan.handle)
        if self.CH <= 0:
            _lib.check(self.CH, "stream_chunk_frames")
        self._set_windows(self.plan, window, hop, max_windows)
        # window: the tile being encoded + the frames that may still be waiting for their spikes + one chunk of LIF history
        self.cap = -(-(self.max_tile + int(lag_frames) + 2 * self.CH) // self.CH) * self.CH
        self._set_track(track, max_track, 2 * self.M, self.G, False, self.cap)
        dev = self.device
        self.nstate = self.lib.micloc_stream_state_bytes(self.plan.handle, self.B)
        self.state = torch.empty(int(self.nstate), dtype=torch.uint8, device=dev)
        self.nloc = self.lib.micloc_stream_localize_state_bytes(self.plan.handle, self.B)
        self.loc = torch.empty(int(self.nloc), dtype=torch.uint8, device=dev)
        self.nws = self.lib.micloc_stream_localize_workspace_bytes(self.plan.handle, self.B, self.cap)

        def scratch(name, shape, dtype):  # a buffer that holds nothing between two tiles
            other = getattr(_share, name, None)
            if other is not None and other.dtype == dtype and other.device == dev and other.dim() == len(shape) and other.numel() >= int(np.prod(shape)) \
                    and (len(shape) == 1 or tuple(other.shape) == tuple(shape)):
                return other
            return torch.empty(shape, dtype=dtype, device=dev)

        self.ws = scratch("ws", (int(self.nws),), torch.uint8)
        self.win = torch.empty((self.B, self.cap, self.C), dtype=torch.int8, device=dev)
        self.win_tmp = scratch("win_tmp", (self.B, self.cap, self.C), torch.int8)  # the slide's staging copy
        self.base = 0  # host mirror of the device clock's window base (the schedule depends on the tile sizes only)
        # tile workspace, allocated once: [history | tile] frames and their planar STHT output (+ one spare row, see _tile)
        self.hist = torch.zeros((self.B, self.halo, self.M), dtype=torch.float64, device=dev)  # zero history (lfilter's zero state)
        self.ext = scratch("ext", (self.B * (self.halo + self.max_tile) * self.M,), torch.float64)
        self.h = scratch("h", ((self.B * self.C + 1) * self.plan.padded_T(self.halo + self.max_tile),), torch.float64)
        self._alloc_results()
        self._reset_window_state("stream_window", hint=" (a complex bf_mat?)")
        self._alloc_track(self.cap)
        self._alloc_peaks()
        self._set_wrap(wrap_tail)
        self.raster = None
        if keep_raster:
            if self.T is None:
                raise ValueError("keep_raster needs total_frames")
            self.raster = torch.zeros((self.B, self.T, self.C), dtype=torch.int8, device=dev)
        # the stream's clock (frames pushed, window base) lives on the device: zeroed here with the states and the window
        _lib.check(self.lib.micloc_stream_reset(self.plan.handle, self.B, runtime._ptr(self.state), self.nstate, runtime._ptr(self.loc), self.nloc,
                                                runtime._ptr(self.win), self.cap, runtime._stream(dev)), "stream_reset")

    # ---- one tile -------------------------------------------------------------------------------------------------------
    def _tile(self, x, n, final):
        lib, plan, B = self.lib, self.plan, self.B
        st = runtime._stream(self.device)
        # clock: t_end = t + n; the window slides forward (whole chunks) if it does not cover [.., t + n)
        _lib.check(lib.micloc_stream_begin_tile(plan.handle, runtime._ptr(self.loc), runtime._ptr(self.win), runtime._ptr(self.win_tmp), B, n, self.cap, st),
                   "stream_begin_tile")
        # one spare row in h: the encoder's loader may read up to `halo` elements past its last row
        ext, h, Ts = self._stht_tile(x, n, self.loc, spare_rows=1)
        h_tile = ctypes.c_void_p(h.data_ptr() + 8 * self.halo)
        _lib.check(lib.micloc_stream_encode_tile_f64(plan.handle, h_tile, B, n, Ts, int(final), runtime._ptr(self.win), self.cap, runtime._ptr(self.state),
                                                     self.nstate, runtime._ptr(self.loc), st), "stream_encode_tile")
        self._localize_tile("stream_localize_tile", plan.handle, runtime._ptr(self.state), runtime._ptr(self.loc), self.nloc, runtime._ptr(self.win), B,
                            self.cap, int(final), runtime._ptr(self.power), runtime._ptr(self.argmax), runtime._ptr(self.ws), self.nws)
        self._keep_history(ext)
        self._peaks_tile()

    def _advance(self, n, final):
        """Host mirror of the device clock (rz_stream_clock_begin_kernel's schedule) and the end-of-stream bookkeeping."""
        if self.t + n > self.base + self.cap:
            self.base = -(-(self.t + n - self.cap) // self.CH) * self.CH
        super()._advance(n, final)

    def _before_slide(self, n):
        if self.raster is not None and self.t + n > self.base + self.cap:
            self._save_window(self.t)  # (keep_raster) the rows about to leave the window

    def _save_window(self, t_end):
        """(keep_raster) copy the window's frames [base, t_end) into the full raster: later copies carry more final data."""
        n = min(t_end, self.base + self.cap) - self.base
        if n > 0:
            self.raster[:, self.base : self.base + n, :].copy_(self.win[:, :n, :])

    # ---- results ----------------------------------------------------------------------------------------------------------
    def status(self):
        """dict(chunks, frames, lag_failures, overflow): synchronises the stream."""
        st4 = (ctypes.c_int * 4)()
        _lib.check(self.lib.micloc_stream_localize_status(runtime._ptr(self.loc), st4, runtime._stream(self.device)), "stream_localize_status")
        lost = ctypes.c_int(0)
        _lib.check(self.lib.micloc_stream_overflow(runtime._ptr(self.state), ctypes.byref(lost), runtime._stream(self.device)), "stream_overflow")
        return dict(chunks=int(st4[0]), frames=int(st4[1]), lag_failures=int(st4[2]), overflow=int(lost.value))

    def finish(self, want_spikes=False):
        """-> dict(power [B, G], argmax [B] int32, spikes [B, T, 2M] int8 (keep_raster only) or None) as device tensors; with window=
        also window_power [B, nW, G], window_argmax [B, nW] and window_count = nW, every window of the recording (a live source
        without total_frames: the max_windows newest, see windows())."""
        self._need_done()
        self._need_spikes_final(self.status(), self.cap)
        spikes = None
        if want_spikes:
            if self.raster is None:
                raise ValueError("spikes are only assembled with keep_raster=True")
            self._save_window(self.t)
            spikes = self.raster
        out = dict(power=self.power, argmax=self.argmax, spikes=spikes)
        return self._finish_track(self._finish_windows(out))

    def _track_count(self):
        return self.status()["frames"]  # a frame is tracked by the launch sequence that beamforms its chunk


class WidebandStreamingLocalizer(_FilterbankFront, _TileStream):
    """The wideband chain (wideband.WidebandSNNLocalizer: a filterbank, one SNNBeamformer chain per band, the power patterns added, one
    arg-max -- what the reference deploys, micloc/localization_demo_snn.py:125-193) as ONE stream that arrives in tiles, with the results of
    `WidebandSNNLocalizer.localize_batch` on the whole recording bit for bit, whatever the tiling (include/micloc_hip.h "wideband
    streaming").  The reference's live loop restarts the filterbank, the STHT, the band-pass, the encoder and the LIF on every pack; here
    every one of them carries its state across the tiles.

    One tile = the filterbank tile (micloc_filterbank_tile_f64: the DF2T states live on the device), then for f ascending band f's tile
    launches (a StreamingLocalizer per band with its own plan, encoder and localize state, raster window, running power and window ring;
    the bands run one after the other on the one stream and share the tile-sized scratch), then the band sum
    (micloc_stream_band_sum_f64).  push_replay() captures that whole sequence as one graph per tile length.

    RING DEPTH of the bands (Kb).  Bands finish a window at different calls; a wideband window is emitted once every band has emitted
    it, so the windows [emitted, count_f) must still be in band f's ring when the band sum runs.  `emitted` is the smallest count after
    the PREVIOUS tile.  A band without a lag failure of its own has beamformed every frame before the base of its raster window, which
    is at most `cap` frames behind the frames pushed, so after the previous tile (t' frames pushed) every band had completed the
    windows of at least t' - cap frames; after this tile (t <= t' + max_tile frames) a band has emitted at most the windows completed by
    t frames, plus the one cut at the end of the recording on the final tile.  The windows completed by two frame counts that are d
    apart differ by at most ceil(d / hop), hence count_f - emitted <= ceil((cap + max_tile) / hop) + 1.  Kb is that bound plus one row
    of slack, or the number of windows of the recording where that is known and smaller.  The band sum counts a failure instead of
    summing an overwritten row should the bound ever be exceeded (only after a band's own lag failure); finish() then raises."""

    def __init__(self, loc, batch, total_frames=None, wrap_tail=None, max_tile=12_000, lag_frames=4096, window=None, hop=None, max_windows=None,
                 track=None, max_track=None, time_vec=None, num_sources=None, doa_list=None, min_separation=None, rel_threshold=0.0):
        """loc: wideband.WidebandSNNLocalizer; the other arguments as StreamingLocalizer's, except
        wrap_tail  [F, batch, L // 2, M]: the last L // 2 frames of every band's FILTERED recording (np.roll's wrap-around happens after
                   the filterbank), or None (zeros, as for a live source).
        track, max_track   the tracked read-out of WidebandSNNLocalizer.track_batch (module docstring, TRACKING); min_track = the bands'
                   raster window capacity.  None: exactly the launches without it.
        time_vec   handed to every band's neuron kernel, where the one-shot call to be matched was given one (track_batch(time_vec=)).
        num_sources, doa_list, min_separation, rel_threshold   the multi-source read-out of the band sum (the running power and the
                   wideband windows), as StreamingLocalizer's; doa_list defaults to loc.doa_list.  None: exactly the launches without it."""
        self._check_window_given(window, hop, max_windows)
        torch = runtime._torch()
        self.loc_def = loc
        self._check_bands(loc, batch, wrap_tail)
        F = self.F
        self._set_peaks(num_sources, getattr(loc, "doa_list", None) if doa_list is None else doa_list, min_separation, rel_threshold, self.G)
        self.T = None if total_frames is None else int(total_frames)
        # the refusals of track= that need no plan, before any device work (the ring depth follows the bands' window, below)
        self._set_track(track, max_track, 2 * self.M, self.G, False, 0)
        if window is not None and hop is not None:
            self._check_hop(int(hop), int(window))
        if max_windows is not None:
            self._check_ring(int(max_windows))
        # the bands: band 0 checks window / hop against the quantum (ValueError) before anything is launched
        self.max_tile = -(-int(max_tile) // 16) * 16
        self.bands = []
        Kb = None
        for f, (beamf, W) in enumerate(zip(loc.beamfs, loc.bf_mats)):
            kw = {}
            if window is not None:
                if Kb is None:
                    Kb = self._ring_depth(window, hop, lag_frames)
                kw = dict(window=window, hop=hop, max_windows=Kb)
            tail = None if wrap_tail is None else wrap_tail[f]
            self.bands.append(StreamingLocalizer(beamf, W, self.B, self.T, wrap_tail=tail, max_tile=max_tile, lag_frames=lag_frames, time_vec=time_vec,
                                                 _share=self.bands[0] if self.bands else None, **kw))
        b0 = self.bands[0]
        self.device, self.lib, self.plan = b0.device, b0.lib, b0.plan
        self.Kb = Kb
        self._set_windows(b0.plan, window, hop, max_windows)  # what every band has accepted
        if any(b.window != self.window or b.hop != self.hop or b.CH != b0.CH for b in self.bands):
            raise ValueError("window and hop must be multiples of every band's chunk length")
        if any(b.cap > self._cap_bound(lag_frames) for b in self.bands):
            raise _lib.MiclocError("a band's raster window is longer than the bound the ring depth was derived from")
        self._alloc_filterbank()
        self.nbs = int(self.lib.micloc_stream_bands_state_bytes())
        self.bands_state = torch.empty(self.nbs, dtype=torch.uint8, device=self.device)
        self._alloc_results()
        vp = ctypes.c_void_p
        self._p_power = (vp * F)(*[b.power.data_ptr() for b in self.bands])
        self._p_rows = self._p_count = None
        if self.window is not None:
            self._p_rows = (vp * F)(*[b.window_power.data_ptr() for b in self.bands])
            self._p_count = (vp * F)(*[self.lib.micloc_stream_window_count_ptr(runtime._ptr(b.wst)) for b in self.bands])
        _lib.check(self.lib.micloc_stream_bands_reset(runtime._ptr(self.bands_state), self.nbs, runtime._stream(self.device)), "stream_bands_reset")
        self._alloc_peaks()
        # track=: one tracked state over the bands' plans, localize states and raster windows (which share cap and CH)
        self.CH, self.cap = b0.CH, b0.cap
        self._set_track(track, max_track, 2 * self.M, self.G, False, self.cap)
        if self.track is not None:
            if any(b.cap != self.cap for b in self.bands):
                raise ValueError("a tracked wideband stream needs one raster window capacity in every band")
            self.handles = (vp * F)(*[b.plan.handle.value for b in self.bands])
            self._p_loc = (vp * F)(*[b.loc.data_ptr() for b in self.bands])
            self._p_win = (vp * F)(*[b.win.data_ptr() for b in self.bands])
            self._alloc_track(self.cap, plans=(self.handles, F))

    MAX_CHUNK = 512  # the longest chunk of the beamforming kernels (include/micloc_hip.h: 256 frames up to 64 channels, 512 beyond)

    def _ring_depth(self, window, hop, lag_frames):
        """Kb of the class docstring, with `cap` bounded from the arguments alone (a chunk is at most MAX_CHUNK frames; the constructor
        checks the bands' real `cap` against it).  A window or hop that does not fit the quantum is left to band 0's constructor."""
        hop = int(window if hop is None else hop)
        if hop < 1 or int(window) < 1:
            return 1
        Kb = -(-(self._cap_bound(lag_frames) + self.max_tile) // hop) + 2
        if self.T is not None and self.T >= 1:
            Kb = min(Kb, utils.windows_complete(self.T, int(window), hop, T=self.T))
        return max(1, Kb)

    def _cap_bound(self, lag_frames):
        return self.max_tile + int(lag_frames) + 3 * self.MAX_CHUNK

    # ---- one tile -------------------------------------------------------------------------------------------------------
    def _check_tile(self, B, n, M, final):
        return self.bands[0]._check_tile(B, n, M, final)  # the bands advance in lock step: one check serves all

    def _tile(self, x, n, final):
        """The launches of one tile, all on the current stream, in a fixed order: filterbank tile, the bands in ascending order, band
        sum.  Nothing else (no allocation, no synchronisation, no absolute time), so a tile of a given length is one replayable graph."""
        lib, F, B = self.lib, self.F, self.B
        st = runtime._stream(self.device)
        xf = self._filterbank_tile(x, n)
        for f, band in enumerate(self.bands):
            band._tile(xf[f], n, final)
        # without window=: window, ring depths, rows, counts and the window tensors are 0 / NULL, and the entry sums the running powers only
        _lib.check(lib.micloc_stream_band_sum_f64(F, B, self.G, self._p_power, self.window or 0, self.Kb or 0, self.max_windows or 0, self._p_rows,
                                                  self._p_count, runtime._ptr(self.bands_state), self.nbs, runtime._ptr(self.power), runtime._ptr(self.argmax),
                                                  runtime._ptr(self.window_power), runtime._ptr(self.window_argmax),
                                                  runtime._ptr(self.latest_power), runtime._ptr(self.latest_argmax), st), "stream_band_sum")
        if self.track is not None:  # behind every band's commit and tick (and behind the band sum, with which it shares no word)
            _lib.check(lib.micloc_stream_bands_track_tile_f64(self.handles, F, self._p_loc, self._p_win, B, self.cap, runtime._ptr(self.tst), self.ntst,
                                                              *self.track, self.max_track, runtime._ptr(self.track_index), runtime._ptr(self.track_peak),
                                                              runtime._ptr(self.latest_index), runtime._ptr(self.latest_peak), runtime._ptr(self.tws),
                                                              self.ntws, st), "stream_bands_track_tile")
        self._peaks_tile()  # behind the band sum's commit

    def _advance(self, n, final):
        for band in self.bands:
            band._advance(n, final)
        super()._advance(n, final)

    # ---- results ----------------------------------------------------------------------------------------------------------
    def _bands_status(self):
        st2 = (ctypes.c_int * 2)()
        _lib.check(self.lib.micloc_stream_bands_status(runtime._ptr(self.bands_state), st2, runtime._stream(self.device)), "stream_bands_status")
        return int(st2[0]), int(st2[1])

    def status(self):
        """StreamingLocalizer.status() over the bands -- chunks / frames: the slowest band's; lag_failures / overflow: summed -- plus
        bands (the per-band dicts) and band_sum_failures (windows given up because a band's ring had overwritten them); with track= also
        tracked, the frames tracked so far (the joint frontier of the bands).  Synchronises."""
        per = [b.status() for b in self.bands]
        out = dict(chunks=min(s["chunks"] for s in per), frames=min(s["frames"] for s in per), lag_failures=sum(s["lag_failures"] for s in per),
                   overflow=sum(s["overflow"] for s in per), bands=per, band_sum_failures=self._bands_status()[1])
        if self.track is not None:
            out["tracked"] = self._track_count()  # the joint frontier: frames every band has beamformed (bands_track_span)
        return out

    def _track_count(self):
        c = ctypes.c_int(0)
        _lib.check(self.lib.micloc_stream_bands_track_status(runtime._ptr(self.tst), ctypes.byref(c), runtime._stream(self.device)),
                   "stream_bands_track_status")
        return int(c.value)

    def _window_count(self):
        """The smallest of the bands' counts at the last push."""
        return self._bands_status()[0]

    def _window_count_ptr(self):
        return self.lib.micloc_stream_bands_window_count_ptr(runtime._ptr(self.bands_state))

    def finish(self):
        """-> dict(power [B, G], argmax [B] int32, band_power [F, B, G]) as device tensors; with window= also window_power [B, nW, G],
        window_argmax [B, nW] and window_count (a live source without total_frames: the max_windows newest, see windows()); with track= also
        track_index [B, T] int32, track_peak_envelope [B, T], track_count and envelope_last [B, G] (a live source: the max_track newest)."""
        torch = runtime._torch()
        self._need_done()
        s = self.status()
        self._need_spikes_final(s, self.bands[0].cap, whose="a band's", by=" by the slowest band")
        if s["band_sum_failures"]:
            raise _lib.MiclocError(f"{s['band_sum_failures']} wideband window(s) were given up: a band's ring of {self.Kb} windows had overwritten them")
        out = dict(power=self.power, argmax=self.argmax, band_power=torch.stack([b.power for b in self.bands]))
        return self._finish_track(self._finish_windows(out))


class ComplexStreamingLocalizer(_TileStream):
    """The non-spiking complex Beamformer (beamformer.Beamformer; what the reference deploys live in micloc/localization_demo.py, restarting
    the chain on every 0.25 s pack) as ONE stream that arrives in tiles, with the results of `Beamformer.localize_batch` on the whole
    recording bit for bit, whatever the tiling (include/micloc_hip.h "streaming, complex Beamformer").

    There are no spikes, no open clusters and no horizon: a frame is final once its tile has been band-passed, so tiles may have ANY
    length (no multiple of 16) and status() has no lag failures.  One tile = STHT of [last L - 1 frames | tile], np.roll's wrap rows, the
    band-pass tile (DF2T state on the device), the one-shot contraction kernel on [carry | tile], the accumulation of the new whole
    chunks, (the window read-out,) the slide of the ragged remainder into the carry with the clock commit -- a chain of launches on one
    stream, one graph per tile length in push_replay().  The state is 2M (CH + n_coef - 1) + 2G doubles per trial however long the stream."""

    def __init__(self, beamf, bf_mat, batch, total_frames=None, wrap_tail=None, max_tile=12_000, window=None, hop=None, max_windows=None, track=None,
                 max_track=None, num_sources=None, doa_list=None, min_separation=None, rel_threshold=0.0):
        """beamf: beamformer.Beamformer; bf_mat [M, G] complex; `batch` recordings are streamed in lock step.
        total_frames  length of the recordings if known (the last tile is then recognised by itself); None: a live source -- pass
                      final=True with the last tile.
        wrap_tail     [batch, L // 2, M]: np.roll's wrap-around rows, np.roll(x, L // 2, axis=1)[:, : L // 2] -- the last L // 2 frames of a
                      recording of at least that length (shorter ones: wrap_rows()) -- or None (zeros: a live source cannot know them).
        max_tile      longest tile push() will be given.
        window, hop, max_windows   the windowed read-out, as StreamingLocalizer's (multiples of the plan's window quantum, hop <= window).
        track, max_track           the tracked read-out, as StreamingLocalizer's (Beamformer.track_batch's rows; up to 8 microphones); a tile
                                   makes its own frames final, so min_track = max_tile.
        num_sources, doa_list, min_separation, rel_threshold   the multi-source read-out, as StreamingLocalizer's
                                   (Beamformer.localize_batch(num_sources=)'s rows)."""
        self._check_window_given(window, hop, max_windows)
        torch = runtime._torch()
        bf_mat = np.asarray(bf_mat)
        if not np.iscomplexobj(bf_mat):
            raise ValueError("ComplexStreamingLocalizer takes the complex bf_mat of a Beamformer (a real one belongs to StreamingLocalizer)")
        self.beamf = beamf
        self.B, self.M = int(batch), len(beamf.geometry)
        if bf_mat.shape[0] != self.M:
            raise ValueError(f"number of channels in the input siganl {bf_mat.shape[0]} should be the same as the number of microphones {self.M}!")
        self.T = None if total_frames is None else int(total_frames)
        self.max_tile = int(max_tile)
        if self.max_tile < 1:
            raise ValueError("max_tile must be at least 1")
        self._set_track(track, max_track, 2 * self.M, bf_mat.shape[1], True, self.max_tile)  # (refusals before any device work)
        self._set_peaks(num_sources, doa_list, min_separation, rel_threshold, bf_mat.shape[1])
        self.plan = beamf.new_plan()  # the stream's own
        self.device = self.plan.device
        self._set_stht(beamf.kernel)
        self.plan.set_bf_mat(bf_mat.astype(np.complex128))
        self.lib = _lib.load()
        self.G = self.plan.G
        self.CH = self.plan.window_quantum()
        self._set_windows(self.plan, window, hop, max_windows)
        dev = self.device
        self.nstate = int(self.lib.micloc_stream_complex_state_bytes(self.plan.handle, self.B))
        self.nws = int(self.lib.micloc_stream_complex_workspace_bytes(self.plan.handle, self.B, self.max_tile))
        if self.nstate == 0 or self.nws == 0:
            raise _lib.MiclocError("micloc stream_complex_state_bytes: the plan, the batch or max_tile do not fit the complex stream's rule")
        self.state = torch.empty(self.nstate, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(self.nws, dtype=torch.uint8, device=dev)
        self._alloc_stht(self.B)
        self._alloc_results()
        self._reset_window_state("stream_complex_window")
        self._alloc_track(self.max_tile)
        self._alloc_peaks()
        self._set_wrap(wrap_tail)
        _lib.check(self.lib.micloc_stream_complex_reset(self.plan.handle, self.B, runtime._ptr(self.state), self.nstate, runtime._stream(dev)),
                   "stream_complex_reset")

    @staticmethod
    def wrap_rows(x, L):
        """wrap_tail of a recording x [B, T, M] (numpy) for an STHT kernel of L taps: np.roll(x, L // 2, axis=1)[:, : L // 2], zero-padded to
        L // 2 rows when the recording is shorter -- the rows the one-shot call's np.roll puts in front of the in-phase channels."""
        x = np.asarray(x, dtype=np.float64)
        half = int(L) // 2
        out = np.zeros((x.shape[0], half, x.shape[2]))
        k = min(half, x.shape[1])
        out[:, :k, :] = np.roll(x, half, axis=1)[:, :k, :]
        return out

    # ---- one tile -------------------------------------------------------------------------------------------------------
    def _tile(self, x, n, final):
        lib, plan, B = self.lib, self.plan, self.B
        st = runtime._stream(self.device)
        ext, h, Ts = self._stht_tile(x, n, self.state)
        _lib.check(lib.micloc_stream_complex_bandpass_tile_f64(plan.handle, runtime._ptr(h), B, n, Ts, self.halo, self.max_tile, runtime._ptr(self.state),
                                                               self.nstate, runtime._ptr(self.ws), self.nws, st), "stream_complex_bandpass_tile")
        self._localize_tile("stream_complex_localize_tile", plan.handle, runtime._ptr(self.state), self.nstate, B, self.max_tile, int(final),
                            runtime._ptr(self.power), runtime._ptr(self.argmax), runtime._ptr(self.ws), self.nws)
        self._keep_history(ext)
        self._peaks_tile()

    # ---- results ----------------------------------------------------------------------------------------------------------
    def status(self):
        """dict(chunks, frames, carry, pushed): chunks and frames contracted, frames waiting in the carry, frames pushed (the device
        clock).  Synchronises the stream."""
        st4 = (ctypes.c_int * 4)()
        _lib.check(self.lib.micloc_stream_complex_status(runtime._ptr(self.state), st4, runtime._stream(self.device)), "stream_complex_status")
        return dict(chunks=int(st4[0]), frames=int(st4[1]), carry=int(st4[2]), pushed=int(st4[3]))

    def finish(self):
        """-> dict(power [B, G], argmax [B] int32) as device tensors; with window= also window_power [B, nW, G], window_argmax [B, nW] and
        window_count (a live source without total_frames: the max_windows newest, see windows())."""
        self._need_done()
        self._need_clock(self.status())
        out = dict(power=self.power, argmax=self.argmax)
        return self._finish_track(self._finish_windows(out))

    def _track_count(self):
        return self.status()["pushed"]  # a frame is tracked by the tile that brings it


class WidebandComplexStreamingLocalizer(_FilterbankFront, _TileStream):
    """The wideband complex chain (wideband.WidebandBeamformerLocalizer: an order-2 filterbank, one complex Beamformer per band, the
    patterns added, one arg-max -- what the reference deploys live in micloc/localization_demo.py, restarting on every 0.25 s pack) as ONE
    stream that arrives in tiles, with the results of `WidebandBeamformerLocalizer.localize_batch` on the whole recording bit for bit,
    whatever the tiling (include/micloc_hip.h "wideband streaming, complex Beamformer").

    The complex chain has no encoder state and no horizon, so the bands advance in lock step: the stream is ONE ComplexStreamingLocalizer
    of F * batch rows with per-band coefficients and per-band bf_mat, behind WidebandStreamingLocalizer's filterbank state carry.  One tile
    = the filterbank tile, ONE STHT launch over the F * batch trials of [last L - 1 filtered frames | filtered tile], np.roll's wrap rows,
    ONE band-pass tile launch over all F * batch * 2M chains, the contraction per band, ONE accumulate / window read-out / slide over the
    F * batch rows, the band sum -- a chain of launches on one stream, one graph per tile length in push_replay().  Tiles may have any
    length.  The bands complete every window in the same tile, so the bands' ring (inside the window state) is as deep as the number of
    windows one tile can complete plus the one cut at the end of the recording, and no window is ever given up."""

    def __init__(self, loc, batch, total_frames=None, wrap_tail=None, max_tile=12_000, window=None, hop=None, max_windows=None, track=None,
                 max_track=None, num_sources=None, doa_list=None, min_separation=None, rel_threshold=0.0):
        """loc: wideband.WidebandBeamformerLocalizer; `batch` recordings are streamed in lock step.
        total_frames  length of the recordings if known (the last tile is then recognised by itself); None: a live source -- pass
                      final=True with the last tile.
        wrap_tail     [F, batch, L // 2, M]: np.roll's wrap-around rows of every band's FILTERED recording (the roll happens after the
                      filterbank; ComplexStreamingLocalizer.wrap_rows of each band's filterbank output), or None (zeros: a live source).
        max_tile      longest tile push() will be given.
        window, hop, max_windows   the windowed read-out, as ComplexStreamingLocalizer's.
        track, max_track           the tracked read-out of WidebandBeamformerLocalizer.track_batch (module docstring, TRACKING); a tile makes
                                   its own frames final in every band, so min_track = max_tile.
        num_sources, doa_list, min_separation, rel_threshold   the multi-source read-out of the band sum, as StreamingLocalizer's; doa_list
                                   defaults to loc.doa_list."""
        self._check_window_given(window, hop, max_windows)
        torch = runtime._torch()
        self.loc_def = loc
        self._check_bands(loc, batch, wrap_tail)
        F = self.F
        if not 1 <= F * self.B <= 65535:
            raise ValueError(f"bands x batch must be 1 .. 65535, got {F} x {self.B}")
        self.T = None if total_frames is None else int(total_frames)
        self._set_stht(loc.beamfs[0].kernel)
        self.max_tile = int(max_tile)
        if self.max_tile < 1:
            raise ValueError("max_tile must be at least 1")
        self._set_track(track, max_track, 2 * self.M, self.G, True, self.max_tile)  # (refusals before any device work)
        self._set_peaks(num_sources, getattr(loc, "doa_list", None) if doa_list is None else doa_list, min_separation, rel_threshold, self.G)
        # the stream's own plans, one per band (the band-pass coefficients and the bf_mat of that band)
        self.plans = []
        for beamf, W in zip(loc.beamfs, loc.bf_mats):
            plan = beamf.new_plan()
            plan.set_bf_mat(np.asarray(W).astype(np.complex128))
            self.plans.append(plan)
        self.plan = self.plans[0]
        self.device = dev = self.plan.device
        self.lib = _lib.load()
        self.handles = (ctypes.c_void_p * F)(*[p.handle.value for p in self.plans])
        self.CH = self.plan.window_quantum()
        self._set_windows(self.plan, window, hop, max_windows)
        self.nstate = int(self.lib.micloc_stream_complex_bands_state_bytes(self.handles, F, self.B))
        self.nws = int(self.lib.micloc_stream_complex_bands_workspace_bytes(self.handles, F, self.B, self.max_tile))
        if self.nstate == 0 or self.nws == 0:
            raise ValueError("micloc stream_complex_bands_state_bytes: the bands do not share the device, the microphones, the DoA grid, the Hilbert "
                             "kernel and the band-pass length, or max_tile does not fit the stream's rule")
        self._alloc_filterbank()
        self.state = torch.empty(self.nstate, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(self.nws, dtype=torch.uint8, device=dev)
        self._alloc_stht(F * self.B)
        self.band_power = torch.zeros((F, self.B, self.G), dtype=torch.float64, device=dev)
        self._alloc_results()
        self._reset_window_state("stream_complex_bands_window", lead=(self.handles, F, self.B, self.max_tile), who="the plans")
        self._alloc_track(self.max_tile, plans=(self.handles, F))
        self._alloc_peaks()
        self._set_wrap(wrap_tail, bands=True)
        _lib.check(self.lib.micloc_stream_complex_bands_reset(self.handles, F, self.B, runtime._ptr(self.state), self.nstate, runtime._stream(dev)),
                   "stream_complex_bands_reset")

    # ---- one tile -------------------------------------------------------------------------------------------------------
    def _tile(self, x, n, final):
        """The launches of one tile, all on the current stream, in a fixed order.  Nothing else (no allocation, no synchronisation, no
        absolute time), so a tile of a given length is one replayable graph."""
        lib, F, B = self.lib, self.F, self.B
        st = runtime._stream(self.device)
        xf = self._filterbank_tile(x, n).view(F * B, n, self.M)
        # [history | filtered tile] of all bands' trials, ONE STHT launch, the wrap rows of every band's filtered recording
        ext, h, Ts = self._stht_tile(xf, n, self.state, rows=F * B)
        _lib.check(lib.micloc_stream_complex_bands_bandpass_tile_f64(self.handles, F, runtime._ptr(h), B, n, Ts, self.halo, self.max_tile, 0,
                                                                     runtime._ptr(self.state), self.nstate, runtime._ptr(self.ws), self.nws, st),
                   "stream_complex_bands_bandpass_tile")
        self._localize_tile("stream_complex_bands_localize_tile", self.handles, F, runtime._ptr(self.state), self.nstate, B, self.max_tile, int(final),
                            runtime._ptr(self.band_power), runtime._ptr(self.power), runtime._ptr(self.argmax), runtime._ptr(self.ws), self.nws)
        self._keep_history(ext)
        self._peaks_tile()

    # ---- results ----------------------------------------------------------------------------------------------------------
    def status(self):
        """dict(chunks, frames, carry, pushed, windows, band_sum_failures): chunks and frames contracted (the same for every band), frames
        waiting in the carry, frames pushed (the device clock), wideband windows emitted, windows given up (always 0: the ring depth
        covers what one tile can complete); with track= also tracked, the frames tracked so far (the frames pushed).  Synchronises the stream."""
        s6 = (ctypes.c_int * 6)()
        _lib.check(self.lib.micloc_stream_complex_bands_status(runtime._ptr(self.state), runtime._ptr(self.wst), s6, runtime._stream(self.device)),
                   "stream_complex_bands_status")
        out = dict(chunks=int(s6[0]), frames=int(s6[1]), carry=int(s6[2]), pushed=int(s6[3]), windows=int(s6[4]), band_sum_failures=int(s6[5]))
        if self.track is not None:
            out["tracked"] = out["pushed"]  # a frame is tracked by the tile that brings it, in every band
        return out

    def _window_count(self):
        return self.status()["windows"]

    def _window_count_ptr(self):
        return self.lib.micloc_stream_complex_bands_window_count_ptr(runtime._ptr(self.wst))

    def _track_count(self):
        return self.status()["pushed"]

    def finish(self):
        """-> dict(power [B, G], argmax [B] int32, band_power [F, B, G]) as device tensors; with window= also window_power [B, nW, G],
        window_argmax [B, nW] and window_count (a live source without total_frames: the max_windows newest, see windows()); with track= also
        track_index [B, T] int32, track_peak_envelope [B, T], track_count and envelope_last [B, G] (a live source: the max_track newest)."""
        self._need_done()
        s = self.status()
        self._need_clock(s)
        if s["band_sum_failures"]:
            raise _lib.MiclocError(f"{s['band_sum_failures']} wideband window(s) were given up by the band sum")
        out = dict(power=self.power, argmax=self.argmax, band_power=self.band_power)
        return self._finish_track(self._finish_windows(out))


class MusicStreamingLocalizer(_TileStream):
    """MUSIC (music_beamformer.MUSIC; what the reference deploys live in micloc/localization_demo_MUSIC.py, one `beamforming` call per
    0.25 s pack) as ONE stream that arrives in tiles, with the results of `MUSIC.localize_batch` on the whole recording bit for bit,
    whatever the tiling (include/micloc_hip.h "streaming, MUSIC").

    A slice of apply_to_signal is this stream's window: window = L = fs * frame_duration samples, hop = L - overlap.  Every slice is
    band-passed from zero state, every FFT frame is transformed on its own and the read-out mean_s P^2 is a left-to-right sum, so the
    stream filters as the samples arrive, transforms a frame when its last sample arrives and closes a slice when its last sample
    arrives; the final tile also closes the reference's leftover slice.  Tiles may have any length; one tile is one C call whose launches
    depend on the tile's length only (the clock is a device word): one graph per tile length in push_replay().

    latest_window() and windows() return slices: a slice's "power" row is its angular spectrum P [G], the row `beamforming` returns, and
    its arg-max the row's first maximum; windows() adds `spectrum` (the same rows) and `sel` (the selected in-band bins)."""

    def __init__(self, music, batch, num_active_freq, duration_overlap, num_fft_bin, total_frames=None, max_tile=12_000, max_slices=None,
                 num_sources=None, min_separation=None, rel_threshold=0.0):
        """music: music_beamformer.MUSIC; `batch` recordings are streamed in lock step.
        num_active_freq, duration_overlap, num_fft_bin   as MUSIC.localize_batch's; the ValueErrors of that call are raised here.
        total_frames  length of the recordings if known (the last tile is then recognised by itself, and a recording whose leftover slice
                      is shorter than num_fft_bin is refused here); None: a live source -- pass final=True with the last tile.
        max_tile      longest tile push() will be given.
        max_slices    rows of the ring the slices are kept in (slice s in row s % max_slices); default: every slice of the recording
                      when total_frames is given, else 64.
        num_sources, min_separation, rel_threshold   the multi-source read-out over music.doa_list, as StreamingLocalizer's: the peaks of
                      the running power (MUSIC.localize_batch(num_sources=)'s rows) and of every slice's spectrum."""
        self.music = music
        self.B, self.M = int(batch), len(music.geometry)
        self._set_peaks(num_sources, music.doa_list, min_separation, rel_threshold, len(music.doa_list))
        self.T = None if total_frames is None else int(total_frames)
        self.N, self.k = int(num_fft_bin), int(num_active_freq)
        _, _, self.L, self.slice_hop = music.slice_plan(self.T if self.T is not None else 0, duration_overlap)  # (its ValueError: overlap >= L)
        music._check([self.L], self.M, self.k, self.N)
        if self.T is not None:
            full, left = self.slices_of(self.T, self.L, self.slice_hop)
            if left is not None:
                music._check([left[1]], self.M, self.k, self.N)
        self.max_tile = int(max_tile)
        if self.max_tile < 1:
            raise ValueError("max_tile must be at least 1")
        if self.B < 1:
            raise ValueError("batch must be at least 1")
        # the stream's windows are the slices
        self.window, self.hop = self.L, self.slice_hop
        if max_slices is not None:
            self.max_windows = int(max_slices)
        else:
            self.max_windows = 64 if self.T is None else max(1, self.slice_count(self.T, self.L, self.slice_hop))
        self._check_ring(self.max_windows)
        # ---- device ----
        torch = runtime._torch()
        self.plan = music.plan(self.N)
        self.device = dev = self.plan.device
        self.lib = _lib.load()
        self.G, self.nbin = self.plan.G, self.plan.nbin
        self.ksel = self.nbin if (self.k == 0 or self.k > self.nbin) else self.k
        self.bb, self.aa, self.ncoef = runtime.pad_ba(*music.filterbank.ba_list[0])
        self._dims = (self.B, self.M, self.L, self.slice_hop, self.N, self.nbin, self.G, self.ksel, self.max_windows)
        self.nstate = int(self.lib.micloc_stream_music_state_bytes(*self._dims))
        if self.nstate == 0:
            raise _lib.MiclocError("micloc stream_music_state_bytes: the slices, the FFT length or the band do not fit the MUSIC stream's rule")
        self.state = torch.empty(self.nstate, dtype=torch.uint8, device=dev)
        self._alloc_results()
        self.window_sel = torch.zeros((self.B, self.max_windows, self.ksel), dtype=torch.int32, device=dev)
        _lib.check(self.lib.micloc_stream_music_reset(runtime._ptr(self.state), self.nstate, *self._dims, runtime._stream(dev)), "stream_music_reset")
        self._alloc_peaks()

    # ---- the host mirror of the device's slice rule (stream_music.hip: ms_leftover) ---------------------------------------------
    @staticmethod
    def slices_of(T, L, hop):
        """(full, leftover) of a recording of T samples: `full` slices [s hop, s hop + L) and the leftover slice (start, length), or None --
        MUSIC.slice_plan's slices in integers."""
        full = (T - L) // hop + 1 if T >= L else 0
        rest = T - full * hop
        return full, ((full * hop, rest) if 2 * rest > L else None)

    @classmethod
    def slice_count(cls, T, L, hop):
        full, left = cls.slices_of(T, L, hop)
        return full + (left is not None)

    # ---- one tile -------------------------------------------------------------------------------------------------------
    def _tile(self, x, n, final):
        pl = self.plan
        B, M, L, hop, N, nbin, G, ksel, ring = self._dims
        _lib.check(self.lib.micloc_stream_music_tile_f64(runtime._ptr(self.state), self.nstate, runtime._ptr(x), B, n, M, int(final),
                                                         runtime._dptr(self.bb), runtime._dptr(self.aa), self.ncoef, L, hop, N, runtime._ptr(pl.W), nbin,
                                                         runtime._ptr(pl.sre), runtime._ptr(pl.sim), G, ksel, ring, runtime._ptr(self.power),
                                                         runtime._ptr(self.argmax), runtime._ptr(self.latest_power), runtime._ptr(self.latest_argmax),
                                                         runtime._ptr(self.window_power), runtime._ptr(self.window_sel), runtime._ptr(self.window_argmax),
                                                         runtime._stream(self.device)), "stream_music_tile")
        self._peaks_tile()

    # ---- results ----------------------------------------------------------------------------------------------------------
    def status(self):
        """dict(pushed, slices, open, short_leftover): samples pushed (the device clock), slices emitted, slices begun and not yet emitted,
        1 after a final tile whose leftover slice was shorter than num_fft_bin.  Synchronises the stream."""
        st4 = (ctypes.c_int * 4)()
        _lib.check(self.lib.micloc_stream_music_status(runtime._ptr(self.state), st4, runtime._stream(self.device)), "stream_music_status")
        return dict(pushed=int(st4[0]), slices=int(st4[1]), open=int(st4[2]), short_leftover=int(st4[3]))

    def _window_count(self):
        return self.status()["slices"]

    def _window_count_ptr(self):
        return self.lib.micloc_stream_music_slice_count_ptr(runtime._ptr(self.state))

    def windows(self):
        """_TileStream.windows() over the slices, plus spectrum [B, k, G] (the rows of window_power under the name localize_batch gives
        them) and sel [B, k, ksel], the selected in-band bins of every slice."""
        w = super().windows()
        rows = runtime._torch().arange(w["first"], w["count"], device=self.device) % self.max_windows
        w.update(spectrum=w["window_power"], sel=self.window_sel.index_select(1, rows))
        return w

    def finish(self):
        """-> dict(spectrum [B, S, G], power [B, G], argmax [B] int32, slice_argmax [B, S] int32, sel [B, S, ksel]) as device tensors: every
        slice of the recording (a live source without total_frames: the max_slices newest, see windows())."""
        self._need_done()
        s = self.status()
        if s["pushed"] != self.t:
            raise _lib.MiclocError(f"the device clock disagrees with the host's: {s} after {self.t} samples")
        if s["short_leftover"]:
            full, left = self.slices_of(self.t, self.L, self.slice_hop)
            self.music._check([left[1]], self.M, self.k, self.N)  # localize_batch's ValueError
        if s["slices"] == 0:
            raise ValueError(f"a signal of {self.t} samples has no slice of at least half a frame ({self.L} samples)")
        if self.T is not None and self.max_windows < s["slices"]:
            raise _lib.MiclocError(f"the recording has {s['slices']} slices and the ring keeps {self.max_windows}: raise max_slices (or read "
                                   "windows() while the stream runs)")
        w = self.windows()
        out = dict(spectrum=w["spectrum"], power=self.power, argmax=self.argmax, slice_argmax=w["window_argmax"], sel=w["sel"],
                   slice_count=w["count"])
        if self.num_sources is not None:  # the slices are this stream's windows: both names
            out.update(slice_peaks=w["window_peaks"], slice_peak_power=w["window_peak_power"], window_peaks=w["window_peaks"],
                       window_peak_power=w["window_peak_power"])
        return self._finish_peaks(out)


class XyloStreamingLocalizer(_TileStream):
    """The Xylo chain (xylo_snn_localization.Demo: per band STHT -> order-1 band-pass -> RZCC spikes -> the Xylo integer LIF layer, then
    rate and peak -- the reference's live loop micloc/xylo_snn_localization.py:446-542, which restarts the chain on every 0.25 s pack) as
    ONE stream that arrives in tiles, with the results of `Demo.counts_batch`, `rate_batch` and `peak_batch` on the whole recording bit
    for bit, whatever the tiling (include/micloc_hip.h "streaming, Xylo").  PARITY UNPINNED like Demo.xylo_process: the LIF equals the
    oracle's restatement of the published update rule, which is not checked against XyloSim (rockpool is absent).

    The Xylo chain has no filterbank in front of the STHT -- the band filter is the plan's band-pass -- so ONE STHT launch per tile
    serves every band.  Behind it, for f ascending, band f's tile launches: its clock and window slide, its encoder tile (band-pass and
    RZCC state on the device), the horizon, the resumable LIF over the chunks of 256 frames that became final, (the band's window
    read-out,) commit and tick; the bands run one after the other on the one stream and share the tile-sized scratch.  Then the
    read-out over the bands.  The network is block diagonal (band f's channels feed band f's neurons only), so each band integrates its
    own block W_in[f C:(f + 1) C, f G:(f + 1) G] of the ALREADY quantised specification: the quantisation stays the global one.

    LIMITS: w_rec == 0 (a recurrent weight couples all bands per step; the paper's -0.1 / N quantises to 0), bipolar spikes, at most 16
    microphones (Cin = 4 M <= 64), at most MICLOC_MAX_BANDS bands.

    Result slots: `power` holds the rate [B, G] (float64), `argmax` the peak index for `win_size`, `counts` the counts [B, F G] (int32).
    Mid-stream each band is read over the frames IT has integrated so far (the bands' horizons differ); after the final tile every band
    has integrated all of them.

    WINDOWS (window=, hop=: multiples of 256 frames): per window the counts, the rate (counts / frames of that window x fs, band mean) and
    the peak, by the window rule of the other streams, the window cut by the end of the recording included.  The network state is NOT
    reset between windows: one stream is one continuous run of the network.  EMISSION RULE: the ring-depth one of
    WidebandStreamingLocalizer -- every band emits its windows into a ring of Kb rows as its own horizon passes them, a window of the
    stream is emitted by the read-out once every band has emitted it; Kb is WidebandStreamingLocalizer._ring_depth's bound with the
    256-frame chunk, and the read-out counts a failure instead of reading an overwritten row (finish() then raises).

    TRACKING (track=, max_track=; one band): the read-out for a MOVING source, Demo.track_batch's rule (include/micloc_hip.h "streaming, Xylo
    tracking") -- every push also emits the neuron (DoA) index and the peak envelope of every frame the LIF integrated in it, bit for bit
    the rows of Demo.track_batch on the whole recording whatever the tiling, into a ring of `max_track` frames: latest_track() / tracked()
    / finish().  The state is the envelope in front of the next frame, two doubles per lane pair beside the LIF state, whatever the length
    of the stream; a tile is still one graph.  PARITY UNPINNED like everything behind the integer LIF."""

    TILE_MULTIPLE = 16  # the encoder takes its frames sixteen at a time
    CHUNK = 256         # frames per chunk of the LIF's stream: the quantum of window and hop

    def __init__(self, demo, batch, total_frames=None, wrap_tail=None, max_tile=12_000, lag_frames=4096, win_size=1, window=None, hop=None,
                 max_windows=None, max_spikes=31, track=None, max_track=None):
        """demo: xylo_snn_localization.Demo; `batch` recordings are streamed in lock step.  total_frames, wrap_tail [batch, L // 2, M],
        max_tile, lag_frames, window, hop, max_windows: as StreamingLocalizer's (the window quantum is 256 frames); win_size: the
        box-car of peak_batch (odd, at most G / 2).
        track      a utils.Envelope: also emit Demo.track_batch's moving-target read-out -- the DoA index and the peak envelope of every
                   frame, as soon as the LIF has integrated it, bit for bit the one-shot rows (latest_track() / tracked() / finish();
                   LIF parity unpinned).  One band only: beyond G columns an index names no direction.  None: exactly the launches without it.
        max_track  rows of the ring the tracked frames are kept in (frame t in row t % max_track), at least min_track = the raster window's
                   capacity; default: total_frames when that is given (never below min_track), else the smallest multiple of 64 >= 4 x
                   min_track."""
        # ---- the refusals, in front of any device work ----
        self._check_window_given(window, hop, max_windows)
        spec = demo.spec
        if int(spec["w_rec"]) != 0:
            raise ValueError(f"the Xylo stream integrates the bands independently and needs w_rec == 0, got {int(spec['w_rec'])} (the paper's "
                             "-0.1 / N quantises to 0 at 8 bits; a non-zero recurrent weight couples all bands per step: use the one-shot calls)")
        if not demo.bipolar_spikes:
            raise ValueError("the Xylo stream needs bipolar_spikes=True (the LIF kernel splits the ternary raster)")
        self.M = len(demo.beamfs[0].geometry)
        if self.M > 16:
            raise ValueError(f"the Xylo stream serves at most 16 microphones (Cin = 4 M <= 64), got {self.M}")
        F = self.F = len(demo.beamfs)
        if not 1 <= F <= _lib.MICLOC_MAX_BANDS:
            raise ValueError(f"a Xylo stream has 1 .. {_lib.MICLOC_MAX_BANDS} bands, got {F}")
        self.B = int(batch)
        self.G = len(demo.doa_list)
        self.T = None if total_frames is None else int(total_frames)
        self.win_size = int(win_size)
        if self.win_size < 1 or self.win_size % 2 != 1 or self.win_size > self.G // 2:
            raise ValueError(f"win_size must be odd and at most G / 2 = {self.G // 2}, got {win_size}")
        self.max_tile = -(-int(max_tile) // 16) * 16
        self.lag_frames = int(lag_frames)
        self._set_windows(None, window, hop, max_windows)
        CH = self.CHUNK
        self.cap = -(-(self.max_tile + self.lag_frames + 2 * CH) // CH) * CH
        if track is not None and F != 1:
            raise ValueError(f"a tracked Xylo stream takes a demo with one band ({F} given): doa_list[index] has no meaning beyond G columns")
        self._set_track(track, max_track, None, self.G, False, self.cap, fused=False)
        W = np.asarray(spec["W_in"])
        C = 2 * self.M
        if W.shape != (2 * F * C, F * self.G):
            raise ValueError(f"the specification's W_in {W.shape} is not [2 x {F} x {C}, {F} x {self.G}]")
        # ---- device work from here on ----
        torch = runtime._torch()
        self.demo = demo
        self.fs = float(demo.fs)
        self.max_spikes = int(max_spikes)
        enc = demo.beamfs[0].spk_encoder
        self.plans = [runtime.Plan(self.M, demo.beamfs[0].kernel, b, a, enc.robust_width, enc.bipolar, device=demo.device)
                      for (b, a) in demo.filterbank.ba_list]  # the stream's own, as Demo._plans() builds them
        self.plan = self.plans[0]
        self.device = dev = self.plan.device
        self.lib = lib = _lib.load()
        self._set_stht(demo.beamfs[0].kernel)
        self.Kb = self._ring_depth() if self.window is not None else 0
        from .xylo_snn_localization import XyloNetwork

        self.nloc = int(lib.micloc_stream_xylo_state_bytes())
        self.nws = int(lib.micloc_stream_xylo_workspace_bytes(self.B, self.G, self.cap)) if self.window is not None else 0
        self.ws = torch.empty(self.nws, dtype=torch.uint8, device=dev) if self.nws else None  # the per-chunk counts of a band's tile
        self.win_tmp = torch.empty((self.B, self.cap, self.C), dtype=torch.int8, device=dev)  # the slide's staging copy
        self.bands = []
        st = runtime._stream(dev)
        for f, plan in enumerate(self.plans):
            band = dict(plan=plan)
            band["net"] = XyloNetwork(self.band_spec(spec, f, F, C, self.G), device=dev)
            band["nstate"] = int(lib.micloc_stream_state_bytes(plan.handle, self.B))
            band["state"] = torch.empty(band["nstate"], dtype=torch.uint8, device=dev)
            band["loc"] = torch.empty(self.nloc, dtype=torch.uint8, device=dev)
            band["win"] = torch.empty((self.B, self.cap, self.C), dtype=torch.int8, device=dev)
            band["nlif"] = int(lib.micloc_xylo_stream_state_bytes(self.B, self.G))
            band["lif"] = torch.empty(band["nlif"], dtype=torch.uint8, device=dev)
            band["counts"] = torch.empty((self.B, self.G), dtype=torch.int32, device=dev)
            band["wst"], band["nwst"] = None, 0
            _lib.check(lib.micloc_stream_xylo_reset(plan.handle, self.B, runtime._ptr(band["state"]), band["nstate"], runtime._ptr(band["loc"]), self.nloc,
                                                    runtime._ptr(band["win"]), self.cap, self.G, runtime._ptr(band["lif"]), band["nlif"],
                                                    runtime._ptr(band["counts"]), st), "stream_xylo_reset")
            if self.window is not None:
                band["nwst"] = int(lib.micloc_stream_xylo_window_state_bytes(self.B, self.G, self.window, self.hop, self.Kb))
                band["wst"] = torch.empty(band["nwst"], dtype=torch.uint8, device=dev)
                _lib.check(lib.micloc_stream_xylo_window_reset(runtime._ptr(band["wst"]), band["nwst"], self.B, self.G, self.window, self.hop, self.Kb, st),
                           "stream_xylo_window_reset")
            self.bands.append(band)
        # the tile workspace of _stht_tile, shared by the bands: zero history (the FIR's zero state), [history | tile] frames and their planar
        # STHT output, with one spare row in h: the encoder's loader may read up to `halo` elements past its last row
        self.hist = torch.zeros((self.B, self.halo, self.M), dtype=torch.float64, device=dev)
        self.ext = torch.empty((self.B * (self.halo + self.max_tile) * self.M,), dtype=torch.float64, device=dev)
        self.h = torch.empty(((self.B * self.C + 1) * self.plan.padded_T(self.halo + self.max_tile),), dtype=torch.float64, device=dev)
        self._alloc_results()
        self.counts = torch.zeros((self.B, F * self.G), dtype=torch.int32, device=dev)
        self.window_counts = self.latest_counts = None
        if self.window is not None:
            self.window_counts = torch.zeros((self.B, self.max_windows, F * self.G), dtype=torch.int32, device=dev)
            self.latest_counts = torch.zeros((self.B, F * self.G), dtype=torch.int32, device=dev)
        self._alloc_track(self.cap)
        self._set_wrap(wrap_tail)
        vp = ctypes.c_void_p
        self._p_counts = (vp * F)(*[b["counts"].data_ptr() for b in self.bands])
        self._p_loc = (vp * F)(*[b["loc"].data_ptr() for b in self.bands])
        self._p_wst = (vp * F)(*[b["wst"].data_ptr() for b in self.bands]) if self.window is not None else None
        self.nro = int(lib.micloc_stream_xylo_readout_state_bytes())
        self.ro = torch.empty(self.nro, dtype=torch.uint8, device=dev)
        _lib.check(lib.micloc_stream_xylo_readout_reset(runtime._ptr(self.ro), self.nro, st), "stream_xylo_readout_reset")

    @staticmethod
    def band_spec(spec, f, F, C, G):
        """Band f's block of the quantised specification of F bands with C ternary channels and G neurons each: the rows of its +1 and its
        -1 events (W_in is [W; -W], xylo_specification) and its columns; dash_* and threshold sliced alike.  Exact: the network is block
        diagonal and the quantisation happened before the slicing."""
        W = np.asarray(spec["W_in"])
        rows = np.r_[f * C : (f + 1) * C, F * C + f * C : F * C + (f + 1) * C]
        cols = slice(f * G, (f + 1) * G)
        return dict(W_in=np.ascontiguousarray(W[rows][:, cols]), w_rec=0, dash_syn=np.asarray(spec["dash_syn"])[cols],
                    dash_mem=np.asarray(spec["dash_mem"])[cols], threshold=np.asarray(spec["threshold"])[cols])

    def _alloc_track(self, capacity):
        """_TileStream's device side of track= with the Xylo stream's own state (the envelopes of the lane pairs, beside the band's LIF
        state), scratch and envelope_last [B, G], which the tracking launch rewrites."""
        if self.track is None:
            return
        torch = runtime._torch()
        dev, lib = self.device, self.lib
        self.ntst = int(lib.micloc_xylo_stream_track_state_bytes(self.B, self.G))
        self.ntws = int(lib.micloc_xylo_stream_track_workspace_bytes(self.B, self.G, int(capacity)))
        if self.ntst == 0 or self.ntws == 0:
            raise ValueError(f"micloc xylo_stream_track_state_bytes: {self.B} trials x {self.G} neurons do not fit the rule")
        self.tst = torch.empty(self.ntst, dtype=torch.uint8, device=dev)
        self.tws = torch.empty(self.ntws, dtype=torch.uint8, device=dev)
        self.track_index = torch.zeros((self.B, self.max_track), dtype=torch.int32, device=dev)
        self.track_peak = torch.zeros((self.B, self.max_track), dtype=torch.float64, device=dev)
        self.latest_index = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        self.latest_peak = torch.zeros((self.B,), dtype=torch.float64, device=dev)
        self.envelope_last = torch.zeros((self.B, self.G), dtype=torch.float64, device=dev)
        _lib.check(lib.micloc_xylo_stream_track_reset(runtime._ptr(self.tst), self.ntst, self.B, self.G, runtime._stream(dev)), "xylo_stream_track_reset")

    def _set_windows(self, plan, window, hop, max_windows):
        """_TileStream's rule with the Xylo stream's own quantum, 256 frames, on the host alone (no plan has been built yet)."""
        self.window = self.hop = self.max_windows = None
        if window is None:
            return
        window = int(window)
        hop = window if hop is None else int(hop)
        q = self.CHUNK
        if window < 1 or hop < 1 or window % q or hop % q:
            raise ValueError(f"window ({window}) and hop ({hop}) must be positive multiples of the Xylo stream's window quantum, {q} frames")
        self._check_hop(hop, window)
        self.window, self.hop = window, hop
        nW = utils.windows_complete(self.T, window, hop, T=self.T) if self.T is not None else 64
        self.max_windows = int(max_windows) if max_windows is not None else nW
        self._check_ring(self.max_windows)

    def _ring_depth(self):
        """Kb: WidebandStreamingLocalizer._ring_depth's bound (its docstring) with this stream's `cap`."""
        Kb = -(-(self.cap + self.max_tile) // self.hop) + 2
        if self.T is not None and self.T >= 1:
            Kb = min(Kb, utils.windows_complete(self.T, self.window, self.hop, T=self.T))
        return max(1, Kb)

    # ---- one tile -------------------------------------------------------------------------------------------------------
    def _tile(self, x, n, final):
        """The launches of one tile, all on the current stream, in a fixed order: the STHT of [history | tile] once, the bands in
        ascending order, the read-out.  Nothing else (no allocation, no synchronisation, no absolute time)."""
        lib, B = self.lib, self.B
        st = runtime._stream(self.device)
        # the wrap rows read the frames-pushed word, which every band ticks behind its own tile: band 0's is still this tile's start
        ext, h, Ts = self._stht_tile(x, n, self.bands[0]["loc"], spare_rows=1)
        h_tile = ctypes.c_void_p(h.data_ptr() + 8 * self.halo)
        for band in self.bands:
            plan = band["plan"]
            loc, win = runtime._ptr(band["loc"]), runtime._ptr(band["win"])
            _lib.check(lib.micloc_stream_xylo_begin_tile(plan.handle, loc, win, runtime._ptr(self.win_tmp), B, n, self.cap, st), "stream_xylo_begin_tile")
            _lib.check(lib.micloc_stream_encode_tile_f64(plan.handle, h_tile, B, n, Ts, int(final), win, self.cap, runtime._ptr(band["state"]),
                                                         band["nstate"], loc, st), "stream_encode_tile")
            net = band["net"]
            tile = (plan.handle, runtime._ptr(band["state"]), loc, self.nloc, win, B, self.cap, int(final), self.G, self.max_spikes,
                    runtime._ptr(band["counts"]), runtime._ptr(band["lif"]), band["nlif"], runtime._ptr(net.ws), net.nbytes)
            if self.track is not None:  # the same launches with the tracking LIF in place of the counting one (NULL state: no windows)
                wargs = (None, 0, None, 0, 0, 0, 0) if self.window is None else \
                    (runtime._ptr(self.ws), self.nws, runtime._ptr(band["wst"]), band["nwst"], self.window, self.hop, self.Kb)
                _lib.check(lib.micloc_stream_xylo_tile_track_i16(*tile, *wargs, runtime._ptr(self.tst), self.ntst, *self.track, self.max_track,
                                                                 runtime._ptr(self.track_index), runtime._ptr(self.track_peak),
                                                                 runtime._ptr(self.latest_index), runtime._ptr(self.latest_peak),
                                                                 runtime._ptr(self.envelope_last), runtime._ptr(self.tws), self.ntws, st),
                           "stream_xylo_tile_track")
            elif self.window is None:
                _lib.check(lib.micloc_stream_xylo_tile_i16(*tile, st), "stream_xylo_tile")
            else:
                _lib.check(lib.micloc_stream_xylo_tile_windows_i16(*tile, runtime._ptr(self.ws), self.nws, runtime._ptr(band["wst"]), band["nwst"],
                                                                   self.window, self.hop, self.Kb, st), "stream_xylo_tile_windows")
        _lib.check(lib.micloc_stream_xylo_readout(self.F, B, self.G, self.fs, self.win_size, self._p_counts, self._p_loc, self.window or 0, self.hop or 0,
                                                  self.Kb, self.max_windows or 0, self._p_wst, runtime._ptr(self.ro), self.nro, runtime._ptr(self.counts),
                                                  runtime._ptr(self.power), runtime._ptr(self.argmax), runtime._ptr(self.window_counts),
                                                  runtime._ptr(self.window_power), runtime._ptr(self.window_argmax), runtime._ptr(self.latest_counts),
                                                  runtime._ptr(self.latest_power), runtime._ptr(self.latest_argmax), st), "stream_xylo_readout")
        self._keep_history(ext)

    # ---- results ----------------------------------------------------------------------------------------------------------
    def _readout_status(self):
        st2 = (ctypes.c_int * 2)()
        _lib.check(self.lib.micloc_stream_xylo_readout_status(runtime._ptr(self.ro), st2, runtime._stream(self.device)), "stream_xylo_readout_status")
        return int(st2[0]), int(st2[1])

    def status(self):
        """dict(chunks, frames, lag_failures, overflow, bands, readout_failures): chunks / frames integrated by the slowest band,
        lag failures and overflowed encoder streams summed over the bands, the per-band dicts, and the windows the read-out gave up
        because a band's ring had overwritten them.  Synchronises the stream."""
        per = []
        for band in self.bands:
            st4 = (ctypes.c_int * 4)()
            _lib.check(self.lib.micloc_stream_xylo_status(runtime._ptr(band["loc"]), st4, runtime._stream(self.device)), "stream_xylo_status")
            lost = ctypes.c_int(0)
            _lib.check(self.lib.micloc_stream_overflow(runtime._ptr(band["state"]), ctypes.byref(lost), runtime._stream(self.device)), "stream_overflow")
            per.append(dict(chunks=int(st4[0]), frames=int(st4[1]), lag_failures=int(st4[2]), pushed=int(st4[3]), overflow=int(lost.value)))
        return dict(chunks=min(s["chunks"] for s in per), frames=min(s["frames"] for s in per), lag_failures=sum(s["lag_failures"] for s in per),
                    overflow=sum(s["overflow"] for s in per), bands=per, readout_failures=self._readout_status()[1] if self.window is not None else 0)

    def _window_count(self):
        return self._readout_status()[0]

    def _track_count(self):
        return self.status()["frames"]  # a frame is tracked by the launch that integrates it: the band's integrated frames

    def latest_window(self):
        """(rate [B, G], peak [B], counts [B, F G]) of the most recently emitted window: device tensors, overwritten when the next window
        is emitted, zeros until the first one exists.  Does not synchronise."""
        self._need_windows()
        return self.latest_power, self.latest_argmax, self.latest_counts

    def windows(self):
        """_TileStream.windows() -- window_power holds the rate, window_argmax the peak -- plus window_counts [B, k, F G]."""
        w = super().windows()
        torch = runtime._torch()
        rows = torch.arange(w["first"], w["count"], device=self.device) % self.max_windows
        w["window_counts"] = self.window_counts.index_select(1, rows)
        w["window_rate"], w["window_peak"] = w["window_power"], w["window_argmax"]
        return w

    def finish(self):
        """-> dict(counts [B, F G] int32, rate [B, G] float64, peak [B] int32; power and argmax name the same rate and peak) as device
        tensors; with window= also window_counts [B, nW, F G], window_rate / window_power [B, nW, G], window_peak / window_argmax [B, nW]
        and window_count (a live source without total_frames: the max_windows newest, see windows()); with track= also track_index [B, T]
        int32, track_peak_envelope [B, T], track_count and envelope_last [B, G] -- Demo.track_batch's index, peak_env and env_last (a live
        source: the max_track newest frames, see tracked()).  LIF parity unpinned."""
        self._need_done()
        s = self.status()
        self._need_spikes_final(s, self.cap, whose="a band's", by=" by the slowest band")
        if s["readout_failures"]:
            raise _lib.MiclocError(f"{s['readout_failures']} window(s) were given up: a band's ring of {self.Kb} windows had overwritten them")
        out = dict(counts=self.counts, rate=self.power, peak=self.argmax, power=self.power, argmax=self.argmax)
        if self.window is not None:
            self._finish_windows(out)
            out.update(window_rate=out["window_power"], window_peak=out["window_argmax"])
        return self._finish_track(out, env_last=self.envelope_last if self.track is not None else None)
