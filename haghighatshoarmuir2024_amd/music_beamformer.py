"""MUSIC with the reference's call surface (micloc/music_beamformer.py), running on MI355X.

reference method                         -> what runs here
  __init__            :23-62             -> the same 1st-order Butterworth band-pass (ButterworthFilterbank); no device needed
  array_response      :64-90             -> the same NumPy expression (host)
  beamforming         :92-176            -> micloc_music_f64 on one slice: band-pass, band-limited DFT on the fp64 matrix
                                            cores, bin power + top-k, steering power (csrc/music.hip)
  apply_to_signal     :178-247           -> the same kernels on all slices at once
  apply_to_template   :249-316           -> host synthesis (same draws from np.random) + the above
plus two entry points the reference does not have:
  localize_batch(sig[B,T,M], ...)        -> spectrum [B,S,G], the scripts' read-out power = mean_s P^2 [B,G] and arg-max [B]
  streaming_localizer(batch, ...)        -> the same for recordings that arrive in tiles (streaming.MusicStreamingLocalizer)

Parity contract: the in-band bins are those of `np.linspace(0, fs, N)` (labels k fs / (N - 1), the reference's quirk, used by the
steering too); the steering table is `exp(-1j 2 pi freq delays)` computed by NumPy for every in-band bin, once per plan; exact ties of
bin power: the later bin sorts later (stable "later index wins").  Deviation: when no bin lies in the band this raises ValueError
(the reference returns a scalar 0).  The checks and ValueErrors run on the host before any device work.
There is no CPU fallback: without the HIP library or a GPU every device call raises.
"""
from numbers import Number

import numpy as np

from . import runtime
from .filterbank import ButterworthFilterbank
from .snn_beamformer import synthesize_array_signal


class MusicPlan:
    """Device tables of one (geometry, band, DoA grid, fs, N): the DFT matrix W [Np][Cp] and the steering table [nbin][M][G]."""

    def __init__(self, music, num_fft_bin, device=None):
        import torch

        self.device = runtime.require_gpu(device)
        N = int(num_fft_bin)
        bins = music.in_band_bins(N)
        self.N, self.bins, self.nbin = N, bins, len(bins)
        Np = (N + 63) // 64 * 64
        Cp = (2 * self.nbin + 15) // 16 * 16
        n = np.arange(N, dtype=np.int64)
        ang = 2 * np.pi * ((bins[None, :] * n[:, None]) % N) / N  # exact index reduction before the angle
        W = np.zeros((Np, Cp))
        W[:N, 0 : 2 * self.nbin : 2] = np.cos(ang)
        W[:N, 1 : 2 * self.nbin : 2] = -np.sin(ang)
        steer = music.array_response(np.linspace(0, music.fs, N)[bins])  # [nbin, M, G] complex, the reference's expression
        self.W = torch.from_numpy(W).to(self.device)
        self.sre = torch.from_numpy(np.ascontiguousarray(steer.real)).to(self.device)
        self.sim = torch.from_numpy(np.ascontiguousarray(steer.imag)).to(self.device)
        self.G = steer.shape[2]

    def to_device(self, x):
        """numpy / torch [B, T, M] -> contiguous float64 tensor on the plan's device (the streams' tiles)."""
        import torch

        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        return x.to(device=self.device, dtype=torch.float64).contiguous()


class MUSIC:
    def __init__(self, geometry, freq_range, doa_list, frame_duration=0.25, fs=48_000, device=None):
        if len(freq_range) != 2 or freq_range[0] > freq_range[1]:
            raise ValueError("frequency range should be a list containing the minimum and maximum frequency!")
        self.freq_range = np.asarray(freq_range)
        self.doa_list = np.asarray(doa_list)
        self.frame_duration = frame_duration
        self.fs = fs
        self.filterbank = ButterworthFilterbank(freq_bands=[freq_range], order=1, fs=fs, device=device)
        self.geometry = geometry
        self.device = device
        self._plans = {}

    # ---- host side ------------------------------------------------------------------------------------------
    def array_response(self, freq_list):
        """Reference :64-90: [num_freq, num_mic, num_DoA]."""
        delays = np.asarray([self.geometry.delays(theta=theta, normalized=False) for theta in self.doa_list]).T
        return np.asarray([np.exp(-1j * 2 * np.pi * freq * delays) for freq in freq_list])

    def in_band_bins(self, num_fft_bin):
        """Indices k with fmin <= linspace(0, fs, N)[k] <= fmax (reference :129-148)."""
        fmin, fmax = self.freq_range
        freq_vec = np.linspace(0, self.fs, num_fft_bin)
        return np.nonzero((fmin <= freq_vec) & (freq_vec <= fmax))[0]

    def slice_plan(self, T, duration_overlap):
        """apply_to_signal's slices (reference :208-245): (starts [S], lengths [S], L, hop)."""
        L = int(self.fs * self.frame_duration)
        ov = int(self.fs * duration_overlap)
        if ov >= L:
            raise ValueError("duration of overlap window is larger than the duration of a single frame!")
        hop = L - ov
        starts, lens = [], []
        idx = 0
        while idx * hop + L <= T:
            starts.append(idx * hop)
            lens.append(L)
            idx += 1
        start = idx * hop
        if (T - start) > 0.5 * L:
            starts.append(start)
            lens.append(T - start)
        return np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64), L, hop

    def _check(self, lens, num_chan, num_active_freq, num_fft_bin):
        """The reference's checks of `beamforming` (:112-125), its broadcast failure for slices shorter than N (:141-146), and the
        empty band (a deviation: the reference returns 0)."""
        fmin, fmax = self.freq_range
        if num_active_freq > int((fmax - fmin) / (self.fs / num_fft_bin)):
            raise ValueError("number of frequencies is quite large: it may happen that most of these frequencies contain noise!")
        if num_chan != len(self.geometry):
            raise ValueError("input signal should be of dim `T x num_mic`!")
        if num_active_freq < 0:
            raise ValueError("num_active_freq must be >= 0")
        if np.any(np.asarray(lens) < num_fft_bin):
            raise ValueError(f"a signal slice of {int(np.min(lens))} samples is shorter than the FFT length {num_fft_bin}")
        if len(self.in_band_bins(num_fft_bin)) == 0:
            raise ValueError("no FFT bin lies in the frequency range")

    def plan(self, num_fft_bin):
        key = (int(num_fft_bin), self.freq_range.tobytes(), np.asarray(self.doa_list, dtype=np.float64).tobytes(), float(self.fs),
               np.asarray(self.geometry.r_vec, dtype=np.float64).tobytes(), np.asarray(self.geometry.theta_vec, dtype=np.float64).tobytes(),
               float(self.geometry.speed))
        p = self._plans.get(key)
        if p is None:
            p = self._plans[key] = MusicPlan(self, num_fft_bin, device=self.device)
        return p

    # ---- device --------------------------------------------------------------------------------------------
    def _run(self, x, L, hop, S, num_active_freq, num_fft_bin, want_spec=True, want_readout=False, want_sel=False):
        """x: [B, T, M] (numpy or device tensor) -> dict of device tensors."""
        import torch

        from . import _lib

        lib = _lib.load()
        pl = self.plan(num_fft_bin)
        dev = pl.device
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        x = x.to(device=dev, dtype=torch.float64).contiguous()
        B, T, M = x.shape
        k = int(num_active_freq)
        ksel = pl.nbin if (k == 0 or k > pl.nbin) else k
        bb, aa, n = runtime.pad_ba(*self.filterbank.ba_list[0])
        out = {}
        spec = torch.empty((B, S, pl.G), dtype=torch.float64, device=dev) if want_spec else None
        sel = torch.empty((B, S, ksel), dtype=torch.int32, device=dev) if want_sel else None
        power = torch.empty((B, pl.G), dtype=torch.float64, device=dev) if want_readout else None
        argmax = torch.empty((B,), dtype=torch.int32, device=dev) if want_readout else None
        nbytes = lib.micloc_music_workspace_bytes(B, T, M, L, hop, S, pl.N, pl.nbin, pl.G, k)
        ws = runtime._op_workspace(dev, nbytes)
        _lib.check(lib.micloc_music_f64(runtime._ptr(x), B, T, M, runtime._dptr(bb), runtime._dptr(aa), n, L, hop, S, pl.N, runtime._ptr(pl.W),
                                        pl.nbin, runtime._ptr(pl.sre), runtime._ptr(pl.sim), pl.G, k, runtime._ptr(sel), runtime._ptr(spec),
                                        runtime._ptr(power), runtime._ptr(argmax), runtime._ptr(ws), nbytes, runtime._stream(dev)), "music")
        if want_spec:
            out["spectrum"] = spec
        if want_sel:
            out["sel"] = sel
        if want_readout:
            out["power"], out["argmax"] = power, argmax
        return out

    # ---- reference call surface ----------------------------------------------------------------------------------
    def beamforming(self, sig_in, num_active_freq, num_fft_bin, to_host=True):
        """Reference :92-176: sig_in [T, M] -> angular power spectrum [G]."""
        T, num_chan = sig_in.shape
        self._check([T], num_chan, num_active_freq, num_fft_bin)
        x = sig_in[None] if not isinstance(sig_in, np.ndarray) else np.asarray(sig_in, dtype=np.float64)[None]
        spec = self._run(x, T, T, 1, num_active_freq, num_fft_bin)["spectrum"][0, 0]
        return runtime.to_host(spec) if to_host else spec

    def apply_to_signal(self, sig_in, num_active_freq, duration_overlap, num_fft_bin, to_host=True):
        """Reference :178-247: sig_in [T, M] -> [S, G] (one row per slice)."""
        T, num_chan = sig_in.shape
        if num_chan != len(self.geometry):
            raise ValueError("number of channels in the input signal should be the same as the number of microphones!")
        starts, lens, L, hop = self.slice_plan(T, duration_overlap)
        if len(starts) == 0:
            return np.asarray([])  # (the reference's np.asarray of an empty list)
        self._check(lens, num_chan, num_active_freq, num_fft_bin)
        x = sig_in[None] if not isinstance(sig_in, np.ndarray) else np.asarray(sig_in, dtype=np.float64)[None]
        spec = self._run(x, L, hop, len(starts), num_active_freq, num_fft_bin)["spectrum"][0]
        return runtime.to_host(spec) if to_host else spec

    def apply_to_template(self, template, num_active_freq, duration_overlap, num_fft_bin, snr_db, to_host=True):
        """Reference :249-316: the array signal of the template at its DoA (constant or moving), noise from the global NumPy
        stream (np.random.randn(T, M), the reference's draw), then apply_to_signal."""
        try:
            time_temp, sig_temp, doa_temp = template
        except Exception:
            raise ValueError("input template should be a tuple containing (time_in, sig_in, doa_in) of the template signal!")
        if not isinstance(doa_temp, Number):
            doa_temp = np.asarray(doa_temp, dtype=np.float64)
        snr = 10 ** (snr_db / 10)
        _, sig_in_vec = synthesize_array_signal(self.geometry, self.fs, time_temp, sig_temp, doa_temp)
        sig_in_vec += np.sqrt(np.mean(sig_in_vec**2)) / np.sqrt(snr) * np.random.randn(*sig_in_vec.shape)
        return self.apply_to_signal(sig_in_vec, num_active_freq=num_active_freq, duration_overlap=duration_overlap, num_fft_bin=num_fft_bin,
                                    to_host=to_host)

    # ---- batched device entry points (not in the reference) ------------------------------------------------------
    def localize_batch(self, sig_batch, num_active_freq, duration_overlap, num_fft_bin, want_spectrum=True, want_sel=False, num_sources=None,
                       min_separation=None, rel_threshold=0.0):
        """sig_batch [B, T, M] (numpy or device tensor) -> dict of device tensors: spectrum [B, S, G] (apply_to_signal per trial),
        power [B, G] = np.mean(np.abs(spectrum) ** 2, axis=1) (the scripts' read-out), argmax [B] int32 (first maximum);
        sel [B, S, k] (in-band bin indices) with want_sel; with num_sources=K also peaks [B, K] int32 and peak_power [B, K], the K
        strongest sources over self.doa_list (utils.find_doa_peaks)."""
        from .utils import _add_peaks

        B, T, M = sig_batch.shape
        if M != len(self.geometry):
            raise ValueError("number of channels in the input signal should be the same as the number of microphones!")
        starts, lens, L, hop = self.slice_plan(T, duration_overlap)
        if len(starts) == 0:
            raise ValueError(f"a signal of {T} samples has no slice of at least half a frame ({L} samples)")
        self._check(lens, M, num_active_freq, num_fft_bin)
        out = self._run(sig_batch, L, hop, len(starts), num_active_freq, num_fft_bin, want_spec=want_spectrum, want_readout=True,
                        want_sel=want_sel)
        return _add_peaks(out, self.doa_list, num_sources, min_separation, rel_threshold)

    def streaming_localizer(self, batch, num_active_freq, duration_overlap, num_fft_bin, total_frames=None, max_tile=12_000, max_slices=None,
                            num_sources=None, min_separation=None, rel_threshold=0.0):
        """localize_batch for recordings that arrive in tiles (streaming.MusicStreamingLocalizer): push / push_replay tiles of any
        length, the same bits after the last one.  The ValueErrors of localize_batch are raised here, before any device work.
        num_sources (with min_separation, rel_threshold as localize_batch's): also the K strongest peaks over self.doa_list of the
        running power and of every slice's spectrum (latest_peaks() / windows() / finish())."""
        from .streaming import MusicStreamingLocalizer

        return MusicStreamingLocalizer(self, batch, num_active_freq, duration_overlap, num_fft_bin, total_frames=total_frames,
                                       max_tile=max_tile, max_slices=max_slices, num_sources=num_sources, min_separation=min_separation,
                                       rel_threshold=rel_threshold)

    def synthesize_batch(self, template, doas, device_delays=False):
        """Noise-free array signals of a batch of trials on the device (as SNNBeamformer.synthesize_batch)."""
        from . import synthesis

        return synthesis.apply_to_template_batch(self.geometry, self.fs, template, doas, device=self.device, device_delays=device_delays)
