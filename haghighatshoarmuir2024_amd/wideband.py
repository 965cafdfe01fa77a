"""Wideband localisation for batches, SNN and complex.

WidebandSNNLocalizer: wideband SNN localisation for batches: the form the reference deploys in its live demo (micloc/localization_demo_snn.py:125-193) --
a filterbank, one SNNBeamformer chain per band (own band-pass, neuron kernel and bf_mat), the angular power patterns added, one
arg-max (:166-190) -- as ONE library call for B recordings (micloc_snn_pipeline_bands_f64): the filterbank kernel for all bands
together, every band's fused pipeline on its slice, the band sum and its arg-max on the device.

`localization_demo_snn.Demo.power_grid` is the same computation one pack and one band at a time; `localize_batch` returns its
numbers (tests/test_hip_wideband.py).  There is no CPU fallback.

WidebandBeamformerLocalizer: the same for the non-spiking complex `Beamformer`, the chain of the reference's other live demo
(micloc/localization_demo.py:43-89,158-182): an order-2 Butterworth filterbank, one Beamformer per band designed on a sine at the band
centre, mean_t |y|^2 per band, the patterns added, one arg-max -- as ONE library call (micloc_beamformer_pipeline_bands_f64) in which the
band dimension is folded into the batch: one STHT launch and one band-pass launch for all bands' chains.  `localization_demo.Demo.power_grid`
is the same computation one pack and one band at a time; `localize_batch` returns its numbers (tests/test_hip_wideband_complex.py).

What a set of bands must share (_WidebandLocalizer) and how the reference's demos design one (design_bands) are stated once for both forms.
"""
import numpy as np

from . import runtime
from .beamformer import Beamformer
from .filterbank import ButterworthFilterbank
from .snn_beamformer import SNNBeamformer, neuron_impulse_response


def design_bands(freq_bands, recording_duration, fs, band, order, device=None):
    """What both of the reference's demos build in __init__ (micloc/localization_demo_snn.py:40-93, micloc/localization_demo.py:43-89): per
    band a beamformer designed on a sine at the band's centre over `recording_duration`, and the Butterworth filterbank of `order`.
    freq_bands: [F, 2], or a single pair; band(freq_range, template) -> (beamformer, bf_mat) builds and designs one band (snn_band /
    complex_band).  -> (beamfs, bf_mats, filterbank)"""
    freq_bands = np.asarray(freq_bands)
    if freq_bands.ndim == 1:
        freq_bands = freq_bands.reshape(1, -1)
    beamfs, bf_mats = [], []
    for freq_range in freq_bands:
        time_temp = np.arange(0, recording_duration, step=1 / fs)
        sig_temp = np.sin(2 * np.pi * np.mean(freq_range) * time_temp)
        beamf, bf_mat = band(freq_range, (time_temp, sig_temp))
        beamfs.append(beamf)
        bf_mats.append(bf_mat)
    return beamfs, bf_mats, ButterworthFilterbank(freq_bands=freq_bands, order=order, fs=fs, device=device)


def snn_band(geometry, doa_list, kernel_duration, bipolar_spikes, fs, device=None):
    """design_bands' `band` for the SNN form: an SNNBeamformer with tau = 1 / (2 pi f_mid) and its real [2M, G] matrix."""
    def band(freq_range, template):
        tau = 1 / (2 * np.pi * np.mean(freq_range))
        beamf = SNNBeamformer(geometry=geometry, kernel_duration=kernel_duration, freq_range=freq_range, tau_vec=[tau, tau],
                              bipolar_spikes=bipolar_spikes, fs=fs, device=device)
        return beamf, beamf.design_from_template(template=template, doa_list=doa_list)

    return band


def complex_band(geometry, doa_list, kernel_duration, fs, device=None):
    """design_bands' `band` for the complex form: a Beamformer and its complex [M, G] matrix (the design also returns the covariances)."""
    def band(freq_range, template):
        beamf = Beamformer(geometry=geometry, kernel_duration=kernel_duration, freq_range=freq_range, fs=fs, device=device)
        bf_vecs, _ = beamf.design_from_template(template=template, doa_list=doa_list)
        return beamf, bf_vecs

    return band


class _WidebandLocalizer:
    """What a set of bands must share -- 1 .. MICLOC_MAX_BANDS of them, a matrix and a filterbank section each, one microphone count, one
    DoA grid -- and the read-out tail of localize_batch.  A subclass states its rule for ONE bf_mat (_as_bf_mat) and the two messages."""

    def __init__(self, beamfs, bf_mats, filterbank):
        from . import _lib

        self.beamfs, self.filterbank = list(beamfs), filterbank
        bf_mats = list(bf_mats)
        F = len(self.beamfs)
        if not 1 <= F <= _lib.MICLOC_MAX_BANDS:
            raise ValueError(f"a wideband localizer has 1 .. {_lib.MICLOC_MAX_BANDS} bands, got {F}")
        if len(bf_mats) != F or len(filterbank.ba_list) != F:
            raise ValueError(f"{F} beamformers need {F} bf_mats and {F} filterbank sections (got {len(bf_mats)}, {len(filterbank.ba_list)})")
        M = len(self.beamfs[0].geometry)
        if any(len(b.geometry) != M for b in self.beamfs):
            raise ValueError(self.MICROPHONES.format(M=M, C=2 * M))
        self.bf_mats = [self._as_bf_mat(W, M) for W in bf_mats]
        if any(W is None for W in self.bf_mats):
            raise ValueError(self.BF_MAT.format(M=M, C=2 * M))
        G = self.bf_mats[0].shape[1]
        if any(W.shape[1] != G for W in self.bf_mats):
            raise ValueError(f"every band's bf_mat needs the same DoA grid ({[W.shape[1] for W in self.bf_mats]} columns)")
        self.num_mic, self.num_grid = M, G
        self.fs = self.beamfs[0].fs
        self.geometry = self.beamfs[0].geometry

    def _read_out(self, out, T, window, hop, doa_list, num_sources, min_separation, rel_threshold):
        """localize_batch's tail: `out` of the band pipeline with window_start (windowed) and the peaks of num_sources."""
        from .utils import _add_peaks, _add_window_peaks, window_bounds

        if doa_list is None:
            doa_list = getattr(self, "doa_list", None)
        if window is not None:
            out["window_start"] = window_bounds(T, window, hop)[0]
            return _add_window_peaks(out, doa_list, num_sources, min_separation, rel_threshold)
        return _add_peaks(out, doa_list, num_sources, min_separation, rel_threshold)

    def _track_shape(self, sig_batch, envelope):
        """track_batch's checks, in front of any device work -> (B, T)."""
        B, T, M = sig_batch.shape
        if M != self.num_mic:
            raise ValueError(f"number of channels in the input siganl {M} should be the same as the number of microphones {self.num_mic}!")
        runtime.envelope_consts(envelope.win_lens[0], envelope.win_lens[1])  # (its refusal of a window below one sample)
        return B, T


class WidebandSNNLocalizer(_WidebandLocalizer):
    """beamfs: one SNNBeamformer per band; bf_mats: their real [2M, G] matrices; filterbank: a Filterbank with one (b, a) section per
    band.  ValueError for bands with different microphone or DoA counts, or more than 16 bands."""

    MICROPHONES = BF_MAT = "every band needs the same {M} microphones and a real bf_mat with {C} rows"

    @staticmethod
    def _as_bf_mat(W, M):
        W = np.asarray(W, dtype=np.float64)
        return W if W.ndim == 2 and W.shape[0] == 2 * M else None

    @classmethod
    def from_bands(cls, geometry, freq_bands, doa_list, recording_duration, kernel_duration, bipolar_spikes, fs, device=None):
        """What localization_demo_snn.Demo.__init__ builds (reference :40-93): per band an SNNBeamformer with tau = 1 / (2 pi f_mid)
        designed on a sine at the band's centre, and the order-1 Butterworth filterbank."""
        loc = cls(*design_bands(freq_bands, recording_duration, fs, snn_band(geometry, doa_list, kernel_duration, bipolar_spikes, fs, device),
                                order=1, device=device))
        loc.doa_list = np.asarray(doa_list)
        return loc

    def streaming_localizer(self, batch=1, **kw):
        """localize_batch for recordings that arrive tile by tile: a streaming.WidebandStreamingLocalizer (push / push_replay / finish;
        total_frames, wrap_tail, max_tile, lag_frames, window, hop, max_windows, track, max_track as there) whose results after the last
        tile are localize_batch's on the whole recording bit for bit.  num_sources= (with min_separation=, rel_threshold=; doa_list=
        defaults to self.doa_list) adds the K strongest peaks of the running pattern and of every window (latest_peaks() / windows() /
        finish())."""
        from .streaming import WidebandStreamingLocalizer

        return WidebandStreamingLocalizer(self, batch, **kw)

    def plans(self, time_vec):
        """The bands' device plans with their neuron kernels (for this time axis) and matrices set."""
        plans = []
        for beamf, W in zip(self.beamfs, self.bf_mats):
            plan = beamf.plan()
            plan.set_neuron_kernel(neuron_impulse_response(time_vec, beamf.tau_vec))
            plan.set_bf_mat(W)
            plans.append(plan)
        return plans

    def localize_batch(self, sig_batch, time_vec=None, return_band_power=False, num_sources=None, doa_list=None, min_separation=None,
                       rel_threshold=0.0, window=None, hop=None):
        """sig_batch [B, T, M] (numpy or device tensor, on the fs grid) -> dict of device tensors: power [B, G] = the bands' powers
        added in ascending band order, argmax [B] int32; return_band_power: band_power [F, B, G] (with `window`: [F, B, nW, G]).
        window=N frames (hop defaults to it; multiples of every band's window quantum): window_power [B, nW, G], window_argmax [B, nW]
        and window_start [nW] (frames, host) INSTEAD of power / argmax.  num_sources=K (with doa_list): the K strongest peaks of the
        summed pattern -- peaks / peak_power [B, K], with `window` window_peaks / window_peak_power [B, nW, K]."""
        B, T, M = sig_batch.shape
        if M != self.num_mic:
            raise ValueError(f"number of channels in the input siganl {M} should be the same as the number of microphones {self.num_mic}!")
        if time_vec is None:
            time_vec = np.arange(T) / self.fs
        plans = self.plans(time_vec)
        x = plans[0].to_device(sig_batch)
        out = runtime.snn_pipeline_bands(plans, self.filterbank.ba_list, x, window=window, hop=hop, want_band_power=return_band_power)
        return self._read_out(out, T, window, hop, doa_list, num_sources, min_separation, rel_threshold)

    def track_batch(self, sig_batch, envelope, time_vec=None, want_envelope_last=False, budget_bytes=1 << 30):
        """The moving-target read-out (SNNBeamformer.track_batch) over all bands: per frame the arg-max over the DoA grid of
        Envelope.evolve(m), m[t, g] = ((|y_0| + |y_1|) + |y_2|) + ... the bands' beamformer outputs added as magnitudes in ascending band
        order -- with one band SNNBeamformer.track_batch on the filterbank's output, bit for bit.  sig_batch [B, T, M] (numpy or device
        tensor) -> dict of device tensors: index [B, T] int32, peak_envelope [B, T] and, with want_envelope_last, envelope_last [B, G].
        One library call (micloc_snn_pipeline_bands_track_f64); up to 16 channels and 512 DoAs one fused kernel without an array of
        size T x G, otherwise the two-step route inside the library over sub-batches of trials within `budget_bytes`."""
        B, T = self._track_shape(sig_batch, envelope)
        if time_vec is None:
            time_vec = np.arange(T) / self.fs
        plans = self.plans(time_vec)
        return runtime.snn_bands_track(plans, self.filterbank.ba_list, plans[0].to_device(sig_batch), envelope.win_lens[0], envelope.win_lens[1],
                                       want_envelope_last=want_envelope_last, budget_bytes=budget_bytes)


class WidebandBeamformerLocalizer(_WidebandLocalizer):
    """beamfs: one Beamformer per band; bf_mats: their complex [M, G] matrices; filterbank: a Filterbank with one (b, a) section per
    band.  ValueError for bands with different microphone or DoA counts, more than 16 bands, or a bf_mat that is not complex [M, G]."""

    MICROPHONES = "every band needs the same {M} microphones"
    BF_MAT = "every band needs a complex bf_mat with {M} rows ([M, G]; a real [2M, G] matrix belongs to WidebandSNNLocalizer)"

    @staticmethod
    def _as_bf_mat(W, M):
        W = np.asarray(W)
        return W.astype(np.complex128, copy=False) if np.iscomplexobj(W) and W.ndim == 2 and W.shape[0] == M else None

    @classmethod
    def from_bands(cls, geometry, freq_bands, doa_list, recording_duration, kernel_duration, fs, device=None):
        """What localization_demo.Demo.__init__ builds (reference micloc/localization_demo.py:43-89): per band a Beamformer designed on a
        sine at the band's centre, and the order-2 Butterworth filterbank."""
        loc = cls(*design_bands(freq_bands, recording_duration, fs, complex_band(geometry, doa_list, kernel_duration, fs, device), order=2,
                                device=device))
        loc.doa_list = np.asarray(doa_list)
        return loc

    def plans(self):
        """The bands' device plans with their matrices set."""
        plans = []
        for beamf, W in zip(self.beamfs, self.bf_mats):
            plan = beamf.plan()
            plan.set_bf_mat(W)
            plans.append(plan)
        return plans

    def streaming_localizer(self, batch=1, **kw):
        """localize_batch for recordings that arrive tile by tile: a streaming.WidebandComplexStreamingLocalizer (push / push_replay /
        finish; total_frames, wrap_tail, max_tile, window, hop, max_windows as there) whose results after the last tile are localize_batch's
        on the whole recording bit for bit.  track= (a utils.Envelope) and max_track= add the per-frame read-out of track_batch for a source
        that moves while the audio arrives (latest_track() / tracked() / finish()); num_sources= (with min_separation=, rel_threshold=;
        doa_list= defaults to self.doa_list) adds the K strongest peaks of the running pattern and of every window (latest_peaks() /
        windows() / finish())."""
        from .streaming import WidebandComplexStreamingLocalizer

        return WidebandComplexStreamingLocalizer(self, batch, **kw)

    def trials_per_call(self, plans, B, T, window, hop, budget_bytes):
        """The largest sub-batch of B whose workspace stays inside budget_bytes (one trial at least)."""
        from . import _lib

        F, handles = runtime._band_handles(plans)
        one = _lib.load().micloc_beamformer_bands_workspace_bytes(handles, F, 1, T, window or 0, hop or 0)
        if one == 0 or budget_bytes is None:
            return B  # (bad arguments: the call itself names them)
        return int(max(1, min(B, int(budget_bytes) // one)))

    def track_batch(self, sig_batch, envelope, time_vec=None, want_envelope_last=False, budget_bytes=1 << 30):
        """WidebandSNNLocalizer.track_batch for the complex chains (|y| = hypot(re, im); with one band Beamformer.track_batch on the
        filterbank's output, bit for bit): micloc_beamformer_pipeline_bands_track_f64.  time_vec is not read (the chains have no neuron
        kernel).  budget_bytes: B is split into sub-batches whose workspace (the filterbank output and two planar copies of every band)
        stays inside it, one trial at least; the results do not depend on the split."""
        import torch

        from . import _lib

        B, T = self._track_shape(sig_batch, envelope)
        plans = self.plans()
        x = plans[0].to_device(sig_batch)
        F, handles = runtime._band_handles(plans)
        one = _lib.load().micloc_beamformer_bands_track_workspace_bytes(handles, F, 1, T)
        step = B if one == 0 or budget_bytes is None else int(max(1, min(B, int(budget_bytes) // one)))
        parts = [runtime.beamformer_bands_track(plans, self.filterbank.ba_list, x[lo : lo + step], envelope.win_lens[0], envelope.win_lens[1],
                                                want_envelope_last=want_envelope_last, budget_bytes=budget_bytes) for lo in range(0, B, step)]
        if len(parts) == 1:
            return parts[0]
        return {k: (None if parts[0][k] is None else torch.cat([p[k] for p in parts], dim=0)) for k in parts[0]}

    def localize_batch(self, sig_batch, return_band_power=False, num_sources=None, doa_list=None, min_separation=None, rel_threshold=0.0,
                       window=None, hop=None, budget_bytes=8 << 30):
        """sig_batch [B, T, M] (numpy or device tensor, on the fs grid) -> dict of device tensors: power [B, G] = the bands' powers
        added in ascending band order, argmax [B] int32; return_band_power: band_power [F, B, G] (with `window`: [F, B, nW, G]).
        window=N frames (hop defaults to it; multiples of every band's window quantum): window_power [B, nW, G], window_argmax [B, nW]
        and window_start [nW] (frames, host) INSTEAD of power / argmax.  num_sources=K (with doa_list): the K strongest peaks of the
        summed pattern -- peaks / peak_power [B, K], with `window` window_peaks / window_peak_power [B, nW, K].
        budget_bytes: B is split into sub-batches whose workspace (the filterbank output and two planar copies of every band: 35 doubles
        per frame, band and 7 microphones) stays inside it, so a speech-length sweep batch fits; the results do not depend on the split."""
        import torch

        B, T, M = sig_batch.shape
        if M != self.num_mic:
            raise ValueError(f"number of channels in the input siganl {M} should be the same as the number of microphones {self.num_mic}!")
        plans = self.plans()
        x = plans[0].to_device(sig_batch)
        step = self.trials_per_call(plans, B, T, window, hop, budget_bytes)
        parts = [runtime.beamformer_pipeline_bands(plans, self.filterbank.ba_list, x[lo : lo + step], window=window, hop=hop,
                                                   want_band_power=return_band_power) for lo in range(0, B, step)]
        out = parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts], dim=1 if k == "band_power" else 0) for k in parts[0]}
        return self._read_out(out, T, window, hop, doa_list, num_sources, min_separation, rel_threshold)
