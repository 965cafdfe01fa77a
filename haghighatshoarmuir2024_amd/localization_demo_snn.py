"""Frame-by-frame SNN localisation with the structure of the reference's live demo
(micloc/localization_demo_snn.py:18-193), minus the hardware: the reference records 0.25 s packs with `sox`
(record.py) and pushes the DoA to a matplotlib process (visualizer.py); here `process_frame` is the body of that loop
for one recorded pack and `run` drives it from any iterable of packs, handing each result to a callback.

Per pack (reference :125-193): activity detection on the raw integers -> order-1 Butterworth filterbank ->
per band SNNBeamformer.apply_to_signal -> power per DoA, summed over the bands -> arg-max.  Everything after the
activity check runs on the MI355X: the filterbank through micloc_lfilter_f64, each band through the fused pipeline
(power only; the T x G product the reference materialises is never formed).
"""
import numpy as np

from .utils import active_packs
from .wideband import WidebandSNNLocalizer, design_bands, snn_band


class Demo:
    def __init__(self, geometry, freq_bands, doa_list, recording_duration, kernel_duration, bipolar_spikes, fs, device=None):
        self.beamfs, self.bf_mats, self.filterbank = design_bands(freq_bands, recording_duration, fs,
                                                                  snn_band(geometry, doa_list, kernel_duration, bipolar_spikes, fs, device), order=1, device=device)
        self.doa_list = np.asarray(doa_list)
        self.recording_duration = recording_duration
        self.kernel_duration = kernel_duration
        self.fs = fs

    def power_grid(self, data):
        """float [T, num_mic] -> angular power pattern [G] summed over the frequency bands (device -> numpy)."""
        data = np.ascontiguousarray(data, dtype=np.float64)
        T = data.shape[0]
        time_vec = np.arange(0, T) / self.fs
        data_filt = self.filterbank.evolve_device(data)  # [F, T, M] on the device
        total = None
        for chan, (bf_mat, beamf) in enumerate(zip(self.bf_mats, self.beamfs)):
            out = beamf.localize_batch(bf_mat, data_filt[chan : chan + 1], time_vec=time_vec)
            total = out["power"][0] if total is None else total + out["power"][0]
        return total.cpu().numpy()

    def process_frame(self, data, rel_threshold=0.0001):
        """One recorded pack (integer samples, last channel unused as on the devkit, reference :141-150) ->
        DoA in degrees, or NaN when the pack is below the activity threshold."""
        sig, active = active_packs(np.asarray(data)[None], rel_threshold)
        if not active[0]:
            return np.nan
        return self.doa_list[int(np.argmax(self.power_grid(sig[0])))] * 180 / np.pi

    def localizer(self):
        """The batched form of this demo's chain (wideband.WidebandSNNLocalizer over the same beamformers, matrices and filterbank):
        B packs per call, the band sum and its arg-max on the device."""
        loc = WidebandSNNLocalizer(self.beamfs, self.bf_mats, self.filterbank)
        loc.doa_list = self.doa_list
        return loc

    def streaming_localizer(self, batch=1, **kw):
        """The live form of this demo's chain: streaming.WidebandStreamingLocalizer over the same bands -- the packs of `batch` sources are
        tiles of ONE stream each (the filterbank, the STHT, the band-pass, the encoder and the LIF carry their state from pack to pack instead
        of restarting as `process_frame` does), one graph launch per pack through push_replay.  **kw: WidebandStreamingLocalizer's -- among
        them track= (a utils.Envelope) and max_track=, the per-frame read-out of localizer().track_batch for a talker who moves while the
        packs arrive (latest_track() / tracked()), and num_sources= (min_separation=, rel_threshold=; the grid is the demo's doa_list), the
        K strongest peaks per pack and per window for several talkers at once (latest_peaks() / windows())."""
        from .streaming import WidebandStreamingLocalizer

        return WidebandStreamingLocalizer(self.localizer(), batch, **kw)

    def process_frames(self, packs, rel_threshold=0.0001):
        """`process_frame` for a batch of recorded packs [B, T, num_mic + 1] of one length: DoA in degrees per pack [B], NaN for the
        packs below the activity threshold (tested per pack, on the host, as in the loop); the others go through ONE
        localizer().localize_batch call."""
        sig, active = active_packs(packs, rel_threshold)  # process_frame's test, pack by pack
        doa = np.full(len(sig), np.nan)
        if active.any():
            idx = self.localizer().localize_batch(np.ascontiguousarray(sig[active]))["argmax"].cpu().numpy()
            doa[active] = self.doa_list[idx] * 180 / np.pi
        return doa

    def run(self, source, sink=print):
        """`source`: iterable of recorded packs ([T, num_mic + 1] integer arrays); `sink(doa_deg)` replaces the visualiser."""
        for data in source:
            sink(self.process_frame(data))
