"""Frame-by-frame localisation with the complex `Beamformer`, with the structure of the reference's live demo
(micloc/localization_demo.py:22-185), minus the hardware: the reference records 0.25 s packs with `sox` (record.py) and pushes the DoA
to a matplotlib process (visualizer.py); here `process_frame` is the body of that loop for one recorded pack and `run` drives it from
any iterable of packs, handing each result to a callback.

Per pack (reference :127-185): activity detection on the raw integers -> order-2 Butterworth filterbank -> per band
Beamformer.apply_to_signal -> mean |y|^2 per DoA, summed over the bands -> arg-max.  Everything after the activity check runs on the
MI355X: `power_grid` band by band (the filterbank through micloc_lfilter_f64, each band through the complex pipeline, power only: the
T x G product the reference materialises is never formed), `localizer()` all bands of B packs as one batch.
"""
import numpy as np

from .beamformer import Beamformer
from .filterbank import ButterworthFilterbank


class Demo:
    def __init__(self, geometry, freq_bands, doa_list, recording_duration, kernel_duration, fs, device=None):
        freq_bands = np.asarray(freq_bands)
        if freq_bands.ndim == 1:
            freq_bands = freq_bands.reshape(1, -1)
        self.beamfs, self.bf_mats = [], []
        for freq_range in freq_bands:
            freq_mid = np.mean(freq_range)
            beamf = Beamformer(geometry=geometry, kernel_duration=kernel_duration, freq_range=freq_range, fs=fs, device=device)
            self.beamfs.append(beamf)
            time_temp = np.arange(0, recording_duration, step=1 / fs)
            sig_temp = np.sin(2 * np.pi * freq_mid * time_temp)
            bf_vecs, _ = beamf.design_from_template(template=(time_temp, sig_temp), doa_list=doa_list)
            self.bf_mats.append(bf_vecs)
        order = 2
        self.filterbank = ButterworthFilterbank(freq_bands=freq_bands, order=order, fs=fs, device=device)
        self.doa_list = np.asarray(doa_list)
        self.recording_duration = recording_duration
        self.kernel_duration = kernel_duration
        self.fs = fs

    def power_grid(self, data):
        """float [T, num_mic] -> angular power pattern [G] summed over the frequency bands (device -> numpy)."""
        data = np.ascontiguousarray(data, dtype=np.float64)
        data_filt = self.filterbank.evolve_device(data)  # [F, T, M] on the device
        total = None
        for chan, (bf_mat, beamf) in enumerate(zip(self.bf_mats, self.beamfs)):
            out = beamf.localize_batch(bf_mat, data_filt[chan : chan + 1])
            total = out["power"][0] if total is None else total + out["power"][0]
        return total.cpu().numpy()

    def process_frame(self, data, rel_threshold=0.0001):
        """One recorded pack (integer samples, last channel unused as on the devkit, reference :127-137) ->
        DoA in degrees, or NaN when the pack is below the activity threshold."""
        data = np.asarray(data)
        max_value = np.iinfo(data.dtype).max if np.issubdtype(data.dtype, np.integer) else 1.0
        threshold = rel_threshold * max_value
        sig = np.asarray(data[:, :-1], dtype=np.float64)
        if np.sqrt(np.mean(sig**2)) < threshold:
            return np.nan
        return self.doa_list[int(np.argmax(self.power_grid(sig)))] * 180 / np.pi

    def localizer(self):
        """The batched form of this demo's chain (wideband.WidebandBeamformerLocalizer over the same beamformers, matrices and
        filterbank): B packs per call, every band's chain in one batch, the band sum and its arg-max on the device."""
        from .wideband import WidebandBeamformerLocalizer

        loc = WidebandBeamformerLocalizer(self.beamfs, self.bf_mats, self.filterbank)
        loc.doa_list = self.doa_list
        return loc

    def process_frames(self, packs, rel_threshold=0.0001):
        """`process_frame` for a batch of recorded packs [B, T, num_mic + 1] of one length: DoA in degrees per pack [B], NaN for the
        packs below the activity threshold (tested per pack, on the host, as in the loop); the others go through ONE
        localizer().localize_batch call."""
        packs = np.asarray(packs)
        max_value = np.iinfo(packs.dtype).max if np.issubdtype(packs.dtype, np.integer) else 1.0
        sig = np.asarray(packs[:, :, :-1], dtype=np.float64)
        active = np.asarray([np.sqrt(np.mean(s**2)) >= rel_threshold * max_value for s in sig], dtype=bool)  # process_frame's test, pack by pack
        doa = np.full(len(packs), np.nan)
        if active.any():
            idx = self.localizer().localize_batch(np.ascontiguousarray(sig[active]))["argmax"].cpu().numpy()
            doa[active] = self.doa_list[idx] * 180 / np.pi
        return doa

    def run(self, source, sink=print):
        """`source`: iterable of recorded packs ([T, num_mic + 1] integer arrays); `sink(doa_deg)` replaces the visualiser."""
        for data in source:
            sink(self.process_frame(data))
