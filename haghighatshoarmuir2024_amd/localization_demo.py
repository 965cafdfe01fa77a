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

from .utils import active_packs
from .wideband import WidebandBeamformerLocalizer, complex_band, design_bands


class Demo:
    def __init__(self, geometry, freq_bands, doa_list, recording_duration, kernel_duration, fs, device=None):
        self.beamfs, self.bf_mats, self.filterbank = design_bands(freq_bands, recording_duration, fs, complex_band(geometry, doa_list, kernel_duration, fs, device),
                                                                  order=2, device=device)
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
        sig, active = active_packs(np.asarray(data)[None], rel_threshold)
        if not active[0]:
            return np.nan
        return self.doa_list[int(np.argmax(self.power_grid(sig[0])))] * 180 / np.pi

    def localizer(self):
        """The batched form of this demo's chain (wideband.WidebandBeamformerLocalizer over the same beamformers, matrices and
        filterbank): B packs per call, every band's chain in one batch, the band sum and its arg-max on the device.  Its
        streaming_localizer(batch, **kw) is the live form (streaming.WidebandComplexStreamingLocalizer), which with track= (a utils.Envelope)
        and max_track= also follows a talker who moves while the packs arrive (latest_track() / tracked()), and with num_sources=
        (min_separation=, rel_threshold=; the grid is the demo's doa_list) reports the K strongest peaks per pack and per window for several
        talkers at once (latest_peaks() / windows())."""
        loc = WidebandBeamformerLocalizer(self.beamfs, self.bf_mats, self.filterbank)
        loc.doa_list = self.doa_list
        return loc

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
