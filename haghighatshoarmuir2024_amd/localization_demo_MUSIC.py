"""Frame-by-frame localisation with MUSIC, with the structure of the reference's live demo (micloc/localization_demo_MUSIC.py:20-194),
minus the hardware: the reference records 0.25 s packs with `sox` (record.py) and pushes the DoA to a matplotlib process (visualizer.py);
here `process_frame` is the body of that loop for one recorded pack and `run` drives it from any iterable of packs, handing each result to
a callback.

Per pack (reference :132-194): activity detection on the raw integers -> MUSIC.beamforming (band-pass, band-limited DFT, the strongest
bins, steering power; csrc/music.hip) -> a DoA from the angular power spectrum by one of three host estimators.  `process_frames` runs the
active packs of a batch through ONE MUSIC.localize_batch call, `streaming_localizer` serves a source whose audio arrives in tiles.

The reference's own defaults (run_demo, :197-231: 100 active frequencies in a 1200-2000 Hz band at N = 2048) fail `beamforming`'s check,
which allows int(800 / 23.4375) = 34; this Demo fails the same way, on the first frame, and does not clamp.
"""
import numpy as np

from .music_beamformer import MUSIC
from .utils import active_packs

METHODS = ["peak", "periodic_ml", "trimmed_periodic_ml"]


class Demo:
    def __init__(self, geometry, freq_range, num_active_freq, doa_list, recording_duration=0.25, num_fft_bin=2048, fs=48_000, device=None):
        self.music = MUSIC(geometry=geometry, freq_range=freq_range, doa_list=doa_list, frame_duration=recording_duration, fs=fs, device=device)
        self.doa_list = doa_list
        self.num_active_freq = num_active_freq
        self.recording_duration = recording_duration
        self.num_fft_bin = num_fft_bin
        self.fs = fs

    def estimate_doa(self, angular_power_spec, method):
        """DoA (rad) from an angular power spectrum [G] (reference :61-105), on the host:
          "peak"                 the DoA of the first maximum;
          "periodic_ml"          the angle of mean(P exp(1j doa));
          "trimmed_periodic_ml"  the same over the indices arange(-(G // 2) // 2, (G // 2) // 2 + 1) - argmax -- the reference's
                                 expression as it stands: negative indices wrap, an index below -G raises IndexError."""
        if method not in METHODS:
            raise ValueError(f"only the following estimation methods are supported:\n{METHODS}")
        doa_list = np.asarray(self.doa_list)
        spec = np.asarray(angular_power_spec)
        if method == "peak":
            return doa_list[np.argmax(spec)]
        if method == "periodic_ml":
            return np.angle(np.mean(spec * np.exp(1j * doa_list)))
        half = len(doa_list) // 2
        idx = np.arange(-half // 2, half // 2 + 1) - np.argmax(spec)
        return np.angle(np.mean(spec[idx] * np.exp(1j * doa_list[idx])))

    def power_grid(self, data):
        """float [T, num_mic] -> angular power spectrum [G] of the pack (numpy): MUSIC.beamforming, ValueErrors included."""
        return self.music.beamforming(np.ascontiguousarray(data, dtype=np.float64), num_active_freq=self.num_active_freq, num_fft_bin=self.num_fft_bin)

    def process_frame(self, data, rel_threshold=0.0001, method="peak"):
        """One recorded pack (integer samples, last channel unused as on the devkit) -> DoA in degrees, or NaN when the pack is below the
        activity threshold."""
        sig, active = active_packs(np.asarray(data)[None], rel_threshold)
        if not active[0]:
            return np.nan
        return self.estimate_doa(self.power_grid(sig[0]), method) / np.pi * 180

    def process_frames(self, packs, rel_threshold=0.0001, method="peak"):
        """`process_frame` for a batch of recorded packs [B, T, num_mic + 1] of one length: DoA in degrees per pack [B], NaN for the packs
        below the activity threshold; the others go through ONE MUSIC.localize_batch call (a pack is one slice: frame_duration is its
        length), the estimator runs on the host per pack."""
        sig, active = active_packs(packs, rel_threshold)
        doa = np.full(len(sig), np.nan)
        if active.any():
            music = self.music
            if sig.shape[1] != int(music.fs * music.frame_duration):  # a pack of another length is still one slice, as in the loop
                music = MUSIC(geometry=music.geometry, freq_range=music.freq_range, doa_list=music.doa_list, frame_duration=sig.shape[1] / music.fs,
                              fs=music.fs, device=music.device)
            spec = music.localize_batch(np.ascontiguousarray(sig[active]), self.num_active_freq, 0.0, self.num_fft_bin)["spectrum"][:, 0].cpu().numpy()
            doa[active] = [self.estimate_doa(p, method) / np.pi * 180 for p in spec]
        return doa

    def streaming_localizer(self, batch=1, **kw):
        """The demo's MUSIC for audio that arrives in tiles (streaming.MusicStreamingLocalizer): a slice is one recording_duration, no
        overlap unless duration_overlap= says so; the other keywords are MUSIC.streaming_localizer's."""
        kw.setdefault("duration_overlap", 0.0)
        return self.music.streaming_localizer(batch, self.num_active_freq, num_fft_bin=self.num_fft_bin, **kw)

    def run(self, source, sink=print):
        """`source`: iterable of recorded packs ([T, num_mic + 1] integer arrays); `sink(doa_deg)` replaces the visualiser."""
        for data in source:
            sink(self.process_frame(data))
