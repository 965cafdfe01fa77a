#!/usr/bin/env python3
"""Generate tests/golden/music_demo.npz by running the *real* reference `micloc.localization_demo_MUSIC.Demo`.

Run where the reference is present (MICLOC_REFERENCE names its checkout):

    MICLOC_REFERENCE=<reference checkout> python tests/golden/make_golden_music_demo.py

The reference module imports its sound-card recorder and its matplotlib visualiser at the top.  Neither is used by the methods run here;
where one of them cannot be imported on this machine, an empty stand-in module of this generator's own (two classes that refuse to be
built) takes its place in sys.modules first.

Only numeric data is written: the recorded packs as the devkit delivers them (int32 [12000, 8], the last channel empty), the reference's
angular power spectrum of every active pack (MUSIC.beamforming, as the loop of run_demo calls it), the three estimators' DoAs of those
spectra, and the three estimators on two synthetic spectra -- one peaked near index 10, one near index 200, where the trimmed estimator's
index range leaves the array and the reference raises IndexError (recorded as NaN and a flag).

The case: the 7-microphone circular array, 225 DoAs, band 1200-2000 Hz, N = 2048, 20 active frequencies (the reference's own default of
100 fails beamforming's check, which allows 34).
"""
import importlib
import os
import sys
import types

REF = os.environ.get("MICLOC_REFERENCE", "")
if not os.path.isdir(REF):
    sys.exit("set MICLOC_REFERENCE to a checkout of the reference: golden vectors can only be regenerated where it is present")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != os.path.abspath(os.path.join(HERE, "..", ".."))]

import numpy as np  # noqa: E402

import micloc  # noqa: E402

assert os.path.abspath(list(micloc.__path__)[0]).startswith(os.path.abspath(REF)), micloc


def _stand_in(name, cls):
    try:
        importlib.import_module(name)
    except Exception:
        mod = types.ModuleType(name)

        def refuse(self, *a, **kw):
            raise RuntimeError(f"{name}.{cls} is a stand-in: the fixture generator has no hardware")

        setattr(mod, cls, type(cls, (), {"__init__": refuse}))
        sys.modules[name] = mod


_stand_in("micloc.record", "AudioRecorder")
_stand_in("micloc.visualizer", "Visualizer")

from micloc.array_geometry import CenterCircularArray  # noqa: E402
from micloc.localization_demo_MUSIC import Demo  # noqa: E402

FS = 48_000
T = 12_000
M = 7
G = 32 * M + 1
N = 2048
K = 20
BAND = (1200.0, 2000.0)
METHODS = ("peak", "periodic_ml", "trimmed_periodic_ml")


def pack(seed, amp, doa, geo):
    """int32 [T, M + 1]: a 1.5 kHz and a 1.8 kHz plane wave from `doa` plus white noise at `amp` of full scale; last channel zero."""
    rng = np.random.RandomState(seed)
    t = np.arange(T) / FS
    d = -np.asarray(geo.r_vec) * np.cos(np.asarray(geo.theta_vec) - doa) / 340.0
    sig = 0.2 * rng.randn(T, M)
    for f, a in ((1500.0, 1.0), (1800.0, 0.7)):
        sig += a * np.sin(2 * np.pi * f * (t[:, None] - d[None, :]))
    out = np.zeros((T, M + 1), dtype=np.int32)
    out[:, :M] = np.round(sig / 4.0 * amp * np.iinfo(np.int32).max).astype(np.int32)
    return out


def estimates(demo, spec):
    """([3] DoAs, [3] flags): NaN and 1 where the reference raises IndexError."""
    doa, err = np.full(3, np.nan), np.zeros(3, dtype=np.int64)
    for i, m in enumerate(METHODS):
        try:
            doa[i] = demo.estimate_doa(angular_power_spec=spec, method=m)
        except IndexError:
            err[i] = 1
    return doa, err


def main():
    geo = CenterCircularArray(radius=4.5e-2, num_mic=M)
    doa_list = np.linspace(-np.pi, np.pi, G)
    demo = Demo(geometry=geo, freq_range=np.asarray(BAND), num_active_freq=K, doa_list=doa_list, recording_duration=T / FS, num_fft_bin=N, fs=FS)
    # two active packs and one below the loop's activity threshold (rms < 1e-4 of full scale)
    packs = np.stack([pack(900, 0.5, 0.9, geo), pack(901, 0.02, -2.4, geo), pack(902, 2e-5, 0.3, geo)])
    rel_threshold = 0.0001
    active, specs, doas, errs = [], [], [], []
    for p in packs:
        data = np.asarray(p[:, :-1], dtype=np.float64)
        is_active = not (np.sqrt(np.mean(data**2)) < rel_threshold * np.iinfo(p.dtype).max)
        active.append(is_active)
        if is_active:
            spec = demo.music.beamforming(sig_in=data, num_active_freq=K, num_fft_bin=N)
            d, e = estimates(demo, spec)
            specs.append(np.asarray(spec, dtype=np.float64))
            doas.append(d)
            errs.append(e)
    assert active == [True, True, False], active
    # synthetic spectra: a von-Mises-like bump on a small floor
    idx = np.arange(G)
    syn = np.stack([0.05 + np.exp(-0.5 * ((idx - c) / 6.0) ** 2) for c in (10.3, 200.4)])
    syn_doa, syn_err = zip(*[estimates(demo, s) for s in syn])
    assert np.asarray(syn_err)[1, 2] == 1 and np.asarray(syn_err).sum() == 1 and np.asarray(errs).sum() in (0, 1, 2)
    np.savez_compressed(os.path.join(HERE, "music_demo.npz"), packs=packs, active=np.asarray(active), ang_pow_spec=np.stack(specs),
                        doa=np.stack(doas), doa_index_error=np.stack(errs), syn_spectrum=syn, syn_doa=np.stack(syn_doa),
                        syn_index_error=np.stack(syn_err), methods=np.asarray(METHODS), fs=FS, N=N, k=K, band=np.asarray(BAND), G=G,
                        radius=4.5e-2, num_mic=M, rel_threshold=rel_threshold)
    print("wrote music_demo.npz:", np.stack(doas), np.stack(errs), np.stack(syn_doa))


if __name__ == "__main__":
    main()
