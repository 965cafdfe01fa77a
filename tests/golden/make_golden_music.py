#!/usr/bin/env python3
"""Generate the MUSIC golden vectors in tests/golden/ by running the *real* reference `micloc.music_beamformer.MUSIC`.

Run in the build container only (the reference must be importable, with PYTHONPATH pointing at it):

    python tests/golden/make_golden_music.py              # all fixtures
    python tests/golden/make_golden_music.py beamforming  # one fixture

Only numeric data is written (.npz): parameters, seeds and the reference's outputs.  Test signals are not stored: they are
regenerated from the recorded seed by `test_signal` below (np.random.RandomState is a stable stream), which the tests restate.

Fixtures
  music_beamforming.npz     MUSIC.beamforming over (geometry, N, k): spectrum and the selected in-band bins
  music_apply_signal.npz    MUSIC.apply_to_signal with overlap > 0: spectra [S, G] and the slice plan (starts, lengths, F)
  music_apply_template.npz  MUSIC.apply_to_template at a constant and a moving DoA (seeded global stream)
  music_noisy_sweep_seed0.npz  the complete noisy-target MUSIC sweep (paper_plots/target_localization_MUSIC.py, 11 SNRs x 100)
  music_speech_seed0.npz    2 SNRs x 1 trial of the speech MUSIC sweep (the PCM of speech_trial.npz)
"""
import os
import sys

REF = os.environ.get("MICLOC_REFERENCE", "/root/reference")
if not os.path.isdir(REF):
    sys.exit("reference not present: golden vectors can only be regenerated in the build container")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != os.path.abspath(os.path.join(HERE, "..", ".."))]

import numpy as np  # noqa: E402

import micloc  # noqa: E402

assert os.path.abspath(list(micloc.__path__)[0]).startswith(os.path.abspath(REF)), micloc

from micloc.array_geometry import CenterCircularArray, LinearArray, Random2DArray  # noqa: E402
from micloc.music_beamformer import MUSIC  # noqa: E402

FS = 48_000


def geometries():
    np.random.seed(1234)
    rnd = Random2DArray(radius=4.5e-2, num_mic=13)
    return {
        "circular7": CenterCircularArray(radius=4.5e-2, num_mic=7),
        "random13": rnd,
        "linear8": LinearArray(spacing=2.0e-2, num_mic=8, radius=4.5e-2),
    }


def test_signal(seed, T, M, r_vec, theta_vec, fs=FS):
    """Two plane waves (1.9 and 2.2 kHz, DoAs 0.7 and -2.1 rad) plus white noise; restated in tests/test_hip_music.py."""
    rng = np.random.RandomState(seed)
    t = np.arange(T) / fs
    sig = 0.5 * rng.randn(T, M)
    for f, doa, amp in ((1900.0, 0.7, 1.0), (2200.0, -2.1, 0.6)):
        d = -np.asarray(r_vec) * np.cos(np.asarray(theta_vec) - doa) / 340.0
        sig += amp * np.sin(2 * np.pi * f * (t[:, None] - d[None, :]))
    return sig


def fix_beamforming():
    out = {}
    geos = geometries()
    cases = []
    i = 0
    for gname, geo in geos.items():
        for N in (2048, 1000, 512):
            band = (1600.0, 2400.0) if N != 512 else (1000.0, 4000.0)
            kmax = int((band[1] - band[0]) / (FS / N))
            for k in (0, 1, 5, kmax):
                G = (57, 121, 449)[i % 3]
                T = (12000, 9001, 6000)[i % 3]
                doa_list = np.linspace(-np.pi, np.pi, G)
                mus = MUSIC(geometry=geo, freq_range=list(band), doa_list=doa_list, fs=FS)
                sig = test_signal(100 + i, T, len(geo), geo.r_vec, geo.theta_vec)
                spec = mus.beamforming(sig, num_active_freq=k, num_fft_bin=N)
                # the selected bins, computed with plain NumPy as the reference does (for the tests' selection check)
                from scipy.signal import lfilter

                b, a = mus.filterbank.ba_list[0]
                y = lfilter(b, a, sig, axis=0)
                F = T // N
                X = np.fft.fft(y[: F * N].T.reshape(len(geo), F, N), axis=-1)
                fv = np.linspace(0, FS, N)
                inb = np.nonzero((band[0] <= fv) & (fv <= band[1]))[0]
                p = np.mean(np.abs(X[:, :, inb]) ** 2, axis=(0, 1))
                sel = inb[np.argsort(p)[-k:]]
                srt = np.sort(p)
                gap = np.min(np.abs(np.diff(srt)) / srt[1:]) if len(srt) > 1 else 1.0
                pre = f"c{i}_"
                out.update({pre + "geometry": gname, pre + "r_vec": np.asarray(geo.r_vec, dtype=np.float64),
                            pre + "theta_vec": np.asarray(geo.theta_vec, dtype=np.float64), pre + "band": np.asarray(band), pre + "N": N,
                            pre + "k": k, pre + "G": G, pre + "T": T, pre + "seed": 100 + i, pre + "spectrum": np.asarray(spec, dtype=np.float64),
                            pre + "sel": sel.astype(np.int64), pre + "b": np.asarray(b), pre + "a": np.asarray(a), pre + "min_gap": gap})
                if i == 0:
                    fr = fv[inb[:3]]
                    out.update(ar_freqs=fr, array_response=mus.array_response(fr))
                cases.append(i)
                i += 1
    out["num_cases"] = len(cases)
    np.savez_compressed(os.path.join(HERE, "music_beamforming.npz"), **out)


def fix_apply_signal():
    out = {}
    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    # (frame_duration, overlap, T): leftover kept, leftover dropped, no full slice (T < L), overlap at the script value 0
    cases = [(0.05, 0.01, 2400 + 3 * 1920 + 1500), (0.05, 0.02, 2400 + 4 * 1440 + 500), (0.05, 0.0, 2000)]
    for i, (fd, ov, T) in enumerate(cases):
        doa_list = np.linspace(-np.pi, np.pi, 121)
        mus = MUSIC(geometry=geo, freq_range=[1000.0, 4000.0], doa_list=doa_list, frame_duration=fd, fs=FS)
        sig = test_signal(500 + i, T, 7, geo.r_vec, geo.theta_vec)
        starts, lens = [], []
        orig = mus.beamforming

        def rec(sig_in, num_active_freq, num_fft_bin, _o=orig):
            # a ramp in channel 0 would change the result: the slice start is found from the slice's own samples instead
            lens.append(len(sig_in))
            starts.append(int(np.nonzero(np.all(sig == sig_in[0], axis=1))[0][0]))
            return _o(sig_in=sig_in, num_active_freq=num_active_freq, num_fft_bin=num_fft_bin)

        mus.beamforming = rec
        spec = mus.apply_to_signal(sig, num_active_freq=3, duration_overlap=ov, num_fft_bin=512)
        pre = f"c{i}_"
        out.update({pre + "frame_duration": fd, pre + "overlap": ov, pre + "T": T, pre + "seed": 500 + i, pre + "N": 512, pre + "k": 3,
                    pre + "spectrum": np.asarray(spec, dtype=np.float64), pre + "starts": np.asarray(starts, dtype=np.int64),
                    pre + "lens": np.asarray(lens, dtype=np.int64), pre + "F": np.asarray(lens, dtype=np.int64) // 512})
    out["num_cases"] = len(cases)
    np.savez_compressed(os.path.join(HERE, "music_apply_signal.npz"), **out)


def fix_apply_template():
    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    doa_list = np.linspace(-np.pi, np.pi, 57)
    mus = MUSIC(geometry=geo, freq_range=[1600.0, 2400.0], doa_list=doa_list, frame_duration=0.05, fs=FS)
    time_temp = np.arange(0, 0.2, step=1 / FS)
    sig_temp = np.sin(2 * np.pi * 2000.0 * time_temp)
    out = {"time_temp": time_temp, "freq": 2000.0}
    np.random.seed(7)
    out["const_doa"] = 1.1
    out["const_spectrum"] = mus.apply_to_template([time_temp, sig_temp, 1.1], num_active_freq=2, duration_overlap=0.01, num_fft_bin=512,
                                                  snr_db=5.0)
    out["const_seed"] = 7
    np.random.seed(8)
    doa_mov = np.linspace(-1.0, 2.0, len(time_temp))
    out["moving_spectrum"] = mus.apply_to_template([time_temp, sig_temp, doa_mov], num_active_freq=2, duration_overlap=0.01, num_fft_bin=512,
                                                   snr_db=5.0)
    out["moving_seed"] = 8
    out.update(k=2, overlap=0.01, N=512, snr_db=5.0, frame_duration=0.05, G=57, band=np.array([1600.0, 2400.0]), doa_lo=-1.0, doa_hi=2.0)
    np.savez_compressed(os.path.join(HERE, "music_apply_template.npz"), **out)


def _trial(args):
    state, time_test, sig_test, doa, snr, fd, grid, N = args
    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    doa_list = np.linspace(-np.pi, np.pi, grid)
    mus = MUSIC(geometry=geo, freq_range=[1600.0, 2400.0], doa_list=doa_list, frame_duration=fd, fs=FS)
    np.random.set_state(state)
    sig_bf = mus.apply_to_template(template=[time_test, sig_test, doa], snr_db=snr, num_active_freq=1, duration_overlap=0.0, num_fft_bin=N)
    power = np.mean(np.abs(sig_bf) ** 2, axis=0)
    am = int(np.argmax(power))
    return am, float(power[am]), power


def _sweep(time_test, sig_test, snr_trial, seed, fd, grid, procs=8):
    """The statistical loop of target_localization_MUSIC.py (rand(1) per trial, then apply_to_template's randn(T, M)); every trial
    runs from the global stream's state at its own draw, so the trials can run in parallel processes with the script's results."""
    import multiprocessing as mp

    np.random.seed(seed)
    T = len(np.arange(time_test.min(), time_test.max(), step=1 / FS))
    doas, jobs = [], []
    for snr in snr_trial:
        doa = np.random.rand(1)[0] * 2 * np.pi
        doas.append(doa)
        jobs.append((np.random.get_state(), time_test, sig_test, doa, snr, fd, grid, 2048))
        np.random.randn(T, 7)
    with mp.Pool(procs) as pool:
        res = pool.map(_trial, jobs, chunksize=4)
    doa_list = np.linspace(-np.pi, np.pi, grid)
    am = np.array([r[0] for r in res], dtype=np.int64)
    pm = np.array([r[1] for r in res])
    doas = np.asarray(doas)
    err = np.arcsin(np.abs(np.sin(doa_list[am] - doas)))
    return doas, am, pm, err, np.stack([r[2] for r in res])


def fix_noisy_sweep():
    fs = FS
    snr_db_vec = np.linspace(-10, 20, 11)
    num_sim = 100
    gain = (fs / 2) / (2400.0 - 1600.0)
    time_test = np.arange(0, 1000e-3, step=1 / fs)
    sig_test = np.sin(2 * np.pi * 2000.0 * time_test)
    snr_trial = np.repeat(snr_db_vec - 10 * np.log10(gain), num_sim)
    doas, am, pm, err, _ = _sweep(time_test, sig_test, snr_trial, 0, 1.0, 8 * 7 + 1)
    shape = (len(snr_db_vec), num_sim)
    np.savez_compressed(os.path.join(HERE, "music_noisy_sweep_seed0.npz"), seed=0, snr_db_vec=snr_db_vec, num_sim=num_sim, grid=57,
                        doa=doas.reshape(shape), argmax=am.reshape(shape), pmax=pm.reshape(shape), err=err.reshape(shape),
                        mae_deg=np.mean(err.reshape(shape), axis=1) * 180 / np.pi)


def fix_speech():
    z = np.load(os.path.join(HERE, "speech_trial.npz"))
    sig = z["pcm16"].astype(np.float64) / 32768.0
    rate = int(z["rate"])
    time_test = np.arange(len(sig)) / rate
    time_fs = np.linspace(time_test[0], time_test[-1], int(len(sig) / rate * FS))
    sig_fs = np.interp(time_fs, time_test, sig)
    snr_db_vec = np.array([0.0, 20.0])
    doas, am, pm, err, power = _sweep(time_fs, sig_fs, np.repeat(snr_db_vec, 1), 0, 1.0, 64 * 7 + 1, procs=2)
    np.savez_compressed(os.path.join(HERE, "music_speech_seed0.npz"), seed=0, snr_db_vec=snr_db_vec, num_sim=1, grid=449,
                        doa=doas.reshape(2, 1), argmax=am.reshape(2, 1), pmax=pm.reshape(2, 1), err=err.reshape(2, 1), power=power)


FIXTURES = {"beamforming": fix_beamforming, "apply_signal": fix_apply_signal, "apply_template": fix_apply_template,
            "noisy_sweep": fix_noisy_sweep, "speech": fix_speech}

if __name__ == "__main__":
    for name in sys.argv[1:] or list(FIXTURES):
        FIXTURES[name]()
        print("wrote", name)
