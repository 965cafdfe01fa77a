"""MUSIC on the MI355X against the reference's goldens (tests/golden/make_golden_music.py) and against an independent NumPy
restatement over a random campaign of shapes."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

from haghighatshoarmuir2024_amd.array_geometry import ArrayGeometry, CenterCircularArray

pytestmark = pytest.mark.gpu

FS = 48_000
SPEC_TOL = 1e-9  # relative to the spectrum's maximum


def test_signal(seed, T, M, r_vec, theta_vec, fs=FS):
    """Restates make_golden_music.test_signal (two plane waves + white noise, seeded RandomState)."""
    rng = np.random.RandomState(seed)
    t = np.arange(T) / fs
    sig = 0.5 * rng.randn(T, M)
    for f, doa, amp in ((1900.0, 0.7, 1.0), (2200.0, -2.1, 0.6)):
        d = -np.asarray(r_vec) * np.cos(np.asarray(theta_vec) - doa) / 340.0
        sig += amp * np.sin(2 * np.pi * f * (t[:, None] - d[None, :]))
    return sig


test_signal.__test__ = False


def _music(**kw):
    from micloc.music_beamformer import MUSIC

    return MUSIC(**kw)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def test_beamforming_matches_the_reference():
    z = np.load(os.path.join(GOLDEN, "music_beamforming.npz"))
    worst = 0.0
    for i in range(int(z["num_cases"])):
        pre = f"c{i}_"
        geo = ArrayGeometry(z[pre + "r_vec"], z[pre + "theta_vec"])
        m = _music(geometry=geo, freq_range=list(z[pre + "band"]), doa_list=np.linspace(-np.pi, np.pi, int(z[pre + "G"])))
        N, k, T = int(z[pre + "N"]), int(z[pre + "k"]), int(z[pre + "T"])
        sig = test_signal(int(z[pre + "seed"]), T, len(geo), geo.r_vec, geo.theta_vec)
        spec = m.beamforming(sig, num_active_freq=k, num_fft_bin=N)
        # the selected bins, from the same kernels on the same single slice
        res = m._run(sig[None], T, T, 1, k, N, want_sel=True)
        sel = m.in_band_bins(N)[res["sel"].cpu().numpy()[0, 0]]
        assert np.array_equal(sel, z[pre + "sel"]), f"case {i}: selected bins differ"
        assert spec.shape == z[pre + "spectrum"].shape
        e = _rel(spec, z[pre + "spectrum"])
        worst = max(worst, e)
        assert e <= SPEC_TOL, f"case {i}: spectrum rel err {e:.3e}"
        # (the linear array's spectrum is mirror-symmetric: exact ties of the arg-max are the grid's, not ours)
        assert spec[np.argmax(z[pre + "spectrum"])] >= spec.max() * (1 - SPEC_TOL)
    print(f"beamforming: {int(z['num_cases'])} cases, worst spectrum rel err {worst:.3e}")


def test_apply_to_signal_and_template_match_the_reference():
    z = np.load(os.path.join(GOLDEN, "music_apply_signal.npz"))
    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    for i in range(int(z["num_cases"])):
        pre = f"c{i}_"
        m = _music(geometry=geo, freq_range=[1000.0, 4000.0], doa_list=np.linspace(-np.pi, np.pi, 121), frame_duration=float(z[pre + "frame_duration"]))
        sig = test_signal(int(z[pre + "seed"]), int(z[pre + "T"]), 7, geo.r_vec, geo.theta_vec)
        spec = m.apply_to_signal(sig, num_active_freq=int(z[pre + "k"]), duration_overlap=float(z[pre + "overlap"]), num_fft_bin=int(z[pre + "N"]))
        assert spec.shape == z[pre + "spectrum"].shape
        assert _rel(spec, z[pre + "spectrum"]) <= SPEC_TOL
        # a device tensor in, a device tensor out
        import torch

        dev = m.apply_to_signal(torch.from_numpy(sig).cuda(), int(z[pre + "k"]), float(z[pre + "overlap"]), int(z[pre + "N"]), to_host=False)
        assert isinstance(dev, torch.Tensor) and np.array_equal(dev.cpu().numpy(), spec)
    t = np.load(os.path.join(GOLDEN, "music_apply_template.npz"))
    m = _music(geometry=geo, freq_range=list(t["band"]), doa_list=np.linspace(-np.pi, np.pi, int(t["G"])), frame_duration=float(t["frame_duration"]))
    sig_temp = np.sin(2 * np.pi * float(t["freq"]) * t["time_temp"])
    kw = dict(num_active_freq=int(t["k"]), duration_overlap=float(t["overlap"]), num_fft_bin=int(t["N"]), snr_db=float(t["snr_db"]))
    np.random.seed(int(t["const_seed"]))
    spec = m.apply_to_template([t["time_temp"], sig_temp, float(t["const_doa"])], **kw)
    assert spec.shape == t["const_spectrum"].shape and _rel(spec, t["const_spectrum"]) <= SPEC_TOL
    np.random.seed(int(t["moving_seed"]))
    spec = m.apply_to_template([t["time_temp"], sig_temp, np.linspace(float(t["doa_lo"]), float(t["doa_hi"]), len(t["time_temp"]))], **kw)
    assert spec.shape == t["moving_spectrum"].shape and _rel(spec, t["moving_spectrum"]) <= SPEC_TOL


def _script_music(grid):
    return _music(geometry=CenterCircularArray(radius=4.5e-2, num_mic=7), freq_range=[1600.0, 2400.0],
                  doa_list=np.linspace(-np.pi, np.pi, grid), frame_duration=1.0, fs=FS)


def test_noisy_sweep_matches_the_reference():
    from haghighatshoarmuir2024_amd.sweep import music_noisy_sweep

    z = np.load(os.path.join(GOLDEN, "music_noisy_sweep_seed0.npz"))
    res = music_noisy_sweep(_script_music(int(z["grid"])), num_sim=int(z["num_sim"]), seed=0, mode="parity")
    assert np.array_equal(res["doa"], z["doa"])
    G = int(z["grid"])
    diff = res["argmax"] != z["argmax"]
    # the grid's two ends, -pi and pi, are one direction: their powers agree to rounding, and which end wins is decided by the
    # summation order of the reference's BLAS product.  Every other arg-max is the reference's.
    wrap = diff & (np.minimum(res["argmax"], z["argmax"]) == 0) & (np.maximum(res["argmax"], z["argmax"]) == G - 1)
    print(f"noisy sweep: {int((~diff).sum())} of {diff.size} arg-max identical, {int(wrap.sum())} at the -pi / pi grid ends")
    assert np.array_equal(diff, wrap), f"{int((diff & ~wrap).sum())} arg-max differ"
    assert wrap.sum() <= 0.01 * diff.size
    assert np.array_equal(res["err"][~diff], z["err"][~diff]) and np.allclose(res["err"], z["err"], rtol=0, atol=1e-12)
    assert np.allclose(res["pmax"], z["pmax"], rtol=1e-9, atol=0)
    assert np.allclose(res["mae_deg"], z["mae_deg"], rtol=0, atol=1e-10)


def test_speech_trials_match_the_reference():
    from haghighatshoarmuir2024_amd.sweep import music_speech_sweep, speech_source

    z = np.load(os.path.join(GOLDEN, "music_speech_seed0.npz"))
    s = np.load(os.path.join(GOLDEN, "speech_trial.npz"))
    res = music_speech_sweep(_script_music(int(z["grid"])), speech_source(FS, pcm16=s["pcm16"], rate=int(s["rate"])), snr_db_vec=z["snr_db_vec"],
                             num_sim=1, seed=0)
    assert np.array_equal(res["doa"], z["doa"]) and np.array_equal(res["argmax"], z["argmax"]) and np.array_equal(res["err"], z["err"])
    assert np.allclose(res["pmax"], z["pmax"], rtol=1e-9, atol=0)


def _numpy_music(sig, b, a, L, hop, S, N, k, fs, band, steer):
    """Independent restatement: per slice, lfilter, frames, FFT, in-band bins of linspace(0, fs, N), stable top-k, steering power."""
    from scipy.signal import lfilter

    fv = np.linspace(0, fs, N)
    inb = np.nonzero((band[0] <= fv) & (fv <= band[1]))[0]
    out, sels, gaps = [], [], []
    for s in range(S):
        x = sig[s * hop : min(s * hop + L, len(sig))]
        F = len(x) // N
        y = lfilter(b, a, x, axis=0)[: F * N]
        X = np.fft.fft(y.T.reshape(y.shape[1], F, N), axis=-1)[:, :, inb]  # [M, F, nbin]
        p = np.mean(X.real**2 + X.imag**2, axis=(0, 1))
        order = np.argsort(p, kind="stable")
        sel = order[len(order) - (len(order) if k == 0 or k > len(order) else k) :]
        srt = p[order]
        kk = len(sel)
        if kk < len(order):
            gaps.append(abs(srt[-kk] - srt[-kk - 1]) / srt[-kk])
        P = np.zeros(steer.shape[2])
        for j in sel:
            z = np.conj(steer[j]).T @ X[:, :, j]  # [G, F]
            P += np.mean(np.abs(z) ** 2, axis=-1)
        out.append(P)
        sels.append(sel)
    return np.asarray(out), sels, (min(gaps) if gaps else 1.0)


def test_random_campaign_against_numpy():
    import torch

    rng = np.random.RandomState(2024)
    ran = skipped = 0
    worst = 0.0
    for case in range(240):
        M = int(rng.randint(2, 17))
        N = int(rng.choice([64, 65, 127, 256, 333, 512, 1000, 1024, 2048, 4096]) if rng.rand() < 0.7 else rng.randint(64, 4097))
        fd = float(rng.choice([0.02, 0.05, 0.1]))
        L = int(FS * fd)
        if N > L:
            N = L
        f_lo = float(rng.uniform(200, 6000))
        band = [f_lo, f_lo + float(rng.uniform(FS / N * 1.5, 4000))]
        geo = ArrayGeometry(rng.uniform(0, 0.06, M), rng.uniform(0, 2 * np.pi, M))
        G = int(rng.randint(1, 200))
        m = _music(geometry=geo, freq_range=band, doa_list=np.sort(rng.uniform(-np.pi, np.pi, G)), frame_duration=fd)
        nb = len(m.in_band_bins(N))
        kmax = int((band[1] - band[0]) / (FS / N))
        if nb == 0 or kmax < 1:
            continue
        k = int(rng.choice([0, 1, min(3, kmax), kmax, rng.randint(0, kmax + 1)]))
        ov = float(rng.choice([0.0, fd / 4, fd / 2]))
        B = int(rng.randint(1, 4))
        T = int(rng.randint(L // 2 + 1, 4 * L))
        starts, lens, L_, hop = m.slice_plan(T, ov)
        if len(starts) == 0 or lens.min() < N:
            continue
        x = rng.randn(B, T, M) + np.sin(2 * np.pi * band[0] * np.arange(T) / FS)[None, :, None]
        out = m.localize_batch(torch.from_numpy(x).cuda(), k, ov, N, want_sel=True)
        spec = out["spectrum"].cpu().numpy()
        sel = out["sel"].cpu().numpy()
        b, a = m.filterbank.ba_list[0]
        steer = m.array_response(np.linspace(0, FS, N)[m.in_band_bins(N)])
        for i in range(B):
            ref, rsel, gap = _numpy_music(x[i], b, a, L_, hop, len(starts), N, k, FS, band, steer)
            if gap < 1e-9:
                skipped += 1
                continue
            for s in range(len(starts)):
                assert np.array_equal(np.sort(sel[i, s]), np.sort(rsel[s])), f"case {case}: selected bins differ"
            e = _rel(spec[i], ref)
            worst = max(worst, e)
            assert e <= SPEC_TOL, f"case {case} (M={M} N={N} k={k} G={G} S={len(starts)}): rel err {e:.3e}"
            pw = np.mean(np.abs(ref) ** 2, axis=0)
            assert np.allclose(out["power"].cpu().numpy()[i], pw, rtol=1e-9, atol=0)
            ran += 1
    print(f"campaign: {ran} trials compared, {skipped} near-ties skipped, worst rel err {worst:.3e}")
    assert ran >= 150


def test_localize_batch_equals_single_calls_bit_for_bit():
    m = _script_music(57)
    rng = np.random.RandomState(5)
    x = rng.randn(5, 20000, 7)
    m.frame_duration = 0.2
    out = m.localize_batch(x, 3, 0.05, 1000)
    spec = out["spectrum"].cpu().numpy()
    for i in range(5):
        one = m.apply_to_signal(x[i], 3, 0.05, 1000)
        assert np.array_equal(one, spec[i])
        p = np.mean(np.abs(one) ** 2, axis=0)
        assert np.array_equal(out["power"].cpu().numpy()[i], p) and int(out["argmax"].cpu()[i]) == int(np.argmax(p))


def test_throughput_sweep_independent_of_batch_size_and_resume(tmp_path):
    from haghighatshoarmuir2024_amd.sweep import music_noisy_sweep

    m = _script_music(57)
    kw = dict(snr_db_vec=[-5.0, 10.0], num_sim=6, seed=3, mode="throughput", test_duration=0.3)
    m.frame_duration = 0.25
    full = music_noisy_sweep(m, batch_trials=12, **kw)
    small = music_noisy_sweep(m, batch_trials=5, **kw)
    assert np.array_equal(full["argmax"], small["argmax"]) and np.array_equal(full["pmax"], small["pmax"])
    # resume: a first run that only finished part of the trials, then the full run from the same directory
    out_dir = str(tmp_path)
    music_noisy_sweep(m, batch_trials=4, out_dir=out_dir, **{**kw})
    import glob

    files = sorted(glob.glob(os.path.join(out_dir, "music-noisy-*", "trials_*.npy")))
    assert len(files) == 3
    os.remove(files[1])  # an interrupted run: one batch missing
    resumed = music_noisy_sweep(m, batch_trials=4, out_dir=out_dir, **kw)
    assert resumed["persistence"]["trials_loaded"] == 8 and resumed["persistence"]["files_written"] == 1
    assert np.array_equal(resumed["argmax"], full["argmax"]) and np.array_equal(resumed["pmax"], full["pmax"])
    # parity mode resumes onto the uninterrupted run's results as well
    pk = dict(kw, mode="parity")
    ref = music_noisy_sweep(m, batch_trials=4, **pk)
    first = music_noisy_sweep(m, batch_trials=4, out_dir=out_dir, **pk)
    assert first["persistence"]["dir"] != resumed["persistence"]["dir"]  # a directory of its own (the key covers the mode)
    os.remove(sorted(glob.glob(os.path.join(first["persistence"]["dir"], "trials_*.npy")))[0])
    again = music_noisy_sweep(m, batch_trials=4, out_dir=out_dir, **pk)
    assert np.array_equal(again["argmax"], ref["argmax"]) and np.array_equal(again["pmax"], ref["pmax"])
