"""The multi-source read-out on the MI355X (micloc_doa_peaks_f64, utils.find_doa_peaks, localize_batch(num_sources=)) against the
NumPy restatement of the rule (tests/multisource_ref.py), and multi_target_sweep against noisy_target_sweep and the restatement."""
import os

import numpy as np
import pytest

import multisource_ref as R
from conftest import GOLDEN, campaign_seeds, golden

pytestmark = pytest.mark.gpu

KINDS = {R.LINEAR: "linear", R.CIRCULAR: "circular", R.CIRCULAR_CLOSED: "circular_closed"}
ROWS = 8


def _grid(rng, kind, G):
    if kind == R.CIRCULAR_CLOSED:
        return np.linspace(-np.pi, np.pi, G)
    if kind == R.CIRCULAR:
        return np.arange(G) * (2 * np.pi / G)
    return np.sort(rng.uniform(-2.0, 2.0, G)) if rng.rand() < 0.5 else np.linspace(-np.pi / 2, np.pi / 2, G)


def _rows(rng, G):
    style = rng.randint(4)
    if style == 0:
        p = rng.randint(0, 5, size=(ROWS, G)).astype(np.float64)  # plateaus and exact ties everywhere
    elif style == 1:
        p = rng.rand(ROWS, G)
    elif style == 2:  # a few smooth bumps of equal height (ties between peaks)
        x = np.arange(G)
        p = np.zeros((ROWS, G))
        for r in range(ROWS):
            for c in rng.randint(0, G, size=rng.randint(1, 6)):
                p[r] += np.exp(-0.5 * ((x - c) / max(1.0, G / 60)) ** 2)
            p[r] = np.round(p[r], 3)
    else:
        p = np.repeat(rng.randn(ROWS, (G + 3) // 4), 4, axis=1)[:, :G]  # plateaus of four
    nan = rng.rand(ROWS, G) < (0.05 if rng.rand() < 0.5 else 0.0)
    p[nan] = np.nan
    if rng.rand() < 0.2:
        p[0] = np.nan
    if G > 1 and rng.rand() < 0.3:
        p[:, -1] = p[:, 0]  # the closed seam tied
    return p


@pytest.mark.parametrize("seed", campaign_seeds("multisource", 40))
def test_doa_peaks_equal_the_restatement(seed):
    import torch

    from haghighatshoarmuir2024_amd import runtime

    rng = np.random.RandomState(1000 + seed)
    G = int(rng.choice([1, 2, 3, 5, 57, 449, int(rng.randint(1, 4097)), 4096]))
    K = int(rng.randint(1, 17))
    kind = int(rng.randint(3))
    doa = _grid(rng, kind, G)
    step = abs(doa[-1] - doa[0]) / max(1, G - 1)
    sep = float(rng.choice([0.0, 2 * step, 3.5 * step, rng.uniform(0, 1.0)]))
    rel = float(rng.choice([0.0, 0.0, 0.3, 0.9]))
    p = _rows(rng, G)
    idx, val = runtime.doa_peaks(torch.from_numpy(p).cuda(), doa, KINDS[kind], K, sep, rel)
    ri, rv = R.peaks(p, doa, K, sep, rel, kind)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri, err_msg=f"G={G} K={K} kind={kind} sep={sep} rel={rel}")
    np.testing.assert_array_equal(val.cpu().numpy(), rv)


def test_find_doa_peaks_surface():
    import torch

    from micloc.utils import find_doa_peaks

    rng = np.random.RandomState(5)
    doa = np.linspace(-np.pi, np.pi, 449)
    p = rng.rand(6, 449)
    i, v = find_doa_peaks(p, doa, 3)  # host in, host out
    assert isinstance(i, np.ndarray) and i.dtype == np.int32 and i.shape == (6, 3) and v.shape == (6, 3)
    ri, rv = R.peaks(p, doa, 3)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(v, rv)
    i1, v1 = find_doa_peaks(p[2], doa, 3)  # one row
    np.testing.assert_array_equal(i1, ri[2])
    d_i, d_v = find_doa_peaks(torch.from_numpy(p).cuda(), doa, 3, min_separation=0.5, rel_threshold=0.2)  # device in, device out
    assert d_i.is_cuda and d_v.is_cuda
    ri, rv = R.peaks(p, doa, 3, 0.5, 0.2)
    np.testing.assert_array_equal(d_i.cpu().numpy(), ri)
    i1, _ = find_doa_peaks(p, doa, 1)
    np.testing.assert_array_equal(i1[:, 0], np.argmax(p, axis=1))
    # the grid kind can be overridden
    i2, _ = find_doa_peaks(p, doa, 3, grid="linear")
    np.testing.assert_array_equal(i2, R.peaks(p, doa, 3, kind=R.LINEAR)[0])
    with pytest.raises(ValueError):
        find_doa_peaks(p, doa, 17)


def _snn(cfg2):
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    tau = 1.0 / (2 * np.pi * 2000)
    return SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=48_000)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
            continue
        np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=k)


def test_localize_batch_k1_is_argmax_and_default_is_unchanged(cfg2):
    from micloc.beamformer import Beamformer

    z = golden("trials_cfg2.npz")
    x = z["sig_in"]
    doa = cfg2["doa_list"]
    bf = _snn(cfg2)
    plain = bf.localize_batch(cfg2["bf_mat"], x)
    assert "peaks" not in plain and "peak_power" not in plain
    np.testing.assert_array_equal(plain["argmax"].cpu().numpy(), z["argmax"])
    multi = bf.localize_batch(cfg2["bf_mat"], x, num_sources=1, doa_list=doa)
    assert set(multi) == set(plain) | {"peaks", "peak_power"}
    _same({k: multi[k] for k in plain}, plain)
    np.testing.assert_array_equal(multi["peaks"].cpu().numpy()[:, 0], plain["argmax"].cpu().numpy())
    pw = plain["power"].cpu().numpy()
    np.testing.assert_array_equal(multi["peak_power"].cpu().numpy()[:, 0], pw[np.arange(3), plain["argmax"].cpu().numpy()])
    m3 = bf.localize_batch(cfg2["bf_mat"], x, num_sources=3, doa_list=doa, min_separation=0.3)
    np.testing.assert_array_equal(m3["peaks"].cpu().numpy(), R.peaks(pw, doa, 3, 0.3)[0])
    with pytest.raises(ValueError, match="doa_list"):
        bf.localize_batch(cfg2["bf_mat"], x, num_sources=2)

    zb = golden("beamformer_c128_g449.npz")
    cbf = Beamformer(bf.geometry, 10e-3, [1000.0, 2000.0], fs=48_000)
    plain = cbf.localize_batch(zb["bf_mat"], x)
    multi = cbf.localize_batch(zb["bf_mat"], x, num_sources=1, doa_list=zb["doa_list"])
    _same({k: multi[k] for k in plain}, plain)
    np.testing.assert_array_equal(multi["peaks"].cpu().numpy()[:, 0], plain["argmax"].cpu().numpy())


def test_music_localize_batch_k1_is_argmax():
    from micloc.array_geometry import CenterCircularArray
    from micloc.music_beamformer import MUSIC
    from test_hip_music import test_signal

    z = np.load(os.path.join(GOLDEN, "music_apply_template.npz"))
    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    m = MUSIC(geometry=geo, freq_range=list(z["band"]), doa_list=np.linspace(-np.pi, np.pi, int(z["G"])), frame_duration=0.25, fs=48_000)
    x = np.stack([test_signal(s, 12_000, 7, geo.r_vec, geo.theta_vec) for s in range(4)])
    plain = m.localize_batch(x, 1, 0.0, 2048, want_spectrum=False)
    multi = m.localize_batch(x, 1, 0.0, 2048, want_spectrum=False, num_sources=1)
    _same({k: multi[k] for k in plain}, plain)
    np.testing.assert_array_equal(multi["peaks"].cpu().numpy()[:, 0], plain["argmax"].cpu().numpy())
    m2 = m.localize_batch(x, 1, 0.0, 2048, want_spectrum=False, num_sources=2)
    np.testing.assert_array_equal(m2["peaks"].cpu().numpy(), R.peaks(plain["power"].cpu().numpy(), m.doa_list, 2)[0])


def test_k_target_synthesis_is_bit_exact_with_gains(cfg2):
    from haghighatshoarmuir2024_amd.sweep import synthesize_targets_batch

    bf = _snn(cfg2)
    t = np.arange(0, 50e-3, 1 / 48_000)
    s = np.sin(2 * np.pi * 1700 * t) + 0.3 * np.sin(2 * np.pi * 2300 * t)
    rng = np.random.RandomState(2)
    for K, gains in ((2, [1.0, 1.0]), (3, [1.0, 0.5, 2.25]), (4, [0.3, 1.0, 0.7, 1.9])):
        doas = rng.rand(5, K) * 2 * np.pi
        time_in, x = synthesize_targets_batch(bf.geometry, 48_000, t, s, doas, gains)
        x = x.cpu().numpy()
        for b in range(5):
            t2, ref = R.synth_targets_host(bf.geometry, 48_000, t, s, doas[b], gains)
            np.testing.assert_array_equal(time_in, t2)
            np.testing.assert_array_equal(x[b], ref, err_msg=f"K={K} trial {b}")


@pytest.mark.parametrize("mode", ["parity", "throughput"])
def test_one_target_sweep_is_the_noisy_sweep(cfg2, mode):
    from haghighatshoarmuir2024_amd.sweep import multi_target_sweep, noisy_target_sweep

    bf = _snn(cfg2)
    kw = dict(snr_db_vec=[-10.0, 0.0, 10.0], num_sim=20, seed=4, mode=mode)
    a = noisy_target_sweep(bf, cfg2["bf_mat"], cfg2["doa_list"], **kw)
    b = multi_target_sweep(bf, cfg2["bf_mat"], cfg2["doa_list"], num_targets=1, **kw)
    np.testing.assert_array_equal(b["doa"][..., 0], a["doa"])
    np.testing.assert_array_equal(b["peaks"][..., 0], a["argmax"])
    np.testing.assert_array_equal(b["peak_power"][..., 0], a["pmax"])
    np.testing.assert_array_equal(b["err"][..., 0], a["err"])
    np.testing.assert_array_equal(b["mae_deg"], a["mae_deg"])


def test_two_target_sweep_peaks_follow_the_rule(cfg2):
    """num_targets = 2, parity mode: the device peaks are the restated rule's on the oracle pipeline's power of the same trials."""
    from haghighatshoarmuir2024_amd.sweep import device_localizer, multi_target_sweep
    from micloc.snn_beamformer import neuron_impulse_response
    from oracle import oracle as O

    bf = _snn(cfg2)
    W, doa = cfg2["bf_mat"], cfg2["doa_list"]
    sep = np.deg2rad(45) / 2
    dev = device_localizer(bf, W, num_sources=2, doa_list=doa, min_separation=sep)
    seen = []

    def loc(sig_batch, time_vec):
        seen.append((np.array(sig_batch), time_vec))
        return dev(sig_batch, time_vec)

    res = multi_target_sweep(bf, W, doa, num_targets=2, snr_db_vec=[20.0], num_sim=4, seed=1, localizer=loc)
    (sig, time_vec), = seen
    nir = neuron_impulse_response(time_vec, bf.tau_vec)
    b, a = bf.bandpass_filter
    pw, _ = O.snn_chain_batch(sig, bf.kernel, b, a, bf.spk_encoder.robust_width, True, nir, W)
    ri, rv = R.peaks(pw, doa, 2, sep)
    np.testing.assert_array_equal(res["peaks"][0], ri)
    np.testing.assert_allclose(res["peak_power"][0], rv, rtol=1e-10)
    assert res["resolved_rate"].shape == (1,) and res["err"].shape == (1, 4, 2)


@pytest.mark.parametrize("case", range(len(R.HAND_CASES)))
def test_hand_cases_on_the_device(case):
    """The rule's hand cases (plateaus, the closed seam, linear edges, NaN rows, thresholds, fewer than K) through find_doa_peaks."""
    import torch

    from micloc.utils import find_doa_peaks

    p, doa, K, sep, rel, kind, want = R.HAND_CASES[case]
    grid = None if kind is None else KINDS[kind]
    p = np.asarray(p, dtype=np.float64)
    i, v = find_doa_peaks(torch.from_numpy(p).cuda(), doa, K, min_separation=sep, rel_threshold=rel, grid=grid)
    assert list(i.cpu().numpy()) == want
    ri, rv = R.peaks(p, doa, K, sep, rel, kind)
    np.testing.assert_array_equal(v.cpu().numpy(), rv[0])


@pytest.mark.parametrize("name", ["snn_sin_1000", "snn_sin_2000", "snn_wideband_2000", "beamformer_sin_1000", "beamformer_sin_2000",
                                  "music_sin_1000", "music_sin_2000"])
def test_device_pipeline_on_the_reference_scenarios(name):
    """paper_plots/multiple_targets_*.py on the device: multi-target synthesis (synthesis.signal_multiple_targets), the golden bf_mat,
    localize_batch(num_sources=2): the reference's power to 1e-12 and its peak set (the two equal-gain peaks nearly tie)."""
    from haghighatshoarmuir2024_amd import synthesis
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer
    from micloc.music_beamformer import MUSIC
    from micloc.snn_beamformer import SNNBeamformer
    from test_multitarget_golden_cpu import scenario

    z = golden("multi_targets.npz")
    t, s, doa_ts, power_ts, band, tau_vec = scenario(z, name)
    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    doa, fs = z["doa_list"], int(z["fs"])
    if name.startswith("music"):
        # multiple_targets_music.py's copy of signal_multiple_targets delays with `time - delays` (the SNN and Beamformer scripts:
        # `time + delays`): the same generator with the delays negated, taken from the host (NumPy's cos)
        from haghighatshoarmuir2024_amd import runtime

        tpl = runtime.Template(t, s, fs)
        delays = -np.stack([geo.delays(float(d), normalized=False) for d in z["doa_targets"]])[None]  # [1, K, M]
        x = runtime.synth_targets(tpl, "signal_from_template", delays=delays)[0]
    else:
        x = synthesis.signal_multiple_targets(geo, t, s, doa_ts, power_ts)
    if name.startswith("snn"):
        bf = SNNBeamformer(geometry=geo, kernel_duration=10e-3, freq_range=band, tau_vec=tau_vec, bipolar_spikes=True, fs=fs)
        out = bf.localize_batch(z[name + "_bf_mat"], x[None], time_vec=t, num_sources=2, doa_list=doa)
    elif name.startswith("beamformer"):
        bf = Beamformer(geometry=geo, kernel_duration=10e-3, freq_range=list(band), fs=fs)
        out = bf.localize_batch(z[name + "_bf_mat"], x[None], num_sources=2, doa_list=doa)
    else:
        m = MUSIC(geometry=geo, freq_range=band, doa_list=doa, frame_duration=float(z["duration"]), fs=fs)
        out = m.localize_batch(x[None], 1, 0.0, 2048, want_spectrum=False, num_sources=2)
    pw = out["power"].cpu().numpy()[0]
    ref = z[name + "_power_bf"]
    assert float(np.max(np.abs(pw - ref)) / np.max(np.abs(ref))) <= 1e-12, name
    assert set(out["peaks"].cpu().numpy()[0]) == set(z[name + "_peaks"]), name
