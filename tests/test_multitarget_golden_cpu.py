"""The multi-target goldens of the reference (tests/golden/multi_targets.npz, from paper_plots/multiple_targets_{snn,beamformer,music}.py
by tests/golden/make_golden_multitarget.py) against the C oracle and the restated peak rule, and the rule's hand cases (CPU)."""
import numpy as np
import pytest

import multisource_ref as R
from conftest import golden


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def scenario(z, name):
    """(time_temp, sig_temp, doa_ts, power_ts, freq_range, tau_vec) of a golden case: the scripts' template and fixed targets."""
    from scipy.signal import butter, lfilter

    fs, T = int(z["fs"]), len(np.arange(0, float(z["duration"]), step=1 / int(z["fs"])))
    t = np.arange(0, float(z["duration"]), step=1 / fs)
    method, kind, f = name.split("_")
    f = float(f)
    if kind == "sin":
        s = np.sin(2 * np.pi * f * t)
        band = np.array([f / 2, 2 * f])
    else:
        band = np.asarray([f - float(z["bandwidth"]) / 2, f + float(z["bandwidth"]) / 2])
        b, a = butter(2, band, btype="pass", analog=False, output="ba", fs=fs)
        np.random.seed(int(z["wideband_seed"]))
        s = lfilter(b, a, np.random.randn(T))
    doa_ts = np.ones((T, 1)) * z["doa_targets"].reshape(1, -1)
    power_ts = np.ones((T, 1)) * z["power_targets"].reshape(1, -1)
    tau = 1 / (2 * np.pi * f)
    return t, s, doa_ts, power_ts, band, np.asarray([tau, tau])


CASES = ["snn_sin_1000", "snn_sin_2000", "snn_wideband_2000", "beamformer_sin_1000", "beamformer_sin_2000"]
MUSIC_CASES = ["music_sin_1000", "music_sin_2000"]


def test_golden_file_is_small_and_complete():
    z = golden("multi_targets.npz")
    for c in CASES + MUSIC_CASES:
        assert z[c + "_power_bf"].shape == (225,) and z[c + "_peaks"].shape == (2,)
    assert z["snn_sin_2000_bf_mat"].shape == (14, 225) and z["beamformer_sin_2000_bf_mat"].shape == (7, 225)
    assert np.iscomplexobj(z["beamformer_sin_2000_bf_mat"])


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference_power_and_peaks(name):
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer
    from micloc.snn_beamformer import SNNBeamformer, neuron_impulse_response
    from oracle import oracle as O

    O.build()
    z = golden("multi_targets.npz")
    t, s, doa_ts, power_ts, band, tau_vec = scenario(z, name)
    x = O.signal_multiple_targets(z["r_vec"], z["theta_vec"], t, s, doa_ts, power_ts)
    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    W = z[name + "_bf_mat"]
    if name.startswith("snn"):
        bf = SNNBeamformer(geometry=geo, kernel_duration=10e-3, freq_range=band, tau_vec=tau_vec, bipolar_spikes=True, fs=int(z["fs"]))
        b, a = bf.bandpass_filter
        pw = O.snn_chain(x, bf.kernel, b, a, bf.spk_encoder.robust_width, True, neuron_impulse_response(t, tau_vec), W, want=("power",))["power"]
    else:
        bf = Beamformer(geometry=geo, kernel_duration=10e-3, freq_range=list(band), fs=int(z["fs"]))
        b, a = bf.bandpass_filter
        pw = O.beamformer_chain(x, bf.kernel, b, a, W, want_y=False)["power"]
    assert _rel(pw, z[name + "_power_bf"]) <= 1e-10, name
    # the restated rule picks the recorded peaks on the reference's power, and the same set on the oracle's
    np.testing.assert_array_equal(R.peaks(z[name + "_power_bf"], z["doa_list"], 2)[0][0], z[name + "_peaks"])
    assert set(R.peaks(pw, z["doa_list"], 2)[0][0]) == set(z[name + "_peaks"])


@pytest.mark.parametrize("name", MUSIC_CASES)
def test_music_golden_peaks_follow_the_rule(name):
    # (the MUSIC script synthesises with `time - delays`; its power is checked on the device, tests/test_hip_multisource.py)
    z = golden("multi_targets.npz")
    np.testing.assert_array_equal(R.peaks(z[name + "_power_bf"], z["doa_list"], 2)[0][0], z[name + "_peaks"])


@pytest.mark.parametrize("case", range(len(R.HAND_CASES)))
def test_hand_cases_of_the_restatement(case):
    p, doa, K, sep, rel, kind, want = R.HAND_CASES[case]
    assert list(R.peaks(np.asarray(p, dtype=np.float64), doa, K, sep, rel, kind)[0][0]) == want


def test_committed_kernel_profile_belongs_to_the_kernel_in_the_tree():
    """profiles/multisource/: the doa_peaks_kernel time quoted in DESIGN.md 4.10 was taken on the sources of the tree."""
    import hashlib
    import json
    import os

    from conftest import ROOT

    rec = json.load(open(os.path.join(ROOT, "profiles", "multisource", "RECORD.json")))
    e = rec["kernel_stats_1100x449_k2.csv"]
    assert os.path.isfile(os.path.join(ROOT, "profiles", "multisource", "kernel_stats_1100x449_k2.csv"))
    for rel, h in e["sources_sha256"].items():
        assert hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() == h, rel
    assert e["box"]["gcn_arch"].startswith("gfx950")
