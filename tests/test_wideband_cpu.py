"""CPU checks of the wideband localizer (tests/test_hip_wideband.py has the device side): the C symbols and the status codes that need
no device, the multi-band reference fixture against the oracle composition (filterbank, chain per band, band sum), the --bands option
and the store key of the wideband sweep."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import csrc_build
from conftest import ROOT, golden

FS = 48_000


def test_header_declares_and_lib_binds_the_wideband_symbols():
    from haghighatshoarmuir2024_amd import _lib

    raw_text = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    names = ("micloc_filterbank_f64", "micloc_band_sum_f64", "micloc_snn_bands_workspace_bytes", "micloc_snn_pipeline_bands_f64")
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert re.search(rf"\b{n}\s*\(", text), f"{n} is not declared in the header"
        assert n in _lib.SYMBOLS and hasattr(raw, n), n
    assert re.search(r"#define\s+MICLOC_MAX_BANDS\s+16\b", text) and _lib.MICLOC_MAX_BANDS == 16
    assert re.search(r"#define\s+MICLOC_ABI_VERSION\s+1\b", text)  # additive: the ABI version stays
    assert _lib.load().micloc_abi_version() == 1
    csrc = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
    src = open(os.path.join(csrc, "filterbank.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower() and "hipStreamSynchronize" not in code and "hipDeviceSynchronize" not in code and "hipMalloc" not in code
    assert "filterbank.hip" in csrc_build.built_sources()


def test_status_codes_before_any_launch():
    """MICLOC_ERR_INVALID of every new entry, returned before any device call (the codes that need a plan -- NOT_SET, SHAPE, WORKSPACE --
    are in tests/test_hip_wideband.py::test_pipeline_status_codes)."""
    from haghighatshoarmuir2024_amd import _lib

    lib = _lib.load()
    INV = _lib.MICLOC_ERR_INVALID
    one = ctypes.c_void_p(256)
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)  # noqa: E731
    b = np.array([[0.1, 0.0, -0.1], [0.2, 0.0, -0.2]])
    a = np.array([[1.0, -1.5, 0.8], [1.0, -1.2, 0.7]])
    a_zero = a.copy()
    a_zero[1, 0] = 0.0
    fb = lib.micloc_filterbank_f64
    assert fb(None, dp(a), 2, 3, one, 1, 10, 7, one, None) == INV
    assert fb(dp(b), None, 2, 3, one, 1, 10, 7, one, None) == INV
    assert fb(dp(b), dp(a), 0, 3, one, 1, 10, 7, one, None) == INV
    assert fb(dp(b), dp(a), 17, 3, one, 1, 10, 7, one, None) == INV
    assert fb(dp(b), dp(a), 2, 0, one, 1, 10, 7, one, None) == INV
    assert fb(dp(b), dp(a), 2, 10, one, 1, 10, 7, one, None) == INV
    assert fb(dp(b), dp(a_zero), 2, 3, one, 1, 10, 7, one, None) == INV
    assert fb(dp(b), dp(a), 2, 3, None, 1, 10, 7, one, None) == INV
    assert fb(dp(b), dp(a), 2, 3, one, 1, 10, 7, None, None) == INV
    for B, T, M in ((0, 10, 7), (1, 0, 7), (1, 10, 0)):
        assert fb(dp(b), dp(a), 2, 3, one, B, T, M, one, None) == INV
    bs = lib.micloc_band_sum_f64
    assert bs(None, 2, 1, 8, one, one, None) == INV
    assert bs(one, 2, 1, 8, None, None, None) == INV
    for F, R, G in ((0, 1, 8), (17, 1, 8), (2, 0, 8), (2, 1, 0)):
        assert bs(one, F, R, G, one, one, None) == INV
    plans = (ctypes.c_void_p * 2)(None, None)
    pb = lib.micloc_snn_pipeline_bands_f64
    args = dict(plans=plans, F=2, b=dp(b), a=dp(a), n=3, x=one, B=1, T=100, window=0, hop=0, bp=None, power=one, argmax=one, ws=one, nbytes=1 << 20)

    def call(**over):
        k = dict(args, **over)
        return pb(k["plans"], k["F"], k["b"], k["a"], k["n"], k["x"], k["B"], k["T"], k["window"], k["hop"], k["bp"], k["power"], k["argmax"], k["ws"],
                  k["nbytes"], None)

    assert call() == INV  # NULL plans in the array
    for over in (dict(plans=None), dict(F=0), dict(F=17), dict(b=None), dict(a=None), dict(n=0), dict(n=10), dict(a=dp(a_zero)), dict(x=None),
                 dict(power=None, argmax=None), dict(B=0), dict(B=65536), dict(T=0), dict(window=-1), dict(hop=-1)):
        assert call(**over) == INV, over
    assert lib.micloc_snn_bands_workspace_bytes(None, 2, 1, 100, 0, 0) == 0
    assert lib.micloc_snn_bands_workspace_bytes(plans, 2, 1, 100, 0, 0) == 0


def _oracle_bands(z, data):
    from scipy.signal import butter

    from oracle import oracle as O

    T = data.shape[0]
    fs = int(z["fs"])
    rows = []
    for fr, W in zip(z["freq_bands"], z["bf_mats"]):
        b1, a1 = butter(1, fr, btype="bandpass", analog=False, output="ba", fs=fs)
        filt = O.iir(b1, a1, data)
        bb, aa = O.bandpass(fs, fr)
        tau = 1 / (2 * np.pi * np.mean(fr))
        nir = O.neuron_kernel(np.arange(T) / fs, [tau, tau])
        rows.append(O.snn_chain(filt, O.stht_kernel(fs, float(z["kernel_duration"])), bb, aa, O.robust_width(fs, fr[1]), True, nir, W,
                                want=("power",))["power"])
    return np.stack(rows)


def test_fixture_is_reproduced_by_the_oracle_composition():
    """tests/golden/wideband_packs.npz (the reference's ButterworthFilterbank + three SNNBeamformers on three packs): the oracle's
    filterbank, its chain per band and a NumPy band sum give the reference's per-band and summed power to 1e-10 and its arg-max."""
    z = golden("wideband_packs.npz")
    assert z["freq_bands"].tolist() == [[1000, 1600], [1600, 2400], [2400, 3400]] and z["bf_mats"].shape == (3, 14, 112)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "wideband_packs.npz")) < 500_000
    packs = z["packs16"].astype(np.int32) << int(z["shift"])
    assert packs.shape == (3, 4800, 8)
    for p, pack in enumerate(packs):
        band = _oracle_bands(z, pack[:, :-1].astype(np.float64))
        np.testing.assert_allclose(band, z["band_power"][p], rtol=1e-10, atol=0)
        total = band[0]
        for row in band[1:]:
            total = total + row
        np.testing.assert_allclose(total, z["power_grid"][p], rtol=1e-10, atol=0)
        assert int(np.argmax(total)) == int(z["doa_index"][p])
        top = np.sort(z["power_grid"][p])[-2:]
        assert top[1] - top[0] > 1e-6 * top[1]  # the arg-max is not a rounding matter


def test_bands_option_parses():
    from haghighatshoarmuir2024_amd.sweep import parse_bands

    assert parse_bands("1000:1600,1600:2400,2400:3400") == [[1000.0, 1600.0], [1600.0, 2400.0], [2400.0, 3400.0]]
    assert parse_bands("500.5:900") == [[500.5, 900.0]]
    for bad in ("", "1000", "1000:900", "1000-1600", "a:b", ",".join(["100:200"] * 17)):
        with pytest.raises(ValueError):
            parse_bands(bad)


def _loc(bands, G=33):
    from micloc.array_geometry import CenterCircularArray
    from micloc.filterbank import ButterworthFilterbank
    from micloc.snn_beamformer import SNNBeamformer
    from micloc.wideband import WidebandSNNLocalizer

    geo = CenterCircularArray(4.5e-2, 7)
    beamfs = []
    for fr in bands:
        tau = 1 / (2 * np.pi * np.mean(fr))
        beamfs.append(SNNBeamformer(geo, 10e-3, fr, [tau, tau], bipolar_spikes=True, fs=FS))
    rng = np.random.RandomState(5)
    return WidebandSNNLocalizer(beamfs, [rng.randn(14, G) for _ in bands], ButterworthFilterbank(freq_bands=bands, order=1, fs=FS))


def _fake_localizer(G, calls):
    def run(sig_batch, time_vec):
        calls.append(len(sig_batch))
        s = np.asarray(sig_batch)
        return (np.abs(s).sum(axis=(1, 2)) * 1000).astype(np.int64) % G, np.abs(s).max(axis=(1, 2))

    return run


def test_store_key_changes_with_the_band_set(tmp_path):
    from haghighatshoarmuir2024_amd.sweep import wideband_speech_sweep

    G = 33
    doa_list = np.linspace(-np.pi, np.pi, G)
    t = np.arange(0, 10e-3, 1 / FS)
    src = (t, np.sin(2 * np.pi * 1500 * t))
    bands = [[1000.0, 1600.0], [1600.0, 2400.0]]

    def run(loc):
        calls = []
        res = wideband_speech_sweep(loc, doa_list, src, snr_db_vec=[5.0], num_sim=2, seed=3, localizer=_fake_localizer(G, calls), out_dir=tmp_path)
        return res, calls

    ref, calls = run(_loc(bands))
    assert calls == [2] and len(os.listdir(tmp_path)) == 1
    again, calls = run(_loc(bands))
    assert calls == [] and again["persistence"]["trials_loaded"] == 2  # the same band set: everything is found
    for k in ("argmax", "pmax", "err", "doa"):
        np.testing.assert_array_equal(again[k], ref[k])
    (sub,) = os.listdir(tmp_path)
    meta = json.load(open(tmp_path / sub / "meta.json"))
    assert sub.startswith("wideband-speech-") and meta["num_bands"] == 2
    for k in ("band_edges", "fb_b", "fb_a", "band0_tau_vec", "band1_tau_vec", "band0_bf_mat_sha256", "band1_bf_mat_sha256", "band0_iir_b"):
        assert k in meta, k
    n = 1
    other_mat = _loc(bands)
    other_mat.bf_mats[1] = other_mat.bf_mats[1] + 1.0
    for loc in (_loc([[1000.0, 1600.0], [1600.0, 2500.0]]), _loc([[1000.0, 1600.0]]), _loc(bands + [[2400.0, 3400.0]]), other_mat):
        _, calls = run(loc)
        n += 1
        assert calls == [2] and len(os.listdir(tmp_path)) == n


def test_localizer_rejects_mismatched_bands():
    from micloc.array_geometry import CenterCircularArray
    from micloc.filterbank import ButterworthFilterbank
    from micloc.snn_beamformer import SNNBeamformer
    from micloc.wideband import WidebandSNNLocalizer

    loc = _loc([[1000.0, 1600.0], [1600.0, 2400.0]])
    fb = loc.filterbank
    with pytest.raises(ValueError):  # G
        WidebandSNNLocalizer(loc.beamfs, [loc.bf_mats[0], loc.bf_mats[1][:, :-1]], fb)
    tau = 1 / (2 * np.pi * 2000)
    other = SNNBeamformer(CenterCircularArray(4.5e-2, 5), 10e-3, [1600.0, 2400.0], [tau, tau], bipolar_spikes=True, fs=FS)
    with pytest.raises(ValueError):  # M
        WidebandSNNLocalizer([loc.beamfs[0], other], [loc.bf_mats[0], np.zeros((10, 33))], fb)
    bands17 = [[1000.0 + 100 * i, 1100.0 + 100 * i] for i in range(17)]
    with pytest.raises(ValueError):  # 17 bands
        WidebandSNNLocalizer([loc.beamfs[0]] * 17, [loc.bf_mats[0]] * 17, ButterworthFilterbank(freq_bands=bands17, order=1, fs=FS))
