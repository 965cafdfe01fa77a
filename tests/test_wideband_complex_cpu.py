"""CPU checks of the wideband complex Beamformer (tests/test_hip_wideband_complex.py has the device side): the C symbols and the status
codes that need no device, the reference fixture against the oracle composition (filterbank, complex chain per band, band sum),
`from_bands` against the reference's construction, the ValueErrors, the store key of the sweep and the `micloc.localization_demo` shim."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import csrc_build
from conftest import ROOT, golden

FS = 48_000
BANDS = [[1000.0, 1600.0], [1600.0, 2400.0]]


def test_header_declares_and_lib_binds_the_symbols():
    from haghighatshoarmuir2024_amd import _lib

    raw_text = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("micloc_beamformer_bands_workspace_bytes", "micloc_beamformer_pipeline_bands_f64", "micloc_beamformer_bands_bandpass_f64"):
        assert re.search(rf"\b{n}\s*\(", text), f"{n} is not declared in the header"
        assert n in _lib.SYMBOLS and hasattr(raw, n), n
    assert re.search(r"#define\s+MICLOC_ABI_VERSION\s+1\b", text)  # additive: the ABI version stays
    assert _lib.load().micloc_abi_version() == 1
    csrc = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "bands_complex.hip")).read())
    assert "atomic" not in code.lower() and "hipStreamSynchronize" not in code and "hipDeviceSynchronize" not in code and "hipMalloc" not in code
    assert "bands_complex.hip" in csrc_build.built_sources()


def test_the_df2t_step_and_the_row_tile_pipeline_are_written_once():
    """csrc/bandpass_rows.h holds the one DF2T step outside the encoder files (rzcc.hip and rzcc_sweep.hip are pinned by profile rounds and
    keep theirs) and the tile pipeline of the complex chains' band-pass kernels, barrier included; what the source checks above ask of
    bands_complex.hip and stream_bands_complex.hip holds for the header their kernels now come from."""
    import glob

    csrc = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
    strip = lambda path: re.sub(r"//[^\n]*", "", open(path).read())  # noqa: E731
    files = [p for p in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
             if os.path.basename(p) not in ("rzcc.hip", "rzcc_sweep.hip")]
    assert len(files) > 20 and os.path.join(csrc, "bandpass_rows.h") in files
    hits = {os.path.basename(p): strip(p).count("z[N - 2] =") for p in files}
    assert {k: v for k, v in hits.items() if v} == {"bandpass_rows.h": 1}, hits
    for name in ("bands_complex.hip", "stream_bands_complex.hip"):
        assert strip(os.path.join(csrc, name)).count("__syncthreads") == 0, name
    code = strip(os.path.join(csrc, "bandpass_rows.h"))
    assert "__syncthreads" in code
    assert "atomic" not in code.lower() and "hipStreamSynchronize" not in code and "hipDeviceSynchronize" not in code and "hipMalloc" not in code
    assert {"bands_complex.o", "stream_bands_complex.o"} <= csrc_build.rebuilt_after_edit("bandpass_rows.h")  # an edit to the header rebuilds its objects


def test_invalid_arguments_before_any_launch():
    """MICLOC_ERR_INVALID of the new entries, returned before any device call (the codes that need a plan -- NOT_SET, SHAPE, WORKSPACE --
    are in tests/test_hip_wideband_complex.py::test_status_codes)."""
    from haghighatshoarmuir2024_amd import _lib

    lib = _lib.load()
    INV = _lib.MICLOC_ERR_INVALID
    one = ctypes.c_void_p(256)
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)  # noqa: E731
    b = np.array([[0.1, 0.0, -0.1], [0.2, 0.0, -0.2]])
    a = np.array([[1.0, -1.5, 0.8], [1.0, -1.2, 0.7]])
    a_zero = a.copy()
    a_zero[1, 0] = 0.0
    plans = (ctypes.c_void_p * 2)(None, None)
    pb = lib.micloc_beamformer_pipeline_bands_f64
    args = dict(plans=plans, F=2, b=dp(b), a=dp(a), n=3, x=one, B=1, T=100, window=0, hop=0, bp=None, power=one, argmax=one, ws=one, nbytes=1 << 20)

    def call(**over):
        k = dict(args, **over)
        return pb(k["plans"], k["F"], k["b"], k["a"], k["n"], k["x"], k["B"], k["T"], k["window"], k["hop"], k["bp"], k["power"], k["argmax"], k["ws"],
                  k["nbytes"], None)

    assert call() == INV  # NULL plans in the array
    for over in (dict(plans=None), dict(F=0), dict(F=17), dict(b=None), dict(a=None), dict(n=0), dict(n=10), dict(a=dp(a_zero)), dict(x=None),
                 dict(power=None, argmax=None), dict(B=0), dict(B=65536), dict(B=40000), dict(T=0), dict(window=-1), dict(hop=-1)):
        assert call(**over) == INV, over
    assert lib.micloc_beamformer_bands_workspace_bytes(None, 2, 1, 100, 0, 0) == 0
    assert lib.micloc_beamformer_bands_workspace_bytes(plans, 2, 1, 100, 0, 0) == 0
    bpf = lib.micloc_beamformer_bands_bandpass_f64
    assert bpf(plans, 2, one, 1, 100, one, one, 104, 1, 1, None) == INV
    for over in ((None, 2, one, 1, 100, one, one), (plans, 0, one, 1, 100, one, one), (plans, 17, one, 1, 100, one, one), (plans, 2, None, 1, 100, one, one),
                 (plans, 2, one, 0, 100, one, one), (plans, 2, one, 1, 0, one, one), (plans, 2, one, 1, 100, None, one), (plans, 2, one, 1, 100, one, None)):
        assert bpf(*over, 104, 1, 1, None) == INV, over


def test_fixture_is_reproduced_by_the_oracle_composition():
    """tests/golden/wideband_complex_packs.npz (the reference's order-2 ButterworthFilterbank + three Beamformers on the three packs of
    wideband_packs.npz): the oracle's filter, its complex chain per band and a NumPy band sum give the reference's per-band and summed
    power to rtol 1e-10 (the project's power contract; relative, because these powers are about 1e13) and its arg-max."""
    from scipy.signal import butter

    from oracle import oracle as O

    z, c = golden("wideband_packs.npz"), golden("wideband_complex_packs.npz")
    assert c["bf_mats"].shape == (3, 7, 112) and c["bf_mats"].dtype == np.complex128 and int(c["filterbank_order"]) == 2
    assert sorted(c.files) == ["band_power", "bf_mats", "doa_index", "filterbank_order", "power_grid"]  # the packs are not stored again
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "wideband_complex_packs.npz")) < 100_000
    assert c["doa_index"].tolist() == [37, 97, 48] and np.argmax(c["band_power"][2], axis=1).tolist() == [11, 76, 48]
    fs = int(z["fs"])
    ker = O.stht_kernel(fs, float(z["kernel_duration"]))
    packs = z["packs16"].astype(np.int32) << int(z["shift"])
    for p, pack in enumerate(packs):
        data = pack[:, :-1].astype(np.float64)
        rows = []
        for fr, W in zip(z["freq_bands"], c["bf_mats"]):
            b2, a2 = butter(2, fr, btype="bandpass", output="ba", fs=fs)
            rows.append(O.beamformer_chain(O.iir(b2, a2, data), ker, *O.bandpass(fs, fr), W, want_y=False)["power"])
        band = np.stack(rows)
        np.testing.assert_allclose(band, c["band_power"][p], rtol=1e-10, atol=0)
        total = band[0]
        for row in band[1:]:
            total = total + row
        np.testing.assert_allclose(total, c["power_grid"][p], rtol=1e-10, atol=0)
        assert int(np.argmax(total)) == int(c["doa_index"][p])
        top = np.sort(c["power_grid"][p])[-2:]
        assert top[1] - top[0] > 1e-6 * top[1]  # the arg-max is not a rounding matter


def _geo(M=7):
    from micloc.array_geometry import CenterCircularArray

    return CenterCircularArray(4.5e-2, M)


def _loc(bands, G=33, seed=5):
    from micloc.beamformer import Beamformer
    from micloc.filterbank import ButterworthFilterbank
    from micloc.wideband import WidebandBeamformerLocalizer

    beamfs = [Beamformer(_geo(), 10e-3, fr, fs=FS) for fr in bands]
    rng = np.random.RandomState(seed)
    return WidebandBeamformerLocalizer(beamfs, [rng.randn(7, G) + 1j * rng.randn(7, G) for _ in bands], ButterworthFilterbank(freq_bands=bands, order=2, fs=FS))


def test_from_bands_builds_what_the_reference_demo_builds(monkeypatch):
    """micloc/localization_demo.py:43-89: per band a Beamformer on the band, designed on sin(2 pi f_mid t) over the recording duration,
    and the order-2 Butterworth filterbank -- from_bands and Demo alike (the design itself needs the device: it is replaced here)."""
    from scipy.signal import butter

    from haghighatshoarmuir2024_amd.beamformer import Beamformer
    from haghighatshoarmuir2024_amd.localization_demo import Demo
    from haghighatshoarmuir2024_amd.wideband import WidebandBeamformerLocalizer

    seen = []

    def design(self, template, doa_list, **kw):
        seen.append((self, template, doa_list))
        rng = np.random.RandomState(len(seen))
        return rng.randn(len(self.geometry), len(doa_list)) + 1j * rng.randn(len(self.geometry), len(doa_list)), []

    monkeypatch.setattr(Beamformer, "design_from_template", design)
    doa_list = np.linspace(-np.pi, np.pi, 33)
    bands = BANDS + [[2400.0, 3400.0]]
    for build in (lambda: WidebandBeamformerLocalizer.from_bands(_geo(), bands, doa_list, recording_duration=0.05, kernel_duration=10e-3, fs=FS),
                  lambda: Demo(_geo(), bands, doa_list, recording_duration=0.05, kernel_duration=10e-3, fs=FS)):
        del seen[:]
        obj = build()
        assert len(obj.beamfs) == 3 and len(seen) == 3
        assert obj.filterbank.order == 2
        for f, fr in enumerate(bands):
            beamf, (t, s), doas = seen[f]
            assert beamf is obj.beamfs[f] and type(beamf) is Beamformer and beamf.freq_range.tolist() == fr and beamf.kernel_duration == 10e-3
            np.testing.assert_array_equal(t, np.arange(0, 0.05, step=1 / FS))
            np.testing.assert_array_equal(s, np.sin(2 * np.pi * np.mean(fr) * t))
            np.testing.assert_array_equal(doas, doa_list)
            b, a = butter(2, fr, btype="bandpass", output="ba", fs=FS)
            np.testing.assert_array_equal(obj.filterbank.ba_list[f][0], b)
            np.testing.assert_array_equal(obj.filterbank.ba_list[f][1], a)
            assert np.iscomplexobj(obj.bf_mats[f]) and obj.bf_mats[f].shape == (7, 33)
        np.testing.assert_array_equal(obj.doa_list, doa_list)
    demo = obj
    assert (demo.recording_duration, demo.kernel_duration, demo.fs) == (0.05, 10e-3, FS)
    assert not hasattr(demo, "streaming_localizer")  # the wideband complex stream is not built
    loc = demo.localizer()
    assert type(loc) is WidebandBeamformerLocalizer and loc.beamfs == demo.beamfs and loc.filterbank is demo.filterbank
    one_band = WidebandBeamformerLocalizer.from_bands(_geo(), [1600.0, 2400.0], doa_list, recording_duration=0.05, kernel_duration=10e-3, fs=FS)
    assert len(one_band.beamfs) == 1  # a single band given as one pair, as in the reference


def test_localizer_rejects_mismatched_bands():
    from micloc.beamformer import Beamformer
    from micloc.filterbank import ButterworthFilterbank
    from micloc.wideband import WidebandBeamformerLocalizer

    loc = _loc(BANDS)
    fb = loc.filterbank
    with pytest.raises(ValueError):  # G
        WidebandBeamformerLocalizer(loc.beamfs, [loc.bf_mats[0], loc.bf_mats[1][:, :-1]], fb)
    other = Beamformer(_geo(5), 10e-3, [1600.0, 2400.0], fs=FS)
    with pytest.raises(ValueError):  # M
        WidebandBeamformerLocalizer([loc.beamfs[0], other], [loc.bf_mats[0], np.zeros((5, 33), dtype=complex)], fb)
    bands17 = [[1000.0 + 100 * i, 1100.0 + 100 * i] for i in range(17)]
    with pytest.raises(ValueError):  # 17 bands
        WidebandBeamformerLocalizer([loc.beamfs[0]] * 17, [loc.bf_mats[0]] * 17, ButterworthFilterbank(freq_bands=bands17, order=2, fs=FS))
    with pytest.raises(ValueError):  # sections
        WidebandBeamformerLocalizer(loc.beamfs, loc.bf_mats, ButterworthFilterbank(freq_bands=BANDS[:1], order=2, fs=FS))
    with pytest.raises(ValueError):  # matrices
        WidebandBeamformerLocalizer(loc.beamfs, loc.bf_mats[:1], fb)
    # a bf_mat that is not complex [M, G]: a real matrix (the SNN form's [2M, G] too), a complex one with 2M rows, a vector
    for bad in (np.zeros((7, 33)), np.zeros((14, 33)), np.zeros((14, 33), dtype=complex), np.zeros(7, dtype=complex)):
        with pytest.raises(ValueError):
            WidebandBeamformerLocalizer(loc.beamfs, [loc.bf_mats[0], bad], fb)
    with pytest.raises(ValueError):  # channels of the input
        loc.localize_batch(np.zeros((1, 64, 6)))


def test_store_key_separates_the_methods(tmp_path):
    """SNN and complex shards of the wideband sweep never mix: the store key carries the method, the band edges, the filterbank's
    coefficients and every band's bf_mat hash (a complex matrix with its imaginary part)."""
    import json

    from haghighatshoarmuir2024_amd.sweep import _wideband_store_key, wideband_speech_sweep
    from micloc.snn_beamformer import SNNBeamformer
    from micloc.wideband import WidebandSNNLocalizer

    G = 33
    doa_list = np.linspace(-np.pi, np.pi, G)
    t = np.arange(0, 10e-3, 1 / FS)
    src = (t, np.sin(2 * np.pi * 1500 * t))

    def fake(calls):
        def run(sig_batch, time_vec):
            calls.append(len(sig_batch))
            s = np.asarray(sig_batch)
            return (np.abs(s).sum(axis=(1, 2)) * 1000).astype(np.int64) % G, np.abs(s).max(axis=(1, 2))

        return run

    def run(loc):
        calls = []
        res = wideband_speech_sweep(loc, doa_list, src, snr_db_vec=[5.0], num_sim=2, seed=3, localizer=fake(calls), out_dir=tmp_path)
        return res, calls

    cpx = _loc(BANDS)
    ref, calls = run(cpx)
    assert calls == [2] and len(os.listdir(tmp_path)) == 1
    again, calls = run(_loc(BANDS))
    assert calls == [] and again["persistence"]["trials_loaded"] == 2  # the same localizer: everything is found
    np.testing.assert_array_equal(again["argmax"], ref["argmax"])
    (sub,) = os.listdir(tmp_path)
    meta = json.load(open(tmp_path / sub / "meta.json"))
    assert meta["method"] == "WidebandBeamformerLocalizer" and meta["num_bands"] == 2
    for k in ("band_edges", "fb_b", "fb_a", "band0_bf_mat_sha256", "band1_bf_mat_sha256", "band0_iir_b", "band0_kernel"):
        assert k in meta, k
    # the SNN localizer over the same bands, the same filterbank object and the real parts of the same matrices
    tau = 1 / (2 * np.pi * 2000)
    snn = WidebandSNNLocalizer([SNNBeamformer(_geo(), 10e-3, fr, [tau, tau], bipolar_spikes=True, fs=FS) for fr in BANDS],
                               [np.vstack([W.real, W.imag]) for W in cpx.bf_mats], cpx.filterbank)
    n = 1
    imag_only = _loc(BANDS)
    imag_only.bf_mats[1] = imag_only.bf_mats[1] + 1j  # only the imaginary part differs
    for loc in (snn, _loc([[1000.0, 1600.0], [1600.0, 2500.0]]), _loc(BANDS[:1]), imag_only):
        _, calls = run(loc)
        n += 1
        assert calls == [2] and len(os.listdir(tmp_path)) == n
    assert _wideband_store_key(snn)["method"] == "WidebandSNNLocalizer"
    with warnings.catch_warnings():  # hashing a complex matrix discards nothing (no ComplexWarning)
        warnings.simplefilter("error")
        _wideband_store_key(cpx)


def test_sweep_cli_takes_the_method(monkeypatch, tmp_path):
    """`--sweep wideband-speech --method beamformer` builds WidebandBeamformerLocalizer.from_bands; --method snn (the default) the SNN form."""
    from haghighatshoarmuir2024_amd import sweep, wideband

    built = []

    class Stop(Exception):
        pass

    def from_bands_c(geometry, freq_bands, doa_list, recording_duration, kernel_duration, fs, device=None):
        built.append(("beamformer", freq_bands, recording_duration, kernel_duration, fs))
        raise Stop

    def from_bands_s(geometry, freq_bands, doa_list, recording_duration, kernel_duration, bipolar_spikes, fs, device=None):
        built.append(("snn", freq_bands, recording_duration, kernel_duration, fs))
        raise Stop

    monkeypatch.setattr(wideband.WidebandBeamformerLocalizer, "from_bands", staticmethod(from_bands_c))
    monkeypatch.setattr(wideband.WidebandSNNLocalizer, "from_bands", staticmethod(from_bands_s))
    npz = tmp_path / "pcm.npz"
    np.savez(npz, pcm16=(np.sin(np.arange(1600) / 7.0) * 1000).astype(np.int16), rate=np.int64(16000))
    for method, want in ((["--method", "beamformer"], "beamformer"), (["--method", "snn"], "snn"), ([], "snn")):
        with pytest.raises(Stop):
            sweep.main(["--sweep", "wideband-speech", "--pcm-npz", str(npz), "--bands", "1000:1600,1600:2400", "--grid", "33"] + method)
        assert built[-1] == (want, [[1000.0, 1600.0], [1600.0, 2400.0]], 0.25, 10.0e-3, 48_000)
    with pytest.raises(SystemExit):
        sweep.main(["--sweep", "wideband-speech", "--pcm-npz", str(npz), "--method", "music"])


def test_micloc_shims():
    import micloc.localization_demo
    import micloc.wideband
    from haghighatshoarmuir2024_amd import localization_demo, wideband

    assert micloc.localization_demo.Demo is localization_demo.Demo
    assert micloc.wideband.WidebandBeamformerLocalizer is wideband.WidebandBeamformerLocalizer
    assert micloc.wideband.WidebandSNNLocalizer is wideband.WidebandSNNLocalizer
    for name in ("power_grid", "process_frame", "process_frames", "localizer", "run"):
        assert callable(getattr(localization_demo.Demo, name))
