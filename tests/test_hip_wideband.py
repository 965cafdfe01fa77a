"""Device tests of the wideband localizer: the filterbank kernel against micloc_lfilter_f64 and the oracle, the band-sum kernel against
a sequential NumPy sum, WidebandSNNLocalizer.localize_batch against Demo.power_grid (the route it replaces) and the reference's
multi-band fixture, windows and multi-source read-outs, graph replay of the C entry, and the wideband speech sweep."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

FS = 48_000
B_SET, M_SET, T_SET = (1, 3, 10), (1, 7, 16), (1, 2, 15, 16, 17, 63, 64, 65, 1001)
F_SET = (1, 2, 3, 5, 16)


def _sections(kind, F):
    """F filter sections of one kind: Butterworth band-passes of order 1, 2, 4 (n = 3, 5, 9) on F different bands, or random stable
    filters of n = 4 without a zero coefficient (poles of modulus <= 0.9, a[0] != 1: the division by a[0] is part of the contract)."""
    from scipy.signal import butter

    if kind == "random":
        rng = np.random.RandomState(100 + F)
        out = []
        for _ in range(F):
            r, th, p = 0.3 + 0.6 * rng.rand(), np.pi * rng.rand(), 0.9 * (2 * rng.rand() - 1)
            a = np.convolve([1.0, -2 * r * np.cos(th), r * r], [1.0, -p]) * (1.5 + rng.rand())
            b = rng.randn(4) + 0.1
            assert np.all(a != 0) and np.all(b != 0)
            out.append((b, a))
        return out
    order = int(kind)
    return [butter(order, [300.0 + 1200 * f, 1200.0 + 1200 * f], btype="bandpass", output="ba", fs=FS) for f in range(F)]


_X = {}


def _x_full():
    """The one input of every filterbank case [10, 1001, 16]: the smaller shapes are its leading slices (a causal filter per column:
    the reference of a slice is the slice of the reference)."""
    if "x" not in _X:
        _X["x"] = np.random.RandomState(7).randn(max(B_SET), max(T_SET), max(M_SET))
    return _X["x"]


def _oracle_full(kind, F):
    from oracle import oracle as O

    key = (kind, F)
    if key not in _X:
        x = _x_full()
        _X[key] = np.stack([np.stack([O.iir(b, a, x[i]) for i in range(len(x))]) for b, a in _sections(kind, F)])
    return _X[key]


@pytest.mark.parametrize("F", F_SET)
@pytest.mark.parametrize("kind", ["1", "2", "4", "random"])
def test_filterbank_equals_lfilter_and_oracle(kind, F):
    """micloc_filterbank_f64 == micloc_lfilter_f64 per band == oracle.iir, as numbers, for every B x M x T of the issue's sets (one
    trial, several, more workgroups than one; M = 1, a row that is no 16-byte multiple, the widest microphone group; T around the
    8-step register group and the 64-frame tile, and many tiles).  xf is dense -- band f + 1 starts where band f ends, so a write past
    a band lands in its neighbour and is seen by the comparison -- and lies between two guard regions that must stay untouched."""
    import torch

    from haghighatshoarmuir2024_amd import runtime

    dev = torch.device("cuda", 0)
    sections = _sections(kind, F)
    ref_full = _oracle_full(kind, F)
    x_full = torch.from_numpy(_x_full()).to(dev)
    GUARD, SENT = 2048, -777.25
    for B, M, T in itertools.product(B_SET, M_SET, T_SET):
        x = x_full[:B, :T, :M].contiguous()
        n = F * B * T * M
        buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float64, device=dev)
        xf = buf[GUARD : GUARD + n].view(F, B, T, M)
        got = runtime.filterbank(sections, x, device=dev, out=xf)
        assert got.data_ptr() == xf.data_ptr()
        host = buf.cpu().numpy()
        assert np.all(host[:GUARD] == SENT) and np.all(host[GUARD + n :] == SENT), (B, M, T)
        res = host[GUARD : GUARD + n].reshape(F, B, T, M)
        np.testing.assert_array_equal(res, ref_full[:, :B, :T, :M], err_msg=f"oracle B={B} M={M} T={T}")
        for f, (b, a) in enumerate(sections):
            np.testing.assert_array_equal(res[f], runtime.lfilter(b, a, x, device=dev).cpu().numpy(), err_msg=f"lfilter B={B} M={M} T={T} f={f}")


def test_filterbank_evolve_batch_equals_evolve_device():
    import torch

    from micloc.filterbank import ButterworthFilterbank

    fb = ButterworthFilterbank(freq_bands=[[1000, 1600], [1600, 2400], [2400, 3400]], order=1, fs=FS)
    x = np.random.RandomState(3).randn(2, 777, 7)
    got = fb.evolve_batch(x)
    assert tuple(got.shape) == (3, 2, 777, 7) and got.dtype == torch.float64
    for i in range(2):
        np.testing.assert_array_equal(got[:, i].cpu().numpy(), fb.evolve_device(x[i]).cpu().numpy())


@pytest.mark.parametrize("F", [1, 2, 5])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 449])
def test_band_sum_kernel(G, R, F):
    import torch

    from haghighatshoarmuir2024_amd import runtime

    rng = np.random.RandomState(G * 100 + R * 10 + F)
    bp = rng.rand(F, R, G) * 10.0 ** rng.randint(-8, 8, size=(F, R, G))  # (magnitudes apart: the order of the additions shows)
    if G > 2:
        bp[:, 0, :] = np.floor(bp[:, 0, :] * 4) / 4  # row 0: small dyadic values, exact sums ...
        bp[:, 0, :] = np.minimum(bp[:, 0, :], 1.0)
        bp[:, 0, G // 3] = 2.0                       # ... with the maximum F * 2 at two columns: an exact tie, the first wins
        bp[:, 0, G - 1] = 2.0
        bp[0, R - 1, 1] = np.nan                     # a NaN column never wins
    want = bp[0].copy()
    for f in range(1, F):
        want = want + bp[f]
    arg = np.array([0 if np.all(np.isnan(r)) else int(np.nanargmax(r)) for r in want])
    power, argmax = runtime.band_sum(torch.from_numpy(bp).cuda())
    np.testing.assert_array_equal(power.cpu().numpy(), want)
    np.testing.assert_array_equal(argmax.cpu().numpy(), arg)
    if G > 2:
        assert arg[0] == G // 3
    # argmax alone, power alone; a row of NaN only gives 0
    bp[:, R - 1, :] = np.nan
    _, a2 = runtime.band_sum(torch.from_numpy(bp).cuda(), want_power=False)
    p2, none = runtime.band_sum(torch.from_numpy(bp).cuda(), want_argmax=False)
    assert none is None and int(a2[R - 1]) == 0 and np.all(np.isnan(p2[R - 1].cpu().numpy()))
    if R > 1:
        np.testing.assert_array_equal(a2[: R - 1].cpu().numpy(), arg[: R - 1])


# ---- the localizer ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setup():
    """The fixture's configuration with the REFERENCE's matrices (no design run): a Demo -- the route the localizer replaces -- and the
    localizer over the same beamformers, matrices and filterbank; the fixture's packs as float64 [3, 4800, 7]."""
    from micloc.array_geometry import CenterCircularArray
    from micloc.filterbank import ButterworthFilterbank
    from micloc.localization_demo_snn import Demo
    from micloc.snn_beamformer import SNNBeamformer

    z = golden("wideband_packs.npz")
    geo = CenterCircularArray(4.5e-2, 7)
    demo = Demo.__new__(Demo)
    demo.beamfs, demo.bf_mats = [], [np.ascontiguousarray(W) for W in z["bf_mats"]]
    for fr in z["freq_bands"]:
        tau = 1 / (2 * np.pi * np.mean(fr))
        demo.beamfs.append(SNNBeamformer(geometry=geo, kernel_duration=float(z["kernel_duration"]), freq_range=fr, tau_vec=[tau, tau],
                                         bipolar_spikes=True, fs=FS))
    demo.filterbank = ButterworthFilterbank(freq_bands=z["freq_bands"], order=1, fs=FS)
    demo.doa_list, demo.fs = z["doa_list"], FS
    demo.recording_duration, demo.kernel_duration = float(z["recording_duration"]), float(z["kernel_duration"])
    packs = z["packs16"].astype(np.int32) << int(z["shift"])
    return dict(z=z, demo=demo, loc=demo.localizer(), packs=packs, data=np.ascontiguousarray(packs[:, :, :-1], dtype=np.float64))


@pytest.mark.parametrize("T", [2400, 4800])
@pytest.mark.parametrize("B", [1, 3])
def test_localize_batch_equals_power_grid(setup, B, T):
    demo, loc = setup["demo"], setup["loc"]
    x = np.ascontiguousarray(setup["data"][:B, :T])
    out = loc.localize_batch(x, return_band_power=True)
    power = out["power"].cpu().numpy()
    assert power.shape == (B, 112) and tuple(out["band_power"].shape) == (3, B, 112)
    want = np.stack([demo.power_grid(x[i]) for i in range(B)])
    np.testing.assert_array_equal(power, want)
    np.testing.assert_array_equal(out["argmax"].cpu().numpy(), np.argmax(want, axis=1))
    filt = demo.filterbank.evolve_batch(x)
    for f, (beamf, W) in enumerate(zip(demo.beamfs, demo.bf_mats)):
        one = beamf.localize_batch(W, filt[f])["power"].cpu().numpy()
        np.testing.assert_array_equal(out["band_power"][f].cpu().numpy(), one)


def test_localize_batch_against_the_reference_fixture(setup):
    """The reference's ButterworthFilterbank + three SNNBeamformers on three packs (tests/golden/make_golden_wideband.py): per-band and
    summed power to 1e-10 relative, the arg-max identical -- the project's tolerances against the reference."""
    z, loc = setup["z"], setup["loc"]
    out = loc.localize_batch(setup["data"], return_band_power=True)
    np.testing.assert_allclose(out["power"].cpu().numpy(), z["power_grid"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(out["band_power"].cpu().numpy().transpose(1, 0, 2), z["band_power"], rtol=1e-10, atol=0)
    np.testing.assert_array_equal(out["argmax"].cpu().numpy(), z["doa_index"])
    # the batch form of the demo's loop body: one silent pack among them
    packs = np.concatenate([setup["packs"], np.zeros_like(setup["packs"][:1])])
    doa = setup["demo"].process_frames(packs)
    assert np.isnan(doa[3])
    np.testing.assert_array_equal(doa[:3], z["doa_list"][z["doa_index"]] * 180 / np.pi)
    assert doa[0] == setup["demo"].process_frame(setup["packs"][0])


def test_windows_and_multi_source(setup):
    from haghighatshoarmuir2024_amd.utils import _add_peaks, _add_window_peaks

    demo, loc = setup["demo"], setup["loc"]
    x = setup["data"]
    doa_list = setup["z"]["doa_list"]
    out = loc.localize_batch(x, window=1024, hop=512, return_band_power=True, num_sources=2, doa_list=doa_list, min_separation=0.3)
    filt = demo.filterbank.evolve_batch(x)
    total = None
    for f, (beamf, W) in enumerate(zip(demo.beamfs, demo.bf_mats)):
        one = beamf.localize_batch(W, filt[f], window=1024, hop=512)
        np.testing.assert_array_equal(out["band_power"][f].cpu().numpy(), one["window_power"].cpu().numpy())
        total = one["window_power"] if total is None else total + one["window_power"]
        np.testing.assert_array_equal(out["window_start"], one["window_start"])
    nW = len(out["window_start"])
    assert nW == 1 + -(-(4800 - 1024) // 512) and tuple(out["window_power"].shape) == (3, nW, 112)
    np.testing.assert_array_equal(out["window_power"].cpu().numpy(), total.cpu().numpy())
    np.testing.assert_array_equal(out["window_argmax"].cpu().numpy(), np.argmax(total.cpu().numpy(), axis=2))
    want = _add_window_peaks(dict(window_power=total), doa_list, 2, 0.3, 0.0)
    np.testing.assert_array_equal(out["window_peaks"].cpu().numpy(), want["window_peaks"].cpu().numpy())
    np.testing.assert_array_equal(out["window_peak_power"].cpu().numpy(), want["window_peak_power"].cpu().numpy())
    # whole recordings: num_sources = 2 is _add_peaks on the summed power
    whole = loc.localize_batch(x, num_sources=2, doa_list=doa_list, min_separation=0.3)
    want = _add_peaks(dict(power=whole["power"].clone()), doa_list, 2, 0.3, 0.0)
    np.testing.assert_array_equal(whole["peaks"].cpu().numpy(), want["peaks"].cpu().numpy())
    np.testing.assert_array_equal(whole["peak_power"].cpu().numpy(), want["peak_power"].cpu().numpy())
    assert tuple(whole["peaks"].shape) == (3, 2) and int(whole["peaks"][0, 0]) == int(whole["argmax"][0])
    with pytest.raises(ValueError):
        loc.localize_batch(x, window=1000)  # not a multiple of the window quantum


def _entry_args(loc, T):
    from haghighatshoarmuir2024_amd import _lib, runtime

    plans = loc.plans(np.arange(T) / FS)
    bb, aa, n = runtime.pad_ba_list(loc.filterbank.ba_list)
    handles = (ctypes.c_void_p * len(plans))(*[p.handle.value for p in plans])
    return _lib.load(), plans, handles, bb, aa, n


def test_graph_replay_of_the_c_entry(setup):
    """micloc_snn_pipeline_bands_f64 captured once on a single stream, replayed on a second pack == the eager call."""
    import torch

    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.runtime import _dptr, _ptr, _stream

    loc, data = setup["loc"], setup["data"]
    B, T, M = 1, 4800, 7
    lib, plans, handles, bb, aa, n = _entry_args(loc, T)
    dev = plans[0].device
    nbytes = lib.micloc_snn_bands_workspace_bytes(handles, 3, B, T, 0, 0)
    assert nbytes > 3 * B * T * M * 8
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    x = torch.from_numpy(data[0:1]).to(dev).contiguous()
    power = torch.zeros((B, 112), dtype=torch.float64, device=dev)
    argmax = torch.zeros((B,), dtype=torch.int32, device=dev)

    def launch():
        _lib.check(lib.micloc_snn_pipeline_bands_f64(handles, 3, _dptr(bb), _dptr(aa), n, _ptr(x), B, T, 0, 0, None, _ptr(power), _ptr(argmax), _ptr(ws),
                                                     nbytes, _stream(dev)), "snn_pipeline_bands")

    launch()  # eager once: nothing is allocated or uploaded inside the capture
    torch.cuda.synchronize()
    np.testing.assert_array_equal(power.cpu().numpy(), loc.localize_batch(data[0:1])["power"].cpu().numpy())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    x.copy_(torch.from_numpy(data[1:2]))
    power.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = loc.localize_batch(data[1:2])
    np.testing.assert_array_equal(power.cpu().numpy(), eager["power"].cpu().numpy())
    np.testing.assert_array_equal(argmax.cpu().numpy(), eager["argmax"].cpu().numpy())


def test_pipeline_status_codes(setup):
    """The status codes that need a plan, each returned before any launch (the outputs keep their sentinel)."""
    import torch

    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.runtime import _dptr, _ptr, _stream
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    loc, data = setup["loc"], setup["data"]
    B, T = 1, 2400
    lib, plans, handles, bb, aa, n = _entry_args(loc, T)
    dev = plans[0].device
    nbytes = lib.micloc_snn_bands_workspace_bytes(handles, 3, B, T, 0, 0)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    x = torch.from_numpy(data[0:1, :T]).to(dev).contiguous()
    power = torch.full((B, 112), -5.0, dtype=torch.float64, device=dev)

    def call(h, F=3, window=0, hop=0, ws_t=ws, ws_bytes=nbytes):
        return lib.micloc_snn_pipeline_bands_f64(h, F, _dptr(bb), _dptr(aa), n, _ptr(x), B, T, window, hop, None, _ptr(power), None, _ptr(ws_t), ws_bytes,
                                                 _stream(dev))

    assert call(handles) == _lib.MICLOC_OK
    power.fill_(-5.0)
    assert call(handles, ws_bytes=nbytes - 1) == _lib.MICLOC_ERR_WORKSPACE
    assert call(handles, ws_t=ws[8:]) == _lib.MICLOC_ERR_WORKSPACE  # misaligned
    assert call(handles, window=1000, hop=1000) == _lib.MICLOC_ERR_SHAPE
    assert call(handles, window=1024, hop=100) == _lib.MICLOC_ERR_SHAPE
    geo = CenterCircularArray(4.5e-2, 7)
    tau = 1 / (2 * np.pi * 2000)
    fresh = SNNBeamformer(geo, 10e-3, [1600.0, 2400.0], [tau, tau], bipolar_spikes=True, fs=FS).new_plan()

    def with_plan(p):
        return (ctypes.c_void_p * 3)(plans[0].handle.value, p.handle.value, plans[2].handle.value)

    assert call(with_plan(fresh)) == _lib.MICLOC_ERR_NOT_SET  # no neuron kernel, no bf_mat
    fresh.set_neuron_kernel(np.ones(8) / 8)
    assert call(with_plan(fresh)) == _lib.MICLOC_ERR_NOT_SET  # no bf_mat
    fresh.set_bf_mat(np.ones((14, 111)))
    assert call(with_plan(fresh)) == _lib.MICLOC_ERR_SHAPE  # another G
    fresh.set_bf_mat(np.ones((7, 112)) + 1j)
    assert call(with_plan(fresh)) == _lib.MICLOC_ERR_SHAPE  # a complex bf_mat
    five = SNNBeamformer(CenterCircularArray(4.5e-2, 5), 10e-3, [1600.0, 2400.0], [tau, tau], bipolar_spikes=True, fs=FS).new_plan()
    five.set_neuron_kernel(np.ones(8) / 8)
    five.set_bf_mat(np.ones((10, 112)))
    assert call(with_plan(five)) == _lib.MICLOC_ERR_SHAPE  # another M
    assert lib.micloc_snn_bands_workspace_bytes(with_plan(five), 3, B, T, 0, 0) == 0
    torch.cuda.synchronize()
    assert np.all(power.cpu().numpy() == -5.0)


def test_from_bands_builds_what_the_demo_builds():
    from micloc.array_geometry import CenterCircularArray
    from micloc.localization_demo_snn import Demo
    from micloc.wideband import WidebandSNNLocalizer

    geo = CenterCircularArray(4.5e-2, 7)
    doa_list = np.linspace(-np.pi, np.pi, 8)
    kw = dict(geometry=geo, freq_bands=[[1000, 1600], [1600, 2400]], doa_list=doa_list, recording_duration=0.05, kernel_duration=10e-3, bipolar_spikes=True,
              fs=FS)
    demo, loc = Demo(**kw), WidebandSNNLocalizer.from_bands(**kw)
    assert len(loc.beamfs) == 2
    for f in range(2):
        np.testing.assert_array_equal(loc.bf_mats[f], demo.bf_mats[f])
        for u, v in zip(loc.filterbank.ba_list[f], demo.filterbank.ba_list[f]):
            np.testing.assert_array_equal(u, v)
        assert loc.beamfs[f].tau_vec == demo.beamfs[f].tau_vec and loc.beamfs[f].kernel_length == demo.beamfs[f].kernel_length
        for u, v in zip(loc.beamfs[f].bandpass_filter, demo.beamfs[f].bandpass_filter):
            np.testing.assert_array_equal(u, v)


def test_wideband_speech_sweep_equals_the_power_grid_route(setup, tmp_path):
    """Parity mode on a 0.1 s cut of the speech source, 2 SNRs x 4 trials: the batched localizer == a localizer composed from
    Demo.power_grid trial by trial; a resumed run returns the same arrays without computing anything."""
    from haghighatshoarmuir2024_amd.sweep import speech_source, wideband_speech_sweep

    demo, loc = setup["demo"], setup["loc"]
    pcm = np.load(os.path.join(ROOT, "tests", "golden", "speech_trial.npz"))
    src = speech_source(FS, pcm16=pcm["pcm16"][20000:21600], rate=int(pcm["rate"]))  # 0.1 s of the utterance
    doa_list = setup["z"]["doa_list"]

    def grid_localizer(sig_batch, time_vec):
        p = np.stack([demo.power_grid(np.asarray(s)) for s in sig_batch])
        a = np.argmax(p, axis=1)
        return a.astype(np.int64), p[np.arange(len(a)), a]

    kw = dict(snr_db_vec=[0.0, 10.0], num_sim=4, seed=11, mode="parity")
    got = wideband_speech_sweep(loc, doa_list, src, out_dir=tmp_path, **kw)
    want = wideband_speech_sweep(loc, doa_list, src, localizer=grid_localizer, **kw)
    for k in ("doa", "argmax", "pmax", "err", "mae_deg"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["argmax"].shape == (2, 4) and got["persistence"]["trials_loaded"] == 0
    calls = []

    def never(sig_batch, time_vec):
        calls.append(len(sig_batch))
        raise AssertionError("a resumed sweep must not compute a finished trial")

    again = wideband_speech_sweep(loc, doa_list, src, out_dir=tmp_path, localizer=never, **kw)
    assert calls == [] and again["persistence"]["trials_loaded"] == 8
    for k in ("doa", "argmax", "pmax", "err", "mae_deg"):
        np.testing.assert_array_equal(again[k], got[k], err_msg=k)


def test_value_errors(setup):
    from micloc.array_geometry import CenterCircularArray
    from micloc.filterbank import ButterworthFilterbank
    from micloc.snn_beamformer import SNNBeamformer
    from micloc.wideband import WidebandSNNLocalizer

    loc = setup["loc"]
    fb2 = ButterworthFilterbank(freq_bands=[[1000, 1600], [1600, 2400]], order=1, fs=FS)
    with pytest.raises(ValueError):  # G mismatch
        WidebandSNNLocalizer(loc.beamfs[:2], [loc.bf_mats[0], loc.bf_mats[1][:, :100]], fb2)
    tau = 1 / (2 * np.pi * 2000)
    five = SNNBeamformer(CenterCircularArray(4.5e-2, 5), 10e-3, [1600.0, 2400.0], [tau, tau], bipolar_spikes=True, fs=FS)
    with pytest.raises(ValueError):  # M mismatch
        WidebandSNNLocalizer([loc.beamfs[0], five], [loc.bf_mats[0], np.zeros((10, 112))], fb2)
    bands17 = [[1000.0 + 100 * i, 1100.0 + 100 * i] for i in range(17)]
    with pytest.raises(ValueError):  # 17 bands
        WidebandSNNLocalizer([loc.beamfs[0]] * 17, [loc.bf_mats[0]] * 17, ButterworthFilterbank(freq_bands=bands17, order=1, fs=FS))
    with pytest.raises(ValueError):  # the input's microphones
        loc.localize_batch(np.zeros((1, 2400, 5)))
    with pytest.raises(ValueError):  # 17 sections through the kernel wrapper
        ButterworthFilterbank(freq_bands=bands17, order=1, fs=FS).evolve_batch(np.zeros((1, 64, 7)))
