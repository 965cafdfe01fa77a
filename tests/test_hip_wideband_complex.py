"""Device tests of the wideband complex Beamformer: bands_bandpass_kernel against the one-shot band-pass rows of every band, the batch
F * B STHT against the F batch-B calls, micloc_beamformer_pipeline_bands_f64 against Beamformer.localize_batch band by band and a
sequential NumPy band sum, WidebandBeamformerLocalizer.localize_batch against Demo.power_grid (the route it replaces) and the
reference's fixture, multi-source read-out, graph replay of the C entry, its status codes, and the wideband speech sweep."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

FS = 48_000
B_SET, M_SET, T_SET = (1, 3), (1, 7, 16), (1, 2, 31, 32, 33, 255, 256, 257, 1001)
F_SET = (1, 2, 3, 16)
BANDS3 = [[1000.0, 1600.0], [1600.0, 2400.0], [2400.0, 3400.0]]


def _band_filters(kind, F):
    """F band-pass sections of one length: Butterworth band-passes of order 1 or 2 (n = 3, 5) on F different bands, or random stable
    filters of n = 9 without a zero coefficient (four pole pairs of modulus <= 0.9, a[0] != 1: the division by a[0] is part of the
    contract)."""
    from scipy.signal import butter

    if kind == "random9":
        rng = np.random.RandomState(900 + F)
        out = []
        for _ in range(F):
            a = np.ones(1)
            for _ in range(4):
                r, th = 0.3 + 0.6 * rng.rand(), np.pi * (0.05 + 0.9 * rng.rand())
                a = np.convolve(a, [1.0, -2 * r * np.cos(th), r * r])
            a = a * (1.5 + rng.rand())
            b = rng.randn(9)
            b = b + 0.1 * np.sign(b)
            assert len(a) == 9 and np.all(a != 0) and np.all(b != 0)
            out.append((b, a))
        return out
    return [butter(int(kind), [300.0 + 1200 * f, 1200.0 + 1200 * f], btype="bandpass", output="ba", fs=FS) for f in range(F)]


_XF = {}


def _xf_full(torch):
    """The one input of every band-pass case [16, 3, 1001, 16] on the device; the smaller shapes are its leading slices."""
    if "xf" not in _XF:
        _XF["xf"] = torch.from_numpy(np.random.RandomState(17).randn(max(F_SET), max(B_SET), max(T_SET), max(M_SET))).cuda()
    return _XF["xf"]


@pytest.mark.parametrize("F", F_SET)
@pytest.mark.parametrize("kind", ["1", "2", "random9"])
def test_bands_bandpass_equals_the_one_shot_rows(kind, F):
    """bands_bandpass_kernel == the `pre` rows of the one-shot band-pass (micloc_bandpass_rzcc_f64 on that band's STHT) for every band
    under assert_array_equal (which lets the sign of a zero differ and nothing else), for every B x M x T of the issue's sets: one
    trial and several; M = 1, 7 and 16 (a workgroup's chains then straddle trials and bands); T around the 8-step register group and
    the 32-frame tile, many tiles, and T shorter than the Hilbert kernel's roll.  The frames [T, Ts) of the one-launch rows are zero.
    The batch F * B STHT of the entry equals the F batch-B calls bit for bit, and the stage entry's per-band launches (one_launch = 0: the
    arm the one launch is measured against) give the same frames.  `pre` lies between two guard regions that must stay untouched."""
    import torch

    from haghighatshoarmuir2024_amd import runtime
    from oracle import oracle as O

    ker = O.stht_kernel(FS, 2e-3)  # 96 taps: a roll of 48 frames, longer than the shortest recordings
    filters = _band_filters(kind, F)
    GUARD, SENT = 2048, -777.25
    for M in M_SET:
        plans = [runtime.Plan(M, ker, b, a, 1, False) for b, a in filters]
        dev = plans[0].device
        for B, T in itertools.product(B_SET, T_SET):
            xf = _xf_full(torch)[:F, :B, :T, :M].contiguous()
            Ts = plans[0].padded_T(T)
            n = F * B * 2 * M * Ts
            buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float64, device=dev)
            pre = buf[GUARD : GUARD + n].view(F * B, 2 * M, Ts)
            h, got = runtime.beamformer_bands_bandpass(plans, xf, pre=pre)
            assert got.data_ptr() == pre.data_ptr()
            _, loop = runtime.beamformer_bands_bandpass(plans, xf, one_launch=False)
            host = buf.cpu().numpy()
            assert np.all(host[:GUARD] == SENT) and np.all(host[GUARD + n :] == SENT), (B, M, T)
            res = host[GUARD : GUARD + n].reshape(F, B, 2 * M, Ts)
            assert not res[..., T:].any(), (B, M, T)
            hq = h.view(F, B, 2 * M, Ts)[:, :, M:, :T]
            for f, plan in enumerate(plans):
                h_f = plan.stht(xf[f])
                assert torch.equal(hq[f], h_f[:, M:, :T]), f"STHT B={B} M={M} T={T} f={f}"
                want, _ = plan.bandpass_rzcc(h_f, T, want_pre=True, want_spikes=False)
                np.testing.assert_array_equal(res[f][..., :T], want[..., :T].cpu().numpy(), err_msg=f"B={B} M={M} T={T} f={f}")
                assert torch.equal(loop.view(F, B, 2 * M, Ts)[f][..., :T], want[..., :T]), f"per-band route B={B} M={M} T={T} f={f}"


def test_bands_bandpass_with_the_demo_kernel_and_more_workgroups():
    """The live demo's 480-tap Hilbert kernel, 3 x 24 x 14 = 1008 chains: 63 workgroups of 16 chains, the last ones of a band shared
    with the next band."""
    import torch

    from haghighatshoarmuir2024_amd import runtime
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer

    geo = CenterCircularArray(4.5e-2, 7)
    plans = [Beamformer(geo, 10e-3, fr, fs=FS).plan() for fr in BANDS3]
    B, T = 24, 700
    xf = torch.from_numpy(np.random.RandomState(2).randn(3, B, T, 7)).cuda()
    h, pre = runtime.beamformer_bands_bandpass(plans, xf)
    for f, plan in enumerate(plans):
        h_f = plan.stht(xf[f])
        want, _ = plan.bandpass_rzcc(h_f, T, want_pre=True, want_spikes=False)
        np.testing.assert_array_equal(pre.view(3, B, 14, -1)[f][..., :T].cpu().numpy(), want[..., :T].cpu().numpy())


# ---- the entry -------------------------------------------------------------------------------------------------------------------------

def _random_localizer(M, G, seed):
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer
    from micloc.filterbank import ButterworthFilterbank
    from micloc.wideband import WidebandBeamformerLocalizer

    geo = CenterCircularArray(4.5e-2, M)
    rng = np.random.RandomState(seed)
    mats = [rng.randn(M, G) + 1j * rng.randn(M, G) for _ in BANDS3]
    return WidebandBeamformerLocalizer([Beamformer(geo, 10e-3, fr, fs=FS) for fr in BANDS3], mats, ButterworthFilterbank(freq_bands=BANDS3, order=2, fs=FS))


@pytest.mark.parametrize("G", [1, 57, 112])
@pytest.mark.parametrize("M", [7, 9])  # the bf_mat-stationary kernel (up to 8 microphones) and the general one
def test_entry_equals_localize_batch_band_by_band(M, G):
    """band_power of the entry == Beamformer.localize_batch of each band on that band's filterbank output (torch.equal), whole
    recordings and windows; power / argmax == the sequential NumPy band sum and its first maximum.  T around one chunk of the serving
    kernel (its window quantum) and the live demo's 4800."""
    import torch

    loc = _random_localizer(M, G, 10 * M + G)
    plans = loc.plans()
    q = plans[0].window_quantum()
    assert all(p.window_quantum() == q for p in plans)
    rng = np.random.RandomState(M + G)
    x_full = rng.randn(3, 4800, M)
    for B, T in itertools.product((1, 3), (q - 1, q, q + 1, 2 * q + 1, 4800)):
        x = np.ascontiguousarray(x_full[:B, :T])
        filt = loc.filterbank.evolve_batch(x)
        for window, hop in ((None, None), (2 * q, q)) if T > q else ((None, None),):
            out = loc.localize_batch(x, return_band_power=True, window=window, hop=hop)
            key = "power" if window is None else "window_power"
            rows = []
            for f, (beamf, W) in enumerate(zip(loc.beamfs, loc.bf_mats)):
                one = beamf.localize_batch(W, filt[f], window=window, hop=hop)
                assert torch.equal(out["band_power"][f], one[key]), f"B={B} T={T} window={window} f={f}"
                rows.append(one[key].cpu().numpy())
            total = rows[0]
            for r in rows[1:]:
                total = total + r
            np.testing.assert_array_equal(out[key].cpu().numpy(), total)
            np.testing.assert_array_equal(out["argmax" if window is None else "window_argmax"].cpu().numpy(), np.argmax(total, axis=-1))
            if window is not None:
                assert tuple(out["window_power"].shape) == (B, 1 + -(-(T - 2 * q) // q) if T > 2 * q else 1, G)
    # the result does not depend on how budget_bytes splits the batch
    x = np.ascontiguousarray(x_full[:, :1000])
    whole = loc.localize_batch(x, return_band_power=True)
    assert loc.trials_per_call(plans, 3, 1000, None, None, 1) == 1 and loc.trials_per_call(plans, 3, 1000, None, None, 1 << 40) == 3
    split = loc.localize_batch(x, return_band_power=True, budget_bytes=1)
    for k in ("power", "argmax", "band_power"):
        assert torch.equal(whole[k], split[k]), k


@pytest.fixture(scope="module")
def setup():
    """The fixture's configuration with the REFERENCE's matrices (no design run): a Demo -- the route the localizer replaces -- and the
    localizer over the same beamformers, matrices and filterbank; the packs of wideband_packs.npz as float64 [3, 4800, 7]."""
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer
    from micloc.filterbank import ButterworthFilterbank
    from micloc.localization_demo import Demo

    z, c = golden("wideband_packs.npz"), golden("wideband_complex_packs.npz")
    geo = CenterCircularArray(4.5e-2, 7)
    demo = Demo.__new__(Demo)
    demo.bf_mats = [np.ascontiguousarray(W) for W in c["bf_mats"]]
    demo.beamfs = [Beamformer(geometry=geo, kernel_duration=float(z["kernel_duration"]), freq_range=fr, fs=FS) for fr in z["freq_bands"]]
    demo.filterbank = ButterworthFilterbank(freq_bands=z["freq_bands"], order=int(c["filterbank_order"]), fs=FS)
    demo.doa_list, demo.fs = z["doa_list"], FS
    demo.recording_duration, demo.kernel_duration = float(z["recording_duration"]), float(z["kernel_duration"])
    packs = z["packs16"].astype(np.int32) << int(z["shift"])
    return dict(z=z, c=c, demo=demo, loc=demo.localizer(), packs=packs, data=np.ascontiguousarray(packs[:, :, :-1], dtype=np.float64))


def test_localize_batch_equals_power_grid_pack_by_pack(setup):
    demo, loc, data = setup["demo"], setup["loc"], setup["data"]
    out = loc.localize_batch(data)
    want = np.stack([demo.power_grid(pack) for pack in data])
    np.testing.assert_array_equal(out["power"].cpu().numpy(), want)
    np.testing.assert_array_equal(out["argmax"].cpu().numpy(), np.argmax(want, axis=1))
    for i in range(3):  # and one pack at a time
        np.testing.assert_array_equal(loc.localize_batch(data[i : i + 1])["power"][0].cpu().numpy(), want[i])


def test_localize_batch_against_the_reference_fixture(setup):
    """The reference's order-2 ButterworthFilterbank + three Beamformers on three packs (tests/golden/make_golden_wideband_complex.py):
    per-band and summed power to 1e-10 relative, the arg-max identical -- the project's tolerances against the reference."""
    z, c, loc = setup["z"], setup["c"], setup["loc"]
    out = loc.localize_batch(setup["data"], return_band_power=True)
    np.testing.assert_allclose(out["power"].cpu().numpy(), c["power_grid"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(out["band_power"].cpu().numpy().transpose(1, 0, 2), c["band_power"], rtol=1e-10, atol=0)
    np.testing.assert_array_equal(out["argmax"].cpu().numpy(), c["doa_index"])
    # the batch form of the demo's loop body: one silent pack among them
    packs = np.concatenate([setup["packs"], np.zeros_like(setup["packs"][:1])])
    doa = setup["demo"].process_frames(packs)
    assert np.isnan(doa[3])
    np.testing.assert_array_equal(doa[:3], z["doa_list"][c["doa_index"]] * 180 / np.pi)
    assert doa[0] == setup["demo"].process_frame(setup["packs"][0])
    seen = []
    setup["demo"].run(setup["packs"][:2], sink=seen.append)
    np.testing.assert_array_equal(seen, doa[:2])


def test_two_sources_on_the_third_pack(setup):
    """The third pack has a different direction per band (per-band arg-maxes 11, 76, 48): num_sources = 2 reads two peaks off the
    summed pattern -- _add_peaks on the summed power, the strongest first."""
    from haghighatshoarmuir2024_amd.utils import _add_peaks

    loc, data, doa_list = setup["loc"], setup["data"], setup["z"]["doa_list"]
    out = loc.localize_batch(data, num_sources=2, doa_list=doa_list, min_separation=0.3)
    want = _add_peaks(dict(power=out["power"].clone()), doa_list, 2, 0.3, 0.0)
    np.testing.assert_array_equal(out["peaks"].cpu().numpy(), want["peaks"].cpu().numpy())
    np.testing.assert_array_equal(out["peak_power"].cpu().numpy(), want["peak_power"].cpu().numpy())
    peaks, pp = out["peaks"].cpu().numpy(), out["peak_power"].cpu().numpy()
    power = out["power"].cpu().numpy()
    assert peaks.shape == (3, 2) and peaks[2, 0] == 48 == int(out["argmax"][2]) and peaks[2, 1] >= 0
    assert pp[2, 0] == power[2, 48] and pp[2, 1] == power[2, peaks[2, 1]] and pp[2, 1] <= pp[2, 0]
    assert peaks[2, 1] != 48


def _entry_args(loc):
    from haghighatshoarmuir2024_amd import _lib, runtime

    plans = loc.plans()
    bb, aa, n = runtime.pad_ba_list(loc.filterbank.ba_list)
    handles = (ctypes.c_void_p * len(plans))(*[p.handle.value for p in plans])
    return _lib.load(), plans, handles, bb, aa, n


def test_graph_replay_of_the_c_entry(setup):
    """micloc_beamformer_pipeline_bands_f64 captured once on a single stream, replayed on a second pack == the eager call."""
    import torch

    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.runtime import _dptr, _ptr, _stream

    loc, data = setup["loc"], setup["data"]
    B, T, M = 1, 4800, 7
    lib, plans, handles, bb, aa, n = _entry_args(loc)
    dev = plans[0].device
    nbytes = lib.micloc_beamformer_bands_workspace_bytes(handles, 3, B, T, 0, 0)
    assert nbytes > 3 * B * (T * M + 2 * 2 * M * T) * 8
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    x = torch.from_numpy(data[0:1]).to(dev).contiguous()
    power = torch.zeros((B, 112), dtype=torch.float64, device=dev)
    argmax = torch.zeros((B,), dtype=torch.int32, device=dev)

    def launch():
        _lib.check(lib.micloc_beamformer_pipeline_bands_f64(handles, 3, _dptr(bb), _dptr(aa), n, _ptr(x), B, T, 0, 0, None, _ptr(power), _ptr(argmax),
                                                            _ptr(ws), nbytes, _stream(dev)), "beamformer_pipeline_bands")

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


def test_status_codes(setup):
    """Every status code of the entry, each returned before any launch (the outputs keep their sentinel), in the header's order."""
    import torch
    from scipy.signal import butter

    from haghighatshoarmuir2024_amd import _lib, runtime
    from haghighatshoarmuir2024_amd.runtime import _dptr, _ptr, _stream
    from oracle import oracle as O

    loc, data = setup["loc"], setup["data"]
    B, T = 1, 2400
    lib, plans, handles, bb, aa, n = _entry_args(loc)
    dev = plans[0].device
    nbytes = lib.micloc_beamformer_bands_workspace_bytes(handles, 3, B, T, 0, 0)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    x = torch.from_numpy(data[0:1, :T]).to(dev).contiguous()
    power = torch.full((B, 112), -5.0, dtype=torch.float64, device=dev)

    def call(h, F=3, Bc=B, Tc=T, window=0, hop=0, ws_t=ws, ws_bytes=nbytes, xp=x, out=power):
        return lib.micloc_beamformer_pipeline_bands_f64(h, F, _dptr(bb), _dptr(aa), n, _ptr(xp), Bc, Tc, window, hop, None, _ptr(out), None, _ptr(ws_t),
                                                        ws_bytes, _stream(dev))

    assert call(handles) == _lib.MICLOC_OK
    torch.cuda.synchronize()
    assert np.all(power.cpu().numpy() >= 0.0)
    power.fill_(-5.0)
    q = plans[0].window_quantum()
    INV, NS, SH, WS = _lib.MICLOC_ERR_INVALID, _lib.MICLOC_ERR_NOT_SET, _lib.MICLOC_ERR_SHAPE, _lib.MICLOC_ERR_WORKSPACE
    # INVALID: null pointers, F outside 1..16, bad B or T -- in front of everything else
    ker = O.stht_kernel(FS, 10e-3)
    b2, a2 = butter(2, [1600.0, 2400.0], btype="bandpass", output="ba", fs=FS)
    fresh = runtime.Plan(7, ker, b2, a2, 1, False)  # no bf_mat

    def with_plan(p):
        return (ctypes.c_void_p * 3)(plans[0].handle.value, p.handle.value, plans[2].handle.value)

    assert call(None) == INV and call(handles, xp=None) == INV and call(handles, out=None) == INV
    assert call((ctypes.c_void_p * 3)(plans[0].handle.value, None, plans[2].handle.value)) == INV
    for over in (dict(F=0), dict(F=17), dict(Bc=0), dict(Bc=65536), dict(Bc=30000), dict(Tc=0), dict(window=-1), dict(hop=-1)):
        assert call(with_plan(fresh), **over) == INV, over  # (although a plan lacks its bf_mat)
    # NOT_SET before SHAPE
    assert call(with_plan(fresh), window=1000) == NS
    assert lib.micloc_beamformer_bands_workspace_bytes(with_plan(fresh), 3, B, T, 0, 0) == 0
    # SHAPE: a real bf_mat; plans that differ in M, G, Hilbert kernel length, Hilbert kernel values or band-pass length; windows
    fresh.set_bf_mat(np.ones((14, 112)))
    assert call(with_plan(fresh)) == SH
    fresh.set_bf_mat(np.ones((7, 111)) + 1j)
    assert call(with_plan(fresh)) == SH
    fresh.set_bf_mat(np.ones((7, 112)) + 1j)
    assert call(with_plan(fresh), ws_bytes=nbytes - 1) == WS  # (a plan that fits: the next check is the workspace)
    five = runtime.Plan(5, ker, b2, a2, 1, False)
    five.set_bf_mat(np.ones((5, 112)) + 1j)
    assert call(with_plan(five)) == SH
    short = runtime.Plan(7, O.stht_kernel(FS, 5e-3), b2, a2, 1, False)
    short.set_bf_mat(np.ones((7, 112)) + 1j)
    assert call(with_plan(short)) == SH
    other = runtime.Plan(7, ker * 1.5, b2, a2, 1, False)
    other.set_bf_mat(np.ones((7, 112)) + 1j)
    assert call(with_plan(other)) == SH
    b1, a1 = butter(1, [1600.0, 2400.0], btype="bandpass", output="ba", fs=FS)
    order1 = runtime.Plan(7, ker, b1, a1, 1, False)
    order1.set_bf_mat(np.ones((7, 112)) + 1j)
    assert call(with_plan(order1)) == SH
    assert lib.micloc_beamformer_bands_workspace_bytes(with_plan(order1), 3, B, T, 0, 0) == 0
    assert call(handles, window=1000, hop=1000) == SH
    assert call(handles, window=2 * q, hop=100) == SH
    assert lib.micloc_beamformer_bands_workspace_bytes(handles, 3, B, T, 1000, 1000) == 0
    # SHAPE before WORKSPACE
    assert call(with_plan(order1), ws_bytes=0) == SH
    # WORKSPACE: too small or misaligned
    assert call(handles, ws_bytes=nbytes - 1) == WS
    assert call(handles, ws_t=ws[8:]) == WS
    assert call(handles, ws_t=None) == WS
    # the stage entry's own SHAPE checks
    xf = torch.zeros((3, 1, 64, 7), dtype=torch.float64, device=dev)
    hh = torch.zeros((3, 14, 64), dtype=torch.float64, device=dev)
    bpf = lib.micloc_beamformer_bands_bandpass_f64
    assert bpf(handles, 3, _ptr(xf), 1, 64, _ptr(hh), _ptr(hh), 63, 1, 1, _stream(dev)) == SH
    assert bpf(with_plan(order1), 3, _ptr(xf), 1, 64, _ptr(hh), _ptr(hh), 64, 1, 1, _stream(dev)) == SH
    torch.cuda.synchronize()
    assert np.all(power.cpu().numpy() == -5.0)
    with pytest.raises(ValueError):
        loc.localize_batch(data[:1], window=1000)  # not a multiple of the window quantum


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
