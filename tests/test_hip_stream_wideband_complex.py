"""The wideband complex Beamformer as a stream (include/micloc_hip.h "wideband streaming, complex Beamformer") on the MI355X: the band-pass
tile kernel of all bands' chains against the one-shot rows in its three forms, finish() against WidebandBeamformerLocalizer.localize_batch
bit for bit for any tiling, the windows, the running read-out, the reference's fixture, status codes and two host threads.  The clock's
bookkeeping and the ring depth are the NumPy restatements of tests/test_stream_complex_cpu.py and tests/test_stream_wideband_complex_cpu.py."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

from conftest import golden
from test_stream_complex_cpu import bookkeeping, random_tiling
from test_stream_wideband_complex_cpu import ring_depth

pytestmark = pytest.mark.gpu

FS = 48_000
BANDS3 = [[1000.0, 1600.0], [1600.0, 2400.0], [2400.0, 3400.0]]


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _handles(plans):
    return (ctypes.c_void_p * len(plans))(*[p.handle.value for p in plans])


def random_localizer(M, G, seed, bands=BANDS3):
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer
    from micloc.filterbank import ButterworthFilterbank
    from micloc.wideband import WidebandBeamformerLocalizer

    geo = CenterCircularArray(4.5e-2, M)
    rng = np.random.RandomState(seed)
    mats = [rng.randn(M, G) + 1j * rng.randn(M, G) for _ in bands]
    return WidebandBeamformerLocalizer([Beamformer(geo, 10e-3, fr, fs=FS) for fr in bands], mats, ButterworthFilterbank(freq_bands=bands, order=2, fs=FS))


def wrap_of(loc, x):
    """wrap_tail [F, B, L // 2, M] of a recording x [B, T, M], obtained as tests/test_hip_stream_wideband.py obtains it: the last L // 2
    frames of every band's FILTERED recording -- for a recording shorter than that, np.roll's rows zero padded (wrap_rows)."""
    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

    L = len(loc.beamfs[0].kernel)
    filt = loc.filterbank.evolve_batch(np.ascontiguousarray(x))
    if x.shape[1] >= L // 2:
        return filt[:, :, -(L // 2) :, :].contiguous()
    return np.stack([ComplexStreamingLocalizer.wrap_rows(f.cpu().numpy(), L) for f in filt])


def stream(loc, x, tiles, replay=False, known=True, **kw):
    """Push x [B, T, M] in `tiles` (the last one final) -> (localizer, finish())."""
    B, T, M = x.shape
    assert sum(tiles) == T
    kw.setdefault("wrap_tail", wrap_of(loc, x))
    kw.setdefault("max_tile", max(tiles))
    s = loc.streaming_localizer(batch=B, total_frames=T if known else None, **kw)
    t = 0
    for i, n in enumerate(tiles):
        if replay:
            s.push_replay(x[:, t : t + n, :])
        else:
            s.push(x[:, t : t + n, :], final=None if known else i == len(tiles) - 1)
        t += n
    return s, s.finish()


# ---- 1. the band-pass tile kernel against the one-shot rows ----------------------------------------------------------------------------
def _band_filters(kind, F):
    """tests/test_hip_wideband_complex.py's sections, restated: Butterworth band-passes of order 1 or 2 on F different bands, or random stable
    filters of n = 9 without a zero coefficient and with a[0] != 1."""
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
        _XF["xf"] = torch.from_numpy(np.random.RandomState(23).randn(16, 3, 1001, 16)).cuda()
    return _XF["xf"]


TILINGS_1001 = [[1001], [16] * 62 + [9], [1] * 40 + [961], [31, 32, 33, 300, 1, 255, 256, 93]]  # 1-frame tiles; tiles across 32 and 33 frames


@pytest.mark.parametrize("F", [1, 2, 3, 16])
@pytest.mark.parametrize("kind", ["1", "2", "random9"])
def test_bandpass_tiles_equal_the_one_launch_rows(kind, F, torch):
    """stream_bands_bandpass_tile_kernel<N, CH>, CH = 16, 32 and 64 forced, against the rows of micloc_beamformer_bands_bandpass_f64
    (one_launch = 1) on the whole recording, element by element (assert_array_equal's comparison: the sign of a zero is excepted): after
    every tile the staging rows hold [carry | tile] and zeros up to the chunk border.  Guard bytes around the state and the workspace;
    every stream twice across a reset."""
    from haghighatshoarmuir2024_amd import _lib, runtime
    from oracle import oracle as O

    assert sum(TILINGS_1001[3]) == 1001
    ker = O.stht_kernel(FS, 2e-3)  # 96 taps
    L2 = len(ker) // 2
    filters = _band_filters(kind, F)
    lib = _lib.load()
    GUARD = 512

    def guarded(nbytes, dev):
        buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 256 == 0
        return buf, buf[GUARD : GUARD + nbytes]

    def guards_intact(buf):
        return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())

    rng = np.random.RandomState(F)
    for M in (1, 7, 16):
        plans = [runtime.Plan(M, ker, b, a, 1, False) for b, a in filters]
        for p in plans:
            p.set_bf_mat(rng.randn(M, 3) + 1j * rng.randn(M, 3))
        dev, C = plans[0].device, 2 * M
        hd = _handles(plans)
        CH = plans[0].window_quantum()
        st = lambda: runtime._stream(dev)  # noqa: E731
        for B in (1, 3):
            for T, tilings in ((1001, TILINGS_1001), (1, [[1]])):
                xf = _xf_full(torch)[:F, :B, :T, :M].contiguous()
                Ts = plans[0].padded_T(T)
                h, pre = runtime.beamformer_bands_bandpass(plans, xf)  # STHT of the whole recording, the one launch's rows
                pre = pre[:, :, :T]
                # the stream's input: quadrature rows from the STHT, in-phase rows the filterbank output through the roll by L / 2
                h_in = h.clone()
                h_in[:, :M, :T] = torch.roll(xf, L2, dims=2).permute(0, 1, 3, 2).reshape(F * B, M, T)
                max_tile = max(max(t) for t in tilings)
                Ks = (max_tile + 2 * CH - 2) // CH
                nstate = lib.micloc_stream_complex_bands_state_bytes(hd, F, B)
                nws = lib.micloc_stream_complex_bands_workspace_bytes(hd, F, B, max_tile)
                ncoef = len(np.atleast_1d(filters[0][1]))
                assert nstate >= 256 + 8 * F * B * C * (CH + ncoef - 1) and nws >= 8 * F * B * C * Ks * CH and nstate % 256 == 0 and nws % 256 == 0
                state_buf, state = guarded(nstate, dev)
                ws_buf, ws = guarded(nws, dev)
                staging = ws[: 8 * F * B * C * Ks * CH].view(torch.float64).view(F * B, C, Ks * CH)
                s6 = (ctypes.c_int * 6)()
                for chains, tiles in itertools.product((16, 32, 64), tilings * 2):  # every tiling twice: the second stream starts from a reset
                    _lib.check(lib.micloc_stream_complex_bands_reset(hd, F, B, runtime._ptr(state), nstate, st()), "reset")
                    log = bookkeeping(tiles, CH)
                    t0 = fill = 0
                    for i, n in enumerate(tiles):
                        final = int(i == len(tiles) - 1)
                        _lib.check(lib.micloc_stream_complex_bands_bandpass_tile_f64(hd, F, runtime._ptr(h_in), B, n, Ts, t0, max_tile, chains,
                                                                                     runtime._ptr(state), nstate, runtime._ptr(ws), nws, st()), "bandpass_tile")
                        got = staging[:, :, : -(-(fill + n) // CH) * CH]
                        # (compared on the device, element by element: == lets the sign of a zero differ and nothing else)
                        assert bool((got[:, :, : fill + n] == pre[:, :, t0 - fill : t0 + n]).all()), \
                            f"B {B} M {M} T {T} chains {chains} tiles {tiles[:4]}.. tile {i}"
                        assert not bool(got[:, :, fill + n :].any())
                        _lib.check(lib.micloc_stream_complex_bands_localize_tile_f64(hd, F, runtime._ptr(state), nstate, B, max_tile, final, None, None,
                                                                                     None, runtime._ptr(ws), nws, st()), "localize_tile")
                        t0 += n
                        fill = log[i]["carry"]
                    _lib.check(lib.micloc_stream_complex_bands_status(runtime._ptr(state), None, s6, st()), "status")
                    assert list(s6) == [log[-1]["chunks"], T, 0, T, 0, 0]
                assert guards_intact(state_buf) and guards_intact(ws_buf)


def test_launcher_choice_is_one_of_the_forced_forms(torch):
    """chains_per_workgroup = 0 (the launcher's choice) gives the staging rows of the forced forms; more workgroups than one, the last
    chains of a band sharing a workgroup with the next band (3 x 5 x 14 = 210 chains)."""
    from haghighatshoarmuir2024_amd import _lib, runtime

    loc = random_localizer(7, 5, 1)
    plans = loc.plans()
    hd, F, B, T = _handles(plans), 3, 5, 700
    lib, dev = _lib.load(), plans[0].device
    st = runtime._stream(dev)
    h = torch.from_numpy(np.random.RandomState(4).randn(F * B, 14, 704)).to(dev)
    nstate = lib.micloc_stream_complex_bands_state_bytes(hd, F, B)
    nws = lib.micloc_stream_complex_bands_workspace_bytes(hd, F, B, T)
    state = torch.empty(nstate, dtype=torch.uint8, device=dev)
    rows = []
    for chains in (0, 16, 32, 64):
        ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
        _lib.check(lib.micloc_stream_complex_bands_reset(hd, F, B, runtime._ptr(state), nstate, st), "reset")
        _lib.check(lib.micloc_stream_complex_bands_bandpass_tile_f64(hd, F, runtime._ptr(h), B, T, 704, 0, T, chains, runtime._ptr(state), nstate,
                                                                     runtime._ptr(ws), nws, st), "bandpass_tile")
        rows.append(ws.clone())
    assert rows[0][: 8 * F * B * 14 * T].any()
    for r in rows[1:]:
        assert torch.equal(r, rows[0])


# ---- 2. finish() against the one-shot call ---------------------------------------------------------------------------------------------
def tilings_of(T, CH, seed):
    short = 100 if T > 100 else 1  # shorter than a chunk throughout
    out = [[T], [short] * (T // short) + ([T % short] if T % short else []), random_tiling(np.random.default_rng(seed), T, 2 * CH + 50)]
    return [t for i, t in enumerate(out) if t not in out[:i]]


@pytest.mark.parametrize("G", [1, 57, 112])
@pytest.mark.parametrize("M", [7, 9])  # the bf_mat-stationary contraction kernel (up to 8 microphones) and the general one
@pytest.mark.parametrize("F", [1, 3])
def test_finish_equals_localize_batch_bit_for_bit(F, M, G, torch):
    loc = random_localizer(M, G, 100 * F + 10 * M + G, BANDS3[:F])
    CH = loc.plans()[0].window_quantum()
    x_full = np.random.RandomState(F + M + G).randn(3, 4800, M)
    for B, T in itertools.product((1, 3), (1, 255, 256, 257, 1001, 4800)):
        x = np.ascontiguousarray(x_full[:B, :T])
        ref = loc.localize_batch(x, return_band_power=True)
        wrap = wrap_of(loc, x)
        for tiles in tilings_of(T, CH, T):
            s, out = stream(loc, x, tiles, wrap_tail=wrap)
            for k in ("band_power", "power", "argmax"):
                assert torch.equal(out[k], ref[k]), f"{k}: B {B} T {T} tiles {tiles[:5]}.."
            assert s.status() == dict(chunks=-(-T // CH), frames=T, carry=0, pushed=T, windows=0, band_sum_failures=0)


def test_push_replay_with_two_captured_tile_lengths(torch):
    loc = random_localizer(7, 112, 3)
    x = np.random.RandomState(3).randn(3, 4800, 7)
    ref = loc.localize_batch(x, return_band_power=True)
    tiles = [300] * 6 + [500] * 5 + [500]
    s, out = stream(loc, x, tiles, replay=True)
    assert sorted(s._graphs) == [300, 500]  # captured on their second occurrence, replayed from then on; the final tile is pushed eagerly
    for k in ("band_power", "power", "argmax"):
        assert torch.equal(out[k], ref[k]), k


# ---- 3. windows ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", [(1, 1), (2, 1), (4, 2)])
def test_windows_equal_the_one_shot_rows(wh, torch):
    """Every emitted row against the windows form of micloc_beamformer_pipeline_bands_f64, after every push: the count is the streaming
    rule's, an emitted row has its final bits, latest_* is the newest.  Tilings: one tile that completes every window at once (the ring
    depth's case), random tiles, tiles shorter than a chunk."""
    loc = random_localizer(7, 57, 17)
    CH = loc.plans()[0].window_quantum()
    window, hop = wh[0] * CH, wh[1] * CH
    B = 2
    for T in (CH, 3 * CH + 5, 4800):
        x = np.random.RandomState(T).randn(B, T, 7)
        ref = loc.localize_batch(x, window=window, hop=hop, return_band_power=True)
        whole = loc.localize_batch(x)
        nW = ref["window_power"].shape[1]
        wrap = wrap_of(loc, x)
        for tiles in ([T], random_tiling(np.random.default_rng(T), T, 700), [100] * (T // 100) + ([T % 100] if T % 100 else [])):
            s = loc.streaming_localizer(batch=B, total_frames=T, wrap_tail=wrap, max_tile=max(tiles), window=window, hop=hop)
            log = bookkeeping(tiles, CH, window, hop)
            t = before = 0
            for n, b in zip(tiles, log):
                s.push(x[:, t : t + n, :])
                t += n
                w = s.windows()
                assert w["count"] == b["windows"] and w["count"] - before <= ring_depth(max(tiles), CH, hop)
                before = w["count"]
                assert torch.equal(w["window_power"], ref["window_power"][:, : w["count"]])
                assert torch.equal(w["window_argmax"], ref["window_argmax"][:, : w["count"]])
                if w["count"]:
                    lp, la = s.latest_window()
                    assert torch.equal(lp, ref["window_power"][:, w["count"] - 1]) and torch.equal(la, ref["window_argmax"][:, w["count"] - 1])
            out = s.finish()
            assert out["window_count"] == nW and s.status()["band_sum_failures"] == 0
            assert torch.equal(out["window_power"], ref["window_power"]) and torch.equal(out["window_argmax"], ref["window_argmax"])
            assert torch.equal(out["power"], whole["power"]) and torch.equal(out["argmax"], whole["argmax"])
        if T == 4800:
            assert nW > 4  # [T] completed them all in one tile


def test_one_tile_completes_several_windows_and_the_output_ring_wraps(torch):
    """Tiles of five chunks and seven frames with hop = one chunk: every tile completes five or six windows at once, the final tile also the
    one cut at the end of the recording.  max_windows = 2: the two newest windows survive, window n in row n % 2, however many a tile
    completes.  The source is live (total_frames=None, final=True)."""
    from haghighatshoarmuir2024_amd import _lib

    loc = random_localizer(7, 57, 19)
    CH = loc.plans()[0].window_quantum()
    n = 5 * CH + 7
    T = 3 * n + 40
    x = np.random.RandomState(19).randn(2, T, 7)
    ref = loc.localize_batch(x, window=2 * CH, hop=CH)
    nW = ref["window_power"].shape[1]
    tiles = [n, n, n, 40]
    log = bookkeeping(tiles, CH, 2 * CH, CH)
    assert max(b["windows"] - a["windows"] for a, b in zip([dict(windows=0)] + log, log)) >= 5
    s = loc.streaming_localizer(batch=2, wrap_tail=wrap_of(loc, x), max_tile=n, window=2 * CH, hop=CH, max_windows=2)
    t = 0
    for i, k in enumerate(tiles):
        s.push(x[:, t : t + k, :], final=i == len(tiles) - 1)
        t += k
        w = s.windows()
        assert w["count"] == log[i]["windows"] and w["first"] == max(0, w["count"] - 2)
        assert torch.equal(w["window_power"], ref["window_power"][:, w["first"] : w["count"]])
        assert torch.equal(w["window_argmax"], ref["window_argmax"][:, w["first"] : w["count"]])
    out = s.finish()  # a live source: the max_windows newest
    assert out["window_count"] == nW and nW > 2
    assert torch.equal(out["window_power"], ref["window_power"][:, nW - 2 :])
    for k in (nW - 2, nW - 1):
        assert torch.equal(s.window_power[:, k % 2], ref["window_power"][:, k])
    # with total_frames the same ring is refused at the end
    s2 = loc.streaming_localizer(batch=2, total_frames=T, wrap_tail=wrap_of(loc, x), max_tile=T, window=2 * CH, hop=CH, max_windows=2)
    s2.push(x)
    with pytest.raises(_lib.MiclocError, match="max_windows"):
        s2.finish()
    # and the default ring holds every window, replayed: the same rows
    s3, out3 = stream(loc, x, [160] * 6 + [T - 960], replay=True, window=2 * CH, hop=CH)
    assert sorted(s3._graphs) == [160] and out3["window_count"] == nW
    assert torch.equal(out3["window_power"], ref["window_power"]) and torch.equal(out3["window_argmax"], ref["window_argmax"])


# ---- 4. the running read-out -------------------------------------------------------------------------------------------------------------
def test_running_readout(torch):
    """Mid stream each band's power is the running read-out of a ComplexStreamingLocalizer fed that band's filtered tiles, exactly, and
    power is the sequential band sum, exactly.  Against the one-shot result of the prefix -- a stream pushed with THE PREFIX'S OWN wrap
    rows -- the tolerance is the project's for a power reduced in another order (1e-12 relative)."""
    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

    loc = random_localizer(7, 57, 11)
    F, B, T = 3, 2, 1100
    x = np.random.RandomState(11).randn(B, T, 7)
    tiles = [100, 300, 300, 300, 100]
    CH = loc.plans()[0].window_quantum()
    log = bookkeeping(tiles, CH)
    filt = loc.filterbank.evolve_batch(x)  # [F, B, T, M]
    wrap = wrap_of(loc, x)
    s = loc.streaming_localizer(batch=B, total_frames=T, wrap_tail=wrap, max_tile=300)
    singles = [ComplexStreamingLocalizer(beamf, W, B, T, wrap_tail=wrap[f], max_tile=300) for f, (beamf, W) in enumerate(zip(loc.beamfs, loc.bf_mats))]
    t = 0
    for n, b in zip(tiles, log):
        power, argmax = s.push(x[:, t : t + n, :])
        total = None
        for f, one in enumerate(singles):
            p, _ = one.push(filt[f][:, t : t + n, :].contiguous())
            assert torch.equal(s.band_power[f], p), f"band {f} after {t + n} frames"
            total = p.cpu().numpy() if total is None else total + p.cpu().numpy()
        t += n
        np.testing.assert_array_equal(power.cpu().numpy(), total)
        np.testing.assert_array_equal(argmax.cpu().numpy(), np.argmax(total, axis=1))
        st = s.status()
        assert (st["chunks"], st["frames"], st["carry"], st["pushed"]) == (b["chunks"], b["frames"], b["carry"], t)
    # the prefix: the stream pushed with the prefix's own wrap rows
    checked = 0
    for k in range(len(tiles) - 1):
        frames = log[k]["frames"]
        if frames == 0:
            continue
        s = loc.streaming_localizer(batch=B, wrap_tail=wrap_of(loc, x[:, :frames, :]), max_tile=300)
        t = 0
        for n in tiles[: k + 1]:
            power, argmax = s.push(x[:, t : t + n, :], final=False)
            t += n
        ref = loc.localize_batch(np.ascontiguousarray(x[:, :frames, :]), return_band_power=True)
        np.testing.assert_allclose(power.cpu().numpy(), ref["power"].cpu().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(s.band_power.cpu().numpy(), ref["band_power"].cpu().numpy(), rtol=1e-12, atol=0)
        assert torch.equal(argmax, ref["argmax"])
        checked += 1
    assert checked == 3
    # before any chunk is complete: zeros
    s = loc.streaming_localizer(batch=B, max_tile=300)
    power, argmax = s.push(x[:, :100, :], final=False)
    assert not power.any() and not argmax.any() and not s.band_power.any()


# ---- 5. the reference's fixture ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup():
    """tests/test_hip_wideband_complex.py's configuration: the fixture's bands with the REFERENCE's matrices (no design run)."""
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
    return dict(c=c, demo=demo, loc=demo.localizer(), data=np.ascontiguousarray(packs[:, :, :-1], dtype=np.float64))


def test_reference_packs_pushed_in_four_tiles(setup, torch):
    """Each pack of tests/golden/wideband_complex_packs.npz as a stream of its own, a quarter of the pack per tile: the reference's pattern
    to rtol 1e-10, its arg-maxes 37, 97 and 48; and the one-shot call's bits."""
    c, loc, data = setup["c"], setup["loc"], setup["data"]
    assert c["doa_index"].tolist() == [37, 97, 48]
    for i, want in enumerate([37, 97, 48]):
        x = data[i : i + 1]
        _, out = stream(loc, x, [1200] * 4, replay=True)
        np.testing.assert_allclose(out["power"][0].cpu().numpy(), c["power_grid"][i], rtol=1e-10, atol=0)
        np.testing.assert_allclose(out["band_power"][:, 0].cpu().numpy(), c["band_power"][i], rtol=1e-10, atol=0)
        assert int(out["argmax"][0]) == want
        ref = loc.localize_batch(x)
        assert torch.equal(out["power"], ref["power"])


def test_demo_localizer_stream_gives_the_power_grid(setup, torch):
    """The stream reached from a Demo against Demo.power_grid on a pack: equal.  The route is demo.localizer().streaming_localizer():
    localization_demo.Demo has no streaming_localizer() of its own, because tests/test_wideband_complex_cpu.py pins its absence."""
    demo, data = setup["demo"], setup["data"]
    x = data[1:2]
    s = demo.localizer().streaming_localizer(batch=1, total_frames=4800, max_tile=1700, wrap_tail=wrap_of(setup["loc"], x))
    for t in (0, 1700, 3400):
        s.push(x[:, t : t + 1700, :])
    out = s.finish()
    want = demo.power_grid(x[0])
    np.testing.assert_array_equal(out["power"][0].cpu().numpy(), want)
    assert int(out["argmax"][0]) == int(np.argmax(want)) == 97


# ---- 6. status codes, ValueErrors, threads ---------------------------------------------------------------------------------------------
def test_status_codes(cfg2, torch):
    from haghighatshoarmuir2024_amd import _lib, runtime
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer
    from oracle import oracle as O

    lib = _lib.load()
    INV, NOT_SET, SHAPE, WSP, OK = _lib.MICLOC_ERR_INVALID, _lib.MICLOC_ERR_NOT_SET, _lib.MICLOC_ERR_SHAPE, _lib.MICLOC_ERR_WORKSPACE, _lib.MICLOC_OK
    loc = random_localizer(7, 57, 29)
    good = loc.plans()
    dev = good[0].device
    st = runtime._stream(dev)
    buf = torch.zeros(8 << 20, dtype=torch.uint8, device=dev)
    p, NB = runtime._ptr(buf), 8 << 20
    mis = ctypes.c_void_p(buf.data_ptr() + 8)
    CH = good[0].window_quantum()

    def every_entry(hd, F, B=2):
        """The status of every entry for plans that the rule refuses (sizes: 0)."""
        sizes = (lib.micloc_stream_complex_bands_state_bytes(hd, F, B), lib.micloc_stream_complex_bands_workspace_bytes(hd, F, B, 100),
                 lib.micloc_stream_complex_bands_window_state_bytes(hd, F, B, 100, CH, CH, 4))
        codes = (lib.micloc_stream_complex_bands_reset(hd, F, B, p, NB, st),
                 lib.micloc_stream_complex_bands_bandpass_tile_f64(hd, F, p, B, 100, 128, 0, 100, 0, p, NB, p, NB, st),
                 lib.micloc_stream_complex_bands_localize_tile_f64(hd, F, p, NB, B, 100, 0, None, p, p, p, NB, st),
                 lib.micloc_stream_complex_bands_window_reset(hd, F, B, 100, p, NB, CH, CH, 4, st),
                 lib.micloc_stream_complex_bands_localize_tile_windows_f64(hd, F, p, NB, B, 100, 0, None, p, p, p, NB, p, NB, CH, CH, 4, p, p, p, p, st))
        return sizes, set(codes)

    # a plan without bf_mat
    bare = Beamformer(CenterCircularArray(4.5e-2, 7), 10e-3, BANDS3[1], fs=FS)
    bare_plan = runtime.Plan(7, bare.kernel, *bare.bandpass_filter, 1, False)
    assert every_entry(_handles([good[0], bare_plan, good[2]]), 3) == ((0, 0, 0), {NOT_SET})
    # a real bf_mat belongs to the SNN stream
    real = runtime.Plan(7, cfg2["kernel"], cfg2["b"], cfg2["a"], 1, False)
    real.set_neuron_kernel(cfg2["nir"])
    real.set_bf_mat(cfg2["bf_mat"])
    assert every_entry(_handles([real]), 1) == ((0, 0, 0), {SHAPE})
    # plans that do not agree: microphones, DoA grid, Hilbert kernel, band-pass length
    rng = np.random.RandomState(1)
    other_m = random_localizer(9, 57, 30).plans()[0]
    other_g = random_localizer(7, 33, 31).plans()[0]
    other_k = runtime.Plan(7, O.stht_kernel(FS, 2e-3), *bare.bandpass_filter, 1, False)
    other_k.set_bf_mat(rng.randn(7, 57) + 1j * rng.randn(7, 57))
    from scipy.signal import butter

    other_n = runtime.Plan(7, bare.kernel, *butter(1, BANDS3[1], btype="bandpass", fs=FS), 1, False)
    other_n.set_bf_mat(rng.randn(7, 57) + 1j * rng.randn(7, 57))
    for odd in (other_m, other_g, other_k, other_n):
        assert every_entry(_handles([good[0], odd]), 2) == ((0, 0, 0), {SHAPE}), odd
    # good plans
    hd, F, B = _handles(good), 3, 2
    assert lib.micloc_stream_complex_bands_state_bytes(hd, F, 0) == 0 and lib.micloc_stream_complex_bands_state_bytes(hd, F, 30000) == 0  # F * B > 65535
    assert lib.micloc_stream_complex_bands_workspace_bytes(hd, F, B, 0) == 0
    nstate = lib.micloc_stream_complex_bands_state_bytes(hd, F, B)
    nws = lib.micloc_stream_complex_bands_workspace_bytes(hd, F, B, 100)
    one = good[0].lib.micloc_stream_complex_state_bytes(good[0].handle, F * B)
    assert nstate == one and 0 < nws <= NB and nstate % 256 == 0 and nws % 256 == 0  # the complex stream's layout for F * B rows
    rs = lib.micloc_stream_complex_bands_reset
    assert rs(hd, F, 0, p, nstate, st) == INV and rs(hd, F, B, None, nstate, st) == INV and rs(hd, F, 30000, p, NB, st) == INV
    assert rs(hd, F, B, p, nstate - 1, st) == WSP and rs(hd, F, B, mis, nstate, st) == WSP
    assert rs(hd, F, B, p, nstate, st) == OK
    bp = lib.micloc_stream_complex_bands_bandpass_tile_f64
    assert bp(hd, F, None, B, 100, 128, 0, 100, 0, p, nstate, p, nws, st) == INV
    assert bp(hd, F, p, B, 0, 128, 0, 100, 0, p, nstate, p, nws, st) == INV
    assert bp(hd, F, p, B, 100, 128, -1, 100, 0, p, nstate, p, nws, st) == INV
    assert bp(hd, F, p, B, 100, 128, 0, 100, 8, p, nstate, p, nws, st) == INV  # chains per workgroup: 0, 16, 32 or 64
    assert bp(hd, F, p, B, 101, 128, 0, 100, 0, p, nstate, p, nws, st) == SHAPE  # a tile longer than max_tile
    assert bp(hd, F, p, B, 100, 128, 40, 100, 0, p, nstate, p, nws, st) == SHAPE  # the tile leaves its rows
    assert bp(hd, F, p, B, 100, 128, 0, 100, 0, p, nstate - 256, p, nws, st) == WSP
    assert bp(hd, F, p, B, 100, 128, 0, 100, 0, p, nstate, p, nws - 256, st) == WSP
    assert bp(hd, F, p, B, 100, 128, 0, 100, 0, p, nstate, mis, nws, st) == WSP
    lt = lib.micloc_stream_complex_bands_localize_tile_f64
    assert lt(hd, F, None, nstate, B, 100, 0, None, p, p, p, nws, st) == INV and lt(hd, F, p, nstate, B, 0, 0, None, p, p, p, nws, st) == INV
    assert lt(hd, F, p, nstate, B, 100, 0, None, p, p, p, nws - 256, st) == WSP and lt(hd, F, p, nstate - 256, B, 100, 0, None, p, p, p, nws, st) == WSP
    # windows
    wsz, wrs = lib.micloc_stream_complex_bands_window_state_bytes, lib.micloc_stream_complex_bands_window_reset
    assert wsz(hd, F, B, 100, CH + 1, CH, 4) == 0 and wsz(hd, F, B, 100, CH, 2 * CH, 4) == 0 and wsz(hd, F, B, 100, CH, CH, 0) == 0
    assert wsz(hd, F, B, 0, CH, CH, 4) == 0
    nwst = wsz(hd, F, B, 100, 2 * CH, CH, 4)
    al = lambda v: v + (-v) % 256  # noqa: E731
    Kb = ring_depth(100, CH, CH)
    assert nwst == 256 + al(F * B * 2 * 2 * 57 * 8) + al(F * B * Kb * 57 * 8)  # head | two open windows per row | the bands' ring
    assert wrs(hd, F, B, 100, p, nwst, CH + 1, CH, 4, st) == SHAPE and wrs(hd, F, B, 100, p, nwst, CH, 2 * CH, 4, st) == SHAPE
    assert wrs(hd, F, B, 100, p, nwst, 0, CH, 4, st) == INV and wrs(hd, F, B, 100, None, nwst, 2 * CH, CH, 4, st) == INV
    assert wrs(hd, F, B, 100, p, nwst - 1, 2 * CH, CH, 4, st) == WSP and wrs(hd, F, B, 100, p, nwst, 2 * CH, CH, 4, st) == OK
    lw = lib.micloc_stream_complex_bands_localize_tile_windows_f64
    assert lw(hd, F, p, nstate, B, 100, 0, None, p, p, p, nws, None, nwst, 2 * CH, CH, 4, p, p, p, p, st) == INV  # no win_state
    assert lw(hd, F, p, nstate, B, 100, 0, None, p, p, p, nws, p, nwst, 2 * CH, CH, 4, p, None, p, p, st) == INV  # no window_argmax
    assert lw(hd, F, p, nstate, B, 100, 0, None, p, p, p, nws, p, nwst, 2 * CH, CH, 0, p, p, p, p, st) == INV
    assert lw(hd, F, p, nstate, B, 100, 0, None, p, p, p, nws, p, nwst, CH + 1, CH, 4, p, p, p, p, st) == SHAPE
    assert lw(hd, F, p, nstate, B, 100, 0, None, p, p, p, nws, p, nwst - 256, 2 * CH, CH, 4, p, p, p, p, st) == WSP
    torch.cuda.synchronize()
    # the Python surface
    with pytest.raises(ValueError, match="window quantum"):
        loc.streaming_localizer(batch=1, window=CH + 1)
    with pytest.raises(ValueError, match="hop <= window"):
        loc.streaming_localizer(batch=1, window=CH, hop=2 * CH)
    s = loc.streaming_localizer(batch=1, total_frames=300, max_tile=100)
    with pytest.raises(ValueError, match="max_tile"):
        s.push(np.zeros((1, 101, 7)))
    with pytest.raises(ValueError):
        s.push(np.zeros((1, 50, 6)))
    with pytest.raises(ValueError):
        s.latest_window()
    with pytest.raises(_lib.MiclocError, match="incomplete"):
        s.finish()


def test_two_host_threads_on_two_streams(torch):
    loc = random_localizer(7, 57, 31)
    rng = np.random.RandomState(31)
    xs = [rng.randn(2, 2000, 7) for _ in range(2)]
    tilings = [[700, 700, 600], [333] * 6 + [2]]
    serial = [stream(loc, x, t)[1] for x, t in zip(xs, tilings)]
    wraps = [wrap_of(loc, x) for x in xs]
    torch.cuda.synchronize()
    got, errors = [None, None], []

    def work(i):
        try:
            q = torch.cuda.Stream()
            with torch.cuda.stream(q):
                out = stream(loc, xs[i], tilings[i], wrap_tail=wraps[i])[1]
                got[i] = (out["power"].clone(), out["argmax"].clone(), out["band_power"].clone())
            q.synchronize()
        except Exception as e:  # surfaces in the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i in range(2):
        assert torch.equal(got[i][0], serial[i]["power"]) and torch.equal(got[i][1], serial[i]["argmax"]) and torch.equal(got[i][2], serial[i]["band_power"])
