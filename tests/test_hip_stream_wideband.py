"""Device tests of the wideband stream (streaming.WidebandStreamingLocalizer, csrc/filterbank.hip's filterbank_tile_kernel,
csrc/stream_bands.hip): a wideband recording pushed tile by tile gives the bits of WidebandSNNLocalizer.localize_batch on the whole
recording -- running power, band powers and windows -- whatever the tiling, eagerly or from a replayed graph.

Fixture: tests/golden/wideband_packs.npz, its three packs as B = 3, T = 4800, M = 7, F = 3, G = 112 (the configuration of
tests/test_hip_wideband.py, which pins the one-shot path to the reference)."""
import ctypes
import itertools

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

FS = 48_000
TILINGS = ([4800], [160] * 30, [16, 240, 1024, 48, 1600, 528, 16, 800, 528])
LIVE_AXIS = np.arange(FS) / FS  # a live source normalises the neuron kernel over 1 s


def _np(t):
    return t.cpu().numpy()


def _cut(tiles, T):
    """A tiling of 4800 frames cut to T: whole tiles while they fit, then the ragged rest."""
    out, t = [], 0
    for n in tiles:
        if t + n >= T:
            break
        out.append(n)
        t += n
    return out + [T - t]


def _sections(kind, F):
    """tests/test_hip_wideband.py's filter sections, restated: Butterworth band-passes of order 1, 2, 4 (n = 3, 5, 9) on F different
    bands, or random stable filters of n = 4 without a zero coefficient and with a[0] != 1."""
    from scipy.signal import butter

    if kind == "random":
        rng = np.random.RandomState(100 + F)
        out = []
        for _ in range(F):
            r, th, p = 0.3 + 0.6 * rng.rand(), np.pi * rng.rand(), 0.9 * (2 * rng.rand() - 1)
            a = np.convolve([1.0, -2 * r * np.cos(th), r * r], [1.0, -p]) * (1.5 + rng.rand())
            b = rng.randn(4) + 0.1
            out.append((b, a))
        return out
    return [butter(int(kind), [300.0 + 1200 * f, 1200.0 + 1200 * f], btype="bandpass", output="ba", fs=FS) for f in range(F)]


# ---- 1. the filterbank tile kernel ------------------------------------------------------------------------------------------------
GUARD, SENT, SGUARD = 256, -777.25, 4096  # doubles between the tiles' outputs; bytes around the state


def _filter_tiles(lib, sections, x, tiles, state_buf, nfb):
    """x [B, T, M] through micloc_filterbank_tile_f64 tile by tile -> [F, B, T, M] (host).  Every tile's output lies between guard
    regions of one buffer, the state between guard bytes of `state_buf`; both are checked."""
    import torch

    from haghighatshoarmuir2024_amd import _lib, runtime

    bb, aa, n = runtime.pad_ba_list(sections)
    F = len(sections)
    B, T, M = x.shape
    assert sum(tiles) == T
    dev = x.device
    buf = torch.full((F * B * T * M + (len(tiles) + 1) * GUARD,), SENT, dtype=torch.float64, device=dev)
    state = state_buf[SGUARD : SGUARD + nfb]
    assert state.data_ptr() % 256 == 0
    spans, off, t = [], GUARD, 0
    for nt in tiles:
        cnt = F * B * nt * M
        xt = x[:, t : t + nt, :].contiguous()
        _lib.check(lib.micloc_filterbank_tile_f64(runtime._dptr(bb), runtime._dptr(aa), F, n, runtime._ptr(xt), B, nt, M, runtime._ptr(state), nfb,
                                                  ctypes.c_void_p(buf.data_ptr() + 8 * off), runtime._stream(dev)), "filterbank_tile")
        spans.append((off, cnt, nt))
        off += cnt + GUARD
        t += nt
    host = buf.cpu().numpy()
    keep = np.ones(len(host), dtype=bool)
    parts = []
    for o, cnt, nt in spans:
        keep[o : o + cnt] = False
        parts.append(host[o : o + cnt].reshape(F, B, nt, M))
    assert np.all(host[keep] == SENT), "a tile wrote outside its output"
    sb = state_buf.cpu().numpy()
    assert np.all(sb[:SGUARD] == 0xA5) and np.all(sb[SGUARD + nfb :] == 0xA5), "the kernel wrote outside its state"
    return np.concatenate(parts, axis=2)


@pytest.mark.parametrize("kind", ["1", "2", "4", "random"])
def test_filterbank_tiles_equal_the_one_shot_call(kind):
    import torch

    from haghighatshoarmuir2024_amd import _lib, runtime

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    x_full = torch.from_numpy(np.random.RandomState(7).randn(3, 1001, 16)).to(dev)
    tilings = ([1001], [1] * 5 + [996], [7, 8, 9, 63, 64, 65, 785], [64] * 15 + [41])
    for B, M, F in itertools.product((1, 3), (1, 7, 16), (1, 3, 16)):
        sections = _sections(kind, F)
        ncoef = runtime.pad_ba_list(sections)[2]
        x = x_full[:B, :, :M].contiguous()
        want = _np(runtime.filterbank(sections, x, device=dev))
        nfb = lib.micloc_filterbank_stream_state_bytes(F, ncoef, B, M)
        assert nfb >= F * B * M * (ncoef - 1) * 8 and nfb % 256 == 0
        state_buf = torch.full((nfb + 2 * SGUARD,), 0xA5, dtype=torch.uint8, device=dev)
        first = None
        for tiles in tilings + ([7, 8, 9, 63, 64, 65, 785],):  # the last one again: a second stream after the reset entry, same bits
            _lib.check(lib.micloc_filterbank_stream_reset(ctypes.c_void_p(state_buf.data_ptr() + SGUARD), nfb, runtime._stream(dev)), "reset")
            got = _filter_tiles(lib, sections, x, tiles, state_buf, nfb)
            np.testing.assert_array_equal(got, want, err_msg=f"B={B} M={M} F={F} tiles={tiles[:4]}...")
            if tiles == tilings[2]:
                if first is None:
                    first = got
                else:
                    np.testing.assert_array_equal(got.view(np.int64), first.view(np.int64))
        # T = 1 as one tile
        _lib.check(lib.micloc_filterbank_stream_reset(ctypes.c_void_p(state_buf.data_ptr() + SGUARD), nfb, runtime._stream(dev)), "reset")
        got = _filter_tiles(lib, sections, x[:, :1, :].contiguous(), [1], state_buf, nfb)
        np.testing.assert_array_equal(got, want[:, :, :1, :], err_msg=f"T=1 B={B} M={M} F={F}")


# ---- the localizer ----------------------------------------------------------------------------------------------------------------
class _Fixture:
    """The fixture's configuration with the REFERENCE's matrices (tests/test_hip_wideband.py's set-up, restated), and the one-shot
    results every test compares against: computed once per case, read-only."""

    def __init__(self):
        from micloc.array_geometry import CenterCircularArray
        from micloc.filterbank import ButterworthFilterbank
        from micloc.localization_demo_snn import Demo
        from micloc.snn_beamformer import SNNBeamformer

        z = self.z = golden("wideband_packs.npz")
        geo = CenterCircularArray(4.5e-2, 7)
        demo = self.demo = Demo.__new__(Demo)
        demo.beamfs, demo.bf_mats = [], [np.ascontiguousarray(W) for W in z["bf_mats"]]
        for fr in z["freq_bands"]:
            tau = 1 / (2 * np.pi * np.mean(fr))
            demo.beamfs.append(SNNBeamformer(geometry=geo, kernel_duration=float(z["kernel_duration"]), freq_range=fr, tau_vec=[tau, tau],
                                             bipolar_spikes=True, fs=FS))
        demo.filterbank = ButterworthFilterbank(freq_bands=z["freq_bands"], order=1, fs=FS)
        demo.doa_list, demo.fs = z["doa_list"], FS
        demo.recording_duration, demo.kernel_duration = float(z["recording_duration"]), float(z["kernel_duration"])
        self.loc = demo.localizer()
        packs = z["packs16"].astype(np.int32) << int(z["shift"])
        self.x = np.ascontiguousarray(packs[:, :, :-1], dtype=np.float64)  # [3, 4800, 7]
        self.L2 = len(demo.beamfs[0].kernel) // 2
        assert self.L2 == 240
        self._one, self._tail = {}, {}

    def one(self, x, key, window=None, hop=None, live=False):
        k = (key, x.shape, window, hop, live)
        if k not in self._one:
            o = self.loc.localize_batch(x, time_vec=LIVE_AXIS if live else None, window=window, hop=hop, return_band_power=True)
            r = {n: _np(v) for n, v in o.items() if n in ("power", "argmax", "band_power", "window_power", "window_argmax")}
            for v in r.values():
                v.setflags(write=False)
            self._one[k] = r
        return self._one[k]

    def tail(self, x, key):
        """wrap_tail [F, B, L // 2, M]: the last L // 2 frames of every band's filtered recording."""
        k = (key, x.shape)
        if k not in self._tail:
            self._tail[k] = self.demo.filterbank.evolve_batch(x)[:, :, -self.L2 :, :].contiguous()
        return self._tail[k]

    def stream(self, x, key, known=True, **kw):
        from haghighatshoarmuir2024_amd.streaming import WidebandStreamingLocalizer

        return WidebandStreamingLocalizer(self.loc, x.shape[0], x.shape[1] if known else None, wrap_tail=self.tail(x, key), **kw)


@pytest.fixture(scope="module")
def fx():
    return _Fixture()


def _push_all(s, x, tiles):
    t = 0
    for n in tiles:
        s.push(x[:, t : t + n, :], final=t + n == x.shape[1])
        t += n
    assert t == x.shape[1]


# ---- 2. stream == one-shot ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", TILINGS, ids=["one", "160s", "irregular"])
def test_stream_equals_the_one_shot_call(fx, tiles):
    x, z = fx.x, fx.z
    one = fx.one(x, "golden")
    s = fx.stream(x, "golden", max_tile=max(tiles))
    _push_all(s, x, tiles)
    out = s.finish()
    assert "window_power" not in out and tuple(out["band_power"].shape) == (3, 3, 112)
    for key in ("power", "argmax", "band_power"):
        np.testing.assert_array_equal(_np(out[key]), one[key], err_msg=key)
    # the reference's pattern, to the tolerance tests/test_hip_wideband.py holds the one-shot path to
    np.testing.assert_allclose(_np(out["power"]), z["power_grid"], rtol=1e-10, atol=0)
    np.testing.assert_array_equal(_np(out["argmax"]), z["doa_index"])
    st = s.status()
    assert len(st["bands"]) == 3 and all(b["frames"] == 4800 and b["overflow"] == 0 and b["lag_failures"] == 0 for b in st["bands"])
    assert st["frames"] == 4800 and st["overflow"] == 0 and st["lag_failures"] == 0 and st["band_sum_failures"] == 0


# ---- 3. windows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4800, 1100, 1024])
@pytest.mark.parametrize("window,hop", [(1024, 512), (256, 256), (1024, 256)])
def test_stream_windows_equal_the_one_shot_rows(fx, window, hop, T):
    from haghighatshoarmuir2024_amd.utils import window_bounds

    x = np.ascontiguousarray(fx.x[:, :T, :])
    one_w, one = fx.one(x, "golden", window, hop), fx.one(x, "golden")
    nW = len(window_bounds(T, window, hop)[0])
    assert one_w["window_power"].shape == (3, nW, 112)
    if (window, hop, T) == (1024, 256, 1100):
        assert nW == 2
    plain = fx.stream(x, "golden", max_tile=T)
    plain.push(x)
    ref = plain.finish()
    for full in TILINGS:
        tiles = _cut(full, T)
        s = fx.stream(x, "golden", max_tile=max(tiles), window=window, hop=hop)
        msg = f"T={T} tiles={tiles[:4]}..."
        if full[0] == 160:  # the count after every push: never decreases, never ahead of the slowest band
            counts, t = [], 0
            for n in tiles:
                s.push(x[:, t : t + n, :], final=t + n == T)
                t += n
                c = s.windows()["count"]
                assert c <= min(b.windows()["count"] for b in s.bands), (msg, t)
                counts.append(c)
            assert counts == sorted(counts) and counts[-1] == nW, msg
        else:
            _push_all(s, x, tiles)
        out = s.finish()
        assert out["window_count"] == nW, msg
        np.testing.assert_array_equal(_np(out["window_power"]), one_w["window_power"], err_msg=msg)
        np.testing.assert_array_equal(_np(out["window_argmax"]), one_w["window_argmax"], err_msg=msg)
        for key in ("power", "argmax"):  # the running read-out is that of a stream built without `window`, and the one-shot call's
            np.testing.assert_array_equal(_np(out[key]), _np(ref[key]), err_msg=msg)
            np.testing.assert_array_equal(_np(out[key]), one[key], err_msg=msg)


# ---- 4. the band-sum kernel alone ---------------------------------------------------------------------------------------------------
def _ring(values, count, Kb):
    """A band's ring [B, Kb, G] once it has emitted `count` windows: window n in row n % Kb for the Kb newest, -1 in rows never written."""
    B, _, G = values.shape
    ring = np.full((B, Kb, G), -1.0)
    for n in range(max(0, count - Kb), count):
        ring[:, n % Kb, :] = values[:, n, :]
    return ring


@pytest.mark.parametrize("G", [1, 65, 449])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F", [1, 3])
def test_band_sum_kernel_alone(F, B, G):
    import torch

    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.runtime import _ptr, _stream

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    Kb, MW, NWIN, SENT_ROW = 4, 3, 8, -9.5
    rng = np.random.RandomState(1000 * F + 10 * B + G)
    vals = rng.rand(F, B, NWIN, G) * 10.0 ** rng.randint(-8, 8, size=(F, B, NWIN, G))  # magnitudes apart: the order of the additions shows
    run = rng.rand(F, B, G) * 10.0 ** rng.randint(-8, 8, size=(F, B, G))
    if G > 2:
        vals[:, 0, 0, :] = np.minimum(np.floor(vals[:, 0, 0, :] * 4) / 4, 1.0)  # window 0 of trial 0: exact sums with a tie, the first wins
        vals[:, 0, 0, G // 3] = 2.0
        vals[:, 0, 0, G - 1] = 2.0
        vals[0, B - 1, 1, 1] = np.nan  # a NaN column never wins
        run[0, 0, 2] = np.nan
    want_w = vals[0].copy()
    want_r = run[0].copy()
    for f in range(1, F):
        want_w = want_w + vals[f]
        want_r = want_r + run[f]
    arg = lambda rows: np.array([0 if np.all(np.isnan(r)) else int(np.nanargmax(r)) for r in rows.reshape(-1, G)]).reshape(rows.shape[:-1])

    nbs = lib.micloc_stream_bands_state_bytes()
    state = torch.empty(nbs, dtype=torch.uint8, device=dev)
    _lib.check(lib.micloc_stream_bands_reset(_ptr(state), nbs, _stream(dev)), "bands_reset")
    run_t = [torch.from_numpy(run[f]).to(dev) for f in range(F)]
    ring_t = [torch.full((B, Kb, G), -1.0, dtype=torch.float64, device=dev) for _ in range(F)]
    count_t = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(F)]
    vp = ctypes.c_void_p
    p_run, p_ring, p_count = ((vp * F)(*[t.data_ptr() for t in ts]) for ts in (run_t, ring_t, count_t))
    power = torch.full((B, G), SENT_ROW, dtype=torch.float64, device=dev)
    argmax = torch.full((B,), -7, dtype=torch.int32, device=dev)
    wp = torch.full((B, MW, G), SENT_ROW, dtype=torch.float64, device=dev)
    wa = torch.full((B, MW), -7, dtype=torch.int32, device=dev)
    lp = torch.full((B, G), SENT_ROW, dtype=torch.float64, device=dev)
    la = torch.full((B,), -7, dtype=torch.int32, device=dev)

    def launch(counts):
        for f in range(F):
            ring_t[f].copy_(torch.from_numpy(_ring(vals[f], counts[f], Kb)))
            count_t[f].fill_(counts[f])
        _lib.check(lib.micloc_stream_band_sum_f64(F, B, G, p_run, 1024, Kb, MW, p_ring, p_count, _ptr(state), nbs, _ptr(power), _ptr(argmax), _ptr(wp),
                                                  _ptr(wa), _ptr(lp), _ptr(la), _stream(dev)), "stream_band_sum")
        st2 = (ctypes.c_int * 2)()
        _lib.check(lib.micloc_stream_bands_status(_ptr(state), st2, _stream(dev)), "bands_status")
        return int(st2[0]), int(st2[1])

    exp_w, exp_a = np.full((B, MW, G), SENT_ROW), np.full((B, MW), -7)
    emitted = 0
    sequence = [(0, 0, 0), (2, 1, 3), (2, 1, 3), (4, 4, 3), (5, 5, 5)]  # (the last one wraps the output ring: windows 3, 4 -> rows 0, 1)
    n_new = []
    for counts in sequence:
        counts = counts[:F]
        e, fails = launch(counts)
        assert fails == 0 and e == min(counts), counts
        n_new.append(e - emitted)
        for n in range(emitted, e):
            exp_w[:, n % MW, :] = want_w[:, n, :]
            exp_a[:, n % MW] = arg(want_w[:, n, :])
        emitted = e
        # the rows emitted now are the sequential sum, the rows emitted before (and those never written) have not changed
        np.testing.assert_array_equal(_np(wp), exp_w, err_msg=str(counts))
        np.testing.assert_array_equal(_np(wa), exp_a, err_msg=str(counts))
        if emitted:
            np.testing.assert_array_equal(_np(lp), want_w[:, emitted - 1, :])
            np.testing.assert_array_equal(_np(la), arg(want_w[:, emitted - 1, :]))
        else:
            assert np.all(_np(lp) == SENT_ROW) and np.all(_np(la) == -7)  # untouched until the first window exists
        np.testing.assert_array_equal(_np(power), want_r)
        np.testing.assert_array_equal(_np(argmax), arg(want_r))
    if F == 3:
        assert n_new == [0, 1, 0, 2, 2]
    if G > 2:
        assert exp_a[0, 0] != G - 1 and arg(want_w[:, 0, :])[0] == G // 3  # the tie of window 0, checked when it was emitted
    # a band that leads by more than its ring: a fresh state, one window emitted, then band 0 runs to 6
    if F == 3:
        _lib.check(lib.micloc_stream_bands_reset(_ptr(state), nbs, _stream(dev)), "bands_reset")
        wp.fill_(SENT_ROW)
        wa.fill_(-7)
        assert launch((1, 1, 1)) == (1, 0)
        before_w, before_a, before_l = _np(wp).copy(), _np(wa).copy(), _np(lp).copy()
        e, fails = launch((6, 1, 1))
        assert fails > 0 and (e, fails) == (2, 1)  # window 1 is given up: band 0's row 1 holds window 5
        np.testing.assert_array_equal(_np(wp), before_w)
        np.testing.assert_array_equal(_np(wa), before_a)
        np.testing.assert_array_equal(_np(lp), before_l)
        assert np.all(before_w[:, 1:, :] == SENT_ROW)


# ---- 5. a live source ---------------------------------------------------------------------------------------------------------------
def test_live_source_equals_the_one_shot_call_on_the_live_axis(fx):
    x = fx.x
    one, one_w = fx.one(x, "golden", live=True), fx.one(x, "golden", 1024, 256, live=True)
    s = fx.stream(x, "golden", known=False, max_tile=400, window=1024, hop=256)
    assert s.windows()["count"] == 0 and not _np(s.latest_window()[0]).any()
    for k in range(12):
        s.push(x[:, 400 * k : 400 * (k + 1), :], final=k == 11)
    out = s.finish()
    for key in ("power", "argmax", "band_power"):
        np.testing.assert_array_equal(_np(out[key]), one[key], err_msg=key)
    assert out["window_count"] == one_w["window_power"].shape[1]
    np.testing.assert_array_equal(_np(out["window_power"]), one_w["window_power"])
    np.testing.assert_array_equal(_np(out["window_argmax"]), one_w["window_argmax"])


# ---- 6. graph replay ----------------------------------------------------------------------------------------------------------------
def test_push_replay_is_one_graph_per_tile_length(fx):
    import torch

    x = np.ascontiguousarray(np.concatenate([fx.x, fx.x[:, :399, :]], axis=1))  # twelve 400-frame tiles and a ragged final one
    one, one_w = fx.one(x, "looped", live=True), fx.one(x, "looped", 1024, 256, live=True)
    kw = dict(known=False, max_tile=400, window=1024, hop=256)
    a, g = fx.stream(x, "looped", **kw), fx.stream(x, "looped", **kw)
    xd = torch.from_numpy(x).cuda()
    for k in range(12):
        pa, aa = a.push(xd[:, 400 * k : 400 * (k + 1), :])
        pg, ag = g.push_replay(xd[:, 400 * k : 400 * (k + 1), :])
        assert torch.equal(pa, pg) and torch.equal(aa, ag), k
        assert all(torch.equal(u, v) for u, v in zip(a.latest_window(), g.latest_window())), k
        assert len(g._graphs) == (0 if k == 0 else 1), k  # first eager, second captured, the rest replayed
    assert a.status() == g.status()
    wa, wg = a.windows(), g.windows()
    assert wa["count"] == wg["count"] > 8 and torch.equal(wa["window_power"], wg["window_power"])
    assert list(g._graphs) == [400] and all(not b._graphs for b in g.bands)  # exactly one graph per tile length, none inside the bands
    a.push(xd[:, 4800:, :], final=True)
    g.push(xd[:, 4800:, :], final=True)  # the final tile is eager
    oa, og = a.finish(), g.finish()
    for key in ("power", "argmax", "band_power"):
        np.testing.assert_array_equal(_np(og[key]), one[key], err_msg=key)
        np.testing.assert_array_equal(_np(oa[key]), _np(og[key]), err_msg=key)
    for key in ("window_power", "window_argmax"):
        np.testing.assert_array_equal(_np(og[key]), one_w[key], err_msg=key)
        np.testing.assert_array_equal(_np(oa[key]), _np(og[key]), err_msg=key)


# ---- 7. a small ring ----------------------------------------------------------------------------------------------------------------
def test_small_ring_keeps_the_newest_windows_and_finish_refuses(fx):
    from haghighatshoarmuir2024_amd import _lib

    x = fx.x
    one_w = fx.one(x, "golden", 256, 256)
    assert one_w["window_power"].shape[1] == 19
    s = fx.stream(x, "golden", max_tile=1600, window=256, hop=256, max_windows=2)
    _push_all(s, x, [1600, 1600, 1600])
    w = s.windows()
    assert w["count"] == 19 and w["first"] == 17 and list(w["window_start"]) == [17 * 256, 18 * 256]
    np.testing.assert_array_equal(_np(w["window_power"]), one_w["window_power"][:, 17:19])
    np.testing.assert_array_equal(_np(w["window_argmax"]), one_w["window_argmax"][:, 17:19])
    np.testing.assert_array_equal(_np(s.latest_window()[0]), one_w["window_power"][:, 18])
    assert s.status()["band_sum_failures"] == 0
    with pytest.raises(_lib.MiclocError, match="max_windows"):
        s.finish()


# ---- 8. status codes and ValueErrors --------------------------------------------------------------------------------------------------
def test_status_codes_before_any_launch():
    import torch

    from haghighatshoarmuir2024_amd import _lib, runtime
    from haghighatshoarmuir2024_amd.runtime import _dptr, _ptr, _stream

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    F, B, n, M, G = 3, 1, 64, 7, 5
    bb, aa, nc = runtime.pad_ba_list(_sections("1", F))
    nfb = lib.micloc_filterbank_stream_state_bytes(F, nc, B, M)
    state = torch.full((nfb + 256,), 0x5A, dtype=torch.uint8, device=dev)
    x = torch.zeros((B, n, M), dtype=torch.float64, device=dev)
    xf = torch.full((F, B, n, M), -5.0, dtype=torch.float64, device=dev)

    def tile(b=bb, F_=F, nc_=nc, x_=x, n_=n, st=state, nbytes=nfb, out=xf):
        return lib.micloc_filterbank_tile_f64(_dptr(b), _dptr(aa), F_, nc_, _ptr(x_), B, n_, M, _ptr(st), nbytes, _ptr(out), _stream(dev))

    assert tile(F_=0) == tile(F_=17) == tile(nc_=0) == tile(nc_=10) == tile(n_=0) == _lib.MICLOC_ERR_INVALID
    assert tile(x_=None) == tile(out=None) == tile(st=None) == _lib.MICLOC_ERR_INVALID
    bad_a = aa.copy()
    bad_a[1, 0] = 0.0
    assert lib.micloc_filterbank_tile_f64(_dptr(bb), _dptr(bad_a), F, nc, _ptr(x), B, n, M, _ptr(state), nfb, _ptr(xf), _stream(dev)) == _lib.MICLOC_ERR_INVALID
    assert tile(nbytes=nfb - 1) == _lib.MICLOC_ERR_WORKSPACE
    assert tile(st=state[8:]) == _lib.MICLOC_ERR_WORKSPACE  # misaligned
    assert lib.micloc_filterbank_stream_reset(_ptr(state[8:]), nfb, _stream(dev)) == _lib.MICLOC_ERR_WORKSPACE
    assert lib.micloc_filterbank_stream_reset(None, nfb, _stream(dev)) == _lib.MICLOC_ERR_INVALID
    # the band sum
    nbs = lib.micloc_stream_bands_state_bytes()
    bst = torch.full((nbs + 256,), 0x5A, dtype=torch.uint8, device=dev)
    run = [torch.zeros((B, G), dtype=torch.float64, device=dev) for _ in range(F)]
    ring = [torch.zeros((B, 4, G), dtype=torch.float64, device=dev) for _ in range(F)]
    cnt = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(F)]
    vp = ctypes.c_void_p
    p_run, p_ring, p_cnt = ((vp * F)(*[t.data_ptr() for t in ts]) for ts in (run, ring, cnt))
    hole = (vp * F)(run[0].data_ptr(), None, run[2].data_ptr())
    power = torch.full((B, G), -5.0, dtype=torch.float64, device=dev)
    wa = torch.full((B, 3), -7, dtype=torch.int32, device=dev)

    def bsum(F_=F, pr=p_run, window=256, Kb=4, mw=3, rings=p_ring, counts=p_cnt, st=bst, nbytes=nbs, pw=power, wa_=wa):
        return lib.micloc_stream_band_sum_f64(F_, B, G, pr, window, Kb, mw, rings, counts, _ptr(st), nbytes, _ptr(pw), None, None, _ptr(wa_), None, None,
                                              _stream(dev))

    I, W = _lib.MICLOC_ERR_INVALID, _lib.MICLOC_ERR_WORKSPACE
    assert bsum(F_=0) == bsum(F_=17) == bsum(pr=None) == bsum(pr=hole) == bsum(st=None) == bsum(pw=None) == I
    assert bsum(mw=0) == bsum(Kb=0) == bsum(rings=None) == bsum(counts=None) == bsum(rings=hole) == bsum(wa_=None) == bsum(window=-1) == I
    assert bsum(nbytes=nbs - 1) == bsum(st=bst[8:]) == W
    assert lib.micloc_stream_bands_reset(_ptr(bst[8:]), nbs, _stream(dev)) == W
    torch.cuda.synchronize()
    assert np.all(_np(xf) == -5.0) and np.all(_np(power) == -5.0) and np.all(_np(wa) == -7)
    assert np.all(_np(state) == 0x5A) and np.all(_np(bst) == 0x5A)


def test_argument_errors_are_value_errors(fx):
    from micloc.filterbank import ButterworthFilterbank
    from micloc.streaming import WidebandStreamingLocalizer
    from micloc.wideband import WidebandSNNLocalizer

    x, loc = fx.x, fx.loc
    for kw, match in ((dict(window=1000), "quantum"), (dict(window=1024, hop=100), "quantum"), (dict(window=1024, hop=2048), "hop <= window"),
                      (dict(hop=256), "window"), (dict(window=1024, max_windows=0), "max_windows")):
        with pytest.raises(ValueError, match=match):
            fx.stream(x, "golden", **kw)
    with pytest.raises(ValueError, match="wrap_tail"):
        WidebandStreamingLocalizer(loc, 3, 4800, wrap_tail=np.zeros((3, 240, 7)))
    with pytest.raises(ValueError, match="wrap_tail"):
        WidebandStreamingLocalizer(loc, 3, 4800, wrap_tail=np.zeros((3, 2, 240, 7)))
    many = WidebandSNNLocalizer.__new__(WidebandSNNLocalizer)  # (its own constructor refuses 17 bands)
    bands17 = [[1000.0 + 100 * i, 1100.0 + 100 * i] for i in range(17)]
    many.beamfs, many.bf_mats, many.filterbank = [loc.beamfs[0]] * 17, [loc.bf_mats[0]] * 17, ButterworthFilterbank(freq_bands=bands17, order=1, fs=FS)
    many.num_mic, many.num_grid = 7, 112
    with pytest.raises(ValueError, match="bands"):
        WidebandStreamingLocalizer(many, 1, 4800)
    s = fx.stream(x, "golden")
    with pytest.raises(ValueError, match="window"):
        s.latest_window()
    with pytest.raises(ValueError):
        s.push(np.zeros((3, 160, 5)))  # the input's microphones


# ---- 9. the demo ----------------------------------------------------------------------------------------------------------------------
def test_demo_streaming_localizer_gives_the_power_grid(fx):
    """The stream normalises the neuron kernel over the T frames it was told, on np.arange(T) / fs -- Demo.power_grid's own time axis --
    so one pack as one tile is power_grid's pattern bit for bit (the issue's 1e-10 holds a fortiori)."""
    x = np.ascontiguousarray(fx.x[:1])
    want = fx.demo.power_grid(x[0])
    s = fx.demo.streaming_localizer(batch=1, total_frames=4800, max_tile=4800, wrap_tail=fx.tail(x, "pack0"))
    s.push(x)
    out = s.finish()
    np.testing.assert_allclose(_np(out["power"])[0], want, rtol=1e-10, atol=0)
    np.testing.assert_array_equal(_np(out["power"])[0], want)
    assert int(out["argmax"][0]) == int(np.argmax(want))
