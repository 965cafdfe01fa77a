"""The tracked wideband streams on the MI355X (csrc/stream_track_bands.hip behind micloc_stream_bands_track_tile_f64 and
micloc_stream_complex_bands_localize_tile_track_f64; the rule: include/micloc_hip.h "wideband streaming, tracking"; streaming.py track=).
Every comparison is bit for bit -- there is no tolerance in this file.  The reference is the wideband localizer's track_batch on the whole
recording (pinned by tests/test_hip_track_bands.py); localizers and signal are built as that file builds them (three bands, 7 microphones,
seeded matrices, a tone in every band plus noise), the wrap rows as tests/test_hip_stream_wideband*.py build them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 48_000
BANDS = [[1000.0, 1600.0], [1600.0, 2400.0], [2400.0, 3400.0]]
KEYS = (("track_index", "index"), ("track_peak_envelope", "peak_envelope"), ("envelope_last", "envelope_last"))
KINDS = ("snn", "complex")
OUT_OF_STEP_SEED = 0  # the signal of test 5, chosen on the device: with every seed 0 .. 9 the bands' frames differ after 7 or 8 of the 129 pushes


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _env():
    from haghighatshoarmuir2024_amd.utils import Envelope

    return Envelope(rise_time=2e-3, fall_time=13e-3, fs=FS)


def _loc(kind, F, G, M=7, seed=0):
    """tests/test_hip_track_bands.py's _loc: F bands with seeded random matrices; the SNN bands have tau = 1 / (2 pi f_mid)."""
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.beamformer import Beamformer
    from haghighatshoarmuir2024_amd.filterbank import ButterworthFilterbank
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer
    from haghighatshoarmuir2024_amd.wideband import WidebandBeamformerLocalizer, WidebandSNNLocalizer

    geo = CenterCircularArray(4.5e-2, M)
    bands = BANDS[:F]
    rng = np.random.RandomState(1000 * F + G + 17 * M + seed)
    if kind == "snn":
        beamfs = [SNNBeamformer(geo, 10e-3, fr, np.asarray([1 / (2 * np.pi * np.mean(fr))] * 2), bipolar_spikes=True, fs=FS) for fr in bands]
        Ws = []
        for _ in bands:
            W = rng.randn(2 * M, G)
            Ws.append(W / np.linalg.norm(W, axis=0, keepdims=True))
        loc = WidebandSNNLocalizer(beamfs, Ws, ButterworthFilterbank(freq_bands=np.asarray(bands), order=1, fs=FS))
    else:
        beamfs = [Beamformer(geo, 10e-3, fr, fs=FS) for fr in bands]
        Ws = [(rng.randn(M, G) + 1j * rng.randn(M, G)) / np.sqrt(2 * M) for _ in bands]
        loc = WidebandBeamformerLocalizer(beamfs, Ws, ButterworthFilterbank(freq_bands=np.asarray(bands), order=2, fs=FS))
    loc.doa_list = np.linspace(-np.pi, np.pi, G)
    return loc


def _signal(rng, B, T, M):
    """B trials [T, M]: a tone inside every band plus noise, each microphone with its own phase."""
    t = np.arange(T) / FS
    x = 0.5 * rng.randn(B, T, M)
    for fr in BANDS:
        x += np.sin(2 * np.pi * np.mean(fr) * t[None, :, None] + rng.uniform(0, 2 * np.pi, size=(B, 1, M)))
    return x


def _wrap(loc, x):
    """wrap_tail [F, B, L // 2, M]: the last L // 2 frames of every band's FILTERED recording -- for a recording shorter than that,
    np.roll's rows zero padded (wrap_rows)."""
    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

    L = len(loc.beamfs[0].kernel)
    filt = loc.filterbank.evolve_batch(np.ascontiguousarray(x))
    if x.shape[1] >= L // 2:
        return filt[:, :, -(L // 2) :, :].contiguous()
    return np.stack([ComplexStreamingLocalizer.wrap_rows(f.cpu().numpy(), L) for f in filt])


class _Cases:
    """Localizers, signals and the one-shot reference, each made once and left unchanged."""

    def __init__(self):
        self._locs, self._x, self._one = {}, {}, {}
        self.env = _env()

    def loc(self, kind, F, G, M=7):
        key = (kind, F, G, M)
        if key not in self._locs:
            self._locs[key] = _loc(kind, F, G, M)
        return self._locs[key]

    def x(self, B, T, M=7, seed=0):
        key = (B, T, M, seed)
        if key not in self._x:
            x = _signal(np.random.RandomState(77 + seed), B, T, M)
            x.setflags(write=False)
            self._x[key] = x
        return self._x[key]

    def one(self, kind, F, G, B, T, M=7, seed=0, live=False):
        """loc.track_batch on the whole recording.  live: the SNN neuron kernels of a live source, normalised over 1 s."""
        key = (kind, F, G, B, T, M, seed, live)
        if key not in self._one:
            tv = np.arange(FS) / FS if live else None
            o = self.loc(kind, F, G, M).track_batch(self.x(B, T, M, seed), self.env, time_vec=tv, want_envelope_last=True)
            r = {k: _np(o[k]) for k in ("index", "peak_envelope", "envelope_last")}
            for v in r.values():
                v.setflags(write=False)
            self._one[key] = r
        return self._one[key]

    def stream(self, kind, loc, x, known=True, track=True, **kw):
        from haghighatshoarmuir2024_amd.streaming import WidebandComplexStreamingLocalizer, WidebandStreamingLocalizer

        cls = WidebandStreamingLocalizer if kind == "snn" else WidebandComplexStreamingLocalizer
        if track:
            kw["track"] = self.env
        return cls(loc, x.shape[0], x.shape[1] if known else None, wrap_tail=_wrap(loc, x), **kw)


@pytest.fixture(scope="module")
def cs(torch):
    return _Cases()


def _push_all(s, x, tiles):
    t = 0
    for n in tiles:
        s.push(x[:, t : t + n, :], final=t + n == x.shape[1])
        t += n
    assert t == x.shape[1]


def _even(T, n):
    k = (T - 1) // n
    return [n] * k + [T - n * k]


def _random(T, seed, lo, hi, mult):
    rng = np.random.RandomState(seed)
    tiles, t = [], 0
    while t < T:
        n = mult * int(rng.randint(lo, hi + 1))
        tiles.append(min(n, T - t))
        t += tiles[-1]
    return tiles


def _assert_finish(out, one, msg):
    for got, want in KEYS:
        np.testing.assert_array_equal(_np(out[got]), one[want], err_msg=f"{got} {msg}")


def _run(cs, kind, F, G, B, T, tiles, M=7, **kw):
    loc, x = cs.loc(kind, F, G, M), cs.x(B, T, M)
    s = cs.stream(kind, loc, x, max_tile=max(tiles), **kw)
    _push_all(s, x, tiles)
    out = s.finish()
    assert out["track_count"] == T and s.status()["tracked"] == T
    _assert_finish(out, cs.one(kind, F, G, B, T, M), f"{kind} F={F} G={G} T={T} tiles={tiles[:4]}...")
    return s, out


# ---- 1. parity for any tiling ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tiling", [("snn", "one"), ("snn", "160"), ("snn", "random16"), ("complex", "one"), ("complex", "160"), ("complex", "random")])
def test_three_bands_equal_track_batch_for_any_tiling(cs, kind, tiling):
    T = 4799
    tiles = {"one": [T], "160": _even(T, 160), "random16": _random(T, 11, 1, 75, 16), "random": _random(T, 23, 1, 997, 1)}[tiling]
    assert tiling != "random" or any(n % 2 for n in tiles)
    s, out = _run(cs, kind, 3, 449, 3, T, tiles)
    band_power = _np(out["band_power"])
    assert band_power.shape == (3, 3, 449) and all(np.any(band_power[f] != 0) for f in range(3))  # the sum over the bands is not vacuous


# ---- 2. band counts, and one band against the single-plan tracked stream -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", [1, 2])
def test_band_counts_and_one_band_equals_the_single_plan_stream(cs, kind, F):
    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer, StreamingLocalizer

    T, G = 1001, 449
    tiles = _even(T, 16)
    _, out = _run(cs, kind, F, G, 1, T, tiles)
    if F == 1:
        loc, x = cs.loc(kind, 1, G), cs.x(1, T)
        filt, wrap = loc.filterbank.evolve_batch(np.ascontiguousarray(x)), _wrap(loc, x)
        cls = StreamingLocalizer if kind == "snn" else ComplexStreamingLocalizer
        single = cls(loc.beamfs[0], loc.bf_mats[0], 1, T, wrap_tail=wrap[0], max_tile=16, track=cs.env)
        _push_all(single, filt[0], tiles)
        so = single.finish()
        for k, _ in KEYS:
            np.testing.assert_array_equal(_np(out[k]), _np(so[k]), err_msg=f"{kind} {k}")


# ---- 3. column groups: the kernel writes the ring itself (G <= 64) / the pairs and the combine (G = 65) ------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G", [1, 64, 65])
def test_column_group_edges(cs, kind, G):
    T = 1001
    _run(cs, kind, 2, G, 1, T, _even(T, 160) if kind == "snn" else _random(T, 5, 1, 300, 1))


# ---- 4. short and ragged recordings: state_0 at frame 0, spans that stay empty for many tiles, the ragged last chunk -----------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", [2, 15, 209, 1001])
def test_short_and_ragged_recordings(cs, kind, T):
    for tiles in ([T], _even(T, 16)):
        _run(cs, kind, 2, 65, 1, T, tiles)


# ---- 5. SNN bands out of step ------------------------------------------------------------------------------------------------------------
def test_snn_bands_out_of_step_track_the_joint_frontier(cs):
    """Tiles of 16 frames: the bands' horizons finish chunks at different pushes.  After every push the device's frontier word equals the
    host rule on the bands' committed chunks (and the smallest of their frames), and the rows emitted so far are the reference's."""
    from haghighatshoarmuir2024_amd.streaming import bands_track_span

    F, B, T, G = 3, 2, 2064, 449
    loc = cs.loc("snn", F, G)
    x = _signal(np.random.RandomState(77 + OUT_OF_STEP_SEED), B, T, 7)
    one = {k: _np(v) for k, v in loc.track_batch(x, cs.env, want_envelope_last=True).items() if v is not None}
    s = cs.stream("snn", loc, x, max_tile=16)
    unequal, prev, t = 0, 0, 0
    for n in _even(T, 16):
        s.push(x[:, t : t + n, :], final=t + n == T)
        t += n
        st = s.status()
        frames = [b["frames"] for b in st["bands"]]
        first, last = bands_track_span(prev, [b["chunks"] for b in st["bands"]], s.CH, t)
        assert first == prev and last == st["tracked"] == min(frames), (t, frames, st["tracked"])
        unequal += len(set(frames)) > 1
        if last > prev or t == T:
            w = s.tracked()
            assert w["count"] == last and w["first"] == 0
            np.testing.assert_array_equal(_np(w["index"]), one["index"][:, :last], err_msg=f"t={t}")
            np.testing.assert_array_equal(_np(w["peak_envelope"]), one["peak_envelope"][:, :last], err_msg=f"t={t}")
        prev = last
    assert prev == T and unequal > 0, "no push saw the bands out of step: the test does not exercise the frontier"
    _assert_finish(s.finish(), one, "out of step")


# ---- 6. the complex channel table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", range(1, 9))
def test_every_row_of_the_complex_channel_table(cs, M):
    T = 1001
    _run(cs, "complex", 2, 57, 1, T, _random(T, 31 + M, 1, 300, 1), M=M)


# ---- 7. a live source, the ring, truncation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_live_source_with_the_smallest_ring_keeps_the_newest_rows(cs, kind):
    F, G, T, n = 3, 449, 4799, 1600 if kind == "snn" else 997
    loc, x = cs.loc(kind, F, G), cs.x(1, T)
    one = cs.one(kind, F, G, 1, T, live=True)
    kw = dict(known=False, max_tile=n, **(dict(lag_frames=1024) if kind == "snn" else {}))
    R = cs.stream(kind, loc, x, **kw).min_track
    assert R < T and R == (n if kind == "complex" else R)  # the ring wraps
    with pytest.raises(ValueError, match="max_track"):
        cs.stream(kind, loc, x, max_track=R - 1, **kw)
    s = cs.stream(kind, loc, x, max_track=R, **kw)
    assert s.max_track == R and s.tracked()["count"] == 0
    for t in range(0, T, n):
        s.push(x[:, t : t + n, :], final=t + n >= T)
        w, frames = s.tracked(), s.status()["tracked"]
        assert w["count"] == frames and w["first"] == max(0, frames - R)
        np.testing.assert_array_equal(_np(w["index"]), one["index"][:, w["first"] : frames], err_msg=f"t={t}")
        np.testing.assert_array_equal(_np(w["peak_envelope"]), one["peak_envelope"][:, w["first"] : frames], err_msg=f"t={t}")
        if frames:
            li, lp = s.latest_track()
            np.testing.assert_array_equal(_np(li), one["index"][:, frames - 1])
            np.testing.assert_array_equal(_np(lp), one["peak_envelope"][:, frames - 1])
    out = s.finish()
    assert out["track_count"] == T and tuple(out["track_index"].shape) == (1, R)
    np.testing.assert_array_equal(_np(out["track_index"]), one["index"][:, T - R :])
    np.testing.assert_array_equal(_np(out["envelope_last"]), one["envelope_last"])


@pytest.mark.parametrize("kind", KINDS)
def test_finish_refuses_a_truncated_array(cs, kind):
    from haghighatshoarmuir2024_amd import _lib

    T, n = 4799, 1600 if kind == "snn" else 997
    loc, x = cs.loc(kind, 3, 449), cs.x(1, T)
    kw = dict(max_tile=n, **(dict(lag_frames=1024) if kind == "snn" else {}))
    s = cs.stream(kind, loc, x, max_track=cs.stream(kind, loc, x, **kw).min_track, **kw)
    _push_all(s, x, _even(T, n))
    with pytest.raises(_lib.MiclocError, match="max_track"):
        s.finish()


# ---- 8. tracking beside the windows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_tracking_beside_the_windowed_read_out(cs, kind):
    F, G, B, T, window, hop = 3, 449, 3, 4799, 1024, 512
    loc, x = cs.loc(kind, F, G), cs.x(B, T)
    tiles = _even(T, 1200)
    p = cs.stream(kind, loc, x, track=False, max_tile=1200, window=window, hop=hop)
    _push_all(p, x, tiles)
    ref = p.finish()
    assert "track_index" not in ref and p.track is None
    with pytest.raises(ValueError, match="track"):
        p.tracked()
    s = cs.stream(kind, loc, x, max_tile=1200, window=window, hop=hop)
    _push_all(s, x, tiles)
    out = s.finish()
    assert out["window_count"] == ref["window_count"] > 0
    for k in ("power", "argmax", "band_power", "window_power", "window_argmax"):
        np.testing.assert_array_equal(_np(out[k]), _np(ref[k]), err_msg=k)
    _assert_finish(out, cs.one(kind, F, G, B, T), "with windows")


# ---- 9. graph replay -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_push_replay_is_one_graph_launch_per_tile(cs, kind, monkeypatch):
    import torch

    F, G, T, n = 3, 449, 4799, 800
    loc, x = cs.loc(kind, F, G), cs.x(1, T)
    one = cs.one(kind, F, G, 1, T, live=True)
    kw = dict(known=False, max_tile=n, max_track=4800, **(dict(lag_frames=1024) if kind == "snn" else {}))  # (a ring that keeps every row)
    a, g = cs.stream(kind, loc, x, **kw), cs.stream(kind, loc, x, **kw)
    calls = dict(tile=0, replay=0)
    tile0, replay0 = g._tile, torch.cuda.CUDAGraph.replay

    def counted_tile(*args):
        calls["tile"] += 1
        return tile0(*args)

    def counted_replay(self):
        calls["replay"] += 1
        return replay0(self)

    g._tile = counted_tile
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counted_replay)
    xd = torch.from_numpy(x).cuda()
    tiles = T // n
    for k in range(tiles):
        before = dict(calls)
        a.push(xd[:, k * n : (k + 1) * n, :])
        g.push_replay(xd[:, k * n : (k + 1) * n, :])
        if k >= 2:
            assert calls["tile"] == before["tile"] and calls["replay"] == before["replay"] + 1, k
        assert a.status() == g.status(), k
        wa, wg = a.tracked(), g.tracked()
        assert wa["count"] == wg["count"] and torch.equal(wa["index"], wg["index"]) and torch.equal(wa["peak_envelope"], wg["peak_envelope"]), k
        assert all(torch.equal(u, v) for u, v in zip(a.latest_track(), g.latest_track())), k
    assert calls == dict(tile=2, replay=tiles - 1) and list(g._graphs) == [n] and wg["count"] > 0
    a.push(xd[:, tiles * n :, :], final=True)
    g.push(xd[:, tiles * n :, :], final=True)
    oa, og = a.finish(), g.finish()
    assert og["track_count"] == T
    _assert_finish(og, one, "replay")
    _assert_finish(oa, one, "push")


# ---- 10. a band's lag failure --------------------------------------------------------------------------------------------------------------
def test_lag_failure_makes_finish_raise_and_no_emitted_row_is_wrong(cs):
    """A raster window too short for the frames the open clusters hold back (a tiny lag_frames, digital silence in the input): the band's
    done count stops, the frontier with it; what was emitted before is the reference's."""
    from haghighatshoarmuir2024_amd import _lib

    F, G, T = 2, 65, 9600
    loc = cs.loc("snn", F, G)
    x = _signal(np.random.RandomState(5), 1, T, 7)
    x[0, 1000:7000, :] = 0.0
    one = loc.track_batch(x, cs.env)
    s = cs.stream("snn", loc, x, max_tile=800, lag_frames=256)
    for t in range(0, T, 800):
        s.push(x[:, t : t + 800, :])
    st = s.status()
    assert st["lag_failures"] > 0 and st["frames"] < T and st["tracked"] <= st["frames"]
    with pytest.raises(_lib.MiclocError, match="window"):
        s.finish()
    w = s.tracked()
    assert w["count"] == st["tracked"] > 0 and w["first"] == 0
    np.testing.assert_array_equal(_np(w["index"]), _np(one["index"])[:, : w["count"]])
    np.testing.assert_array_equal(_np(w["peak_envelope"]), _np(one["peak_envelope"])[:, : w["count"]])


# ---- 11. argument errors and sets that are not served ----------------------------------------------------------------------------------------
def test_argument_errors_of_the_entries_are_status_codes_before_any_launch(cs, torch):
    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.runtime import _ptr, _stream

    lib = _lib.load()
    T, G = 1001, 449
    x = cs.x(1, T)
    s = cs.stream("snn", cs.loc("snn", 2, G), x, max_tile=160)
    c = cs.stream("complex", cs.loc("complex", 2, G), x, max_tile=100)
    for o in (s, c):
        o.track_index.fill_(-7)
    assert lib.micloc_stream_bands_track_state_bytes(s.handles, 2, 1) == s.ntst == 256 + 8 * 64 * 8
    assert lib.micloc_stream_bands_track_state_bytes(c.handles, 2, 1) == c.ntst == 256 + 8 * 64 * 8
    assert lib.micloc_stream_bands_track_state_bytes(s.handles, 2, 0) == 0 and lib.micloc_stream_bands_track_state_bytes(s.handles, 0, 1) == 0
    assert lib.micloc_stream_bands_track_workspace_bytes(s.handles, 2, 1, 0) == 0
    assert lib.micloc_stream_bands_track_workspace_bytes(s.handles, 2, 1, s.cap + 16) == 0  # no multiple of the chunk length

    def snn(handles=None, state=True, ws_bytes=None, R=None, cap=None, loc_states=True):
        return lib.micloc_stream_bands_track_tile_f64(
            handles or s.handles, 2, s._p_loc if loc_states else None, s._p_win, 1, s.cap if cap is None else cap, _ptr(s.tst) if state else None, s.ntst,
            *s.track, s.max_track if R is None else R, _ptr(s.track_index), _ptr(s.track_peak), _ptr(s.latest_index), _ptr(s.latest_peak), _ptr(s.tws),
            s.ntws if ws_bytes is None else ws_bytes, _stream(s.device))

    def cpx(handles=None, state=True, ws_bytes=None, R=None):
        return lib.micloc_stream_complex_bands_localize_tile_track_f64(
            handles or c.handles, 2, _ptr(c.state), c.nstate, 1, c.max_tile, 0, _ptr(c.band_power), _ptr(c.power), _ptr(c.argmax), _ptr(c.ws), c.nws,
            None, 0, 0, 0, 0, None, None, None, None, _ptr(c.tst) if state else None, c.ntst, *c.track, c.max_track if R is None else R,
            _ptr(c.track_index), _ptr(c.track_peak), _ptr(c.latest_index), _ptr(c.latest_peak), _ptr(c.tws), c.ntws if ws_bytes is None else ws_bytes,
            _stream(c.device))

    INV, SHAPE, WS = _lib.MICLOC_ERR_INVALID, _lib.MICLOC_ERR_SHAPE, _lib.MICLOC_ERR_WORKSPACE
    assert s.ntws > 256 and c.ntws > 256  # eight column groups: the pair scratch is real
    assert snn(R=s.cap - 1) == SHAPE and cpx(R=c.max_tile - 1) == SHAPE  # a ring one tile can overrun
    assert snn(state=False) == INV and cpx(state=False) == INV and snn(loc_states=False) == INV
    assert snn(ws_bytes=s.ntws - 1) == WS and cpx(ws_bytes=c.ntws - 1) == WS
    assert snn(handles=c.handles) == SHAPE and cpx(handles=s.handles) == SHAPE  # a set of the other kind
    assert snn(cap=s.cap + 16) == SHAPE  # window_frames that is no multiple of the chunk length
    assert lib.micloc_stream_bands_track_reset(s.handles, 2, 1, _ptr(s.tst), s.ntst - 1, _stream(s.device)) == WS
    assert lib.micloc_stream_bands_track_reset(s.handles, 2, 1, None, s.ntst, _stream(s.device)) == INV
    torch.cuda.synchronize()
    for o in (s, c):
        assert int((o.track_index != -7).sum()) == 0 and o.status()["tracked"] == 0  # nothing was launched
    # the objects still work
    _push_all(s, x, _even(T, 160))
    _assert_finish(s.finish(), cs.one("snn", 2, G, 1, T), "after the refusals")
    _push_all(c, x, _even(T, 100))
    _assert_finish(c.finish(), cs.one("complex", 2, G, 1, T), "after the refusals")


@pytest.mark.parametrize("kind", KINDS)
def test_a_set_the_fused_kernels_do_not_serve_is_refused(cs, kind):
    from haghighatshoarmuir2024_amd import _lib, runtime

    loc = _loc(kind, 2, 33, M=20)
    x = np.zeros((1, 480, 20))
    with pytest.raises(ValueError, match="track_batch"):
        cs.stream(kind, loc, x, max_tile=160)
    plans = loc.plans(np.arange(480) / FS) if kind == "snn" else loc.plans()
    F, handles = runtime._band_handles(plans)
    lib = _lib.load()
    assert lib.micloc_stream_bands_track_state_bytes(handles, F, 1) == 0 and lib.micloc_stream_bands_track_workspace_bytes(handles, F, 1, 4096) == 0
    state = runtime._torch().zeros(4096, dtype=runtime._torch().uint8, device=plans[0].device)
    assert lib.micloc_stream_bands_track_reset(handles, F, 1, runtime._ptr(state), 4096, runtime._stream(plans[0].device)) == _lib.MICLOC_ERR_SHAPE


# ---- 12. the sweep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_sweep_through_the_tracked_wideband_stream_equals_the_fused_call(cs, kind):
    from haghighatshoarmuir2024_amd.sweep import wideband_moving_target_sweep, wideband_stream_track_localizer

    loc = cs.loc(kind, 3, 65)
    kw = dict(snr_db_vec=[0.0, 20.0], num_sim=4, seed=7, settle_frames=2400, batch_trials=4)
    ref = wideband_moving_target_sweep(loc, cs.env, **kw)
    got = wideband_moving_target_sweep(loc, cs.env, localizer=wideband_stream_track_localizer(loc, cs.env, tile=1600), **kw)
    keys = [k for k, v in ref.items() if isinstance(v, np.ndarray)]
    assert {"phase", "err", "med", "track_mae_deg"} <= set(keys) and ref["err"].shape == (2, 4)
    for k in keys:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
