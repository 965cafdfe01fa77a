"""The tracked stream on the MI355X (csrc/stream_track.hip behind micloc_stream_localize_tile_track_f64 and
micloc_stream_complex_localize_tile_track_f64; StreamingLocalizer / ComplexStreamingLocalizer with track=): a recording pushed tile by
tile emits the DoA index and the peak envelope of every frame as soon as the frame is final -- bit for bit the rows of the one-shot
track_batch on the whole recording, whatever the tiling, eagerly or from a replayed graph, alone or beside the windowed read-out.

One fixture: config 2 (7 microphones, 14 channels), the three golden trials of 4799 frames, the bipolar chirp bf_mat (G = 449 = 8 column
groups of the kernels), Envelope(10 ms, 100 ms).  Every one-shot reference is computed once, shared and read-only."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

FS = 48_000
KEYS = (("track_index", "index"), ("track_peak_envelope", "peak_envelope"), ("envelope_last", "envelope_last"))


def _np(t):
    return t.cpu().numpy()


def _env():
    from haghighatshoarmuir2024_amd.utils import Envelope

    return Envelope(rise_time=10e-3, fall_time=100e-3, fs=FS)


def _wrap(x, L2):
    """np.roll's wrap-around rows of the in-phase channels, [B, L2, M] (zeros past a recording shorter than L2)."""
    w = np.roll(x, L2, axis=1)[:, :L2, :]
    return np.concatenate([w, np.zeros((x.shape[0], L2 - w.shape[1], x.shape[2]))], axis=1) if w.shape[1] < L2 else w


class _Fixture:
    def __init__(self, cfg2):
        from micloc.array_geometry import CenterCircularArray
        from micloc.beamformer import Beamformer
        from micloc.snn_beamformer import SNNBeamformer

        tau = 1 / (2 * np.pi * 2000)
        geo = CenterCircularArray(4.5e-2, 7)
        self.bf = SNNBeamformer(geo, 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=FS)
        self.bm = Beamformer(geo, 10e-3, [1000.0, 2000.0], fs=FS)
        self.W = np.asarray(cfg2["bf_mat"], dtype=np.float64)
        self.doa_list = cfg2["doa_list"]
        self.x = np.ascontiguousarray(golden("trials_cfg2.npz")["sig_in"])  # [3, 4799, 7]
        self.x.setflags(write=False)
        self.L2 = len(self.bf.kernel) // 2
        self.env = _env()
        self._one = {}

    def _keep(self, key, make):
        if key not in self._one:
            o = make()
            r = {k: _np(o[k]) for k in ("index", "peak_envelope", "envelope_last")}
            for v in r.values():
                v.setflags(write=False)
            self._one[key] = r
        return self._one[key]

    def one(self, trials=3, T=4799, G=449, live=False):
        """track_batch on the whole recording.  live: with the neuron kernel of a live source, normalised over 1 s."""
        tv = np.arange(FS) / FS if live else None
        return self._keep(("snn", trials, T, G, live), lambda: self.bf.track_batch(self.W[:, :G], self.x[:trials, :T], self.env, time_vec=tv,
                                                                                  want_envelope_last=True))

    def Wc(self, G):
        rng = np.random.RandomState(3 + G)
        return (rng.randn(7, G) + 1j * rng.randn(7, G)) / np.sqrt(14)

    def one_complex(self, G):
        return self._keep(("complex", G), lambda: self.bm.track_batch(self.Wc(G), self.x[:2], self.env, want_envelope_last=True))

    def localizer(self, x, known=True, G=449, track=True, **kw):
        from haghighatshoarmuir2024_amd.streaming import StreamingLocalizer

        if track:
            kw["track"] = self.env
        return StreamingLocalizer(self.bf, self.W[:, :G], x.shape[0], x.shape[1] if known else None, wrap_tail=_wrap(x, self.L2), **kw)

    def complex_localizer(self, x, G, **kw):
        from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

        return ComplexStreamingLocalizer(self.bm, self.Wc(G), x.shape[0], x.shape[1], wrap_tail=ComplexStreamingLocalizer.wrap_rows(x, len(self.bm.kernel)),
                                         track=self.env, **kw)


@pytest.fixture(scope="module")
def fx(cfg2):
    return _Fixture(cfg2)


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


# ---- 1. parity with the one-shot call, SNN -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiling", ["one", "160", "1200", "random16"])
def test_snn_config2_trials_equal_track_batch_for_any_tiling(fx, tiling):
    x, T = fx.x, 4799
    one = fx.one()
    assert one["index"].shape == (3, T) and one["envelope_last"].shape == (3, 449)
    tiles = {"one": [T], "160": _even(T, 160), "1200": _even(T, 1200), "random16": _random(T, 11, 1, 75, 16)}[tiling]
    s = fx.localizer(x, max_tile=max(tiles))
    _push_all(s, x, tiles)
    out = s.finish()
    assert out["track_count"] == T and s.status()["frames"] == T
    _assert_finish(out, one, f"tiles={tiles[:4]}...")


@pytest.mark.parametrize("G", [1, 63, 64, 65])
def test_column_group_edges(fx, G):
    """G <= 64: the kernel writes the ring itself; 65: two column groups and the combine launch."""
    x = fx.x[:1]
    s = fx.localizer(x, G=G, max_tile=160)
    _push_all(s, x, _even(4799, 160))
    _assert_finish(s.finish(), fx.one(trials=1, G=G), f"G={G}")


@pytest.mark.parametrize("T", [2, 15, 209, 1001])
def test_short_and_ragged_recordings(fx, T):
    """state_0 at frame 0, the ragged last chunk, ranges that stay empty for many tiles."""
    x = fx.x[:1, :T]
    one = fx.one(trials=1, T=T)
    for tiles in [[T]] + ([[16] * 62 + [9]] if T == 1001 else []):
        s = fx.localizer(x, max_tile=max(tiles))
        _push_all(s, x, tiles)
        _assert_finish(s.finish(), one, f"T={T} tiles={tiles[:3]}...")


# ---- 2. the ring, graphs, windows ---------------------------------------------------------------------------------------------------
def test_live_source_with_the_smallest_ring_wraps_and_keeps_the_newest_rows(fx):
    x, T = fx.x[:1], 4799
    one = fx.one(trials=1, live=True)
    kw = dict(known=False, max_tile=1600, lag_frames=1024)
    R = fx.localizer(x, **kw).min_track
    assert R < T  # the ring wraps
    with pytest.raises(ValueError, match="max_track"):
        fx.localizer(x, max_track=R - 1, **kw)
    s = fx.localizer(x, max_track=R, **kw)
    assert s.max_track == R == s.cap
    li, lp = s.latest_track()
    assert not _np(li).any() and s.tracked()["count"] == 0
    counts = []
    for t in range(0, T, 1600):
        s.push(x[:, t : t + 1600, :], final=t + 1600 >= T)
        w, frames = s.tracked(), s.status()["frames"]
        assert w["count"] == frames and w["first"] == max(0, frames - R)
        counts.append(frames)
        np.testing.assert_array_equal(_np(w["index"]), one["index"][:, w["first"] : frames], err_msg=f"t={t}")
        np.testing.assert_array_equal(_np(w["peak_envelope"]), one["peak_envelope"][:, w["first"] : frames], err_msg=f"t={t}")
        if frames:
            li, lp = s.latest_track()
            np.testing.assert_array_equal(_np(li), one["index"][:, frames - 1])
            np.testing.assert_array_equal(_np(lp), one["peak_envelope"][:, frames - 1])
    assert counts == sorted(counts) and counts[-1] == T and 0 < counts[1] < T
    out = s.finish()  # a live source: the newest rows, and how many frames there were
    assert out["track_count"] == T and tuple(out["track_index"].shape) == (1, R)
    np.testing.assert_array_equal(_np(out["track_index"]), one["index"][:, T - R :])
    np.testing.assert_array_equal(_np(out["envelope_last"]), one["envelope_last"])


def test_finish_refuses_a_truncated_array(fx):
    from haghighatshoarmuir2024_amd import _lib

    x = fx.x[:1]
    s = fx.localizer(x, max_tile=1600, lag_frames=1024, max_track=3328)
    _push_all(s, x, _even(4799, 1600))
    with pytest.raises(_lib.MiclocError, match="max_track"):
        s.finish()


def test_push_replay_is_one_graph_launch_per_tile(fx, monkeypatch):
    import torch

    x, T, n = fx.x[:1], 4799, 800
    one = fx.one(trials=1, live=True)
    kw = dict(known=False, max_tile=n, lag_frames=1024)
    a, g = fx.localizer(x, **kw), fx.localizer(x, **kw)
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
    np.testing.assert_array_equal(_np(og["track_index"]), one["index"])
    np.testing.assert_array_equal(_np(og["track_peak_envelope"]), one["peak_envelope"])
    np.testing.assert_array_equal(_np(og["envelope_last"]), one["envelope_last"])
    np.testing.assert_array_equal(_np(oa["track_index"]), _np(og["track_index"]))


def test_tracking_beside_the_windowed_read_out(fx):
    x, T, window, hop = fx.x, 4799, 1024, 512
    one, tiles = fx.one(), _even(4799, 1200)
    ref = fx.bf.localize_batch(fx.W, x, window=window, hop=hop)
    s = fx.localizer(x, max_tile=1200, window=window, hop=hop)
    _push_all(s, x, tiles)
    out = s.finish()
    for k in ("power", "argmax", "window_power", "window_argmax"):
        np.testing.assert_array_equal(_np(out[k]), _np(ref[k]), err_msg=k)
    _assert_finish(out, one, "with windows")
    # without track=: the same power and arg-max, and no tracking keys
    for kw in (dict(window=window, hop=hop), {}):
        p = fx.localizer(x, track=False, max_tile=1200, **kw)
        _push_all(p, x, tiles)
        po = p.finish()
        assert "track_index" not in po and p.track is None
        np.testing.assert_array_equal(_np(po["power"]), _np(ref["power"]))
        np.testing.assert_array_equal(_np(po["argmax"]), _np(ref["argmax"]))
        with pytest.raises(ValueError, match="track"):
            p.tracked()


# ---- 3. failures ----------------------------------------------------------------------------------------------------------------------
def test_lag_failure_makes_finish_raise_and_no_emitted_row_is_wrong(fx):
    from haghighatshoarmuir2024_amd import _lib

    rng = np.random.RandomState(5)
    T = 9600
    x = rng.randn(1, T, 7)
    x[0, 1000:7000, :] = 0.0  # digital silence: the open clusters hold their frames back longer than a short window keeps them
    one = fx.bf.track_batch(fx.W, x, fx.env)
    s = fx.localizer(x, max_tile=800, lag_frames=256)
    for t in range(0, T, 800):
        s.push(x[:, t : t + 800, :])
    st = s.status()
    assert st["lag_failures"] > 0 and st["frames"] < T
    with pytest.raises(_lib.MiclocError, match="window"):
        s.finish()
    w = s.tracked()  # what was emitted before the failure is the one-shot call's
    assert w["count"] == st["frames"] > 0 and w["first"] == 0
    np.testing.assert_array_equal(_np(w["index"]), _np(one["index"])[:, : w["count"]])
    np.testing.assert_array_equal(_np(w["peak_envelope"]), _np(one["peak_envelope"])[:, : w["count"]])


def test_argument_errors_of_the_entries_are_status_codes_before_any_launch(fx):
    import torch

    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.runtime import _ptr, _stream
    from haghighatshoarmuir2024_amd.snn_beamformer import neuron_impulse_response

    lib = _lib.load()
    x = fx.x[:1]
    s = fx.localizer(x, max_tile=160)
    c = fx.complex_localizer(x, 449, max_tile=100)
    for o in (s, c):
        o.track_index.fill_(-7)
    wrong = fx.bf.new_plan()  # a real plan's tables with a complex bf_mat
    wrong.set_neuron_kernel(neuron_impulse_response(np.arange(4799) / FS, fx.bf.tau_vec))
    wrong.set_bf_mat(fx.Wc(449))
    assert lib.micloc_stream_track_state_bytes(s.plan.handle, 1) == s.ntst == 8 * 64 * 8
    assert lib.micloc_stream_track_workspace_bytes(s.plan.handle, 1, 0) == 0 and lib.micloc_stream_track_state_bytes(s.plan.handle, 0) == 0

    def snn(plan=None, state=True, ws_bytes=None, R=None):
        st = _stream(s.device)
        return lib.micloc_stream_localize_tile_track_f64(
            (plan or s.plan).handle, _ptr(s.state), _ptr(s.loc), s.nloc, _ptr(s.win), 1, s.cap, 0, _ptr(s.power), _ptr(s.argmax), _ptr(s.ws), s.nws,
            None, 0, 0, 0, 0, None, None, None, None, _ptr(s.tst) if state else None, s.ntst, *s.track, s.max_track if R is None else R,
            _ptr(s.track_index), _ptr(s.track_peak), _ptr(s.latest_index), _ptr(s.latest_peak), _ptr(s.tws), s.ntws if ws_bytes is None else ws_bytes, st)

    def cpx(plan=None, state=True, ws_bytes=None, R=None):
        st = _stream(c.device)
        return lib.micloc_stream_complex_localize_tile_track_f64(
            (plan or c.plan).handle, _ptr(c.state), c.nstate, 1, c.max_tile, 0, _ptr(c.power), _ptr(c.argmax), _ptr(c.ws), c.nws,
            None, 0, 0, 0, 0, None, None, None, None, _ptr(c.tst) if state else None, c.ntst, *c.track, c.max_track if R is None else R,
            _ptr(c.track_index), _ptr(c.track_peak), _ptr(c.latest_index), _ptr(c.latest_peak), _ptr(c.tws), c.ntws if ws_bytes is None else ws_bytes, st)

    assert s.ntws > 256 and c.ntws > 256  # eight column groups: the pair scratch is real
    assert snn(R=s.cap - 1) == _lib.MICLOC_ERR_SHAPE and cpx(R=c.max_tile - 1) == _lib.MICLOC_ERR_SHAPE  # a ring one tile can overrun
    assert snn(state=False) == _lib.MICLOC_ERR_INVALID and cpx(state=False) == _lib.MICLOC_ERR_INVALID
    assert snn(ws_bytes=s.ntws - 1) == _lib.MICLOC_ERR_WORKSPACE and cpx(ws_bytes=c.ntws - 1) == _lib.MICLOC_ERR_WORKSPACE
    assert snn(plan=wrong) == _lib.MICLOC_ERR_SHAPE  # a complex bf_mat on the SNN entry
    assert cpx(plan=s.plan) == _lib.MICLOC_ERR_SHAPE  # a real one on the complex entry
    assert lib.micloc_stream_track_reset(s.plan.handle, 1, _ptr(s.tst), s.ntst - 1, _stream(s.device)) == _lib.MICLOC_ERR_WORKSPACE
    torch.cuda.synchronize()
    for o in (s, c):
        assert int((o.track_index != -7).sum()) == 0 and o.status()["frames"] == 0  # nothing was launched
    # the objects still work
    _push_all(s, x, _even(4799, 160))
    np.testing.assert_array_equal(_np(s.finish()["track_index"]), fx.one(trials=1)["index"])


# ---- 4. the complex Beamformer and the sweep -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [57, 449])
def test_complex_beamformer_equals_track_batch_for_any_tiling(fx, G):
    x, T = fx.x[:2], 4799
    one = fx.one_complex(G)
    assert one["index"].shape == (2, T)
    for tiles in ([T], _even(T, 100), _random(T, 23, 1, 1200, 1)):  # 100: no multiple of 64, the carry fill takes many values
        s = fx.complex_localizer(x, G, max_tile=max(tiles))
        _push_all(s, x, tiles)
        out = s.finish()
        assert out["track_count"] == T
        _assert_finish(out, one, f"G={G} tiles={tiles[:4]}...")


@pytest.mark.parametrize("M", range(1, 9))
def test_every_row_of_the_complex_channel_table_equals_track_batch(fx, M):
    """C = 2M = 2 .. 16 channels: every <KM, KV> of csrc/track_rows.h's table.  G = 65: two column groups and the combine launch; tiles of
    100 frames: the carry fill is no multiple of 16."""
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer
    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

    bm = Beamformer(CenterCircularArray(4.5e-2, M), 10e-3, [1000.0, 2000.0], fs=FS)
    rng = np.random.RandomState(260 + M)
    T, G = 209, 65
    W = (rng.randn(M, G) + 1j * rng.randn(M, G)) / np.sqrt(2 * M)
    x = rng.randn(1, T, M)
    one = {k: _np(v) for k, v in bm.track_batch(W, x, fx.env, want_envelope_last=True).items() if k in ("index", "peak_envelope", "envelope_last")}
    for tiles in ([T], [100, 100, 9]):
        s = ComplexStreamingLocalizer(bm, W, 1, T, wrap_tail=ComplexStreamingLocalizer.wrap_rows(x, len(bm.kernel)), track=fx.env, max_tile=max(tiles))
        _push_all(s, x, tiles)
        out = s.finish()
        assert out["track_count"] == T
        _assert_finish(out, one, f"M={M} tiles={tiles}")


def test_sweep_through_the_tracked_stream_equals_the_fused_call(fx):
    from haghighatshoarmuir2024_amd.sweep import moving_target_sweep, stream_track_localizer

    kw = dict(snr_db_vec=[0.0, 20.0], num_sim=4, seed=7, settle_frames=2400, batch_trials=4)
    ref = moving_target_sweep(fx.bf, fx.W, fx.doa_list, fx.env, **kw)
    got = moving_target_sweep(fx.bf, fx.W, fx.doa_list, fx.env, localizer=stream_track_localizer(fx.bf, fx.W, fx.env, tile=1600), **kw)
    keys = [k for k, v in ref.items() if isinstance(v, np.ndarray)]
    assert {"phase", "err", "med", "track_mae_deg"} <= set(keys) and ref["err"].shape == (2, 4)
    for k in keys:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
