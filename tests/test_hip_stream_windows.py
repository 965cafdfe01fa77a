"""Streaming windows on the MI355X (csrc/stream_windows.hip behind micloc_stream_localize_tile_windows_f64,
StreamingLocalizer(window=, hop=, max_windows=)): a recording pushed tile by tile emits power and arg-max per window of the rule in
include/micloc_hip.h as soon as a window's last chunk is final -- bit for bit the rows of the one-shot localize_batch(window=, hop=),
whatever the tiling, eagerly or from a replayed graph, with the running power / arg-max unchanged.

One fixture: config 2 (7 microphones, 14 channels), the three golden trials of 4799 frames, the bipolar chirp bf_mat (G = 449)."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 512), (256, 256), (5120, 256), (1024, 256)]


def _beamformer():
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    tau = 1 / (2 * np.pi * 2000)
    return SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=48_000)


def _np(t):
    return t.cpu().numpy()


def _wrap(x, L2):
    """np.roll's wrap-around rows of the in-phase channels, [B, L2, M]: row t is x[(t - L2) mod T] (zeros past a recording shorter than L2)."""
    w = np.roll(x, L2, axis=1)[:, :L2, :]
    return np.concatenate([w, np.zeros((x.shape[0], L2 - w.shape[1], x.shape[2]))], axis=1) if w.shape[1] < L2 else w


class _Fixture:
    def __init__(self, cfg2):
        self.bf = _beamformer()
        self.W = cfg2["bf_mat"]
        self.x = np.ascontiguousarray(golden("trials_cfg2.npz")["sig_in"])  # [3, 4799, 7]
        self.L2 = len(self.bf.kernel) // 2
        self._one = {}

    def one(self, x, window, hop, live=False, key=None):
        """The one-shot rows (computed once per case, read-only).  live: with the neuron kernel of a live source, which is normalised over
        1 s because the length is not known (StreamingLocalizer's total_frames=None) -- the sum differs from the one over T frames
        in the last bit."""
        k = (key, x.shape, window, hop, live)
        if key is None or k not in self._one:
            tv = np.arange(int(self.bf.fs)) / self.bf.fs if live else None
            o = self.bf.localize_batch(self.W, x, time_vec=tv, window=window, hop=hop)
            r = {n: _np(o[n]) for n in ("window_power", "window_argmax", "power", "argmax")}
            for v in r.values():
                v.setflags(write=False)
            if key is None:
                return r
            self._one[k] = r
        return self._one[k]

    def localizer(self, x, known=True, **kw):
        from haghighatshoarmuir2024_amd.streaming import StreamingLocalizer

        return StreamingLocalizer(self.bf, self.W, x.shape[0], x.shape[1] if known else None, wrap_tail=_wrap(x, self.L2), **kw)


@pytest.fixture(scope="module")
def fx(cfg2):
    return _Fixture(cfg2)


def _push_all(s, x, tiles):
    t = 0
    for n in tiles:
        s.push(x[:, t : t + n, :], final=t + n == x.shape[1])
        t += n
    assert t == x.shape[1]


def _tilings(T):
    irregular = [n for n in (16, 240, 1024, 48, 1600, 528, 16, 800) if n % 16 == 0]
    cut, t = [], 0
    for n in irregular:
        if t + n >= T:
            break
        cut.append(n)
        t += n
    cut.append(T - t)  # the ragged last tile
    return [[T], [160] * ((T - 1) // 160) + [T - 160 * ((T - 1) // 160)], cut]


# ---- 1. one-shot bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,hop", SHAPES)
def test_stream_windows_equal_the_one_shot_rows_for_any_tiling(fx, window, hop):
    from haghighatshoarmuir2024_amd.utils import window_bounds

    for T in (4799, 1100, 1024):  # 1100: windows that start before T but do not exist in the rule; 1024: an exact fit
        x = fx.x[:, :T, :]
        one = fx.one(x, window, hop, key="golden")
        nW = len(window_bounds(T, window, hop)[0])
        assert one["window_power"].shape == (3, nW, 449)
        plain = fx.localizer(x, max_tile=T)
        plain.push(x)
        ref = plain.finish()
        assert "window_power" not in ref
        for tiles in _tilings(T):
            s = fx.localizer(x, max_tile=max(tiles), window=window, hop=hop)
            _push_all(s, x, tiles)
            out = s.finish()
            msg = f"T={T} tiles={tiles[:4]}..."
            assert out["window_count"] == nW and s.status()["frames"] == T, msg
            np.testing.assert_array_equal(_np(out["window_power"]), one["window_power"], err_msg=msg)
            np.testing.assert_array_equal(_np(out["window_argmax"]), one["window_argmax"], err_msg=msg)
            # the running read-out is the one of a localizer built without `window` (and of the one-shot call)
            np.testing.assert_array_equal(_np(out["power"]), _np(ref["power"]), err_msg=msg)
            np.testing.assert_array_equal(_np(out["argmax"]), _np(ref["argmax"]), err_msg=msg)
            np.testing.assert_array_equal(_np(out["power"]), one["power"], err_msg=msg)
    if (window, hop) == (1024, 256):
        assert len(window_bounds(1100, window, hop)[0]) == 2  # not 5


# ---- 2. a live source ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,hop", [(1024, 256), (256, 256)])
def test_live_source_emits_each_window_when_its_last_chunk_is_final(fx, window, hop):
    from haghighatshoarmuir2024_amd.utils import window_bounds, windows_complete

    x, T = fx.x, fx.x.shape[1]
    one = fx.one(x, window, hop, live=True, key="golden")
    nW = len(window_bounds(T, window, hop)[0])
    s = fx.localizer(x, known=False, max_tile=400, window=window, hop=hop)
    lp, la = s.latest_window()
    assert not _np(lp).any() and s.windows()["count"] == 0  # untouched until the first window exists
    counts, t = [], 0
    while t < T:
        n = min(400, T - t)
        s.push(x[:, t : t + n, :], final=t + n == T)
        t += n
        w, frames = s.windows(), s.status()["frames"]
        assert w["count"] == windows_complete(frames, window, hop, T=T if t == T else None), (t, frames)
        counts.append(w["count"])
        k = w["count"] - w["first"]
        assert w["first"] == 0 and tuple(w["window_power"].shape) == (3, k, 449) and tuple(w["window_argmax"].shape) == (3, k)
        np.testing.assert_array_equal(w["window_start"], np.arange(k) * hop)
        # every row present already is the one-shot row (the leftover window exists only after the final tile)
        np.testing.assert_array_equal(_np(w["window_power"]), one["window_power"][:, :k], err_msg=f"t={t}")
        np.testing.assert_array_equal(_np(w["window_argmax"]), one["window_argmax"][:, :k], err_msg=f"t={t}")
        if k:
            lp, la = s.latest_window()
            np.testing.assert_array_equal(_np(lp), one["window_power"][:, k - 1])
            np.testing.assert_array_equal(_np(la), one["window_argmax"][:, k - 1])
    assert counts == sorted(counts) and counts[-1] == nW and 0 < counts[len(counts) // 2] < nW
    out = s.finish()
    assert out["window_count"] == nW
    np.testing.assert_array_equal(_np(out["window_power"]), one["window_power"])
    np.testing.assert_array_equal(_np(out["power"]), one["power"])


# ---- 3. the ring ---------------------------------------------------------------------------------------------------------------------
def test_ring_keeps_the_newest_windows_and_finish_refuses_a_truncated_array(fx):
    from haghighatshoarmuir2024_amd import _lib

    x, T = fx.x, fx.x.shape[1]
    one = fx.one(x, 1024, 512, key="golden")
    assert one["window_power"].shape[1] == 9
    s = fx.localizer(x, max_tile=1600, window=1024, hop=512, max_windows=2)
    _push_all(s, x, [1600, 1600, T - 3200])
    w = s.windows()
    assert w["count"] == 9 and w["first"] == 7 and list(w["window_start"]) == [7 * 512, 8 * 512]
    np.testing.assert_array_equal(_np(w["window_power"]), one["window_power"][:, 7:9])
    np.testing.assert_array_equal(_np(w["window_argmax"]), one["window_argmax"][:, 7:9])
    lp, la = s.latest_window()
    np.testing.assert_array_equal(_np(lp), one["window_power"][:, 8])
    with pytest.raises(_lib.MiclocError, match="max_windows"):
        s.finish()  # total_frames was given: 9 windows do not fit 2 rows
    # a live source keeps the newest rows and says how many there were
    one_live = fx.one(x, 1024, 512, live=True, key="golden")
    live = fx.localizer(x, known=False, max_tile=1600, window=1024, hop=512, max_windows=2)
    _push_all(live, x, [1600, 1600, T - 3200])
    out = live.finish()
    assert out["window_count"] == 9 and tuple(out["window_power"].shape) == (3, 2, 449)
    np.testing.assert_array_equal(_np(out["window_power"]), one_live["window_power"][:, 7:9])


# ---- 4. replayed against eager pushes ------------------------------------------------------------------------------------------------
def test_windowed_push_replay_is_one_graph_per_tile(fx):
    """test_stream_push_replay_is_one_graph_per_tile (test_hip_streaming.py) with windows on: the read-out is part of the tile's graph."""
    import torch

    rng = np.random.RandomState(9)
    n, tiles, window, hop = 800, 11, 1024, 256
    T = tiles * n + 799
    x = rng.randn(2, T, 7)
    x[:, :4799, :] += fx.x[:2]
    one = fx.one(x, window, hop, live=True)
    kw = dict(known=False, max_tile=n, lag_frames=1024, window=window, hop=hop)
    a = fx.localizer(x, **kw)  # eager pushes
    g = fx.localizer(x, **kw)  # graph replays
    xd = torch.from_numpy(x).cuda()
    for k in range(tiles):
        pa, aa = a.push(xd[:, k * n : (k + 1) * n, :])
        pg, ag = g.push_replay(xd[:, k * n : (k + 1) * n, :])
        assert torch.equal(pa, pg) and torch.equal(aa, ag), k
        assert a.status() == g.status(), k
        wa, wg = a.windows(), g.windows()
        assert wa["count"] == wg["count"] and wa["first"] == wg["first"], k
        assert torch.equal(wa["window_power"], wg["window_power"]) and torch.equal(wa["window_argmax"], wg["window_argmax"]), k
        assert all(torch.equal(u, v) for u, v in zip(a.latest_window(), g.latest_window())), k
    assert list(g._graphs) == [n] and g.base > 0 and wg["count"] > 20  # ONE captured graph; the window slid inside it
    a.push(xd[:, tiles * n :, :], final=True)
    g.push(xd[:, tiles * n :, :], final=True)
    oa, og = a.finish(), g.finish()
    assert og["window_count"] == one["window_power"].shape[1] <= 64
    for key in ("window_power", "window_argmax", "power", "argmax"):
        np.testing.assert_array_equal(_np(og[key]), one[key], err_msg=key)
        np.testing.assert_array_equal(_np(oa[key]), _np(og[key]), err_msg=key)


# ---- 5. the wide kernel family -------------------------------------------------------------------------------------------------------
def test_wide_kernel_family_with_512_frame_chunks():
    from micloc.array_geometry import CircularArray
    from micloc.snn_beamformer import SNNBeamformer
    from haghighatshoarmuir2024_amd.streaming import StreamingLocalizer

    tau = 1 / (2 * np.pi * 2000)
    bf = SNNBeamformer(CircularArray(0.1, 40), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=48_000)
    rng = np.random.RandomState(40)
    W = rng.randn(80, 130)
    W /= np.linalg.norm(W, axis=0, keepdims=True)
    T, window, hop = 5937, 1024, 512
    x = rng.randn(3, T, 40)
    one = bf.localize_batch(W, x, window=window, hop=hop)
    L2 = len(bf.kernel) // 2
    with pytest.raises(ValueError, match="512"):
        StreamingLocalizer(bf, W, 3, T, window=768, hop=256)  # multiples of 256 only: this family's chunks are 512 frames
    for tiles in ([T], [2048, 512, T - 2560]):
        s = StreamingLocalizer(bf, W, 3, T, wrap_tail=_wrap(x, L2), max_tile=max(tiles), lag_frames=2048, window=window, hop=hop)
        assert s.CH == 512
        _push_all(s, x, tiles)
        out = s.finish()
        assert out["window_count"] == 11
        for key in ("window_power", "window_argmax", "power", "argmax"):
            np.testing.assert_array_equal(_np(out[key]), _np(one[key]), err_msg=f"{key} tiles={tiles}")


# ---- 6. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_value_errors(fx):
    x = fx.x
    for kw, match in ((dict(window=1000), "quantum"), (dict(window=1024, hop=100), "quantum"), (dict(window=1024, hop=2048), "hop <= window"),
                      (dict(window=1024, hop=0), "quantum"), (dict(window=0), "quantum"), (dict(window=-256), "quantum"),
                      (dict(hop=256), "window"), (dict(max_windows=4), "window"), (dict(window=1024, max_windows=0), "max_windows")):
        with pytest.raises(ValueError, match=match):
            fx.localizer(x, **kw)
    s = fx.localizer(x)  # built without window: today's object
    assert s.window is None
    with pytest.raises(ValueError, match="window"):
        s.latest_window()
    with pytest.raises(ValueError, match="window"):
        s.windows()


# ---- 7. seeded campaign --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_random_lengths_windows_tilings_eager_and_replayed(fx, seed):
    import torch

    rng = np.random.RandomState(700 + seed)
    T = int(rng.randint(16, 6001))
    window = 256 * int(rng.randint(1, 9))
    hop = 256 * int(rng.randint(1, window // 256 + 1))
    sizes = [int(v) for v in rng.choice([64, 160, 256, 400, 1024, 1600], size=2, replace=False)]
    live = bool(rng.rand() < 0.5)
    x = rng.randn(2, T, 7)
    k = min(T, 4799)
    x[:, :k, :] += fx.x[:2, :k, :]
    one = fx.one(x, window, hop, live=live)
    s = fx.localizer(x, known=not live, max_tile=max(sizes), lag_frames=1536, window=window, hop=hop, max_windows=one["window_power"].shape[1])
    xd = torch.from_numpy(x).cuda()
    t = 0
    while True:
        n = int(rng.choice(sizes))
        if t + n >= T:
            s.push(xd[:, t:, :], final=True)  # the ragged rest
            break
        (s.push_replay if rng.rand() < 0.6 else s.push)(xd[:, t : t + n, :])
        t += n
    out = s.finish()
    msg = f"T={T} window={window} hop={hop} sizes={sizes} live={live}"
    assert out["window_count"] == one["window_power"].shape[1], msg
    for key in ("window_power", "window_argmax", "power", "argmax"):
        np.testing.assert_array_equal(_np(out[key]), one[key], err_msg=f"{key} {msg}")
