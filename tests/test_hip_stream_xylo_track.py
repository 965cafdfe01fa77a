"""The tracked Xylo stream (include/micloc_hip.h "streaming, Xylo tracking"): the tracking form of the packed integer LIF
walk resumed across launches (XyloNetwork.track_resume) equals the host reference of tests/xylo_track_ref.py AND XyloNetwork.track on
the whole raster for every cut, and XyloStreamingLocalizer(track=) emits Demo.track_batch's rows for every tiling -- as a live source with
a ring that wraps, beside window=, as one graph per tile, up to a lag failure, and through the moving-target sweep.  Every comparison is
exact (doubles by their bits); the reference is never the stream itself.  PARITY UNPINNED for the integer LIF like every Xylo test: the
oracle is the published rule, not XyloSim."""
import functools

import numpy as np
import pytest

import xylo_track_ref as R

pytestmark = pytest.mark.gpu

B = 3
WINDOWS = ((1, 1), (48, 480))  # (w_rise, w_fall)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


# ---- by value: track_resume over a list of cuts ----------------------------------------------------------------------------------
# (N, Cin, T).  Cin = 28 is the recipe of xylo_track_ref (14 ternary channels); (64, 40, 300) is the same recipe -- grouped columns, a
# raster whose active channels change every 37 frames, trial 1 firing every channel -- on 20 ternary channels: two 32-channel k-steps.
# "513b" is (513, 28, 300) with neuron 512, the only one of the second block, made the strict winner of some frames (see _case).
SHAPES = [(33, 28, 300), (449, 28, 700), (513, 28, 300), (1100, 28, 300), (64, 40, 300), (33, 28, 1)]


@functools.lru_cache(maxsize=None)
def _case(N, Cin, T, variant=""):
    if Cin == 2 * R.C_RECIPE:
        spec, raster = R.recipe(N, T)
    else:
        rng = np.random.RandomState(N + T + Cin)
        spec = R.grouped_spec(rng, Cin, N)
        raster = R.all_fire(rng, R.blocked_raster(rng, B, T, Cin // 2))
        raster.setflags(write=False)
    if variant == "b":
        # The recipe deals every column to about four neurons, and the first-maximum rule lets the lowest of them win: the lone neuron
        # of the second block (512) never does.  Here it gets the column of the recipe's most frequent winner with three quarters of
        # its threshold: it spikes more often than its twin and takes some frames strictly.
        idx = R.recipe_reference(N, T, 1, 1)["index"][0]
        w = int(np.bincount(idx).argmax())
        spec = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in spec.items()}
        for k in ("dash_syn", "dash_mem"):
            spec[k][N - 1] = spec[k][w]
        spec["W_in"][:, N - 1] = spec["W_in"][:, w]
        spec["threshold"][N - 1] = max(int(spec["threshold"][w]) * 3 // 4, 1)
    return spec, raster


@functools.lru_cache(maxsize=None)
def _spikes(N, Cin, T, cap, variant=""):
    """The oracle's raster and counts of the whole recording: computed once, shared, never changed."""
    spec, raster = _case(N, Cin, T, variant)
    out, rate = R.lif_reference(spec, R.events_of(raster), cap)
    out.setflags(write=False)
    return out, rate


@functools.lru_cache(maxsize=None)
def _reference(N, Cin, T, cap, w_rise, w_fall, Tp, variant=""):
    """The host reference over the first Tp frames (the rule is causal: a prefix of the raster is a recording of its own)."""
    out, _ = _spikes(N, Cin, T, cap, variant)
    head = out[:, :Tp]
    return R.track_reference(head, head.sum(axis=1, dtype=np.int64).astype(np.int32), w_rise, w_fall)


def _cuts(kind, T):
    """-> (cuts, frames walked).  tail1 ends on a range of ONE frame, which starts at a multiple of 16 like every range."""
    if kind == "one" or T <= 16:
        return [T], T
    if kind == "every16":
        return list(range(16, T, 16)) + [T], T
    if kind == "random16":
        rt = np.random.RandomState(T)
        inner = np.sort(rt.choice(np.arange(1, (T - 1) // 16 + 1), size=min(7, (T - 1) // 16), replace=False)) * 16
        return [int(c) for c in inner] + [T], T
    last = (T - 1) // 16 * 16
    return [last, last + 1], last + 1  # "tail1"


def _walk(net, dev, cuts, env, cap, out=None):
    state, tstate = net.new_state(dev.shape[0]), net.new_track_state(dev.shape[0])
    t = 0
    for c in cuts:
        out = net.track_resume(dev, t, c - t, state, tstate, env, out=out, max_spikes=cap)
        t = c
    return out, state, tstate


def _net(spec):
    from haghighatshoarmuir2024_amd.xylo_snn_localization import XyloNetwork

    return XyloNetwork(spec)


def _check_by_value(N, Cin, T, cap, variant=""):
    import torch

    spec, raster = _case(N, Cin, T, variant)
    net = _net(spec)
    dev = torch.from_numpy(np.array(raster)).cuda()
    for w_rise, w_fall in WINDOWS:
        env = R.envelope(w_rise, w_fall)
        one = {}
        for kind in ("one", "every16", "random16", "tail1"):
            cuts, Tp = _cuts(kind, T)
            got, state, _ = _walk(net, dev, cuts, env, cap)
            tag = f"N{N} Cin{Cin} T{T}{variant} cap{cap} ({w_rise}, {w_fall}) {kind}"
            g = dict(index=got["index"][:, :Tp], peak_env=got["peak_env"][:, :Tp], env_last=got["env_last"], rate=got["rate"])
            R.assert_equal_bits(g, _reference(N, Cin, T, cap, w_rise, w_fall, Tp, variant), tag + " vs host")
            if Tp not in one:
                one[Tp] = net.track(dev[:, :Tp].contiguous(), env, ternary=True, max_spikes=cap, want_rate=True)
            R.assert_equal_bits(g, one[Tp], tag + " vs XyloNetwork.track")
            assert int(got["index"][:, Tp:].abs().sum()) == 0 and float(got["peak_env"][:, Tp:].abs().sum()) == 0.0  # rows behind the range: untouched
            assert torch.equal(got["latest_index"], got["index"][:, Tp - 1]) and torch.equal(got["latest_peak"], got["peak_env"][:, Tp - 1]), tag
            assert got["rate"] is state["counts"]


@pytest.mark.parametrize("cap", [1, 3, 31])
@pytest.mark.parametrize("N,Cin,T", SHAPES)
def test_track_resume_equals_the_reference_and_the_one_shot_call_for_any_cut(N, Cin, T, cap):
    _check_by_value(N, Cin, T, cap)


def test_track_resume_with_a_winner_in_the_second_block_of_513():
    _check_by_value(513, 28, 300, 31, variant="b")


def _stats(ref, out):
    idx, pk, env = ref["index"], ref["peak_env"], ref["env"]
    ties = int((((env == pk[..., None]).sum(axis=2) > 1) & (pk > 0)).sum())
    return dict(max_count=int(out.max()), ties=ties, winners=[len(set(i.tolist())) for i in idx], blocks=sorted(set((idx.ravel() // 512).tolist())))


def test_the_by_value_cases_are_not_vacuous():
    """On the REFERENCE, windows (1, 1), cap 31.  (449, 28, 700) is tests/test_xylo_track_cpu.py's shape: ties in at least half of the
    frames of the random trials, five winners or more, ties across waves -- asserted there; only the re-walk is asserted here."""
    for N, Cin, T, variant in [(33, 28, 300, ""), (513, 28, 300, ""), (513, 28, 300, "b"), (1100, 28, 300, ""), (64, 40, 300, "")]:
        out, _ = _spikes(N, Cin, T, 31, variant)
        st = _stats(_reference(N, Cin, T, 31, 1, 1, T, variant), out)
        print(N, Cin, T, variant, st)
        assert st["max_count"] >= 2, st                   # second spikes within a step: groups walked again
        assert st["ties"] > 0, st                         # ties at a positive maximum
        assert max(st["winners"]) > 1, st                 # the winner moves
        if (N, variant) in ((513, "b"), (1100, "")):
            assert len(st["blocks"]) > 1, st              # winners in more than one neuron block
    # The recipe at N = 513 has NO winner in its second block, which holds neuron 512 alone (a column shared with lower neurons never
    # wins first): its block pairs lose or tie every frame, which the combine must get right too; "513b" is the case with such winners.
    assert _stats(_reference(513, 28, 300, 31, 1, 1, 300), _spikes(513, 28, 300, 31)[0])["blocks"] == [0]
    assert int(_spikes(449, 28, 700, 31)[0].max()) >= 2
    # the caps bind: with max_spikes 1 and 3 the counts differ from the uncapped ones
    for cap in (1, 3):
        assert int(_spikes(449, 28, 700, cap)[0].max()) == cap < int(_spikes(449, 28, 700, 31)[0].max())


def test_empty_range_and_interleaved_states():
    import torch

    N, Cin, T = 1100, 28, 300
    spec, raster = _case(N, Cin, T)
    net = _net(spec)
    rd = torch.from_numpy(np.array(raster)).cuda()
    rev = torch.from_numpy(np.ascontiguousarray(raster[::-1])).cuda()  # the trials in another order: another recording
    env = R.envelope(48, 480)
    ref = _reference(N, Cin, T, 31, 48, 480, T)
    a, ta, b, tb = net.new_state(B), net.new_track_state(B), net.new_state(B), net.new_track_state(B)
    oa = net.track_resume(rd, 0, 128, a, ta, env)
    before = [v.clone() for v in (a["state"], a["counts"], ta["state"], oa["index"], oa["peak_env"], oa["latest_index"], oa["latest_peak"], oa["env_last"])]
    net.track_resume(rd, 128, 0, a, ta, env, out=oa)  # an empty range rewrites nothing
    after = (a["state"], a["counts"], ta["state"], oa["index"], oa["peak_env"], oa["latest_index"], oa["latest_peak"], oa["env_last"])
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert int(a["counts"].sum()) > 0 and float(oa["env_last"].sum()) > 0
    # two states on one network, interleaved: each ends on the bits it reaches alone
    ob = net.track_resume(rev, 0, 64, b, tb, env)
    net.track_resume(rd, 128, 112, a, ta, env, out=oa)
    net.track_resume(rev, 64, T - 64, b, tb, env, out=ob)
    net.track_resume(rd, 240, T - 240, a, ta, env, out=oa)
    R.assert_equal_bits(oa, ref, "state a")
    R.assert_equal_bits(ob, {k: ref[k][::-1] for k in ("index", "peak_env", "env_last", "rate")}, "state b")
    # a ring shorter than the recording: frame t sits in row t % R, the newest R frames survive
    ring = 128
    small = dict(index=torch.zeros((B, ring), dtype=torch.int32, device="cuda"), peak_env=torch.zeros((B, ring), dtype=torch.float64, device="cuda"),
                 latest_index=torch.zeros((B,), dtype=torch.int32, device="cuda"), latest_peak=torch.zeros((B,), dtype=torch.float64, device="cuda"),
                 env_last=torch.zeros((B, N), dtype=torch.float64, device="cuda"))
    _walk(net, rd, [112, 240, T], env, 31, out=small)
    rows = np.arange(T - ring, T) % ring
    np.testing.assert_array_equal(_host(small["index"])[:, rows], ref["index"][:, T - ring :])
    np.testing.assert_array_equal(_bits(_host(small["peak_env"])[:, rows]), _bits(ref["peak_env"][:, T - ring :]))
    with pytest.raises(ValueError):
        net.track_resume(rd, 0, ring + 1, net.new_state(B), net.new_track_state(B), env, out=small)  # more frames than the ring holds
    with pytest.raises(ValueError):
        net.track_resume(rd, 8, 16, a, ta, env)


# ---- stream level: XyloStreamingLocalizer(track=) against Demo.track_batch ---------------------------------------------------------
FS = 48_000
_oneshot, _inputs = {}, {}


@functools.lru_cache(maxsize=None)
def _demo(bands=((1000, 2000),)):
    """test_hip_stream_xylo.py's small demo: 7 microphones, 33 DoAs, w_rec_coef = 0 (the paper's -0.1 / N quantises to 0 at its 449 DoAs
    and to -1 at these 33, which the stream refuses): W_in, the decays and the thresholds are the demo's own."""
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.xylo_snn_localization import Demo, xylo_specification

    demo = Demo(CenterCircularArray(0.045, 7), [list(b) for b in bands], doa_list=np.linspace(-np.pi, np.pi, 33), recording_duration=0.05)
    spec0 = xylo_specification(demo.bf_mats, demo.tau_vecs, demo.fs, 1e-3, demo.bipolar_spikes, w_rec_coef=0.0)
    assert spec0["w_rec"] == 0 and all(np.array_equal(spec0[k], demo.spec[k]) for k in ("W_in", "dash_syn", "dash_mem", "threshold"))
    demo.spec = spec0
    return demo


def _env():
    from haghighatshoarmuir2024_amd.utils import Envelope

    return Envelope(rise_time=1e-3, fall_time=10e-3, fs=FS)  # 48 and 480 frames


def _input(T, zero_tail=0):
    """Two trials: a 1 to 2 kHz chirp from a source that sweeps over the DoAs (two phases), plus seeded noise at about 10 dB."""
    key = (T, zero_tail)
    if key not in _inputs:
        from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
        from haghighatshoarmuir2024_amd.sweep import moving_doa_path
        from haghighatshoarmuir2024_amd.xylo_snn_localization import signal_from_template

        geom = CenterCircularArray(0.045, 7)
        time = np.arange(max(T, 64)) / FS
        sig = np.sin(2 * np.pi * np.cumsum(1000 + 1000 * time / time[-1]) / FS)
        x = np.stack([signal_from_template(geom, (time, sig, moving_doa_path(time, time[-1], np.pi / 2, 1.5, np.asarray(ph)))) for ph in (0.3, 2.0)])
        x = x[:, :T, :] + np.random.RandomState(T).randn(2, T, 7) * np.sqrt(0.5 / 10.0)
        if zero_tail:
            x[:, T - zero_tail :, :] = 0.0
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


def _one_shot(T, zero_tail=0, x=None):
    """Demo.track_batch on the whole recording: computed once per input, shared, never changed."""
    key = (T, zero_tail) if x is None else None
    if key is None or key not in _oneshot:
        got = _demo().track_batch(np.array(_input(T, zero_tail) if x is None else x), _env(), want_rate=True)
        one = {k: v.cpu().numpy() for k, v in got.items()}
        if key is None:
            return one
        _oneshot[key] = one
    return _oneshot[key]


def _assert_one_shot_is_not_vacuous(one):
    for b in range(2):
        assert float(one["peak_env"][b].max()) > 0.0, b               # both trials have a positive peak envelope somewhere
        assert len(set(one["index"][b].tolist())) >= 2, b             # and at least two distinct winners


def _tiles(kind, T):
    if kind == "one":
        return [T]
    if kind == "by16":
        return [16] * (T // 16) + ([T % 16] if T % 16 else [])
    if kind == "by1200":
        return [1200] * (T // 1200) + ([T % 1200] if T % 1200 else [])
    rt = np.random.RandomState(T + 1)
    cuts = np.sort(rt.choice(np.arange(1, T // 16), size=9, replace=False)) * 16
    return [int(n) for n in np.diff(np.concatenate([[0], cuts, [T]]))]


def _check_finish(out, one, T):
    assert out["track_count"] == T
    np.testing.assert_array_equal(_host(out["track_index"]), one["index"])
    np.testing.assert_array_equal(_bits(_host(out["track_peak_envelope"])), _bits(one["peak_env"]))
    np.testing.assert_array_equal(_bits(_host(out["envelope_last"])), _bits(one["env_last"]))
    np.testing.assert_array_equal(_host(out["counts"]), one["rate"])


def _stream(T, x, tiles, track=True, **kw):
    demo = _demo()
    L2 = len(demo.beamfs[0].kernel) // 2
    wrap = np.zeros((2, L2, 7))
    k = min(L2, T)
    wrap[:, :k] = np.roll(x, L2, axis=1)[:, :k]  # np.roll's wrap-around rows (a recording shorter than L2: zeros behind it)
    return demo.streaming_localizer(2, total_frames=T, wrap_tail=wrap, max_tile=max(tiles), lag_frames=2048, track=_env() if track else None, **kw)


@pytest.mark.parametrize("tiling", ["one", "by16", "random16", "by1200"])
@pytest.mark.parametrize("T", [4799, 6000])
def test_tracked_stream_equals_track_batch_for_any_tiling(T, tiling):
    x, one = _input(T), _one_shot(T)
    _assert_one_shot_is_not_vacuous(one)
    tiles = _tiles(tiling, T)
    s = _stream(T, x, tiles)
    assert s.max_track == max(T, s.cap) and s.min_track == s.cap
    t = 0
    for n in tiles:
        s.push(x[:, t : t + n, :])
        t += n
    _check_finish(s.finish(), one, T)
    st = s.status()
    assert st["frames"] == T and st["lag_failures"] == 0 and st["overflow"] == 0


@pytest.mark.parametrize("T", [2, 15, 209])
def test_a_single_final_tile(T):
    x, one = _input(T), _one_shot(T)
    s = _stream(T, x, [T])
    s.push(x)
    _check_finish(s.finish(), one, T)


def test_live_source_with_the_smallest_ring_which_wraps():
    """No total_frames, no wrap rows (the one-shot call on a recording whose last L // 2 frames are zero rolls the same zeros in front),
    max_track = min_track: after every push tracked() holds the newest rows and latest_track() the newest one."""
    import torch

    demo = _demo()
    L2 = len(demo.beamfs[0].kernel) // 2
    T = 4799
    x, one = _input(T, zero_tail=L2), _one_shot(T, zero_tail=L2)
    _assert_one_shot_is_not_vacuous(one)
    probe = demo.streaming_localizer(2, max_tile=400, lag_frames=2048, track=_env())
    ring = probe.min_track
    assert probe.max_track == -(-4 * ring // 64) * 64 and ring == probe.cap == 3072  # the default; the smallest is the window's capacity
    s = demo.streaming_localizer(2, max_tile=400, lag_frames=2048, track=_env(), max_track=ring)
    assert T > ring
    tiles = [400] * (T // 400) + [T % 400]
    t, seen, wrapped = 0, 0, False
    for i, n in enumerate(tiles):
        s.push(x[:, t : t + n, :], final=(i == len(tiles) - 1))
        t += n
        w = s.tracked()
        assert w["count"] == s.status()["frames"] >= seen and w["first"] == max(0, w["count"] - ring)
        lo, hi = w["first"], w["count"]
        np.testing.assert_array_equal(_host(w["index"]), one["index"][:, lo:hi])
        np.testing.assert_array_equal(_bits(_host(w["peak_envelope"])), _bits(one["peak_env"][:, lo:hi]))
        if hi:
            li, lp = s.latest_track()
            assert torch.equal(li, w["index"][:, -1]) and torch.equal(lp, w["peak_envelope"][:, -1])
        seen, wrapped = hi, wrapped or lo > 0
    assert wrapped and seen == T
    out = s.finish()
    assert out["track_count"] == T and out["track_index"].shape == (2, ring)
    np.testing.assert_array_equal(_host(out["track_index"]), one["index"][:, T - ring :])
    np.testing.assert_array_equal(_bits(_host(out["envelope_last"])), _bits(one["env_last"]))
    with pytest.raises(ValueError):
        s.windows()  # built without window=
    plain = demo.streaming_localizer(2, max_tile=400)
    with pytest.raises(ValueError):
        plain.latest_track()


def test_track_beside_window_leaves_the_other_results_unchanged():
    import torch

    T, window, hop = 4799, 1024, 512
    x, one = _input(T), _one_shot(T)
    tiles = _tiles("by1200", T)
    res = []
    for track in (True, False):
        s = _stream(T, x, tiles, track=track, window=window, hop=hop)
        t = 0
        for n in tiles:
            s.push(x[:, t : t + n, :])
            t += n
        res.append(s.finish())
    with_track, without = res
    _check_finish(with_track, one, T)
    assert "track_index" not in without
    for k in ("counts", "rate", "peak", "window_counts", "window_rate", "window_peak"):
        assert torch.equal(with_track[k], without[k]), k
    assert with_track["window_count"] == without["window_count"] > 0 and int(without["window_counts"].sum()) > 0


def test_push_replay_is_one_graph_launch_per_tile(monkeypatch):
    """Five 1200-frame tiles of a live source: the first is an eager push, the second is captured, from the third on a tile is exactly ONE
    graph launch and no launch of its own; the tracked rows equal push()'s on a twin stream after every tile and the one-shot rows."""
    import torch

    demo = _demo()
    n, tiles = 1200, 5
    T = n * tiles + 16
    x, one = _input(T), _one_shot(T)
    L2 = len(demo.beamfs[0].kernel) // 2
    kw = dict(total_frames=None, wrap_tail=x[:, T - L2 :, :], max_tile=n, lag_frames=2048, track=_env())
    a, g = demo.streaming_localizer(2, **kw), demo.streaming_localizer(2, **kw)
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
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for k in range(tiles):
        a.push(xd[:, k * n : (k + 1) * n, :])
        before = dict(calls)
        g.push_replay(xd[:, k * n : (k + 1) * n, :])
        if k >= 2:
            assert calls["tile"] == before["tile"] and calls["replay"] == before["replay"] + 1, k
        wa, wg = a.tracked(), g.tracked()
        assert wa["count"] == wg["count"] and torch.equal(wa["index"], wg["index"]) and torch.equal(wa["peak_envelope"], wg["peak_envelope"]), k
        assert all(torch.equal(p, q) for p, q in zip(a.latest_track(), g.latest_track())), k
        assert torch.equal(a.counts, g.counts) and a.status() == g.status(), k
        np.testing.assert_array_equal(_host(wg["index"]), one["index"][:, : wg["count"]])
    assert calls == dict(tile=2, replay=tiles - 1) and list(g._graphs) == [n]
    a.push(xd[:, tiles * n :, :], final=True)
    g.push(xd[:, tiles * n :, :], final=True)
    assert g.max_track >= T
    _check_finish(g.finish(), one, T)
    _check_finish(a.finish(), one, T)


def test_window_lag_failure_raises_and_the_rows_in_front_are_the_one_shot_rows():
    """test_hip_stream_xylo.py's lag failure: lag_frames=0 and 16-frame tiles leave a raster window of 768 frames, digital silence holds
    the horizon back for 2000 frames, the window slides past frames that were never integrated and finish() refuses.  What was emitted
    before is final: the one-shot rows."""
    from haghighatshoarmuir2024_amd import _lib

    T = 3200
    x = np.array(_input(4799)[:, :T, :])
    x[:, 600:2600, :] = 0.0
    one = _one_shot(T, x=x)
    demo = _demo()
    L2 = len(demo.beamfs[0].kernel) // 2
    s = demo.streaming_localizer(2, total_frames=T, wrap_tail=x[:, T - L2 :, :], max_tile=16, lag_frames=0, track=_env())
    assert s.cap == 768 and s.max_track == T
    for t in range(0, T, 16):
        s.push(x[:, t : t + 16, :])
    st = s.status()
    assert st["lag_failures"] > 0 and 0 < st["frames"] < T
    w = s.tracked()
    assert w["count"] == st["frames"] and w["first"] == 0
    np.testing.assert_array_equal(_host(w["index"]), one["index"][:, : w["count"]])
    np.testing.assert_array_equal(_bits(_host(w["peak_envelope"])), _bits(one["peak_env"][:, : w["count"]]))
    assert float(one["peak_env"][:, : w["count"]].max()) > 0.0
    with pytest.raises(_lib.MiclocError, match="window"):
        s.finish()


def test_finish_refuses_a_ring_shorter_than_the_recording():
    from haghighatshoarmuir2024_amd import _lib

    T = 4799
    x = _input(T)
    tiles = _tiles("by1200", T)
    s = _stream(T, x, tiles, max_track=4096)
    assert s.min_track <= 4096 < T
    t = 0
    for n in tiles:
        s.push(x[:, t : t + n, :])
        t += n
    with pytest.raises(_lib.MiclocError, match="max_track"):
        s.finish()


def test_two_bands_are_refused_before_any_device_work(monkeypatch):
    from haghighatshoarmuir2024_amd import runtime

    two = _demo(bands=((1000, 1600), (1600, 2400)))
    assert two.streaming_localizer(2, max_tile=400) is not None  # (the stream itself serves two bands)

    def no_plan(*a, **k):
        raise AssertionError("a plan was built before the refusal")

    monkeypatch.setattr(runtime, "Plan", no_plan)
    with pytest.raises(ValueError, match="one band"):
        two.streaming_localizer(2, max_tile=400, track=_env())
    with pytest.raises(ValueError, match="one band"):
        two.track_batch(np.array(_input(209)), _env())


@pytest.mark.parametrize("mode", ["parity", "throughput"])
def test_sweep_through_the_tracked_stream_equals_the_fused_call(mode):
    from haghighatshoarmuir2024_amd.sweep import xylo_moving_target_sweep, xylo_stream_track_localizer, xylo_track_localizer

    demo, env = _demo(), _env()
    kw = dict(snr_db_vec=[10.0, 20.0], num_sim=2, seed=5, mode=mode, batch_trials=2)  # T = 4799: three tiles of 1600
    ref = xylo_moving_target_sweep(demo, env, localizer=xylo_track_localizer(demo, env, max_batch=2), **kw)
    got = xylo_moving_target_sweep(demo, env, localizer=xylo_stream_track_localizer(demo, env, tile=1600, max_batch=2), **kw)
    keys = [k for k, v in ref.items() if isinstance(v, np.ndarray)]
    assert {"phase", "err", "med", "track_mae_deg", "track_median_deg"} <= set(keys) and ref["err"].shape == (2, 2)
    assert got["parity"] == "unpinned (integer LIF)"
    for k in keys:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert np.all(ref["err"] > 0)
    with pytest.raises(ValueError):
        xylo_stream_track_localizer(demo, env, tile=0)
