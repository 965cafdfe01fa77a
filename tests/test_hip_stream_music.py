"""MUSIC as a stream on the MI355X (streaming.MusicStreamingLocalizer, csrc/stream_music.hip): any tiling ends on MUSIC.localize_batch's
bits; the shapes at which the kernels take another path; push_replay, the ring, two streams at once; the stream and
localization_demo_MUSIC.Demo against the reference's goldens (tests/golden/make_golden_music.py, make_golden_music_demo.py)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

from haghighatshoarmuir2024_amd import _lib
from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray

pytestmark = pytest.mark.gpu

FS = 8000
L = 512
SPEC_TOL = 1e-9  # relative to the spectrum's maximum (tests/test_hip_music.py)


def _music(G=33, band=(1000.0, 2000.0), fs=FS, frame_duration=L / FS, M=7):
    from micloc.music_beamformer import MUSIC

    return MUSIC(geometry=CenterCircularArray(radius=4.5e-2, num_mic=M), freq_range=list(band), doa_list=np.linspace(-np.pi, np.pi, G),
                 frame_duration=frame_duration, fs=fs)


def _signal(seed, B, T, M=7, fs=FS):
    """Two tones inside the band from two directions plus white noise, per trial."""
    rng = np.random.RandomState(seed)
    t = np.arange(T) / fs
    x = 0.3 * rng.randn(B, T, M)
    for b in range(B):
        for f, amp in ((1300.0 + 40 * b, 1.0), (1700.0, 0.5)):
            x[b] += amp * np.sin(2 * np.pi * f * t[:, None] + rng.uniform(0, 2 * np.pi, M)[None, :])
    return x


def _tilings(T, seed=0):
    rng = np.random.RandomState(seed)
    rnd = []
    while sum(rnd) < T:
        rnd.append(int(min(rng.randint(1, 700), T - sum(rnd))))
    out = {"one": [T], "random": rnd}
    for n in (7, 128, L, L + 1, 2 * L + 5):
        out[str(n)] = [n] * (T // n) + ([T % n] if T % n else [])
    return out


def _host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _one_shot(m, x, k, ov, N):
    return _host(m.localize_batch(x, k, ov, N, want_sel=True))


def _stream(m, x, k, ov, N, tiles, total=True, **kw):
    """x: device tensor [B, T, M]; -> (finish() on the host, the localizer)."""
    B, T, _ = x.shape
    loc = m.streaming_localizer(B, k, ov, N, total_frames=T if total else None, max_tile=max(tiles), **kw)
    t = 0
    for i, n in enumerate(tiles):
        loc.push(x[:, t : t + n, :], final=None if total else i == len(tiles) - 1)
        t += n
    return _host(loc.finish()), loc


def _assert_same_bits(got, ref, what):
    for key, rkey in (("spectrum", "spectrum"), ("sel", "sel"), ("power", "power"), ("argmax", "argmax")):
        assert got[key].shape == ref[rkey].shape and np.array_equal(got[key], ref[rkey]), f"{what}: {key} differs"
    assert np.array_equal(got["slice_argmax"], np.argmax(ref["spectrum"], axis=2)), f"{what}: slice_argmax differs"


# ---- 1. any tiling, localize_batch's bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 128, 384])
@pytest.mark.parametrize("k", [0, 1, 16])
def test_any_tiling_gives_localize_batch_bits(overlap, k):
    import torch

    N, B, T = 128, 3, 3 * L + 300
    m = _music()
    assert len(m.in_band_bins(N)) == 16  # k = 16 is nbin
    x = _signal(10 + overlap, B, T)
    ov = overlap / FS
    ref = _one_shot(m, x, k, ov, N)
    starts, lens, _, _ = m.slice_plan(T, ov)
    # the last slice is the leftover one, with fewer frames than a full slice (without overlap: F' = 2 < F = 4)
    assert L // 2 < lens[-1] < L and lens[-1] // N == (2 if overlap < 384 else 3) and ref["spectrum"].shape == (B, len(starts), 33)
    xd = torch.from_numpy(x).cuda()
    for name, tiles in _tilings(T).items():
        got, loc = _stream(m, xd, k, ov, N, tiles)
        _assert_same_bits(got, ref, f"overlap {overlap}, k {k}, tiling {name}")
        assert got["slice_count"] == len(starts)
        assert loc.status() == dict(pushed=T, slices=len(starts), open=0, short_leftover=0)


# ---- 2. the shapes at which the kernels can go wrong -----------------------------------------------------------------------------------
SHAPES = {
    "N=100 (Np=128, 2 nbin=24)": dict(N=100),
    "N=127 (odd)": dict(N=127),
    "2 nbin=26": dict(band=(1000.0, 1800.0)),
    "B=10 (rows cross a 64-row block)": dict(B=10),
    "G=130": dict(G=130),
    "G=257 (two passes of the steering loop)": dict(G=257),
    "leftover of exactly L/2: no leftover slice": dict(T=2 * L + L // 2, slices=2),
    "leftover of L/2 + 1": dict(T=2 * L + L // 2 + 1, slices=3),
    "T < L: only a leftover slice": dict(T=300, slices=1),
    # (every leftover slice is shorter than N = L: lengths without one)
    "N = L: one frame per slice, back to back": dict(N=L, band=(1000.0, 1100.0), T=4 * L, slices=4, overlaps=(0, 256)),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_edge_shapes(name):
    import torch

    c = dict(N=128, band=(1000.0, 2000.0), B=2, G=33, T=2 * L + 300, slices=None, overlaps=(0, 384))
    c.update(SHAPES[name])
    m = _music(G=c["G"], band=c["band"])
    x = _signal(77, c["B"], c["T"])
    nbin = len(m.in_band_bins(c["N"]))
    k = min(3, nbin)
    xd = torch.from_numpy(x).cuda()
    for ov in (o / FS for o in c["overlaps"]):
        ref = _one_shot(m, x, k, ov, c["N"])
        if c["slices"] is not None and ov == 0.0:
            assert ref["spectrum"].shape[1] == c["slices"]
        for tiles in ([c["T"]], [97] * (c["T"] // 97) + ([c["T"] % 97] if c["T"] % 97 else [])):
            got, _ = _stream(m, xd, k, ov, c["N"], tiles)
            _assert_same_bits(got, ref, f"{name}, overlap {ov}, tiles of {tiles[0]}")


def test_recordings_without_a_usable_slice_raise_what_localize_batch_raises():
    import torch

    m = _music()
    # T <= L / 2: no slice at all
    x = _signal(5, 1, L // 2)
    with pytest.raises(ValueError) as one:
        m.localize_batch(x, 1, 0.0, 128)
    loc = m.streaming_localizer(1, 1, 0.0, 128)
    loc.push(x[:, :100]), loc.push(x[:, 100:], final=True)
    with pytest.raises(ValueError) as two:
        loc.finish()
    assert str(one.value) == str(two.value) and "has no slice" in str(two.value)
    assert loc.status() == dict(pushed=L // 2, slices=0, open=0, short_leftover=0)
    # a leftover slice of more than L / 2 and fewer than N samples: localize_batch's broadcast refusal, with the same text
    x = _signal(6, 2, L + 300)
    with pytest.raises(ValueError) as one:
        m.localize_batch(x, 1, 0.0, 400)
    loc = m.streaming_localizer(2, 1, 0.0, 400)  # a live source: the length is not known in advance
    loc.push(torch.from_numpy(x).cuda(), final=True)
    assert loc.status() == dict(pushed=L + 300, slices=1, open=0, short_leftover=1)
    with pytest.raises(ValueError) as two:
        loc.finish()
    assert str(one.value) == str(two.value) and "shorter than the FFT length 400" in str(two.value)
    with pytest.raises(_lib.MiclocError, match="the stream has ended"):
        loc.push(x[:, :10])


# ---- 3. push_replay, the ring, the newest slice ----------------------------------------------------------------------------------------
def test_push_replay_equals_push_and_the_ring_keeps_the_newest_slices():
    import torch

    N, B, n, tiles, k, ov = 128, 2, 96, 19, 2, 384 / FS  # hop = 128 is no multiple of the tile
    T = n * tiles
    m = _music()
    x = _signal(21, B, T)
    ref = _one_shot(m, x, k, ov, N)
    S = ref["spectrum"].shape[1]
    assert S == 12
    xd = torch.from_numpy(x).cuda()
    got, _ = _stream(m, xd, k, ov, N, [n] * tiles)
    _assert_same_bits(got, ref, "push")
    loc = m.streaming_localizer(B, k, ov, N, total_frames=T, max_tile=n)
    small = m.streaming_localizer(B, k, ov, N, total_frames=T, max_tile=n, max_slices=5)
    for i in range(tiles):
        loc.push_replay(xd[:, i * n : (i + 1) * n]), small.push_replay(xd[:, i * n : (i + 1) * n])
        if i == 9:  # 960 samples: slices 0 .. 3 have ended, the slices that began at 512 .. 896 are open
            assert loc.status() == dict(pushed=960, slices=4, open=4, short_leftover=0)
            lp, la = (v.cpu().numpy() for v in loc.latest_window())
            assert np.array_equal(lp, ref["spectrum"][:, 3]) and np.array_equal(la, np.argmax(ref["spectrum"][:, 3], axis=1))
    assert set(loc._graphs) == {n} and loc.done
    _assert_same_bits(_host(loc.finish()), ref, "push_replay")
    lp, la = (v.cpu().numpy() for v in loc.latest_window())
    assert np.array_equal(lp, ref["spectrum"][:, -1]) and np.array_equal(la, np.argmax(ref["spectrum"][:, -1], axis=1))
    # a ring of 5 rows: the newest 5 slices, the running read-out over all 12
    w = _host(small.windows())
    assert (w["count"], w["first"]) == (S, S - 5) and np.array_equal(w["window_start"], np.arange(S - 5, S) * 128)
    assert np.array_equal(w["spectrum"], ref["spectrum"][:, S - 5 :]) and np.array_equal(w["sel"], ref["sel"][:, S - 5 :])
    assert np.array_equal(w["window_argmax"], np.argmax(ref["spectrum"][:, S - 5 :], axis=2))
    assert np.array_equal(small.power.cpu().numpy(), ref["power"]) and np.array_equal(small.argmax.cpu().numpy(), ref["argmax"])
    with pytest.raises(_lib.MiclocError, match="the ring keeps 5"):
        small.finish()


# ---- 4. against the reference -------------------------------------------------------------------------------------------------------------
def test_stream_matches_the_reference_apply_to_signal():
    import torch

    from test_hip_music import test_signal

    z = np.load(os.path.join(GOLDEN, "music_apply_signal.npz"))
    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    for i in range(int(z["num_cases"])):
        pre = f"c{i}_"
        m = _music(G=121, band=(1000.0, 4000.0), fs=48_000, frame_duration=float(z[pre + "frame_duration"]))
        T = int(z[pre + "T"])
        sig = test_signal(int(z[pre + "seed"]), T, 7, geo.r_vec, geo.theta_vec)
        tiles = [1000] * (T // 1000) + ([T % 1000] if T % 1000 else [])
        got, _ = _stream(m, torch.from_numpy(sig[None]).cuda(), int(z[pre + "k"]), float(z[pre + "overlap"]), int(z[pre + "N"]), tiles)
        want = z[pre + "spectrum"]
        assert got["spectrum"][0].shape == want.shape
        err = float(np.max(np.abs(got["spectrum"][0] - want)) / np.max(np.abs(want)))
        print(f"apply_to_signal case {i}: stream vs reference, rel err {err:.3e}")
        assert err <= SPEC_TOL


def test_demo_matches_the_reference_loop():
    from micloc.localization_demo_MUSIC import Demo

    z = np.load(os.path.join(GOLDEN, "music_demo.npz"))
    G = int(z["G"])
    demo = Demo(geometry=CenterCircularArray(radius=float(z["radius"]), num_mic=int(z["num_mic"])), freq_range=z["band"], num_active_freq=int(z["k"]),
                doa_list=np.linspace(-np.pi, np.pi, G), recording_duration=0.25, num_fft_bin=int(z["N"]), fs=int(z["fs"]))
    packs, active, methods = z["packs"], z["active"], [str(s) for s in z["methods"]]
    assert active.tolist() == [True, True, False]
    rows = iter(range(int(active.sum())))
    for p, a in zip(packs, active):
        if not a:
            assert np.isnan(demo.process_frame(p))  # the same NaN pack
            continue
        r = next(rows)
        spec = demo.power_grid(np.asarray(p[:, :-1], dtype=np.float64))
        err = float(np.max(np.abs(spec - z["ang_pow_spec"][r])) / np.max(np.abs(z["ang_pow_spec"][r])))
        print(f"demo pack {r}: spectrum rel err {err:.3e}")
        assert err <= SPEC_TOL
        for i, method in enumerate(methods):
            assert not z["doa_index_error"][r, i]
            got = demo.process_frame(p, method=method)
            if method == "peak":
                assert got == z["doa"][r, i] / np.pi * 180  # the same peak DoA
            else:
                print(f"demo pack {r}: {method} differs by {abs(got * np.pi / 180 - z['doa'][r, i]):.3e} rad")
                assert abs(got * np.pi / 180 - z["doa"][r, i]) <= 1e-9
    for i, method in enumerate(methods):
        got = demo.process_frames(packs, method=method)
        assert np.isnan(got[~active]).all() and not np.isnan(got[active]).any()
        assert np.array_equal(got[active], [demo.process_frame(p, method=method) for p in packs[active]])  # one batch, the loop's bits
    # the demo's stream: a pack per tile, the slice of a tile is the pack's `beamforming`
    loc = demo.streaming_localizer(batch=1)
    for p in packs[active]:
        sig = np.asarray(p[None, :, :-1], dtype=np.float64)
        loc.push_replay(sig)
        assert np.array_equal(loc.latest_window()[0].cpu().numpy()[0], demo.power_grid(sig[0]))
    assert loc.status()["slices"] == int(active.sum())


# ---- 5. two streams on two HIP streams ---------------------------------------------------------------------------------------------------
def test_two_interleaved_streams_end_on_the_bits_of_each_alone():
    import torch

    N, B, T, k = 128, 2, 2 * L + 300, 2
    m = _music()
    xs = [torch.from_numpy(_signal(40 + i, B, T)).cuda() for i in range(2)]
    ovs = (0.0, 128 / FS)
    tiles = ([200] * 6 + [124], [333] * 3 + [325])
    alone = [_stream(m, x, k, ov, N, t)[0] for x, ov, t in zip(xs, ovs, tiles)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    locs = []
    for s, ov, t in zip(streams, ovs, tiles):
        with torch.cuda.stream(s):
            locs.append(m.streaming_localizer(B, k, ov, N, total_frames=T, max_tile=max(t)))
    pos = [0, 0]
    for step in range(max(len(t) for t in tiles)):
        for i in range(2):
            if step < len(tiles[i]):
                with torch.cuda.stream(streams[i]):
                    n = tiles[i][step]
                    locs[i].push(xs[i][:, pos[i] : pos[i] + n])
                    pos[i] += n
    for i in range(2):
        with torch.cuda.stream(streams[i]):
            got = _host(locs[i].finish())
        for key in ("spectrum", "sel", "power", "argmax", "slice_argmax"):
            assert np.array_equal(got[key], alone[i][key]), (i, key)
    torch.cuda.synchronize()
