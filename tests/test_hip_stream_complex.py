"""The complex Beamformer as a stream (include/micloc_hip.h "streaming, complex Beamformer") on the MI355X: band-pass tiles against the
one-shot rows, finish() against Beamformer.localize_batch bit for bit for any tiling, the running read-out, the windows, the reference's
fixture, status codes.  The clock's bookkeeping is the NumPy restatement of tests/test_stream_complex_cpu.py."""
import ctypes
import threading

import numpy as np
import pytest

from conftest import golden
from test_stream_complex_cpu import bookkeeping, random_tiling

pytestmark = pytest.mark.gpu

FS = 48_000


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_BEAMF = {}


def beamformer(M):
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer

    if M not in _BEAMF:
        _BEAMF[M] = Beamformer(CenterCircularArray(4.5e-2, M), 10e-3, [1000.0, 2000.0], fs=FS)
    return _BEAMF[M]


def random_bf_mat(rng, M, G):
    return rng.standard_normal((M, G)) + 1j * rng.standard_normal((M, G))


def stream(bf, W, x, tiles, replay=False, **kw):
    """Push x [B, T, M] in `tiles` (the last one final) -> (localizer, finish())."""
    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

    B, T, M = x.shape
    assert sum(tiles) == T
    kw.setdefault("wrap_tail", ComplexStreamingLocalizer.wrap_rows(x, len(bf.kernel)))
    kw.setdefault("max_tile", max(tiles))
    loc = bf.streaming_localizer(W, batch=B, total_frames=T, **kw)
    t = 0
    for n in tiles:
        (loc.push_replay if replay else loc.push)(x[:, t : t + n, :])
        t += n
    return loc, loc.finish()


# ---- 1. the band-pass tile kernel against the one-shot rows ----------------------------------------------------------------------------
def _filters():
    from scipy.signal import butter

    rng = np.random.default_rng(5)
    poles = np.array([0.7, 0.5 + 0.6j, 0.5 - 0.6j])
    return {"butter1": butter(1, [1000.0, 2000.0], btype="bandpass", fs=FS), "butter2": butter(2, [1000.0, 2000.0], btype="bandpass", fs=FS),
            "random4": (rng.uniform(0.2, 1.0, 4) * np.array([1, -1, 1, -1]), np.real(np.poly(poles)))}


@pytest.mark.parametrize("filt", ["butter1", "butter2", "random4"])
@pytest.mark.parametrize("M", [1, 7, 16])
@pytest.mark.parametrize("B", [1, 3])
def test_bandpass_tiles_equal_the_one_shot_rows(B, M, filt, cfg2, torch):
    from haghighatshoarmuir2024_amd import _lib, runtime

    b, a = _filters()[filt]
    assert np.all(np.asarray(b) != 0) or filt != "random4"
    rng = np.random.default_rng(100 * B + M)
    plan = runtime.Plan(M, cfg2["kernel"], b, a, 1, False)
    plan.set_bf_mat(random_bf_mat(rng, M, 3))
    lib, dev, C = plan.lib, plan.device, 2 * M
    CH = plan.window_quantum()
    st = lambda: runtime._stream(dev)
    GUARD = 512  # bytes of sentinel on either side of the state and of the workspace

    def guarded(nbytes):
        buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 256 == 0
        return buf, buf[GUARD : GUARD + nbytes]

    def guards_intact(buf):
        return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())

    for T, tilings in ((1001, [[1001], [16] * 62 + [9], [1] * 40 + [961], random_tiling(np.random.default_rng(7), 1001, 300)]), (1, [[1]])):
        Ts = plan.padded_T(T)
        h = torch.from_numpy(rng.standard_normal((B, C, Ts))).to(dev)
        pre, _ = plan.bandpass_rzcc(h, T, want_pre=True, want_spikes=False)  # the one-shot launch's `pre` rows
        pre = pre.cpu().numpy()
        max_tile = max(max(t) for t in tilings)
        Ks = (max_tile + 2 * CH - 2) // CH
        nstate = lib.micloc_stream_complex_state_bytes(plan.handle, B)
        nws = lib.micloc_stream_complex_workspace_bytes(plan.handle, B, max_tile)
        assert nstate >= 256 + 8 * B * C * (CH + len(np.atleast_1d(a)) - 1) and nws >= 8 * B * C * Ks * CH
        state_buf, state = guarded(nstate)
        ws_buf, ws = guarded(nws)
        staging = ws[: 8 * B * C * Ks * CH].view(torch.float64).view(B, C, Ks * CH)
        for tiles in tilings * 2:  # every tiling twice: the second stream starts from a reset, not from a fresh allocation
            _lib.check(lib.micloc_stream_complex_reset(plan.handle, B, runtime._ptr(state), nstate, st()), "reset")
            log = bookkeeping(tiles, CH)
            t0 = fill = 0
            for i, n in enumerate(tiles):
                final = int(i == len(tiles) - 1)
                _lib.check(lib.micloc_stream_complex_bandpass_tile_f64(plan.handle, runtime._ptr(h), B, n, Ts, t0, max_tile, runtime._ptr(state), nstate,
                                                                       runtime._ptr(ws), nws, st()), "bandpass_tile")
                got = staging[:, :, : -(-(fill + n) // CH) * CH].cpu().numpy()
                # [carry | tile] are the one-shot rows of the frames [t0 - fill, t0 + n); zeros up to the chunk border
                np.testing.assert_array_equal(got[:, :, : fill + n], pre[:, :, t0 - fill : t0 + n], err_msg=f"T {T} tiles {tiles[:4]}.. tile {i}")
                assert not got[:, :, fill + n :].any()
                _lib.check(lib.micloc_stream_complex_localize_tile_f64(plan.handle, runtime._ptr(state), nstate, B, max_tile, final, None, None,
                                                                       runtime._ptr(ws), nws, st()), "localize_tile")
                t0 += n
                fill = log[i]["carry"]
            st4 = (ctypes.c_int * 4)()
            _lib.check(lib.micloc_stream_complex_status(runtime._ptr(state), st4, st()), "status")
            assert list(st4) == [log[-1]["chunks"], T, 0, T]
        assert guards_intact(state_buf) and guards_intact(ws_buf)


# ---- 2. finish() against the one-shot call ---------------------------------------------------------------------------------------------
def tilings_of(T, CH, seed):
    short = 100 if T > 100 else 1  # shorter than a chunk throughout
    out = [[T], [short] * (T // short) + ([T % short] if T % short else []), random_tiling(np.random.default_rng(seed), T, 2 * CH + 50)]
    return [t for i, t in enumerate(out) if t not in out[:i]]


@pytest.mark.parametrize("G", [1, 57, 449])
@pytest.mark.parametrize("M", [7, 9, 20])  # beamform_wsc_kernel (up to 8 microphones), beamform_gen_kernel with 2 and 3 channel tiles
@pytest.mark.parametrize("B", [1, 3])
def test_finish_equals_localize_batch_bit_for_bit(B, M, G, torch):
    bf = beamformer(M)
    rng = np.random.default_rng(1000 * B + 10 * M + G)
    W = random_bf_mat(rng, M, G)
    bf.plan().set_bf_mat(W)
    CH = bf.plan().window_quantum()
    for T in (1, 2, CH - 1, CH, CH + 1, 2 * CH + 3, 4799):
        x = rng.standard_normal((B, T, M))
        ref = bf.localize_batch(W, x)
        for tiles in tilings_of(T, CH, T):
            loc, out = stream(bf, W, x, tiles)
            assert torch.equal(out["power"], ref["power"]), f"T {T} tiles {tiles[:5]}.."
            assert torch.equal(out["argmax"], ref["argmax"]), f"T {T} tiles {tiles[:5]}.."
            assert loc.status() == dict(chunks=-(-T // CH), frames=T, carry=0, pushed=T)


def test_push_replay_with_two_captured_tile_lengths(torch):
    bf = beamformer(7)
    rng = np.random.default_rng(3)
    W = random_bf_mat(rng, 7, 449)
    x = rng.standard_normal((3, 4799, 7))
    ref = bf.localize_batch(W, x)
    tiles = [300] * 6 + [500] * 5 + [499]
    loc, out = stream(bf, W, x, tiles, replay=True)
    assert sorted(loc._graphs) == [300, 500]  # captured on their second occurrence, replayed from then on
    assert torch.equal(out["power"], ref["power"]) and torch.equal(out["argmax"], ref["argmax"])


# ---- 3. the running read-out -------------------------------------------------------------------------------------------------------------
def test_running_readout_is_the_prefix_result(torch):
    """Mid-stream the power is the mean over the whole chunks contracted so far.  It is compared with localize_batch on that prefix for a
    stream pushed with wrap_tail set to THE PREFIX'S OWN wrap rows (np.roll wraps the prefix, not the recording), to the project's
    tolerance for a power reduced in another order (1e-12 relative)."""
    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

    bf = beamformer(7)
    rng = np.random.default_rng(11)
    W = random_bf_mat(rng, 7, 57)
    B, T = 2, 1100
    x = rng.standard_normal((B, T, 7))
    tiles = [100, 300, 300, 300, 100]
    CH = bf.plan().window_quantum()
    log = bookkeeping(tiles, CH)
    checked = 0
    for k in range(len(tiles) - 1):
        frames = log[k]["frames"]
        wrap = ComplexStreamingLocalizer.wrap_rows(x[:, : max(frames, 1), :], len(bf.kernel))
        loc = bf.streaming_localizer(W, batch=B, wrap_tail=wrap, max_tile=300)
        t = 0
        for n in tiles[: k + 1]:
            power, argmax = loc.push(x[:, t : t + n, :], final=False)
            t += n
        s = loc.status()
        assert s == dict(chunks=log[k]["chunks"], frames=frames, carry=log[k]["carry"], pushed=t)
        if frames == 0:  # no chunk is complete yet
            assert not power.any() and not argmax.any()
            continue
        ref = bf.localize_batch(W, x[:, :frames, :])
        np.testing.assert_allclose(power.cpu().numpy(), ref["power"].cpu().numpy(), rtol=1e-12, atol=0)
        assert torch.equal(argmax, ref["argmax"])
        checked += 1
    assert checked == 3


# ---- 4. windows ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tname", ["CH", "3CH+5", "4799"])
@pytest.mark.parametrize("wh", [(1, 1), (2, 1), (4, 2)])
def test_windows_equal_the_one_shot_rows(wh, Tname, torch):
    bf = beamformer(7)
    rng = np.random.default_rng(17)
    W = random_bf_mat(rng, 7, 57)
    bf.plan().set_bf_mat(W)
    CH = bf.plan().window_quantum()
    T = {"CH": CH, "3CH+5": 3 * CH + 5, "4799": 4799}[Tname]
    window, hop = wh[0] * CH, wh[1] * CH
    B = 2
    x = rng.standard_normal((B, T, 7))
    ref = bf.localize_batch(W, x, window=window, hop=hop)
    nW = ref["window_power"].shape[1]
    for tiles in ([T], random_tiling(np.random.default_rng(T), T, 700), [100] * (T // 100) + ([T % 100] if T % 100 else [])):
        from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

        loc = bf.streaming_localizer(W, batch=B, total_frames=T, wrap_tail=ComplexStreamingLocalizer.wrap_rows(x, len(bf.kernel)), max_tile=max(tiles),
                                     window=window, hop=hop)
        log = bookkeeping(tiles, CH, window, hop)
        t = 0
        for n, s in zip(tiles, log):
            loc.push(x[:, t : t + n, :])
            t += n
            w = loc.windows()
            assert w["count"] == s["windows"]  # emitted as soon as the window's last chunk has been contracted
            assert torch.equal(w["window_power"], ref["window_power"][:, : w["count"]])  # an emitted row has its final bits
            if w["count"]:
                lp, la = loc.latest_window()
                assert torch.equal(lp, ref["window_power"][:, w["count"] - 1]) and torch.equal(la, ref["window_argmax"][:, w["count"] - 1])
        out = loc.finish()
        assert out["window_count"] == nW
        assert torch.equal(out["window_power"], ref["window_power"]) and torch.equal(out["window_argmax"], ref["window_argmax"])
        assert torch.equal(out["power"], ref["power"]) and torch.equal(out["argmax"], ref["argmax"])


def test_windows_not_in_the_count_are_not_emitted_and_the_ring_wraps(torch):
    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

    bf = beamformer(7)
    rng = np.random.default_rng(19)
    W = random_bf_mat(rng, 7, 57)
    bf.plan().set_bf_mat(W)
    CH = bf.plan().window_quantum()
    # the header's case: T = 1100, window = 4 CH, hop = CH: windows 2, 3 and 4 start before T but are not in the count of 2
    x = rng.standard_normal((1, 1100, 7))
    ref = bf.localize_batch(W, x, window=4 * CH, hop=CH)
    assert ref["window_power"].shape[1] == 2
    loc, out = stream(bf, W, x, [300, 300, 300, 200], window=4 * CH, hop=CH)
    assert out["window_count"] == 2
    assert torch.equal(out["window_power"], ref["window_power"]) and torch.equal(out["window_argmax"], ref["window_argmax"])
    # a ring of two rows: the two newest windows survive, window n in row n % 2
    T = 4799
    x = rng.standard_normal((2, T, 7))
    ref = bf.localize_batch(W, x, window=CH, hop=CH)
    nW = ref["window_power"].shape[1]
    loc = bf.streaming_localizer(W, batch=2, wrap_tail=ComplexStreamingLocalizer.wrap_rows(x, len(bf.kernel)), max_tile=700, window=CH, hop=CH,
                                 max_windows=2)
    tiles = random_tiling(np.random.default_rng(23), T, 700)
    t = 0
    for i, n in enumerate(tiles):
        loc.push(x[:, t : t + n, :], final=i == len(tiles) - 1)
        t += n
    w = loc.finish()
    assert w["window_count"] == nW and nW > 2
    assert torch.equal(w["window_power"], ref["window_power"][:, nW - 2 :]) and torch.equal(w["window_argmax"], ref["window_argmax"][:, nW - 2 :])
    for n in (nW - 2, nW - 1):
        assert torch.equal(loc.window_power[:, n % 2], ref["window_power"][:, n])


@pytest.mark.parametrize("G", [57, 449])  # Ghp padded past G; two columns per thread
def test_replayed_windows_on_folded_rows(G, torch):
    """The window read-out on folded rows inside a captured graph: two windows open at once, the last one cut at the end of the recording,
    a ring shorter than the recording -- push_replay against push after every tile, and every row against the one-shot call."""
    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

    bf = beamformer(7)
    rng = np.random.default_rng(29)
    W = random_bf_mat(rng, 7, G)
    bf.plan().set_bf_mat(W)
    CH = bf.plan().window_quantum()
    B, T = 2, 3 * CH + 5
    window, hop = 2 * CH, CH
    x = rng.standard_normal((B, T, 7))
    tiles = [160] * 4 + [T - 640]  # the first 160 eager, captured on the second and replayed for tiles 2, 3 and 4; the final tile is pushed eagerly
    ref = bf.localize_batch(W, x, window=window, hop=hop)
    nW = ref["window_power"].shape[1]
    assert nW == 3
    kw = dict(batch=B, total_frames=T, wrap_tail=ComplexStreamingLocalizer.wrap_rows(x, len(bf.kernel)), max_tile=160, window=window, hop=hop)
    replayed = bf.streaming_localizer(W, max_windows=2, **kw)
    eager = bf.streaming_localizer(W, max_windows=2, **kw)
    t = 0
    for n, s in zip(tiles, bookkeeping(tiles, CH, window, hop)):
        pr, ar = replayed.push_replay(x[:, t : t + n, :])
        pe, ae = eager.push(x[:, t : t + n, :])
        t += n
        assert torch.equal(pr, pe) and torch.equal(ar, ae)
        wr, we = replayed.windows(), eager.windows()
        assert wr["count"] == we["count"] == s["windows"] and wr["first"] == we["first"] == max(0, s["windows"] - 2)
        assert torch.equal(wr["window_power"], we["window_power"]) and torch.equal(wr["window_argmax"], we["window_argmax"])
        assert torch.equal(wr["window_power"], ref["window_power"][:, wr["first"] : wr["count"]])  # the rows in the ring: the one-shot bits
        assert torch.equal(wr["window_argmax"], ref["window_argmax"][:, wr["first"] : wr["count"]])
        for a, b in zip(replayed.latest_window(), eager.latest_window()):
            assert torch.equal(a, b)
        if wr["count"]:
            assert torch.equal(replayed.latest_window()[0], ref["window_power"][:, wr["count"] - 1])
    assert wr["count"] == nW
    assert sorted(replayed._graphs) == [160] and not eager._graphs
    for loc in (replayed, eager):
        with pytest.raises(_lib.MiclocError, match="max_windows"):  # a ring of 2 rows for 3 windows
            loc.finish()
    # every row against the one-shot call: the same input once more with the default ring depth
    loc, out = stream(bf, W, x, tiles, replay=True, window=window, hop=hop)
    assert sorted(loc._graphs) == [160] and out["window_count"] == nW
    assert torch.equal(out["window_power"], ref["window_power"]) and torch.equal(out["window_argmax"], ref["window_argmax"])
    assert torch.equal(out["power"], ref["power"]) and torch.equal(out["argmax"], ref["argmax"])


# ---- 5. the reference's fixture ------------------------------------------------------------------------------------------------------------
def test_reference_trial_pushed_in_packs(torch):
    """The noisy trial of the reference's Beamformer (tests/golden/beamformer_c128_g449.npz, the tolerances of tests/test_hip_pins_r5.py for
    it) pushed the way a live loop delivers audio: equal packs, a quarter of the recording each."""
    z = golden("beamformer_c128_g449.npz")
    bf = beamformer(7)
    x = z["sig_in"][None]
    T = x.shape[1]
    pack = -(-T // 4)
    tiles = [pack] * 3 + [T - 3 * pack]
    _, out = stream(bf, z["bf_mat"], x, tiles, replay=True)
    np.testing.assert_allclose(out["power"][0].cpu().numpy(), z["power"], rtol=1e-10)
    assert int(out["argmax"][0]) == int(z["argmax"])


# ---- 6. status codes, ValueErrors, threads ---------------------------------------------------------------------------------------------
def test_status_codes_and_value_errors(cfg2, torch):
    from haghighatshoarmuir2024_amd import _lib, runtime

    bf = beamformer(7)
    rng = np.random.default_rng(29)
    W = random_bf_mat(rng, 7, 57)
    plan = runtime.Plan(7, cfg2["kernel"], cfg2["b"], cfg2["a"], 1, False)
    lib, dev = plan.lib, plan.device
    st = runtime._stream(dev)
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    p = runtime._ptr(buf)
    # no bf_mat
    assert lib.micloc_stream_complex_state_bytes(plan.handle, 1) == 0
    assert lib.micloc_stream_complex_reset(plan.handle, 1, p, 1 << 20, st) == _lib.MICLOC_ERR_NOT_SET
    # a real bf_mat belongs to the SNN stream
    plan.set_neuron_kernel(cfg2["nir"])
    plan.set_bf_mat(cfg2["bf_mat"])
    assert lib.micloc_stream_complex_state_bytes(plan.handle, 1) == 0
    assert lib.micloc_stream_complex_workspace_bytes(plan.handle, 1, 100) == 0
    assert lib.micloc_stream_complex_reset(plan.handle, 1, p, 1 << 20, st) == _lib.MICLOC_ERR_SHAPE
    assert lib.micloc_stream_complex_localize_tile_f64(plan.handle, p, 1 << 20, 1, 100, 0, None, None, p, 1 << 20, st) == _lib.MICLOC_ERR_SHAPE
    with pytest.raises(ValueError):
        bf.streaming_localizer(cfg2["bf_mat"][:7].real, batch=1)
    # a complex one
    plan.set_bf_mat(W)
    CH = plan.window_quantum()
    nstate = lib.micloc_stream_complex_state_bytes(plan.handle, 2)
    nws = lib.micloc_stream_complex_workspace_bytes(plan.handle, 2, 100)
    assert 0 < nstate <= 1 << 20 and 0 < nws <= 1 << 20 and nstate % 256 == 0 and nws % 256 == 0
    assert lib.micloc_stream_complex_reset(plan.handle, 0, p, nstate, st) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_complex_reset(plan.handle, 2, p, nstate - 1, st) == _lib.MICLOC_ERR_WORKSPACE  # short state
    assert lib.micloc_stream_complex_reset(plan.handle, 2, ctypes.c_void_p(buf.data_ptr() + 8), nstate, st) == _lib.MICLOC_ERR_WORKSPACE  # misaligned
    assert lib.micloc_stream_complex_reset(plan.handle, 2, p, nstate, st) == _lib.MICLOC_OK
    bp = lib.micloc_stream_complex_bandpass_tile_f64
    assert bp(plan.handle, p, 2, 0, 128, 0, 100, p, nstate, p, nws, st) == _lib.MICLOC_ERR_INVALID
    assert bp(plan.handle, p, 2, 101, 128, 0, 100, p, nstate, p, nws, st) == _lib.MICLOC_ERR_SHAPE  # a tile longer than max_tile
    assert bp(plan.handle, p, 2, 100, 128, 40, 100, p, nstate, p, nws, st) == _lib.MICLOC_ERR_SHAPE  # the tile leaves its rows
    assert bp(plan.handle, p, 2, 100, 128, 0, 100, p, nstate - 256, p, nws, st) == _lib.MICLOC_ERR_WORKSPACE
    assert bp(plan.handle, p, 2, 100, 128, 0, 100, p, nstate, p, nws - 256, st) == _lib.MICLOC_ERR_WORKSPACE
    loc_w = lib.micloc_stream_complex_localize_tile_f64
    assert loc_w(plan.handle, p, nstate, 2, 100, 0, None, None, p, nws - 256, st) == _lib.MICLOC_ERR_WORKSPACE
    # windows
    wsz = lib.micloc_stream_complex_window_state_bytes
    wrs = lib.micloc_stream_complex_window_reset
    assert wsz(plan.handle, 2, CH + 1, CH, 4) == 0 and wsz(plan.handle, 2, CH, 2 * CH, 4) == 0 and wsz(plan.handle, 2, CH, CH, 0) == 0
    nwst = wsz(plan.handle, 2, 2 * CH, CH, 4)
    assert nwst == 256 + 2 * 2 * 2 * 57 * 8 + (-(2 * 2 * 2 * 57 * 8) % 256)
    assert wrs(plan.handle, 2, p, nwst, CH + 1, CH, 4, st) == _lib.MICLOC_ERR_SHAPE
    assert wrs(plan.handle, 2, p, nwst, CH, 2 * CH, 4, st) == _lib.MICLOC_ERR_SHAPE  # hop > window
    assert wrs(plan.handle, 2, p, nwst, 0, CH, 4, st) == _lib.MICLOC_ERR_INVALID
    assert wrs(plan.handle, 2, p, nwst - 1, 2 * CH, CH, 4, st) == _lib.MICLOC_ERR_WORKSPACE
    torch.cuda.synchronize()
    # the Python surface
    with pytest.raises(ValueError, match="window quantum"):
        bf.streaming_localizer(W, batch=1, window=CH + 1)
    with pytest.raises(ValueError, match="hop <= window"):
        bf.streaming_localizer(W, batch=1, window=CH, hop=2 * CH)
    with pytest.raises(ValueError, match="give window as well"):
        bf.streaming_localizer(W, batch=1, hop=CH)
    loc = bf.streaming_localizer(W, batch=1, total_frames=300, max_tile=100)
    with pytest.raises(ValueError, match="max_tile"):
        loc.push(np.zeros((1, 101, 7)))
    with pytest.raises(ValueError):
        loc.push(np.zeros((1, 50, 6)))
    with pytest.raises(ValueError):
        loc.latest_window()
    with pytest.raises(_lib.MiclocError, match="incomplete"):
        loc.finish()
    # StreamingLocalizer keeps refusing a Beamformer
    from haghighatshoarmuir2024_amd.streaming import StreamingLocalizer

    with pytest.raises(Exception):
        StreamingLocalizer(bf, W, 1)


def test_two_host_threads_on_two_streams(torch):
    bf = beamformer(7)
    rng = np.random.default_rng(31)
    W = random_bf_mat(rng, 7, 57)
    xs = [rng.standard_normal((2, 2000, 7)) for _ in range(2)]
    tilings = [[700, 700, 600], [333] * 6 + [2]]
    serial = [stream(bf, W, x, t)[1] for x, t in zip(xs, tilings)]
    torch.cuda.synchronize()
    got, errors = [None, None], []

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                out = stream(bf, W, xs[i], tilings[i])[1]
                got[i] = (out["power"].clone(), out["argmax"].clone())
            s.synchronize()
        except Exception as e:  # surfaces in the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i in range(2):
        assert torch.equal(got[i][0], serial[i]["power"]) and torch.equal(got[i][1], serial[i]["argmax"])
