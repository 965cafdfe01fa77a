"""Time-resolved Xylo DoA for batches (XyloNetwork.run_windows, Demo.windows_batch, xylo_windowed_target_sweep; include/micloc_hip.h
"time-resolved DoA, Xylo").  The reference is the oracle's raster O.xylo_lif(...), window-summed in NumPy
(tests/test_xylo_windows_cpu.py checks its premise); every comparison is exact.  PARITY UNPINNED for the integer LIF like every Xylo
test: the oracle restates the published update rule, it is not checked against XyloSim."""
import ctypes
import functools

import numpy as np
import pytest

import xylo_track_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

WINDOWS = ((256, 256), (512, 256), (768, 256), (1024, 256), (1024, 1024), (8192, 256))
B_ALL = 3


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _window_sums(out, T, window, hop):
    """out [B, T, N] (the oracle's raster) -> int32 [B, nW, N] by utils.window_bounds"""
    from haghighatshoarmuir2024_amd.utils import window_bounds

    start, stop = window_bounds(T, window, hop)
    return np.stack([out[:, a:b].astype(np.int64).sum(axis=1) for a, b in zip(start, stop)], axis=1).astype(np.int32), start, stop


@functools.lru_cache(maxsize=None)
def _case(N, Cin, T, w_rec=0):
    """(spec, raster int8 [3, T, Cin / 2], events uint8 [3, T, Cin] with one row of event counts above 1, the oracle's raster of the
    ternary input, the oracle's raster of the events): computed once, shared, never changed.  Thresholds from 50 to 4000 against input
    currents of up to Cin x 127: some steps emit two spikes and more (the re-walk and the cap), trial 1 fires every channel."""
    rng = np.random.RandomState(1000 * N + 10 * Cin + T + (7 if w_rec else 0))
    spec = R.random_spec(rng, Cin, N, 50, 4000, 6, w_rec=w_rec)
    raster = R.all_fire(rng, R.blocked_raster(rng, B_ALL, T, Cin // 2))
    events = R.events_of(raster)
    events[:, min(100, T - 1)] *= 3  # event counts > 1 (the ternary raster cannot say this)
    out_t, _ = R.lif_reference(spec, R.events_of(raster))
    out_e, _ = R.lif_reference(spec, events)
    for a in (raster, events, out_t, out_e):
        a.setflags(write=False)
    return spec, raster, events, out_t, out_e


def _net(spec):
    from haghighatshoarmuir2024_amd.xylo_snn_localization import XyloNetwork

    return XyloNetwork(spec)


def _check_windows(net, spikes, ternary, ref_out, T, what):
    """run_windows on every (window, hop) for B = 1 and 3 against the window sums of ref_out; counts against run() and the raster"""
    for B in (1, B_ALL):
        sp = spikes[:B].contiguous()
        counts_run = net.run(sp, ternary=ternary, queued=False)[1].cpu().numpy()
        np.testing.assert_array_equal(counts_run, ref_out[:B].astype(np.int64).sum(axis=1), err_msg=what)
        for window, hop in WINDOWS:
            ref, start, _ = _window_sums(ref_out[:B], T, window, hop)
            got = net.run_windows(sp, window, hop, ternary=ternary)
            wc, counts = got["window_counts"].cpu().numpy(), got["counts"].cpu().numpy()
            assert wc.dtype == np.int32 and wc.shape == ref.shape, (what, B, window, hop)
            np.testing.assert_array_equal(got["window_start"], start)
            np.testing.assert_array_equal(wc, ref, err_msg=f"{what} B={B} {window}/{hop}")
            np.testing.assert_array_equal(counts, counts_run, err_msg=f"{what} B={B} {window}/{hop} counts")
            if hop == window:
                np.testing.assert_array_equal(wc.astype(np.int64).sum(axis=1), counts)
            if window >= T:
                assert wc.shape[1] == 1 and np.array_equal(wc[:, 0], counts)  # one window: the counts, bit for bit


# ---- 1. the chunk-count kernels against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 255, 256, 257, 1100, 4799])
@pytest.mark.parametrize("Cin", [28, 36])
@pytest.mark.parametrize("N", [33, 130, 513])
def test_window_counts_equal_the_window_sums_of_the_oracle_raster(N, Cin, T):
    """N: a partial wave; a second wave with two live neurons; a second neuron block.  Cin: KQ 1 and 2.  T: one frame, one short of a
    chunk, a chunk, one more, a cut window (1100 with 1024 / 256: the second one holds 844 frames), many chunks with a ragged end.
    The packed kernel (the ternary raster) and the general one (the same network on uint8 event counts)."""
    import torch

    spec, raster, events, out_t, out_e = _case(N, Cin, T)
    if T >= 255:
        assert int(out_t.max()) >= 2 and int(out_e.max()) >= 2  # the re-walk and the division run
    net = _net(spec)
    rd, ed = torch.from_numpy(np.array(raster)).cuda(), torch.from_numpy(np.array(events)).cuda()
    assert rd.data_ptr() % 16 == 0
    _check_windows(net, rd, True, out_t, T, "packed")
    _check_windows(net, ed, False, out_e, T, "general")


def test_cut_windows_of_the_issue():
    from haghighatshoarmuir2024_amd.utils import window_bounds

    s, e = window_bounds(1100, 1024, 256)
    assert list(s) == [0, 256] and list(e - s) == [1024, 844]
    assert len(window_bounds(1100, 768, 256)[0]) == 3


def test_unaligned_raster_takes_the_general_kernel():
    import torch

    spec, raster, _, out_t, _ = _case(130, 28, 1100)
    net = _net(spec)
    flat = torch.zeros(raster.size + 16, dtype=torch.int8, device="cuda")
    view = flat[1 : 1 + raster.size].view(raster.shape)
    view.copy_(torch.from_numpy(np.array(raster)))
    assert view.is_contiguous() and view.data_ptr() % 16 == 1
    _check_windows(net, view, True, out_t, 1100, "unaligned")


@pytest.mark.parametrize("Cin", [8, 32])
def test_general_kernel_with_two_and_eight_input_dwords(Cin):
    """The general kernel unrolls its contraction over NQ packed dwords; Cin = 14, 28 and 36 elsewhere in this file reach NQ = 4, 7 and 16,
    these reach 2 and 8.  uint8 event counts, a chunk and one frame, three trials: counts and window counts against the oracle's raster."""
    import torch

    spec, _, events, _, out_e = _case(33, Cin, 257)
    _check_windows(_net(spec), torch.from_numpy(np.array(events)).cuda(), False, out_e, 257, f"general Cin={Cin}")


def test_recurrent_network():
    import torch

    spec, _, events, _, out_e = _case(33, 28, 1100, w_rec=-1)
    assert spec["w_rec"] == -1
    free, _ = R.lif_reference(dict(spec, w_rec=0), events)
    assert not np.array_equal(free, out_e)  # the recurrent weight matters on this input
    net = _net(spec)
    _check_windows(net, torch.from_numpy(np.array(events)).cuda(), False, out_e, 1100, "recurrent")
    with pytest.raises(ValueError):
        net.new_state(1)  # the stream still refuses it


def test_value_errors_before_any_device_work():
    import torch

    spec, raster, events, _, _ = _case(33, 28, 257)
    net = _net(spec)
    rd = torch.from_numpy(np.array(raster)).cuda()
    for window, hop in ((1000, 256), (1024, 100), (0, 256), (256, 0), (256, 512), (-256, 256)):
        with pytest.raises(ValueError):
            net.run_windows(rd, window, hop, ternary=True)
    with pytest.raises(ValueError):
        net.run_windows(rd, 256, ternary=False)          # int8 given as events
    with pytest.raises(ValueError):
        net.run_windows(rd[:, :, :13], 256, ternary=True)  # not contiguous, wrong channel count
    with pytest.raises(ValueError):
        net.run_windows(rd, 256, ternary=True, max_spikes=0)


# ---- 2. rate and peak of the window rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win_size", [1, 5])
@pytest.mark.parametrize("N,bands", [(33, 1), (130, 2)])
def test_window_rate_and_peak_are_the_one_shot_expressions(N, bands, win_size):
    """window_rate == micloc_rate_from_counts_f64 row by row with the window's own frame count (bits); window_peak ==
    micloc_peak_location_i32 on the rows, and utils.find_peak_location on the host -- there on the rows' band sums themselves, integers in
    float64, whose box-car sums are exact (the reference's normalisation by the maximum and by T / fs are positive factors)."""
    import torch

    from haghighatshoarmuir2024_amd import _lib, runtime
    from haghighatshoarmuir2024_amd.utils import find_peak_location

    T, fs, G = 1100, 48_000.0, N // bands
    spec, raster, _, out_t, _ = _case(N, 28, T)
    net, lib = _net(spec), _lib.load()
    rd = torch.from_numpy(np.array(raster)).cuda()
    for window, hop in ((256, 256), (1024, 256), (768, 256), (8192, 256)):
        got = net.run_windows(rd, window, hop, ternary=True)
        wc = got["window_counts"]
        ref, start, stop = _window_sums(out_t, T, window, hop)
        nW = len(start)
        rate = torch.empty((B_ALL, nW, G), dtype=torch.float64, device="cuda")
        peak = torch.empty((B_ALL, nW), dtype=torch.int32, device="cuda")
        _lib.check(lib.micloc_xylo_window_readout(runtime._ptr(wc), B_ALL, T, window, hop, G, bands, fs, win_size, runtime._ptr(rate),
                                                  runtime._ptr(peak), runtime._stream(wc.device)), "readout")
        only_rate = torch.empty_like(rate)
        only_peak = torch.empty_like(peak)
        _lib.check(lib.micloc_xylo_window_readout(runtime._ptr(wc), B_ALL, T, window, hop, G, bands, fs, 0, runtime._ptr(only_rate), None,
                                                  runtime._stream(wc.device)), "readout, rate only")  # (win_size is the peak's)
        _lib.check(lib.micloc_xylo_window_readout(runtime._ptr(wc), B_ALL, T, window, hop, G, bands, fs, win_size, None, runtime._ptr(only_peak),
                                                  runtime._stream(wc.device)), "readout, peak only")
        assert torch.equal(only_rate, rate) and torch.equal(only_peak, peak)
        for n in range(nW):
            rows = torch.from_numpy(np.ascontiguousarray(ref[:, n])).cuda()
            want = torch.empty((B_ALL, G), dtype=torch.float64, device="cuda")
            _lib.check(lib.micloc_rate_from_counts_f64(runtime._ptr(rows), B_ALL, G, bands, int(stop[n] - start[n]), fs, runtime._ptr(want),
                                                       runtime._stream(rows.device)), "rate_from_counts")
            assert np.array_equal(_bits(rate[:, n]), _bits(want)), (window, hop, n)
            np.testing.assert_array_equal(peak[:, n].cpu().numpy(), runtime.peak_location(rows, G, win_size).cpu().numpy())
            pw = ref[:, n].reshape(B_ALL, bands, G).astype(np.float64).sum(axis=1)
            host = [int(find_peak_location(sig_in=p, win_size=win_size)) for p in pw]
            np.testing.assert_array_equal(peak[:, n].cpu().numpy(), host)
        if (window, hop) == (1024, 256):
            assert nW == 2 and int(stop[1] - start[1]) == 844  # the cut window's own frame count went into its rate


# ---- 3. the demo: unipolar, and stream == batch ----------------------------------------------------------------------------------------
BANDS = {"one": [[1000, 2000]], "two": [[1000, 1600], [1600, 2400]]}
G_DEMO = 57


@functools.lru_cache(maxsize=None)
def _demo(bands, bipolar=True):
    """A 57-DoA demo.  Bipolar: without the recurrent weight (the stream refuses w_rec != 0; at this small grid -0.1 / N quantises to
    -1, at the paper's 449 to 0), W_in, decays and thresholds the demo's own -- as tests/test_hip_stream_xylo.py."""
    from micloc.array_geometry import CenterCircularArray

    from haghighatshoarmuir2024_amd.xylo_snn_localization import Demo, xylo_specification

    demo = Demo(CenterCircularArray(0.045, 7), BANDS[bands], doa_list=np.linspace(-np.pi, np.pi, G_DEMO), recording_duration=0.05,
                bipolar_spikes=bipolar)
    if bipolar:
        spec0 = xylo_specification(demo.bf_mats, demo.tau_vecs, demo.fs, 1e-3, True, w_rec_coef=0.0)
        assert spec0["w_rec"] == 0 and all(np.array_equal(spec0[k], demo.spec[k]) for k in ("W_in", "dash_syn", "dash_mem", "threshold"))
        demo.spec = spec0
    return demo


@functools.lru_cache(maxsize=None)
def _input(T):
    """B = 2 trials: a 1.5 kHz sine from two DoAs through the array, plus seeded noise at about 10 dB"""
    from micloc.array_geometry import CenterCircularArray

    from haghighatshoarmuir2024_amd.xylo_snn_localization import signal_from_template

    geom = CenterCircularArray(0.045, 7)
    time = np.arange(T) / 48_000
    sig = np.sin(2 * np.pi * 1500 * time)
    rng = np.random.RandomState(T)
    x = np.stack([signal_from_template(geom, (time, sig, doa)) for doa in (-1.0, 2.0)])
    return x + rng.randn(*x.shape) * np.sqrt(0.5 / 10.0)  # (shared: the tests only read it)


def test_unipolar_demo_through_windows_batch():
    """A unipolar demo (14 uint8 event channels; w_rec = -1 at this grid: the recurrent general kernel) against the oracle's LIF on the
    demo's own event raster; rate, peak, counts and their whole-recording twins against the one-shot calls."""
    import torch

    demo = _demo("one", bipolar=False)
    T, window, hop, win = 1100, 512, 256, 5
    x = _input(T)
    events = demo.raster_device(x).view(dtype=torch.uint8).cpu().numpy()
    assert events.shape == (2, T, 14) and events.max() == 1
    out, _ = R.lif_reference(demo.spec, events)
    ref, start, stop = _window_sums(out, T, window, hop)
    assert int(ref.sum()) > 0
    got = demo.windows_batch(x, window, hop, win_size=win)
    np.testing.assert_array_equal(got["window_counts"].cpu().numpy(), ref)
    np.testing.assert_array_equal(got["window_start"], start)
    np.testing.assert_array_equal(got["counts"].cpu().numpy(), demo.counts_batch(x).cpu().numpy())
    assert np.array_equal(_bits(got["rate"]), _bits(demo.rate_batch(x)))
    np.testing.assert_array_equal(got["peak"].cpu().numpy(), demo.peak_batch(x, win).cpu().numpy())
    frames = (stop - start).astype(np.float64)
    rate = ref.astype(np.float64) / frames[None, :, None] * 48000.0 / 1.0
    assert np.array_equal(_bits(got["window_rate"]), _bits(rate))
    no_peak = demo.windows_batch(x, window, hop)
    assert "window_peak" not in no_peak and "peak" not in no_peak and torch.equal(no_peak["window_rate"], got["window_rate"])
    with pytest.raises(ValueError):
        demo.windows_batch(x, window, hop, win_size=4)
    with pytest.raises(ValueError):
        demo.windows_batch(x, 500)


@pytest.mark.parametrize("window,hop", [(1024, 512), (1024, 1024), (8192, 256)])
@pytest.mark.parametrize("T", [4799, 6000])
@pytest.mark.parametrize("bands", ["one", "two"])
def test_stream_equals_batch(bands, T, window, hop):
    """1200-frame tiles through XyloStreamingLocalizer(window=, hop=, max_windows=nW) with the wrap rows given: after finish() the
    stream's window counts, rates and peaks are windows_batch's, bit for bit."""
    import torch

    demo, x = _demo(bands), _input(T)
    win = 5
    batch = demo.windows_batch(x, window, hop, win_size=win)
    nW = len(batch["window_start"])
    assert int(batch["window_counts"].sum()) > 0
    L2 = len(demo.beamfs[0].kernel) // 2
    s = demo.streaming_localizer(2, total_frames=T, wrap_tail=x[:, T - L2 :, :], max_tile=1200, lag_frames=2048, win_size=win, window=window, hop=hop,
                                 max_windows=nW)
    for t in range(0, T, 1200):
        s.push(x[:, t : t + 1200, :])
    out = s.finish()
    assert out["window_count"] == nW
    assert torch.equal(out["window_counts"].reshape(batch["window_counts"].shape), batch["window_counts"])
    assert np.array_equal(_bits(out["window_rate"]), _bits(batch["window_rate"]))
    assert torch.equal(out["window_peak"], batch["window_peak"])
    assert torch.equal(out["counts"], batch["counts"]) and np.array_equal(_bits(out["rate"]), _bits(batch["rate"]))
    assert torch.equal(out["peak"], batch["peak"])


# ---- 4. footprint, re-entrancy, graphs --------------------------------------------------------------------------------------------------
def test_footprint_stays_far_below_the_raster():
    """One trial of T = 240 000 (the script's 5 s), N = 449, window = 12 288: the rise of the peak allocation across run_windows stays
    below T N bytes, the raster the alternative stores (108 MB); by the layout it is 938 x 449 x 4 B = 1.7 MB of chunk rows plus the
    outputs (20 windows and the counts: 38 KB)."""
    import torch

    T, N, window = 240_000, 449, 12_288
    rng = np.random.RandomState(3)
    net = _net(R.random_spec(rng, 28, N, 50, 4000, 6))
    raster = torch.from_numpy(rng.choice([-1, 0, 1], size=(1, T, 14), p=[0.035, 0.93, 0.035]).astype(np.int8)).cuda()
    net.run_windows(raster[:, :512].contiguous(), 256, ternary=True)  # (code objects loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = net.run_windows(raster, window, ternary=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"run_windows T={T} N={N} window={window}: peak allocation rises by {rise} bytes (chunk rows {938 * N * 4}, a raster {T * N})")
    assert rise < T * N
    assert got["window_counts"].shape == (1, 20, N)
    assert torch.equal(got["window_counts"].sum(dim=1), got["counts"]) and int(got["counts"].sum()) > 0
    assert torch.equal(got["counts"], net.run(raster, ternary=True, queued=False)[1])


def test_two_streams_with_workspaces_of_their_own():
    import torch

    spec, raster, events, _, _ = _case(513, 36, 4799)
    net = _net(spec)
    rd, ed = torch.from_numpy(np.array(raster)).cuda(), torch.from_numpy(np.array(events)).cuda()
    one = net.run_windows(rd, 1024, 256, ternary=True)
    two = net.run_windows(ed, 512, 256, ternary=False)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(s1):
            a = net.run_windows(rd, 1024, 256, ternary=True)
        with torch.cuda.stream(s2):
            b = net.run_windows(ed, 512, 256, ternary=False)
    torch.cuda.synchronize()
    for k in ("window_counts", "counts"):
        assert torch.equal(a[k], one[k]) and torch.equal(b[k], two[k]), k


def test_graph_capture_replays_to_the_same_bits():
    import torch

    from haghighatshoarmuir2024_amd import _lib, runtime

    spec, raster, _, _, _ = _case(130, 28, 1100)
    net, lib = _net(spec), _lib.load()
    rd = torch.from_numpy(np.array(raster)).cuda()
    other = torch.from_numpy(np.ascontiguousarray(np.array(raster)[::-1])).cuda()
    window, hop, G, bands = 768, 256, 65, 2
    eager, eager_other = net.run_windows(rd, window, hop, ternary=True), net.run_windows(other, window, hop, ternary=True)
    assert not torch.equal(eager["window_counts"], eager_other["window_counts"])
    nW = len(eager["window_start"])

    def readout(wc, rate, peak):
        _lib.check(lib.micloc_xylo_window_readout(runtime._ptr(wc), B_ALL, 1100, window, hop, G, bands, 48_000.0, 5, runtime._ptr(rate),
                                                  runtime._ptr(peak), runtime._stream(wc.device)), "readout")

    rate_e = torch.empty((B_ALL, nW, G), dtype=torch.float64, device="cuda")
    peak_e = torch.empty((B_ALL, nW), dtype=torch.int32, device="cuda")
    readout(eager_other["window_counts"], rate_e, peak_e)
    static_in = rd.clone()
    rate_g, peak_g = torch.empty_like(rate_e), torch.empty_like(peak_e)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.run_windows(static_in, window, hop, ternary=True)  # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = net.run_windows(static_in, window, hop, ternary=True)
        readout(cap["window_counts"], rate_g, peak_g)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap["window_counts"], eager["window_counts"]) and torch.equal(cap["counts"], eager["counts"])
    static_in.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap["window_counts"], eager_other["window_counts"]) and torch.equal(cap["counts"], eager_other["counts"])
    assert torch.equal(rate_g, rate_e) and torch.equal(peak_g, peak_e)


# ---- 5. the sweep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parity", "throughput"])
def test_xylo_windowed_sweep(mode, tmp_path):
    """num_sim = 2, two SNRs, a 57-DoA demo, a 0.1 s test signal (4800 frames): with window >= T the argmax is xylo_target_sweep's index
    on the same draws (peak="device"); with 1024 / 512 the record has nW columns; a finished out_dir recomputes nothing."""
    from haghighatshoarmuir2024_amd.sweep import xylo_target_sweep, xylo_window_localizer, xylo_windowed_target_sweep
    from haghighatshoarmuir2024_amd.utils import window_bounds

    demo = _demo("one")
    kw = dict(snr_db_vec=[10.0, 20.0], num_sim=2, seed=5, mode=mode, test_duration=0.1, batch_trials=3)
    ref = xylo_target_sweep(demo, peak="device", **kw)
    one = xylo_windowed_target_sweep(demo, 8192, **kw)
    assert one["window_argmax"].shape == (2, 2, 1) and one["parity"] == "unpinned (integer LIF)" and one["win_size"] == ref["win_size"]
    np.testing.assert_array_equal(one["argmax"], ref["index"])
    np.testing.assert_array_equal(one["window_argmax"][..., 0], ref["index"])
    np.testing.assert_array_equal(one["doa"], ref["doa"])
    np.testing.assert_array_equal(one["err"], ref["err"])
    nW = len(window_bounds(4800, 1024, 512)[0])
    got = xylo_windowed_target_sweep(demo, 1024, 512, **kw)
    assert nW == 9 and got["window_argmax"].shape == (2, 2, nW) and got["window_pmax"].shape == (2, 2, nW)
    assert list(got["window_start"]) == list(range(0, 512 * nW, 512))
    assert (got["window_pmax"] >= 0).all() and got["window_pmax"].max() > 0  # the value of a window: its rate at the peak index
    print(f"xylo windowed-noisy [{mode}] 1024/512 window_mae_deg {got['window_mae_deg']} mae_deg {got['mae_deg']}")
    first = xylo_windowed_target_sweep(demo, 1024, 512, out_dir=tmp_path, **kw)

    def never(sig_batch, time_vec):
        raise AssertionError("the resumed sweep recomputed a batch")

    res = xylo_windowed_target_sweep(demo, 1024, 512, localizer=never, out_dir=tmp_path, **kw)
    assert res["persistence"]["trials_loaded"] == 4
    for k in ("window_argmax", "window_pmax", "argmax", "err", "doa"):
        np.testing.assert_array_equal(first[k], got[k], err_msg=f"stored {k}")
        np.testing.assert_array_equal(res[k], got[k], err_msg=f"resumed {k}")
    # another window is another record: nothing is loaded across
    other = xylo_windowed_target_sweep(demo, 2048, 512, out_dir=tmp_path, localizer=xylo_window_localizer(demo, 2048, 512, ref["win_size"]), **kw)
    assert other["persistence"]["trials_loaded"] == 0
