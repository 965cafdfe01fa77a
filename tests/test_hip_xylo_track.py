"""Fused Xylo moving-target tracking (XyloNetwork.track, Demo.track_batch, xylo_moving_target_sweep): index, peak_env,
env_last and rate of every case equal, bit for bit, the host reference of tests/xylo_track_ref.py (the oracle's integer LIF, then
Envelope.evolve and np.argmax) AND the device two-step route (run(want_spikes=True) followed by Envelope.track).  PARITY UNPINNED for
the integer LIF like every Xylo test: the oracle is the published rule, not XyloSim."""
import functools
import subprocess
import sys
import threading

import numpy as np
import pytest

import xylo_track_ref as R
from conftest import ROOT, campaign_seeds, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


def _net(spec):
    from haghighatshoarmuir2024_amd.xylo_snn_localization import XyloNetwork

    return XyloNetwork(spec)


def _two_step(net, spikes, env, ternary, cap=31):
    """The device two-step route: the stored raster, then Envelope.track on it."""
    out, rate = net.run(spikes, ternary=ternary, want_spikes=True, max_spikes=cap)
    index, e = env.track(out, want_envelope=True)
    peak = e.gather(2, index.long().unsqueeze(2)).squeeze(2)
    return dict(index=index, peak_env=peak, env_last=e[:, -1, :].contiguous(), rate=rate)


def _check(torch, spec, raster, windows, cap=31, what=""):
    """Fused call on the ternary raster against the host reference and the device two-step route, for every window pair."""
    net = _net(spec)
    dev = torch.from_numpy(np.array(raster)).cuda()
    assert net.track_is_fused(True, cap)
    out, rate = R.lif_reference(spec, R.events_of(raster), cap)
    for w_rise, w_fall in windows:
        env = R.envelope(w_rise, w_fall)
        got = net.track(dev, env, ternary=True, max_spikes=cap, want_rate=True)
        tag = f"{what} windows ({w_rise}, {w_fall})"
        R.assert_equal_bits(got, R.track_reference(out, rate, w_rise, w_fall), tag + " vs host")
        R.assert_equal_bits(got, _two_step(net, dev, env, True, cap), tag + " vs two-step")
    return out


# ---- 1. the recipe's networks: ties and moving winners across lanes, halves, waves and blocks -------------------------------------------
@pytest.mark.parametrize("N,T", [(449, 700), (513, 300), (1100, 200), (130, 129), (17, 257), (33, 127)])
def test_recipe_networks_equal_the_reference_and_the_two_step_route(torch, N, T):
    spec, raster = R.recipe(N, T)
    net = _net(spec)
    dev = torch.from_numpy(np.array(raster)).cuda()
    for w_rise, w_fall in R.WINDOWS:
        env = R.envelope(w_rise, w_fall)
        got = net.track(dev, env, ternary=True, want_rate=True)
        R.assert_equal_bits(got, R.recipe_reference(N, T, w_rise, w_fall), f"({w_rise}, {w_fall}) vs host")
        R.assert_equal_bits(got, _two_step(net, dev, env, True), f"({w_rise}, {w_fall}) vs two-step")


# ---- 2. edge shapes of the packed kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(
    "C,N,T,thr_lo,thr_hi,cap,dash_hi",
    [
        (14, 449, 1037, 5, 60, 31, 3),        # many spikes per step: the exact 32-bit path, groups walked again
        (14, 449, 1037, 5, 60, 1, 3),         # ... with the cap at 1: every positive frame is a tie
        (14, 449, 1037, 5, 60, 3, 3),         # ... and at 3
        (1, 1, 16, 1, 2, 31, 2),              # one channel, one neuron, exactly one 16-step group
        (14, 130, 1, 10, 50, 31, 2),          # a single step
        (32, 1100, 15, 30000, 32767, 31, 4),  # silent trials: index 0 everywhere; shorter than a group; three blocks
        (20, 513, 255, 200, 3000, 31, 15),    # 40 input channels (KQ = 2), a second block
    ],
)
def test_edge_shapes_equal_the_reference_and_the_two_step_route(torch, C, N, T, thr_lo, thr_hi, cap, dash_hi):
    rng = np.random.RandomState(C * 1000 + N + T + cap)
    spec = R.random_spec(rng, 2 * C, N, thr_lo, thr_hi, dash_hi)
    raster = R.all_fire(rng, rng.choice([-1, 0, 1], size=(3, T, C), p=[0.15, 0.7, 0.15]).astype(np.int8))
    out = _check(torch, spec, raster, R.WINDOWS, cap, what=f"C{C} N{N} T{T} cap{cap}")
    if thr_lo >= 30000:  # (trial 1, every channel firing, may reach a threshold; the random trials do not)
        assert int(out[0].sum()) == 0 and int(out[2].sum()) == 0
    elif N == 449 and cap > 1:
        assert int(out.max()) > 1  # second spikes within a step did occur
    if cap == 1 and N == 449:
        pos = out[0].max(axis=1) > 0
        assert pos.any() and ((out[0] == 1).sum(axis=1)[pos] > 1).all()  # windows (1, 1): every positive frame is a tie


# ---- 3. random campaign -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", campaign_seeds("xylo_track", 8))
def test_random_campaign(torch, seed):
    rng = np.random.RandomState(9000 + seed)
    C, N, T = int(rng.randint(1, 33)), int(rng.randint(1, 1101)), int(rng.randint(1, 601))
    w_rise = int(rng.randint(1, 601))
    w_fall = int(rng.randint(w_rise, 601))
    cap = int(rng.choice([1, 3, 31]))
    if seed % 2 == 0:
        spec = R.grouped_spec(rng, 2 * C, N)
        raster = R.blocked_raster(rng, 2, T, C)
    else:
        spec = R.random_spec(rng, 2 * C, N, 5, int(rng.choice([60, 4000])), int(rng.choice([3, 15])))
        raster = rng.choice([-1, 0, 1], size=(2, T, C), p=[0.15, 0.7, 0.15]).astype(np.int8)
    _check(torch, spec, raster, [(w_rise, w_fall)], cap, what=f"seed {seed}: C{C} N{N} T{T} cap{cap}")


# ---- 4. the route: what the fused kernel does not serve runs the two-step route inside the call --------------------------------------------
def test_other_networks_take_the_two_step_route_inside_the_call(torch):
    rng = np.random.RandomState(41)
    env = R.envelope(2, 5)
    # a recurrent weight, uint8 event counts
    spec = R.random_spec(rng, 28, 100, 50, 900, 5, w_rec=-3)
    events = ((rng.rand(5, 300, 28) < 0.15) * rng.randint(1, 4, size=(5, 300, 28))).astype(np.uint8)
    net = _net(spec)
    assert not net.track_is_fused(False)
    dev = torch.from_numpy(events).cuda()
    out, rate = R.lif_reference(spec, events)
    ref = R.track_reference(out, rate, 2, 5)
    small = net.track(dev, env, want_rate=True, budget_bytes=0)  # the minimum workspace: one trial per sub-batch
    big = net.track(dev, env, want_rate=True, budget_bytes=10 * 5 * 9 * 300 * 100)
    two = net.track(dev, env, want_rate=True, budget_bytes=2 * (9 * 300 * 100 + 512))  # two trials out of five: sub-batches of 2, 2 and 1
    R.assert_equal_bits(small, ref, "recurrent, minimum workspace")
    R.assert_equal_bits(two, ref, "recurrent, two trials at a time")
    R.assert_equal_bits(big, ref, "recurrent, ten times the workspace")
    R.assert_equal_bits(small, _two_step(net, dev, env, False), "recurrent vs two-step")
    # the same recurrent network fed the ternary raster: still not fused
    raster = rng.choice([-1, 0, 1], size=(2, 200, 14), p=[0.15, 0.7, 0.15]).astype(np.int8)
    assert not net.track_is_fused(True)
    out, rate = R.lif_reference(spec, R.events_of(raster))
    R.assert_equal_bits(net.track(torch.from_numpy(raster).cuda(), env, ternary=True, want_rate=True), R.track_reference(out, rate, 2, 5), "recurrent, ternary")
    # a fused network with the minimum workspace and ten times as much: the C entry directly
    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.runtime import _ptr, _stream

    spec, raster = R.recipe(1100, 200)
    net = _net(spec)
    dev = torch.from_numpy(np.array(raster)).cuda()
    B, T, C = raster.shape
    need = net.lib.micloc_xylo_track_workspace_bytes(C, 2 * C, 1100, 0, B, T)
    res = []
    for nbytes in (need, 10 * need):
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        idx = torch.empty((B, T), dtype=torch.int32, device="cuda")
        peak = torch.empty((B, T), dtype=torch.float64, device="cuda")
        _lib.check(net.lib.micloc_xylo_lif_track_i16(_ptr(dev), C, B, T, 2 * C, 1100, 0, 31, 0.5, 0.5, 0.8, _ptr(idx), _ptr(peak), None, None, _ptr(net.ws),
                                                     net.nbytes, _ptr(ws), nbytes, _stream(net.device)), "xylo_lif_track")
        res.append(dict(index=idx, peak_env=peak))
    R.assert_equal_bits(res[0], R.recipe_reference(1100, 200, 2, 5), "minimum workspace")
    R.assert_equal_bits(res[1], res[0], "ten times the workspace")


def _moving_signal(geo, fs, duration, snr_db, seed):
    from haghighatshoarmuir2024_amd.sweep import moving_doa_path
    from haghighatshoarmuir2024_amd.xylo_snn_localization import signal_from_template

    t = np.arange(0, duration, 1 / fs)
    s = np.sin(2 * np.pi * np.cumsum(1000 + 1000 * (t % t[-1]) / t[-1]) / fs)
    doa = moving_doa_path(t, duration, np.pi / 3, 0.5, np.asarray(0.3))
    sig = signal_from_template(geo, (t, s, doa))
    rng = np.random.RandomState(seed)
    return sig + np.sqrt(np.mean(sig**2) / 10 ** (snr_db / 10)) * rng.randn(*sig.shape), doa


@functools.lru_cache(maxsize=None)
def _demo(bipolar=True, bands=((1000, 2000),)):
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.xylo_snn_localization import Demo

    geo = CenterCircularArray(4.5e-2, 7)
    doa_list = np.linspace(-np.pi, np.pi, 8 * 7 + 1)  # the geometry of golden/filterbank.npz: 57 DoAs
    return Demo(geometry=geo, freq_bands=[list(b) for b in bands], doa_list=doa_list, recording_duration=0.1, bipolar_spikes=bipolar), geo, doa_list


def test_unipolar_demo_takes_the_two_step_route_and_equals_the_host(torch):
    from haghighatshoarmuir2024_amd.utils import Envelope

    demo, geo, _ = _demo(bipolar=False)
    sig, _ = _moving_signal(geo, 48_000, 0.05, 20.0, 3)
    env = Envelope(rise_time=1e-3, fall_time=10e-3, fs=48_000)
    assert not demo.network().track_is_fused(False)
    got = demo.track_batch(sig[None], env, want_rate=True)
    spikes = demo.xylo_process(demo.spike_encoding(sig))
    np.testing.assert_array_equal(got["index"][0].cpu().numpy(), env.track(spikes))
    np.testing.assert_array_equal(got["rate"][0].cpu().numpy(), spikes.sum(axis=0))
    assert int(spikes.sum()) > 0


# ---- 5. footprint -----------------------------------------------------------------------------------------------------------------------
def test_footprint_at_the_script_recording_length(torch, cfg2):
    """One trial of the script's 5 s: the peak allocation across the call rises by less than the T x N bytes of the raster the two-step
    route would store (and 8 T N more for its envelope)."""
    from haghighatshoarmuir2024_amd.xylo_snn_localization import xylo_specification

    T, N = 240_000, 449
    tau = 1 / (2 * np.pi * 1500)
    spec = xylo_specification([cfg2["bf_mat"]], [[tau, tau]], fs=48_000, target_dt=1e-3, bipolar_spikes=True)
    assert spec["W_in"].shape == (28, N)
    net = _net(spec)
    rng = np.random.RandomState(6)
    raster = torch.from_numpy(R.blocked_raster(rng, 1, T, 14)).cuda()
    env = R.envelope(48, 480)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    got = net.track(raster, env, ternary=True, want_rate=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"footprint: rise {rise / 1e6:.2f} MB, raster of the two-step route {T * N / 1e6:.1f} MB")
    assert rise < T * N
    # prefixes are causal: the first 20 000 frames, tracked again, equal the two-step route on them
    Tp = 20_000
    head = raster[:, :Tp].contiguous()
    again = net.track(head, env, ternary=True, want_rate=True)
    two = _two_step(net, head, env, True)
    R.assert_equal_bits(dict(index=again["index"], peak_env=again["peak_env"], env_last=again["env_last"], rate=again["rate"]), two, "T = 20 000")
    assert torch.equal(got["index"][:, :Tp], again["index"]) and torch.equal(got["peak_env"][:, :Tp], again["peak_env"])
    assert int(got["rate"].sum()) > 0 and int(got["index"].max()) > 0


# ---- 6. Demo.track_batch ------------------------------------------------------------------------------------------------------------------
def test_demo_track_batch_equals_the_host_chain_and_tracks_a_moving_chirp(torch):
    """Bits: the host chain of the script.  Plausibility only for the unpinned stage, as test_demo_spike_encoding_pinned_and_end_to_end
    states it: after the settle time the median tracking error at 20 dB is below the same 15 degrees."""
    from haghighatshoarmuir2024_amd.sweep import track_errors
    from haghighatshoarmuir2024_amd.utils import Envelope

    fs = 48_000
    demo, geo, doa_list = _demo()
    z = golden("filterbank.npz")
    assert z["spikes_in"].shape[1] == 28 and len(doa_list) == 57
    sig, doa = _moving_signal(geo, fs, 0.25, 20.0, 0)
    env = Envelope(rise_time=2e-3, fall_time=20e-3, fs=fs)
    got = demo.track_batch(sig[None], env, want_rate=True)
    spikes = demo.xylo_process(demo.spike_encoding(sig))  # [T, 57] on the host
    idx, e = env.track(spikes, want_envelope=True)
    ref = dict(index=idx[None], peak_env=e[np.arange(len(idx)), idx][None], env_last=e[-1][None], rate=spikes.sum(axis=0)[None])
    R.assert_equal_bits(got, ref, "Demo.track_batch vs host chain")
    lag, settle = int(demo.kernel_duration * fs), int(fs * env.fall_time)
    _, med = track_errors(doa_list, got["index"], doa[None], lag, settle)
    print(f"Demo.track_batch: median tracking error {np.degrees(med[0]):.2f} deg at 20 dB")
    assert np.degrees(med[0]) < 15.0
    two, _, _ = _demo(bands=((1000, 1600), (1600, 2400)))
    with pytest.raises(ValueError):
        two.track_batch(sig[None], env)


# ---- 7. the sweep -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parity", "throughput"])
def test_sweep_with_the_fused_call_equals_the_two_step_localizer(torch, tmp_path, mode):
    from haghighatshoarmuir2024_amd.sweep import xylo_moving_target_sweep
    from haghighatshoarmuir2024_amd.utils import Envelope

    demo, _, _ = _demo()
    env = Envelope(rise_time=1e-3, fall_time=10e-3, fs=48_000)

    def two_step(sig_batch, time_vec):
        raster = demo.raster_device(sig_batch)
        return _two_step(demo.network(), raster, env, True)["index"]

    kw = dict(snr_db_vec=[10.0, 20.0], num_sim=3, seed=5, mode=mode, batch_trials=3)  # T = 4799
    ref = xylo_moving_target_sweep(demo, env, localizer=two_step, **kw)
    got = xylo_moving_target_sweep(demo, env, **kw)
    keys = [k for k, v in ref.items() if isinstance(v, np.ndarray)]
    assert {"phase", "err", "med", "track_mae_deg", "track_median_deg"} <= set(keys) and ref["err"].shape == (2, 3)
    assert got["parity"] == "unpinned (integer LIF)"
    for k in keys:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    print(f"xylo moving-noisy [{mode}] track_mae_deg {got['track_mae_deg']} track_median_deg {got['track_median_deg']}")
    # out_dir: a finished run, run again, recomputes nothing
    first = xylo_moving_target_sweep(demo, env, out_dir=tmp_path, **kw)

    def never(sig_batch, time_vec):
        raise AssertionError("the resumed sweep recomputed a batch")

    res = xylo_moving_target_sweep(demo, env, localizer=never, out_dir=tmp_path, **kw)
    assert res["persistence"]["trials_loaded"] == 6
    for k in keys:
        np.testing.assert_array_equal(first[k], ref[k], err_msg=f"stored {k}")
        np.testing.assert_array_equal(res[k], ref[k], err_msg=f"resumed {k}")


def test_cli_runs_the_xylo_moving_sweep():
    r = subprocess.run([sys.executable, "-m", "haghighatshoarmuir2024_amd.sweep", "--sweep", "moving-noisy", "--method", "xylo", "--num-sim", "1", "--grid", "57",
                        "--mode", "throughput"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Median tracking errors" in r.stdout and "SNR:" in r.stdout


# ---- 8. concurrency and graphs --------------------------------------------------------------------------------------------------------------
def test_two_host_threads_on_two_streams_equal_the_serial_run(torch):
    work = []
    for i, (N, T) in enumerate([(449, 700), (1100, 200)]):
        spec, raster = R.recipe(N, T)
        work.append((_net(spec), torch.from_numpy(np.array(raster)).cuda(), R.envelope(*R.WINDOWS[1 + i])))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]

    def run(i, start=None):
        net, dev, env = work[i]
        outs = []
        with torch.cuda.stream(streams[i]):
            if start is not None:
                start.wait()
            for _ in range(8):
                outs.append(net.track(dev, env, ternary=True, want_rate=True))  # (a workspace of its own per call)
        streams[i].synchronize()
        return [{k: v.cpu().numpy() for k, v in o.items()} for o in outs]

    serial = [run(i) for i in range(2)]
    results, errors = [None, None], []
    start = threading.Barrier(2)

    def worker(i):
        try:
            results[i] = run(i, start)
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors
    for i, (N, T) in enumerate([(449, 700), (1100, 200)]):
        R.assert_equal_bits(serial[i][0], R.recipe_reference(N, T, *R.WINDOWS[1 + i]), f"serial {i}")
        for k, got in enumerate(results[i]):
            R.assert_equal_bits(got, serial[i][k], f"thread {i} call {k}")


def test_captured_into_a_graph_and_replayed(torch):
    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.runtime import _ptr

    spec, raster = R.recipe(1100, 200)
    net = _net(spec)
    B, T, C = raster.shape
    dev = torch.from_numpy(np.array(raster)).cuda()
    nbytes = net.lib.micloc_xylo_track_workspace_bytes(C, 2 * C, 1100, 0, B, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = dict(index=torch.zeros((B, T), dtype=torch.int32, device="cuda"), peak_env=torch.zeros((B, T), dtype=torch.float64, device="cuda"),
               env_last=torch.zeros((B, 1100), dtype=torch.float64, device="cuda"), rate=torch.zeros((B, 1100), dtype=torch.int32, device="cuda"))
    ref = R.recipe_reference(1100, 200, 2, 5)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _lib.check(net.lib.micloc_xylo_lif_track_i16(_ptr(dev), C, B, T, 2 * C, 1100, 0, 31, 0.5, 0.5, 0.8, _ptr(out["index"]), _ptr(out["peak_env"]),
                                                         _ptr(out["env_last"]), _ptr(out["rate"]), _ptr(net.ws), net.nbytes, _ptr(ws), nbytes,
                                                         torch.cuda.current_stream().cuda_stream), "xylo_lif_track")
    torch.cuda.current_stream().wait_stream(s)
    for rep in range(2):
        for v in out.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        R.assert_equal_bits(out, ref, f"replay {rep}")
