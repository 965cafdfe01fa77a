"""Fused moving-target tracking (csrc/track.hip; the tracking rule of include/micloc_hip.h): `track_batch` = beamforming + Envelope.evolve
+ the arg-max per time step (ref:paper_plots/target_snn_localization.py:595-622) without the T x G arrays, against
  1. the two-step route `Envelope.track(apply_to_signal(..., to_host=False))` -- bit for bit, every frame;
  2. the reference's own moving-target trial (tests/golden/moving_target.npz);
  3. oracle.envelope + np.argmax on the device's own y over a seeded random campaign -- bit for bit;
  4. the device-memory footprint at the script's recording length;
  5. two host threads on two streams, and the argument errors of the C entries."""
import ctypes
import threading
import warnings

import numpy as np
import pytest

from conftest import campaign_seeds, golden
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FS = 48_000


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _snn(num_mic=7):
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    tau = 1 / (2 * np.pi * 2000)
    return SNNBeamformer(CenterCircularArray(4.5e-2, num_mic), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=FS)


def _env(rise=10e-3, fall=100e-3):
    from micloc.utils import Envelope

    return Envelope(rise_time=rise, fall_time=fall, fs=FS)


def _two_step(bf, W, sig, env):
    """(index [T], peak [T], last [G]) of one trial by the route the library had before: y and its envelope stored."""
    y = bf.apply_to_signal(W, (np.arange(sig.shape[0]) / FS, sig), to_host=False) if hasattr(bf, "tau_vec") else bf.apply_to_signal(W, sig, to_host=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        idx, e = env.track(y, want_envelope=True)
    return idx.cpu().numpy(), e.max(dim=1).values.cpu().numpy(), e[-1].cpu().numpy()


def _check_batch(bf, W, sigs, env, G):
    out = bf.track_batch(W, np.stack(sigs), env, want_envelope_last=True)
    B, T = len(sigs), sigs[0].shape[0]
    assert out["index"].dtype.is_floating_point is False and tuple(out["index"].shape) == (B, T)
    assert tuple(out["peak_envelope"].shape) == (B, T) and tuple(out["envelope_last"].shape) == (B, G)
    idx, peak, last = (out[k].cpu().numpy() for k in ("index", "peak_envelope", "envelope_last"))
    assert idx.dtype == np.int32
    for b, s in enumerate(sigs):
        wi, wp, wl = _two_step(bf, W, s, env)
        np.testing.assert_array_equal(idx[b], wi, err_msg=f"trial {b}")
        np.testing.assert_array_equal(peak[b], wp, err_msg=f"trial {b}")
        np.testing.assert_array_equal(last[b], wl, err_msg=f"trial {b}")


# ---- 1. the same bits as the two-step route --------------------------------------------------------------------------------------
def test_snn_config2_trials_equal_the_two_step_route(cfg2, torch):
    z = golden("trials_cfg2.npz")
    bf = _snn()
    _check_batch(bf, cfg2["bf_mat"], [z["sig_in"][i] for i in range(3)], _env(), 449)
    assert bf.plan().track_is_fused()


def test_snn_moving_recording_equals_the_two_step_route_and_the_reference(cfg2, torch):
    """... and 2.: the reference's DoA index wherever its two best envelopes are not tied to rounding (the rule and the cap of
    test_hip_tracking.py::test_moving_target_trial_against_the_reference)."""
    z = golden("moving_target.npz")
    sig = z["trial_sig_q"].astype(np.float64) / 4096.0
    bf = _snn()
    _check_batch(bf, cfg2["bf_mat"], [sig], _env(), 449)
    idx = bf.track_batch(cfg2["bf_mat"], sig[None], _env())["index"][0].cpu().numpy()
    clear = z["trial_margin"] > 1e-7
    assert clear.mean() > 0.99
    np.testing.assert_array_equal(idx[clear], z["trial_index"][clear])


@pytest.mark.parametrize("G", [1, 63, 64, 65, 449, 1440])
def test_snn_ragged_batches_equal_the_two_step_route(cfg2, torch, G):
    z = golden("trials_cfg2.npz")
    rng = np.random.RandomState(G)
    W = rng.randn(14, G)
    W /= np.linalg.norm(W, axis=0, keepdims=True)
    bf = _snn()
    for T in (2, 15, 209, 1001):  # (not multiples of 16, 32 or 256)
        sigs = [z["sig_in"][i % 3][7 * i : 7 * i + T] * (0.5 + i) for i in range(3)]
        _check_batch(bf, W, sigs, _env(2e-3, 13e-3), G)
    assert bf.plan().track_is_fused() == (G <= 512)


@pytest.mark.parametrize("G", [57, 449])
def test_complex_beamformer_equals_the_two_step_route(torch, G):
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer

    bm = Beamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], fs=FS)
    rng = np.random.RandomState(3 + G)
    W = (rng.randn(7, G) + 1j * rng.randn(7, G)) / np.sqrt(14)
    for T in (2400, 777):
        sigs = [rng.randn(T, 7) for _ in range(2)]
        _check_batch(bm, W, sigs, _env(), G)
    assert bm.plan().track_is_fused()


# every row of the complex channel table of csrc/track_rows.h (C = 2M = 2 .. 16 -> <KM, KV>): G = 65 is two column groups, the second one
# of a single column, so the combine launch runs; 15 frames are less than one 16-frame tile, 130 are two full chunks and a 2-frame ragged one
@pytest.mark.parametrize("M", range(1, 9))
def test_every_row_of_the_complex_channel_table_equals_the_two_step_route(torch, M):
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer

    bm = Beamformer(CenterCircularArray(4.5e-2, M), 10e-3, [1000.0, 2000.0], fs=FS)
    rng = np.random.RandomState(160 + M)
    W = (rng.randn(M, 65) + 1j * rng.randn(M, 65)) / np.sqrt(2 * M)
    for T in (15, 130):
        _check_batch(bm, W, [rng.randn(T, M) for _ in range(2)], _env(2e-3, 13e-3), 65)
    assert bm.plan().track_is_fused()


@pytest.mark.parametrize("M", [1, 5, 8])
def test_snn_channel_counts_equal_the_two_step_route(torch, M):
    """The same shapes on the spike raster: 2, 10 and 16 channels (at 16 the channel padding of the spike tile vanishes)."""
    bf = _snn(num_mic=M)
    rng = np.random.RandomState(170 + M)
    W = rng.randn(2 * M, 65)
    W /= np.linalg.norm(W, axis=0, keepdims=True)
    for T in (15, 130):
        _check_batch(bf, W, [rng.randn(T, M) for _ in range(2)], _env(2e-3, 13e-3), 65)
    assert bf.plan().track_is_fused()


def test_forty_channel_plan_takes_the_two_step_route_inside_the_call(torch):
    bf = _snn(num_mic=20)
    rng = np.random.RandomState(40)
    W = rng.randn(40, 97)
    W /= np.linalg.norm(W, axis=0, keepdims=True)
    sigs = [rng.randn(1500, 20) for _ in range(3)]
    _check_batch(bf, W, sigs, _env(), 97)
    assert not bf.plan().track_is_fused()
    # a budget that holds one trial at a time: the same results
    a = bf.track_batch(W, np.stack(sigs), _env(), want_envelope_last=True, budget_bytes=1)
    b = bf.track_batch(W, np.stack(sigs), _env(), want_envelope_last=True)
    for k in ("index", "peak_envelope", "envelope_last"):
        assert torch.equal(a[k], b[k]), k


def _call_pipeline_track(torch, plan, x, env, nbytes, want_rc=0):
    """The plan's pipeline tracking entry itself with a workspace of exactly nbytes."""
    B, T, _ = x.shape
    inv = 1 / np.asarray([int(env.win_lens[0]), int(env.win_lens[1])])  # (fall, rise)
    a = 1 - inv
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=x.device)
    out = dict(index=torch.empty((B, T), dtype=torch.int32, device=x.device), peak_envelope=torch.empty((B, T), dtype=torch.float64, device=x.device),
               envelope_last=torch.empty((B, plan.G), dtype=torch.float64, device=x.device))
    fn = plan.lib.micloc_beamformer_pipeline_track_f64 if plan.w_complex else plan.lib.micloc_snn_pipeline_track_f64
    rc = fn(plan.handle, x.data_ptr(), B, T, float(a[1]), float(inv[1]), float(a[0]), out["index"].data_ptr(), out["peak_envelope"].data_ptr(),
            out["envelope_last"].data_ptr(), ws.data_ptr(), int(nbytes), torch.cuda.current_stream().cuda_stream)
    assert rc == want_rc, rc
    torch.cuda.synchronize()
    return out


def _sub_batch_cases(torch, bf, plan, W, sigs, env, cells_y, trials):
    """The entry with workspaces that hold exactly `trials` trials of the two-step route at a time, against the Python two-step route.
    One trial's region: y (cells_y cells of T x G doubles, one 256-B aligned block) and its envelope (one cell)."""
    from haghighatshoarmuir2024_amd import _lib

    assert not plan.track_is_fused()
    B, T, G = len(sigs), sigs[0].shape[0], plan.G
    want = [np.stack(v) for v in zip(*(_two_step(bf, W, s, env) for s in sigs))]
    x = plan.to_device(np.stack(sigs))
    al = lambda v: (v + 255) // 256 * 256  # noqa: E731
    per_trial = al(cells_y * 8 * T * G) + al(8 * T * G)
    need = plan.lib.micloc_track_workspace_bytes(plan.handle, B, T)
    assert need > per_trial
    for n in trials:  # n == 2 of B == 3: sub-batches of 2 and 1
        out = _call_pipeline_track(torch, plan, x, env, need + (n - 1) * per_trial)
        for k, w in zip(("index", "peak_envelope", "envelope_last"), want):
            np.testing.assert_array_equal(out[k].cpu().numpy(), w, err_msg=f"{k}, {n} trials at a time")
    _call_pipeline_track(torch, plan, x, env, need - 256, want_rc=_lib.MICLOC_ERR_WORKSPACE)


def test_forty_channel_plan_with_a_ragged_last_sub_batch(torch):
    """The shape above (the encoder needs the frames to spike) with the workspace of two trials out of three."""
    from micloc.snn_beamformer import neuron_impulse_response

    bf = _snn(num_mic=20)
    rng = np.random.RandomState(40)
    W = rng.randn(40, 97)
    W /= np.linalg.norm(W, axis=0, keepdims=True)
    sigs = [rng.randn(1500, 20) for _ in range(3)]
    plan = bf.plan()
    plan.set_neuron_kernel(neuron_impulse_response(np.arange(1500) / FS, bf.tau_vec))
    plan.set_bf_mat(W)
    _sub_batch_cases(torch, bf, plan, W, sigs, _env(), 1, (2,))


def test_forty_channel_complex_plan_takes_the_two_step_route_inside_the_call(torch):
    """20 microphones are 40 channels, off the fused route: the complex two-step route inside the call, one, two (then one) and three
    trials at a time."""
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer

    bm = Beamformer(CenterCircularArray(4.5e-2, 20), 10e-3, [1000.0, 2000.0], fs=FS)
    rng = np.random.RandomState(41)
    W = (rng.randn(20, 97) + 1j * rng.randn(20, 97)) / np.sqrt(40)
    sigs = [rng.randn(130, 20) for _ in range(3)]
    plan = bm.plan()
    plan.set_bf_mat(W)
    _sub_batch_cases(torch, bm, plan, W, sigs, _env(2e-3, 13e-3), 2, (1, 2, 3))
    _check_batch(bm, W, sigs, _env(2e-3, 13e-3), 97)  # and through track_batch


# ---- 3. a seeded random campaign against the oracle on the device's own y -------------------------------------------------------------
def _plan(cfg2, bipolar=True):
    from haghighatshoarmuir2024_amd.runtime import Plan

    return Plan(7, cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], bipolar)


@pytest.mark.parametrize("seed", campaign_seeds("track_fused", 8))
def test_random_campaign_against_the_oracle(cfg2, torch, seed):
    from haghighatshoarmuir2024_amd import runtime

    rng = np.random.RandomState(9000 + seed)
    cpx = bool(seed & 1)
    T = int(rng.choice([1, 2, 17, 64, 65, int(rng.randint(1, 3001))]))
    G = int(rng.choice([1, 64, 65, int(rng.randint(1, 513 if not cpx else 1501))]))
    if T * G > 600_000:
        T = max(1, 600_000 // G)
    wf = int(rng.randint(1, 5001))
    wr = int(rng.randint(1, wf + 1))
    B = 2
    p = _plan(cfg2)
    if cpx:
        W = rng.randn(7, G) + 1j * rng.randn(7, G)
        p.set_bf_mat(W)
        Ts = p.padded_T(T)
        pre = torch.from_numpy(rng.randn(B, 14, Ts)).cuda()
        y = p.beamform_c128(pre, T, want_y=True, want_power=False)["y"]
        # |y| by the device library's hypot (what the rule names): the envelope kernel's own magnitude of every value as a one-frame trial
        mag = torch.cat([runtime.envelope_track(y[b].reshape(T, 1, G), 1, 1, want_index=False)[0].reshape(1, T, G) for b in range(B)]).cpu().numpy()
        out = p.track(pre, wf, wr, kind="planar", T=T, want_envelope_last=True)
    else:
        p.set_neuron_kernel(cfg2["nir"][: int(rng.randint(1, len(cfg2["nir"]) + 1))])
        p.set_bf_mat(rng.randn(14, G))
        spk = torch.from_numpy(rng.randint(-1, 2, size=(B, T, 14)).astype(np.int8)).cuda()
        mag = p.lif_beamform(spk, want_y=True, want_power=False)["y"].cpu().numpy()
        out = p.track(spk, wf, wr, kind="spikes", want_envelope_last=True)
    assert p.track_is_fused()
    for b in range(B):
        want = O.envelope(mag[b], wf, wr)
        tag = f"seed {seed} complex={cpx} T={T} G={G} w=({wf},{wr}) trial {b}"
        np.testing.assert_array_equal(out["index"][b].cpu().numpy(), np.argmax(want, axis=1), err_msg=tag)
        np.testing.assert_array_equal(out["peak_envelope"][b].cpu().numpy(), want.max(axis=1), err_msg=tag)
        np.testing.assert_array_equal(out["envelope_last"][b].cpu().numpy(), want[-1], err_msg=tag)


# ---- 4. footprint ---------------------------------------------------------------------------------------------------------------------
def test_footprint_at_the_script_recording_length(cfg2, torch):
    """B = 2 trials of the script's 5 s (239 999 frames) at G = 449: the rise of the peak allocation across the call stays under a
    quarter of ONE T x G float64 array per trial -- the two-step route needs eight times that."""
    B, T, G = 2, 239_999, 449
    bf = _snn()
    rng = np.random.RandomState(5)
    t = np.arange(T) / FS
    x = torch.from_numpy(np.sin(2 * np.pi * 1500 * t)[None, :, None] * np.ones((B, 1, 7)) + 0.1 * rng.randn(B, T, 7)).cuda()
    W = np.asarray(cfg2["bf_mat"], dtype=np.float64)
    env = _env()
    plan = bf.plan()  # tables first: bf_mat and the neuron kernel are resident before the call
    from haghighatshoarmuir2024_amd.snn_beamformer import neuron_impulse_response

    plan.set_neuron_kernel(neuron_impulse_response(t, bf.tau_vec))
    plan.set_bf_mat(W)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = bf.track_batch(W, x, env)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    bound = B * T * G * 8 // 4
    print(f"footprint: rise {rise / 1e6:.1f} MB, bound {bound / 1e6:.1f} MB, workspace {plan.ws.buf.numel() / 1e6:.1f} MB")
    assert rise < bound
    idx = out["index"].cpu().numpy()
    assert idx.shape == (B, T) and idx.min() >= 0 and idx.max() < G


# ---- 5. re-entrancy and argument errors ---------------------------------------------------------------------------------------------
def test_two_host_threads_on_two_streams_equal_the_serial_run(cfg2, torch):
    z = golden("trials_cfg2.npz")
    work = []
    for i in range(2):
        p = _plan(cfg2)
        p.set_neuron_kernel(cfg2["nir"] if i == 0 else cfg2["nir"][:20])
        rng = np.random.RandomState(70 + i)
        p.set_bf_mat(cfg2["bf_mat"] if i == 0 else rng.randn(14, 96))
        T = 4799 if i == 0 else 3100
        xs = [p.to_device(z["sig_in"][[k % 3, (k + 1) % 3], :T] * (0.5 + rng.rand()) + 0.2 * rng.randn(2, T, 7)) for k in range(12)]
        work.append((p, xs))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]

    def run(i, start=None):
        p, xs = work[i]
        outs = []
        with torch.cuda.stream(streams[i]):
            if start is not None:
                start.wait()
            for x in xs:
                outs.append(p.track(x, 4800, 480, want_envelope_last=True))
        streams[i].synchronize()
        return [tuple(o[k].cpu().numpy() for k in ("index", "peak_envelope", "envelope_last")) for o in outs]

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
    for i in range(2):
        for k, (got, want) in enumerate(zip(results[i], serial[i])):
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w, err_msg=f"thread {i} call {k}")


def test_argument_errors_are_status_codes(cfg2, torch):
    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.runtime import _ptr, _stream

    lib = _lib.load()
    p = _plan(cfg2)
    p.set_neuron_kernel(cfg2["nir"])
    p.set_bf_mat(cfg2["bf_mat"])
    B, T = 2, 300
    n = lib.micloc_track_workspace_bytes(p.handle, B, T)
    assert n > 0 and lib.micloc_track_workspace_bytes(p.handle, B, 0) == 0 and lib.micloc_track_workspace_bytes(p.handle, 65535, 65535) == 0
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    spk = torch.zeros((B, T, 14), dtype=torch.int8, device="cuda")
    idx = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    st = _stream(p.device)
    call = lambda b, t, w, nbytes: lib.micloc_lif_beamform_track_f64(p.handle, _ptr(spk), b, t, 0.9, 0.1, 0.99, _ptr(idx), None, None, w, nbytes, st)  # noqa: E731
    assert call(B, 0, _ptr(ws), n) == _lib.MICLOC_ERR_SHAPE
    assert call(65535, 65535, _ptr(ws), n) == _lib.MICLOC_ERR_SHAPE  # B * T > 2^31 - 1
    assert call(B, T, _ptr(ws), n - 1) == _lib.MICLOC_ERR_WORKSPACE
    assert call(B, T, ctypes.c_void_p(0), n) == _lib.MICLOC_ERR_WORKSPACE
    assert call(B, T, ctypes.c_void_p(ws.data_ptr() + 8), n) == _lib.MICLOC_ERR_WORKSPACE
    x = torch.zeros((B, T, 7), dtype=torch.float64, device="cuda")
    assert lib.micloc_beamformer_pipeline_track_f64(p.handle, _ptr(x), B, T, 0.9, 0.1, 0.99, _ptr(idx), None, None, _ptr(ws), n, st) == _lib.MICLOC_ERR_SHAPE
    torch.cuda.synchronize()
    assert int((idx != -7).sum()) == 0  # nothing was launched
    assert call(B, T, _ptr(ws), n) == _lib.MICLOC_OK
    torch.cuda.synchronize()
    assert int((idx < 0).sum()) == 0
    with pytest.raises(ValueError):
        _snn().track_batch(cfg2["bf_mat"], np.zeros((1, 10, 6)), _env())


# ---- 6. the sweep: fused localizer == a localizer built from the two-step route ---------------------------------------------------------
@pytest.mark.parametrize("mode", ["parity", "throughput"])
def test_sweep_with_the_fused_call_equals_the_two_step_localizer(cfg2, torch, tmp_path, mode):
    from haghighatshoarmuir2024_amd.sweep import moving_target_sweep, track_localizer

    bf, env = _snn(), _env()
    W, doa_list = cfg2["bf_mat"], cfg2["doa_list"]

    def two_step(sig_batch, time_vec):
        rows = []
        for sig in sig_batch:
            s = sig.cpu().numpy() if hasattr(sig, "cpu") else np.asarray(sig)
            rows.append(env.track(bf.apply_to_signal(W, (time_vec, s), to_host=False)))
        return torch.stack(rows)

    kw = dict(snr_db_vec=[0.0, 10.0, 20.0], num_sim=8, seed=7, mode=mode, settle_frames=2400, batch_trials=8)  # T = 4799, lag 480
    ref = moving_target_sweep(bf, W, doa_list, env, localizer=two_step, **kw)
    got = moving_target_sweep(bf, W, doa_list, env, **kw)
    keys = [k for k, v in ref.items() if isinstance(v, np.ndarray)]
    assert {"phase", "err", "med", "track_mae_deg", "track_median_deg"} <= set(keys) and ref["err"].shape == (3, 8)
    for k in keys:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    print(f"moving-noisy [{mode}] track_mae_deg {got['track_mae_deg']} track_median_deg {got['track_median_deg']}")
    # a run that stops after its first batch, resumed: the uninterrupted bits
    fused = track_localizer(bf, W, env, max_batch=8)
    calls = []

    def dies(sig_batch, time_vec):
        if calls:
            raise KeyboardInterrupt
        calls.append(len(sig_batch))
        return fused(sig_batch, time_vec)

    with pytest.raises(KeyboardInterrupt):
        moving_target_sweep(bf, W, doa_list, env, localizer=dies, out_dir=tmp_path, **kw)
    res = moving_target_sweep(bf, W, doa_list, env, out_dir=tmp_path, **kw)
    assert res["persistence"]["trials_loaded"] == 8
    for k in keys:
        np.testing.assert_array_equal(res[k], ref[k], err_msg=f"resumed {k}")
