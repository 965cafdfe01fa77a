"""The time-resolved read-out on the MI355X (csrc/windows.hip behind micloc_*_windows_f64, Plan.snn_pipeline / beamformer_pipeline
(window=), localize_batch(window=), windowed_target_sweep): against the reference's windowed power (tests/golden/windows.npz), against a
NumPy restatement of the window rule on the device's own per-chunk partial sums (bit for bit), and against the unwindowed calls."""
import ctypes
import threading

import numpy as np
import pytest

from conftest import campaign_seeds, golden
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BLOCK = 32  # STREAM_BLOCK_CHUNKS


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _snn():
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    tau = 1.0 / (2 * np.pi * 2000)
    return SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=48_000)


def _cbf():
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer

    return Beamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], fs=48_000)


def _np(t):
    return t.cpu().numpy()


# ---- golden parity ------------------------------------------------------------------------------------------------------
def test_golden_a_noisy_trials(cfg2):
    """Three config-2 noisy trials, window 1024 / hop 512 (9 windows, the last 703 frames): the reference's mean(y[s:e]**2) per
    window to 1e-10 relative (the tolerance of the device-vs-golden power tests), its arg-max in EVERY window."""
    from micloc.utils import window_bounds

    g, z = golden("windows.npz"), golden("trials_cfg2.npz")
    out = _snn().localize_batch(cfg2["bf_mat"], z["sig_in"], window=int(g["a_window"]), hop=int(g["a_hop"]))
    assert tuple(out["window_power"].shape) == (3, 9, 449) and tuple(out["window_argmax"].shape) == (3, 9)
    start, stop = window_bounds(4799, 1024, 512)
    np.testing.assert_array_equal(out["window_start"], g["a_start"])
    np.testing.assert_array_equal(start, g["a_start"])
    np.testing.assert_array_equal(stop, g["a_stop"])
    rel = np.abs(_np(out["window_power"]) - g["a_power"]).max() / g["a_power"].max()
    print(f"golden a: max |dp| / max p = {rel:.3g}")
    np.testing.assert_allclose(_np(out["window_power"]), g["a_power"], rtol=1e-10, atol=0)
    np.testing.assert_array_equal(_np(out["window_argmax"]), g["a_argmax"])
    # the whole-recording results of the same call are the unwindowed ones
    np.testing.assert_array_equal(_np(out["argmax"]), z["argmax"])
    np.testing.assert_allclose(_np(out["power"]), z["power"], rtol=1e-10, atol=0)


def test_golden_b_moving_target(cfg2):
    """The reference's moving-DoA trial (0.5 s), windows of 2048 hopping by 1024: the per-window arg-max follows the target."""
    g, m = golden("windows.npz"), golden("moving_target.npz")
    sig = m["trial_sig_q"].astype(np.float64) / 4096.0
    out = _snn().localize_batch(cfg2["bf_mat"], sig[None], time_vec=m["trial_time"], window=int(g["b_window"]), hop=int(g["b_hop"]))
    assert tuple(out["window_power"].shape) == (1, 23, 449)
    np.testing.assert_array_equal(out["window_start"], g["b_start"])
    np.testing.assert_allclose(_np(out["window_power"])[0], g["b_power"], rtol=1e-10, atol=0)
    np.testing.assert_array_equal(_np(out["window_argmax"])[0], g["b_argmax"])
    assert len(np.unique(g["b_argmax"])) > 3


def test_golden_c_complex_beamformer():
    """The complex Beamformer: mean |y|^2 per window from the re / im partial pairs."""
    g, c = golden("windows.npz"), golden("beamformer_c128_g449.npz")
    out = _cbf().localize_batch(c["bf_mat"], c["sig_in"][None], window=int(g["c_window"]), hop=int(g["c_hop"]))
    np.testing.assert_array_equal(out["window_start"], g["c_start"])
    np.testing.assert_allclose(_np(out["window_power"])[0], g["c_power"], rtol=1e-10, atol=0)
    np.testing.assert_array_equal(_np(out["window_argmax"])[0], g["c_argmax"])
    assert int(out["argmax"][0]) == int(c["argmax"])
    np.testing.assert_allclose(_np(out["power"])[0], c["power"], rtol=1e-10, atol=0)


# ---- rule parity: the NumPy restatement on the device's own chunk sums ---------------------------------------------------
def restate(re, im, T, q, window, hop):
    """The window rule on per-chunk partial sums re [nch, G] (and im, complex plans): windows from the rule, the chunks of a window
    added ascending in blocks of 32 counted from its first chunk, the block sums ascending onto the total, divided by the window's
    frame count; first maximum, a NaN never wins."""
    nch, G = re.shape
    nW = 1 if T <= window else 1 + -(-(T - window) // hop)
    power = np.zeros((nW, G))
    for n in range(nW):
        c0 = n * hop // q
        nc = max(0, min(window // q, nch - c0))
        total = np.zeros(G)
        for b0 in range(0, nc, BLOCK):
            s = np.zeros(G)
            for ch in range(b0, min(b0 + BLOCK, nc)):
                s = s + re[c0 + ch]
                if im is not None:
                    s = s + im[c0 + ch]
            total = total + s
        frames = min(T - n * hop, window)
        power[n] = total / float(frames) if frames > 0 else np.nan
    best = np.where(np.isnan(power), -1.0, power)
    return power, np.argmax(best, axis=1).astype(np.int32)


def _random_plan(rng, kind):
    """kind 0: SNN, 7 mics (bf_mat-stationary kernel, 256-frame chunks); 1: SNN, 20 mics (general kernel, 256); 2: SNN, 64 mics -- the
    stress shape, C = 128 (general kernel, 512-frame chunks); 3: complex, 7 mics (bf_mat-stationary complex kernel, 256); 4: complex,
    12 mics (general kernel, 256)."""
    from haghighatshoarmuir2024_amd.runtime import Plan

    fs = 48_000
    M = (7, 20, 64, 7, 12)[kind]
    cplx = kind >= 3
    G = int(rng.choice([1, 16, 57, 130, 449, int(rng.randint(1, 600))]))
    if kind == 2:
        G = int(rng.choice([64, 200, 449]))
    ker = O.stht_kernel(fs, 10e-3)
    b, a = O.bandpass(fs, [1000.0, 2000.0])
    plan = Plan(M, ker, b, a, 1 if cplx else O.robust_width(fs, 2000.0), False if cplx else bool(rng.randint(2)))
    if cplx:
        W = rng.randn(M, G) + 1j * rng.randn(M, G)
        plan.set_bf_mat(W / np.linalg.norm(W, axis=0, keepdims=True))
    else:
        tau = 1 / (2 * np.pi * 2000.0)
        plan.set_neuron_kernel(O.neuron_kernel(np.arange(4800) / fs, [tau, tau]))
        W = rng.randn(2 * M, G)
        plan.set_bf_mat(W / np.linalg.norm(W, axis=0, keepdims=True))
    return plan, M, G, cplx


def _stage_windows(plan, x, T, cplx, torch, **kw):
    """The stage-level windowed entry, and the raw partial sums [B, nch, Gp] it left at the start of the workspace."""
    B = x.shape[0]
    if cplx:
        pre, _ = plan.bandpass_rzcc(plan.stht(x), T, want_pre=True, want_spikes=False)
        out = plan.beamform_c128(pre, T, **kw)
        Gp = 2 * 16 * ((plan.G + 15) // 16)
    else:
        spikes = plan.snn_pipeline(x, want_spikes=True, want_power=False)["spikes"]
        out = plan.lif_beamform(spikes, **kw)
        Gp = 16 * ((plan.G + 15) // 16)
    q = plan.window_quantum()
    nch = (T + q - 1) // q
    raw = plan.ws.buf[: B * nch * Gp * 8].view(torch.float64).reshape(B, nch, Gp).clone()
    return out, _np(raw), Gp


@pytest.mark.parametrize("seed", campaign_seeds("windows", 30))
def test_window_rule_bit_for_bit(seed, torch):
    """Random T, window, hop (multiples of the quantum), G, both power forms and all three chunk lengths' kernels: the device equals
    the restatement on its own per-chunk partial sums BIT FOR BIT.  The rows are the partial sums the stage-level entry leaves in its
    workspace; the window = hop = quantum call must return exactly those rows divided by their frame counts (its definition for
    one-chunk windows: 0 + row), and for full chunks -- a power of two frames, an exact division -- nothing else is possible.  (The
    ragged last chunk's sum cannot be recovered from its mean exactly, hence the rows themselves.)"""
    rng = np.random.RandomState(7000 + seed)
    kind = seed % 5
    plan, M, G, cplx = _random_plan(rng, kind)
    q = plan.window_quantum()
    assert q == (512 if kind == 2 else 256)
    B = int(rng.randint(1, 4))
    style = seed // 5 % 6
    if style == 0:  # nW = 1: window >= T
        T = int(rng.randint(50, 5 * q))
        window, hop = q * ((T + q - 1) // q + int(rng.randint(0, 3))), q * int(rng.randint(1, 4))
    elif style == 1:  # hop > window (the last window may hold no frame)
        T = int(rng.randint(2 * q, 12 * q))
        window = q * int(rng.randint(1, 3))
        hop = window + q * int(rng.randint(1, 4))
    elif style == 2:  # T a multiple of the chunk, exact fit
        window, hop = q * int(rng.randint(1, 4)), q * int(rng.randint(1, 3))
        T = window + hop * int(rng.randint(0, 6))
    elif style == 3 and kind in (0, 3):  # long windows: more than 128 chunks, the four-slice kernel; more than one block of 32
        T = int(rng.randint(140 * q, 150 * q))
        window, hop = q * int(rng.randint(129, 140)), q * int(rng.randint(1, 8))
    else:
        T = int(rng.randint(50, 40 * q)) | 1  # (odd: never a multiple of the chunk)
        window, hop = q * int(rng.randint(1, 36)), q * int(rng.randint(1, 12))
    x = plan.to_device(rng.randn(B, T, M))
    msg = f"kind={kind} style={style} B={B} T={T} G={G} q={q} window={window} hop={hop}"

    out, raw, Gp = _stage_windows(plan, x, T, cplx, torch, window=window, hop=hop)
    re = raw[:, :, :G]
    im = raw[:, :, Gp // 2 : Gp // 2 + G] if cplx else None
    nch = raw.shape[1]
    # the one-chunk windows are the rows
    rows, _, _ = _stage_windows(plan, x, T, cplx, torch, window=q, hop=q)
    frames = np.minimum(T - np.arange(nch) * q, q).astype(np.float64)
    np.testing.assert_array_equal(_np(rows["window_power"]), (re + im if cplx else re) / frames[None, :, None], err_msg=msg)
    full = nch - 1 if T % q else nch
    np.testing.assert_array_equal(_np(rows["window_power"])[:, :full] * float(q), (re + im if cplx else re)[:, :full], err_msg=msg)

    nW = plan.window_count(T, window, hop)[0]
    assert tuple(out["window_power"].shape) == (B, nW, G), msg
    for b in range(B):
        p, a = restate(re[b], None if im is None else im[b], T, q, window, hop)
        np.testing.assert_array_equal(_np(out["window_power"])[b], p, err_msg=msg)
        np.testing.assert_array_equal(_np(out["window_argmax"])[b], a, err_msg=msg)
    # the pipeline-level entry: the same launches, the same bits; and the whole-recording results of the same call
    pipe = plan.beamformer_pipeline(x, window=window, hop=hop) if cplx else plan.snn_pipeline(x, window=window, hop=hop)
    plain = plan.beamformer_pipeline(x) if cplx else plan.snn_pipeline(x)
    for k in ("window_power", "window_argmax", "power", "argmax"):
        np.testing.assert_array_equal(_np(pipe[k]), _np(out[k]), err_msg=f"{k} {msg}")
    np.testing.assert_array_equal(_np(pipe["power"]), _np(plain["power"]), err_msg=msg)
    np.testing.assert_array_equal(_np(pipe["argmax"]), _np(plain["argmax"]), err_msg=msg)
    if nW == 1:  # a single window with window >= T: the bits of the unwindowed call
        np.testing.assert_array_equal(_np(pipe["window_power"])[:, 0], _np(plain["power"]), err_msg=msg)
        np.testing.assert_array_equal(_np(pipe["window_argmax"])[:, 0], _np(plain["argmax"]), err_msg=msg)


# ---- unwindowed equivalence ------------------------------------------------------------------------------------------------
def test_single_window_is_the_unwindowed_call_and_default_is_unchanged(cfg2):
    z = golden("trials_cfg2.npz")
    bf = _snn()
    plain = bf.localize_batch(cfg2["bf_mat"], z["sig_in"])
    assert set(plain) == {"spikes", "y", "power", "argmax"}  # exactly today's keys: no window entries without `window`
    np.testing.assert_array_equal(_np(plain["argmax"]), z["argmax"])
    np.testing.assert_allclose(_np(plain["power"]), z["power"], rtol=1e-10, atol=0)
    for window in (4864, 5120, 1 << 20):
        one = bf.localize_batch(cfg2["bf_mat"], z["sig_in"], window=window)
        assert set(one) == set(plain) | {"window_power", "window_argmax", "window_start"}
        assert tuple(one["window_power"].shape) == (3, 1, 449) and list(one["window_start"]) == [0]
        np.testing.assert_array_equal(_np(one["window_power"])[:, 0], _np(plain["power"]))
        np.testing.assert_array_equal(_np(one["window_argmax"])[:, 0], _np(plain["argmax"]))
        np.testing.assert_array_equal(_np(one["power"]), _np(plain["power"]))
        np.testing.assert_array_equal(_np(one["argmax"]), _np(plain["argmax"]))
    again = bf.localize_batch(cfg2["bf_mat"], z["sig_in"])
    assert set(again) == set(plain)
    np.testing.assert_array_equal(_np(again["power"]), _np(plain["power"]))

    c = golden("beamformer_c128_g449.npz")
    cbf = _cbf()
    plain = cbf.localize_batch(c["bf_mat"], z["sig_in"])
    assert set(plain) == {"y", "power", "argmax"}
    one = cbf.localize_batch(c["bf_mat"], z["sig_in"], window=5120, hop=256)
    np.testing.assert_array_equal(_np(one["window_power"])[:, 0], _np(plain["power"]))
    np.testing.assert_array_equal(_np(one["window_argmax"])[:, 0], _np(plain["argmax"]))


def test_value_errors_name_the_quantum(cfg2):
    from haghighatshoarmuir2024_amd import _lib

    z = golden("trials_cfg2.npz")
    bf = _snn()
    bf.localize_batch(cfg2["bf_mat"], z["sig_in"])
    q = bf.plan().window_quantum()
    assert q == 256
    for kw in (dict(window=1000), dict(window=1024, hop=100), dict(window=0), dict(window=1024, hop=0), dict(window=-256)):
        with pytest.raises(ValueError, match="quantum, 256 frames"):
            bf.localize_batch(cfg2["bf_mat"], z["sig_in"], **kw)
    with pytest.raises(ValueError, match="direct"):
        bf.localize_batch(cfg2["bf_mat"], z["sig_in"], window=1024, power_mode="covariance")
    with pytest.raises(ValueError, match="doa_list"):
        bf.localize_batch(cfg2["bf_mat"], z["sig_in"], window=1024, num_sources=2)
    # the C entry points: the stated status codes, before any launch
    plan, lib = bf.plan(), _lib.load()
    x = plan.to_device(z["sig_in"])
    ws, nbytes = plan.workspace(3, 4799)
    one = ctypes.c_void_p(x.data_ptr())  # (a valid device pointer: the failing calls never write through it)
    st = ctypes.c_void_p(0)
    call = lambda window, hop, wsb: lib.micloc_snn_pipeline_windows_f64(plan.handle, one, 3, 4799, window, hop, None, one, None, None, None,  # noqa: E731
                                                                       ctypes.c_void_p(ws.data_ptr()), wsb, st)
    assert call(1000, 1000, nbytes) == _lib.MICLOC_ERR_SHAPE
    assert call(1024, 0, nbytes) == _lib.MICLOC_ERR_SHAPE
    assert call(1024, 100, nbytes) == _lib.MICLOC_ERR_SHAPE
    assert call(1024, 512, nbytes - 256) == _lib.MICLOC_ERR_WORKSPACE
    assert lib.micloc_snn_pipeline_windows_f64(plan.handle, one, 3, 4799, 1024, 512, None, None, None, one, one, ctypes.c_void_p(ws.data_ptr()), nbytes,
                                               st) == _lib.MICLOC_ERR_INVALID  # neither window output
    assert lib.micloc_beamformer_pipeline_windows_f64(plan.handle, one, 3, 4799, 1024, 512, one, None, None, None, ctypes.c_void_p(ws.data_ptr()), nbytes,
                                                      st) == _lib.MICLOC_ERR_SHAPE  # a real bf_mat on the complex entry
    assert lib.micloc_window_workspace_bytes(plan.handle, 3, 4799, 1000, 1000, 1) == 0
    assert lib.micloc_window_workspace_bytes(plan.handle, 3, 4799, 1024, 512, 1) == lib.micloc_workspace_bytes(plan.handle, 3, 4799)
    assert lib.micloc_window_workspace_bytes(plan.handle, 3, 4799, 1024, 512, 0) == lib.micloc_lif_beamform_workspace_bytes(plan.handle, 3, 4799)


# ---- per-window peaks ---------------------------------------------------------------------------------------------------------
def test_per_window_peaks(cfg2):
    from micloc.utils import find_doa_peaks

    z = golden("trials_cfg2.npz")
    doa = cfg2["doa_list"]
    out = _snn().localize_batch(cfg2["bf_mat"], z["sig_in"], window=1024, hop=512, num_sources=2, doa_list=doa, min_separation=0.4)
    assert tuple(out["window_peaks"].shape) == (3, 9, 2) and tuple(out["window_peak_power"].shape) == (3, 9, 2)
    idx, val = find_doa_peaks(out["window_power"].reshape(27, 449), doa, 2, min_separation=0.4)
    np.testing.assert_array_equal(_np(out["window_peaks"]).reshape(27, 2), _np(idx))
    np.testing.assert_array_equal(_np(out["window_peak_power"]).reshape(27, 2), _np(val))
    np.testing.assert_array_equal(_np(out["window_peaks"])[:, :, 0], _np(out["window_argmax"]))  # the strongest peak is the arg-max
    # the whole-recording peaks of the same call are the unwindowed ones
    plain = _snn().localize_batch(cfg2["bf_mat"], z["sig_in"], num_sources=2, doa_list=doa, min_separation=0.4)
    np.testing.assert_array_equal(_np(out["peaks"]), _np(plain["peaks"]))


# ---- speech shape -----------------------------------------------------------------------------------------------------------
def test_speech_shape(cfg2, torch):
    """T = 332 157 frames (the speech configuration), window 4096: it runs; the window powers weighted by their frame counts sum to
    the whole-recording power within 1e-12 relative; no T x G buffer: the workspace is the unwindowed call's, the partial sums are a
    256th of T x G, and the outputs are B x nW x G."""
    from haghighatshoarmuir2024_amd import _lib
    from micloc.utils import window_bounds

    T, B, G = 332_157, 4, 449
    bf = _snn()
    rng = np.random.RandomState(11)
    t = np.arange(T) / 48_000
    x = np.sin(2 * np.pi * 1500 * t)[None, :, None] * np.ones((B, 1, 7)) + 0.5 * rng.randn(B, T, 7)
    out = bf.localize_batch(cfg2["bf_mat"], x, window=4096)
    plan = bf.plan()
    assert plan.window_quantum() == 256 and 4096 % 256 == 0
    start, stop = window_bounds(T, 4096)
    nW = len(start)
    assert nW == 82 and tuple(out["window_power"].shape) == (B, nW, G)
    w = (stop - start).astype(np.float64)
    tot = (_np(out["window_power"]) * w[None, :, None]).sum(axis=1) / T
    np.testing.assert_allclose(tot, _np(out["power"]), rtol=1e-12, atol=0)
    lib = _lib.load()
    ws_pipe = lib.micloc_window_workspace_bytes(plan.handle, B, T, 4096, 4096, 1)
    assert ws_pipe == lib.micloc_workspace_bytes(plan.handle, B, T) and plan.ws.buf.numel() == ws_pipe
    ws_stage = lib.micloc_window_workspace_bytes(plan.handle, B, T, 4096, 4096, 0)
    assert 0 < ws_stage <= B * ((T + 255) // 256) * 464 * 8 + 256 < B * T * G * 8 // 200
    # overlapping windows at this length
    ov = bf.localize_batch(cfg2["bf_mat"], x, window=4096, hop=2048)
    assert tuple(ov["window_power"].shape) == (B, 1 + -(-(T - 4096) // 2048), G)
    np.testing.assert_array_equal(_np(ov["window_power"])[:, ::2][:, : nW - 1], _np(out["window_power"])[:, : nW - 1])


# ---- re-entrancy ------------------------------------------------------------------------------------------------------------
def test_two_host_threads_on_two_streams(cfg2, torch):
    """Two host threads, each with its own plan and stream, issue windowed calls at the same time: the serial run's bits."""
    z = golden("trials_cfg2.npz")
    bf = _snn()
    rng = np.random.RandomState(3)
    plans, xs = [bf.plan(), bf.new_plan()], []
    for i, p in enumerate(plans):
        p.set_neuron_kernel(cfg2["nir"])
        p.set_bf_mat(cfg2["bf_mat"] if i == 0 else cfg2["bf_mat"][:, ::3])
        xs.append([p.to_device(z["sig_in"] * (0.5 + rng.rand()) + 0.2 * rng.randn(3, 4799, 7)) for _ in range(20)])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in plans]
    kws = [dict(window=1024, hop=512), dict(window=768, hop=256)]

    def run(i, start=None):
        outs = []
        with torch.cuda.stream(streams[i]):
            if start is not None:
                start.wait()
            for x in xs[i]:
                outs.append(plans[i].snn_pipeline(x, **kws[i]))
        streams[i].synchronize()
        return [tuple(_np(o[k]) for k in ("window_power", "window_argmax", "power", "argmax")) for o in outs]

    serial = [run(0), run(1)]
    results, errors = [None, None], []
    barrier = threading.Barrier(2)

    def worker(i):
        try:
            results[i] = run(i, barrier)
        except BaseException as e:  # noqa: BLE001
            errors.append((i, repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors
    assert all(not t.is_alive() for t in threads)
    for i in range(2):
        for k, (got, want) in enumerate(zip(results[i], serial[i])):
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w, err_msg=f"thread {i} call {k}")


# ---- sweep --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parity", "throughput"])
def test_windowed_sweep_with_one_window_is_the_noisy_sweep(cfg2, mode, tmp_path):
    from haghighatshoarmuir2024_amd.sweep import noisy_target_sweep, windowed_target_sweep

    bf = _snn()
    kw = dict(snr_db_vec=[-5.0, 10.0], num_sim=4, seed=3, mode=mode, batch_trials=5)
    ref = noisy_target_sweep(bf, cfg2["bf_mat"], cfg2["doa_list"], **kw)
    one = windowed_target_sweep(bf, cfg2["bf_mat"], cfg2["doa_list"], 5120, **kw)
    assert one["window_argmax"].shape == (2, 4, 1)
    for k in ("doa", "argmax", "pmax", "err", "mae_deg"):
        np.testing.assert_array_equal(one[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(one["window_argmax"][:, :, 0], ref["argmax"])
    np.testing.assert_array_equal(one["window_pmax"][:, :, 0], ref["pmax"])
    # several windows, persisted and resumed: the same results, nothing recomputed
    a = windowed_target_sweep(bf, cfg2["bf_mat"], cfg2["doa_list"], 1024, hop=512, out_dir=tmp_path, **kw)
    assert a["window_argmax"].shape == (2, 4, 9) and a["window_mae_deg"].shape == (2, 9) and a["persistence"]["files_written"] == 2
    b = windowed_target_sweep(bf, cfg2["bf_mat"], cfg2["doa_list"], 1024, hop=512, out_dir=tmp_path, **kw)
    assert b["persistence"]["files_written"] == 0 and b["persistence"]["trials_loaded"] == 8
    for k in ("window_argmax", "window_pmax", "argmax", "err"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(a["doa"], ref["doa"])
