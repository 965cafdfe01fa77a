"""CPU checks of the time-resolved read-out: utils.window_bounds against hand cases, the C oracle's y windowed in NumPy against the
reference's windowed power (tests/golden/windows.npz, from the real reference: tests/golden/make_golden_windows.py), the new C-ABI
symbols and their status codes, the ValueError paths, and windowed_target_sweep over gloo (world 2 = world 1, resume, resume key)
with an injected host localizer (the C oracle: allowed in tests)."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import csrc_build
from conftest import ROOT, golden

from haghighatshoarmuir2024_amd import _lib
from haghighatshoarmuir2024_amd.utils import window_bounds


# ---- the rule -------------------------------------------------------------------------------------------------------------
def test_window_bounds_hand_cases():
    def wb(*a):
        s, e = window_bounds(*a)
        assert s.dtype == np.int64 and e.dtype == np.int64
        return list(s), list(e)

    assert wb(100, 256) == ([0], [100])                      # T <= window: one window, cut at T
    assert wb(256, 256) == ([0], [256])
    assert wb(1024, 256) == ([0, 256, 512, 768], [256, 512, 768, 1024])  # an exact fit, hop defaults to window
    assert wb(1024, 512, 256) == ([0, 256, 512], [512, 768, 1024])       # an exact fit with overlap
    assert wb(4799, 1024, 512) == ([0, 512, 1024, 1536, 2048, 2560, 3072, 3584, 4096],
                                   [1024, 1536, 2048, 2560, 3072, 3584, 4096, 4608, 4799])  # a leftover window of 703 frames
    assert wb(1000, 256, 256) == ([0, 256, 512, 768], [256, 512, 768, 1000])
    assert wb(257, 256, 1024) == ([0, 1024], [256, 1024])    # hop > window: 1 + ceil(1 / 1024) windows, the second one empty
    assert wb(1792, 256, 512) == ([0, 512, 1024, 1536], [256, 768, 1280, 1792])  # hop > window: gaps between the windows
    assert wb(1000, 256, 512) == ([0, 512, 1024], [256, 768, 1024])             # ... and a last window past the recording: empty
    for bad in ((0, 256), (100, 0), (100, 256, 0), (100, -256), (100, 256, -1)):
        with pytest.raises(ValueError):
            window_bounds(*bad)
    # the C side counts the same windows
    lib = _lib.load()
    rng = np.random.RandomState(0)
    for _ in range(200):
        q = int(rng.choice([256, 512]))
        T, window, hop = int(rng.randint(1, 400_000)), q * int(rng.randint(1, 40)), q * int(rng.randint(1, 40))
        assert lib.micloc_window_count(T, window, hop, q) == len(window_bounds(T, window, hop)[0]), (T, window, hop)


def test_abi_symbols_and_status_codes_without_a_gpu():
    lib = _lib.load()
    names = ("micloc_window_quantum", "micloc_window_count", "micloc_window_workspace_bytes", "micloc_lif_beamform_windows_f64",
             "micloc_beamform_c128_windows_f64", "micloc_snn_pipeline_windows_f64", "micloc_beamformer_pipeline_windows_f64")
    header = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    for n in names:
        assert n in _lib.SYMBOLS and hasattr(lib, n) and f"{n}(" in header, n
    assert lib.micloc_abi_version() == 1
    # the window rule's argument errors (pure function)
    assert lib.micloc_window_count(4799, 1024, 512, 256) == 9
    assert lib.micloc_window_count(4799, 5120, 256, 256) == 1
    assert lib.micloc_window_count(332_157, 4096, 2048, 256) == 162
    assert lib.micloc_window_count(4799, 1000, 512, 256) == _lib.MICLOC_ERR_SHAPE   # window not a multiple of the quantum
    assert lib.micloc_window_count(4799, 1024, 100, 256) == _lib.MICLOC_ERR_SHAPE   # hop not a multiple
    assert lib.micloc_window_count(4799, 1024, 0, 256) == _lib.MICLOC_ERR_SHAPE     # zero hop
    assert lib.micloc_window_count(4799, 0, 256, 256) == _lib.MICLOC_ERR_SHAPE
    assert lib.micloc_window_count(4799, 768, 512, 512) == _lib.MICLOC_ERR_SHAPE == -2  # 512-frame chunks (more than 64 channels)
    assert lib.micloc_window_count(4799, 1536, 512, 512) == 8
    assert lib.micloc_window_count(0, 1024, 512, 256) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_window_count(4799, 1024, 512, 0) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_window_count(2**31 - 1, 256, 256, 256) == (2**31 - 1 + 255) // 256  # no 32-bit overflow inside
    # plan entries validate before any device call
    vp = ctypes.c_void_p
    one = vp(256)
    assert lib.micloc_window_quantum(None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_window_workspace_bytes(None, 1, 4799, 1024, 512, 1) == 0
    assert lib.micloc_lif_beamform_windows_f64(None, one, 1, 4799, 1024, 512, one, one, None, None, one, 1 << 20, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_beamform_c128_windows_f64(None, one, 1, 4799, 4800, 1024, 512, one, one, None, None, one, 1 << 20, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_snn_pipeline_windows_f64(None, one, 1, 4799, 1024, 512, None, one, one, None, None, one, 1 << 20, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_beamformer_pipeline_windows_f64(None, one, 1, 4799, 1024, 512, one, one, None, None, one, 1 << 20, None) == _lib.MICLOC_ERR_INVALID


def test_windows_source_has_no_atomics_and_is_built():
    """The new kernels live in their own file, use no atomics and are part of the library."""
    text = open(os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc", "windows.hip")).read().lower()
    assert "atomic" not in text.replace("no atomics", "")
    assert "window_power_kernel" in text
    assert "windows.hip" in csrc_build.built_sources()


def test_value_error_paths():
    from haghighatshoarmuir2024_amd.sweep import median_window_index, windowed_target_sweep
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    tau = 1.0 / (2 * np.pi * 2000)
    bf = SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=48_000)
    W, doa = np.zeros((14, 5)), np.linspace(-np.pi, np.pi, 5)
    loc = lambda s, t: (_ for _ in ()).throw(AssertionError("no trial may run"))  # noqa: E731
    with pytest.raises(ValueError, match="at least 1"):
        windowed_target_sweep(bf, W, doa, 0, localizer=loc)
    with pytest.raises(ValueError, match="at least 1"):
        windowed_target_sweep(bf, W, doa, 256, hop=0, localizer=loc)
    with pytest.raises(ValueError, match="hop <= window"):
        windowed_target_sweep(bf, W, doa, 256, hop=512, localizer=loc)
    with pytest.raises(ValueError, match="mode"):
        windowed_target_sweep(bf, W, doa, 256, mode="fast", localizer=loc)
    # the median-over-windows estimate: the sample with the least summed pi-periodic distance to the others
    grid = np.deg2rad(np.arange(-180, 180, 10.0))
    idx = np.array([[3, 4, 30, 4, 5], [0, 1, 2, 1, 35], [7, 7, 7, 7, 7], [2, 9, 2, 9, 3]])
    #  row 1: -180, -170, -160, -170, 170 degrees are 0, 10, 20, 10, -10 on the half circle: the median is 10 (index 1)
    #  row 3: -160, -90, -160, -90, -150: summed distances 150, 200, 150, 200 and 140: the median is -150 (index 3)
    assert list(median_window_index(grid, idx)) == [4, 1, 7, 3]
    assert list(median_window_index(grid, idx[:, :1])) == [3, 0, 7, 2]


# ---- the oracle's y, windowed in NumPy, is the reference's windowed power ---------------------------------------------
def _windowed(y, window, hop):
    start, stop = window_bounds(len(y), window, hop)
    p = np.stack([np.mean(np.abs(y[s:e]) ** 2, axis=0) for s, e in zip(start, stop)])
    return p, np.argmax(p, axis=1)


def test_oracle_windowed_power_equals_the_golden(cfg2):
    from oracle import oracle as O

    O.build()
    g, z = golden("windows.npz"), golden("trials_cfg2.npz")
    for i in range(3):
        y = O.snn_chain(z["sig_in"][i], cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True, cfg2["nir"], cfg2["bf_mat"], want=("y",))["y"]
        p, a = _windowed(y, int(g["a_window"]), int(g["a_hop"]))
        np.testing.assert_allclose(p, g["a_power"][i], rtol=1e-10, atol=0)
        np.testing.assert_array_equal(a, g["a_argmax"][i])
    m = golden("moving_target.npz")
    tau = 1 / (2 * np.pi * 2000)
    y = O.snn_chain(m["trial_sig_q"].astype(np.float64) / 4096.0, cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True,
                    O.neuron_kernel(m["trial_time"], [tau, tau]), cfg2["bf_mat"], want=("y",))["y"]
    p, a = _windowed(y, int(g["b_window"]), int(g["b_hop"]))
    np.testing.assert_allclose(p, g["b_power"], rtol=1e-10, atol=0)
    np.testing.assert_array_equal(a, g["b_argmax"])
    assert len(np.unique(a)) > 3  # the arg-max moves with the target
    c = golden("beamformer_c128_g449.npz")
    y = O.beamformer_chain(c["sig_in"], cfg2["kernel"], cfg2["b"], cfg2["a"], c["bf_mat"])["y"]
    p, a = _windowed(y, int(g["c_window"]), int(g["c_hop"]))
    np.testing.assert_allclose(p, g["c_power"], rtol=1e-10, atol=0)
    np.testing.assert_array_equal(a, g["c_argmax"])
    # the generator's promise: no window's arg-max hangs on rounding
    for k in "abc":
        top = np.sort(g[f"{k}_power"].reshape(-1, 449), axis=1)[:, -2:]
        assert ((top[:, 1] - top[:, 0]) / top[:, 1]).min() > 1e-9


# ---- windowed_target_sweep over gloo ------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys, json
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
rank, world, port, out_dir, res_dir, window, die_after = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5], int(sys.argv[6]), int(sys.argv[7])
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
import torch.distributed as dist
from haghighatshoarmuir2024_amd.sweep import windowed_target_sweep
from haghighatshoarmuir2024_amd.utils import window_bounds
from micloc.array_geometry import CenterCircularArray
from micloc.snn_beamformer import SNNBeamformer, neuron_impulse_response
from oracle import oracle as O

if world > 1:
    dist.init_process_group("gloo", rank=rank, world_size=world)
bfz = np.load(os.path.join(%(root)r, "tests", "golden", "bf_mat_chirp449_bipolar.npz"))
tau = 1.0 / (2 * np.pi * 2000)
beamf = SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=48_000)
calls = []
HOP = 256

def oracle_localizer(sig_batch, time_vec):
    if die_after >= 0 and len(calls) == die_after:
        os._exit(17)
    calls.append(len(sig_batch))
    nir = neuron_impulse_response(time_vec, beamf.tau_vec)
    b, a = beamf.bandpass_filter
    am, pm = [], []
    for sig in sig_batch:
        y = O.snn_chain(sig, beamf.kernel, b, a, beamf.spk_encoder.robust_width, True, nir, bfz["bf_mat"], want=("y",))["y"]
        start, stop = window_bounds(len(y), window, HOP)
        p = np.stack([np.mean(y[s:e] ** 2, axis=0) for s, e in zip(start, stop)])
        am.append(np.argmax(p, axis=1))
        pm.append(p.max(axis=1))
    return np.asarray(am, dtype=np.int64), np.asarray(pm)

res = windowed_target_sweep(beamf, bfz["bf_mat"], bfz["doa_list"], window, hop=HOP, snr_db_vec=[0.0, 10.0], num_sim=5, seed=5, mode="parity", rank=rank,
                            world_size=world, localizer=oracle_localizer, batch_trials=2, test_duration=20e-3,
                            out_dir=out_dir if out_dir != "-" else None, store_key=dict(localizer="oracle"))
np.savez(os.path.join(res_dir, f"w{world}_r{rank}.npz"), **{k: v for k, v in res.items() if isinstance(v, np.ndarray)})
json.dump({"calls": calls, "persistence": res.get("persistence"), "exchange": res["exchange"]}, open(os.path.join(res_dir, f"w{world}_r{rank}.json"), "w"))
if world > 1:
    dist.barrier()
    dist.destroy_process_group()
""" % {"root": ROOT}

KEYS = ("doa", "window_argmax", "window_pmax", "window_err", "window_mae_deg", "window_start", "argmax", "pmax", "err", "mae_deg")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _job(world, out_dir, res_dir, window=512, die=None, timeout=240):
    port = str(_free_port())
    procs = []
    for r in range(world):
        da = die[1] if die and die[0] == r else -1
        procs.append(subprocess.Popen([sys.executable, "-c", CHILD, str(r), str(world), port, str(out_dir), str(res_dir), str(window), str(da)],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    codes = [None] * world
    if die:
        codes[die[0]] = procs[die[0]].wait(timeout=timeout)
        for r, p in enumerate(procs):
            if r != die[0]:
                try:
                    codes[r] = p.wait(timeout=20)
                except subprocess.TimeoutExpired:
                    p.terminate()
                    codes[r] = p.wait(timeout=20)
    else:
        for r, p in enumerate(procs):
            codes[r] = p.wait(timeout=timeout)
            assert codes[r] == 0, p.stderr.read().decode(errors="replace")[-3000:]
    return codes


@pytest.mark.timeout(900)
def test_windowed_sweep_world2_resume_and_key(tmp_path):
    from oracle import oracle as O

    O.build()
    store, r_ref, r_a, r_b, r_c, r_d = (tmp_path / n for n in ("store", "ref", "a", "b", "c", "d"))
    for d in (store, r_ref, r_a, r_b, r_c, r_d):
        d.mkdir()
    # world 1, uninterrupted, no persistence: 10 trials of 959 frames, windows of 512 hopping by 256: 3 windows
    assert _job(1, "-", r_ref) == [0]
    ref = np.load(r_ref / "w1_r0.npz")
    assert ref["window_argmax"].shape == (2, 5, 3) and ref["window_mae_deg"].shape == (2, 3) and list(ref["window_start"]) == [0, 256, 512]
    assert ref["argmax"].shape == (2, 5) and ref["mae_deg"].shape == (2,)
    # world 2 equals world 1 on every rank, with ONE all-gather
    assert _job(2, "-", r_a) == [0, 0]
    for r in range(2):
        got = np.load(r_a / f"w2_r{r}.npz")
        for k in KEYS:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"rank {r} {k}")
        assert json.load(open(r_a / f"w2_r{r}.json"))["exchange"]["collectives"] == 1
    # world 2 with persistence; rank 1 dies at its second batch; the resumed run ends on the uninterrupted bits
    codes = _job(2, store, r_b, die=(1, 1))
    assert codes[1] == 17
    (sub,) = os.listdir(store)
    meta = json.load(open(store / sub / "meta.json"))
    assert sub.startswith("windowed-noisy-") and meta["window"] == 512 and meta["hop"] == 256 and meta["record_width"] == 3
    assert meta["method"] == "SNNBeamformer" and "tau_vec" in meta and "kernel" in meta and "iir_b" in meta and meta["localizer"] == "oracle"
    assert any(f.startswith("trials_00000005_00000007_2_") for f in os.listdir(store / sub))  # rank 1's first batch
    assert _job(2, store, r_c) == [0, 0]
    for r in range(2):
        got = np.load(r_c / f"w2_r{r}.npz")
        for k in KEYS:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"resumed rank {r} {k}")
    info = json.load(open(r_c / "w2_r1.json"))
    assert info["calls"] == [2, 1] and info["persistence"]["trials_loaded"] >= 2  # rank 1: trials 7, 8 and 9 were missing
    # a changed window starts a fresh directory (and computes everything)
    assert _job(1, store, r_d, window=768) == [0]
    assert len(os.listdir(store)) == 2
    info = json.load(open(r_d / "w1_r0.json"))
    assert info["calls"] == [2] * 5 and info["persistence"]["trials_loaded"] == 0
    assert np.load(r_d / "w1_r0.npz")["window_argmax"].shape == (2, 5, 2)
