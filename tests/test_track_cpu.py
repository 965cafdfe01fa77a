"""CPU checks of the moving-target sweep and of the tracking entries (tests/test_hip_track_fused.py has the device side): the DoA path,
the lag / settle alignment, the error metric and its median against a plain NumPy restatement through an injected localizer, the
store key, the C symbols and their status codes, and moving_target_sweep over gloo (world 2 = world 1)."""
import ctypes
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import csrc_build
from conftest import ROOT

FS = 48_000


def _beamf():
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    tau = 1.0 / (2 * np.pi * 2000)
    return SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=FS)


def _env(rise=1e-3, fall=5e-3):
    from micloc.utils import Envelope

    return Envelope(rise_time=rise, fall_time=fall, fs=FS)


def test_path_generation():
    from haghighatshoarmuir2024_amd.sweep import moving_doa_path

    t = np.arange(0, 0.1, 1 / FS)
    p = moving_doa_path(t, 0.1, np.pi / 2, 0.5, np.asarray([0.0, 1.25]))
    assert p.shape == (2, len(t))
    # phase 0: the script's own path (paper_plots/target_snn_localization.py:595-597)
    np.testing.assert_array_equal(p[0], np.pi / 2 * np.sin(0.5 * np.pi * t / 0.1 + 0.0))
    np.testing.assert_array_equal(p[1], np.pi / 2 * np.sin(0.5 * np.pi * t / 0.1 + 1.25))
    assert np.abs(p).max() <= np.pi / 2
    np.testing.assert_array_equal(moving_doa_path(t, 0.1, 1.0, 2.0, 0.3), np.sin(2.0 * np.pi * t / 0.1 + 0.3))


def test_lag_and_settle_alignment_and_the_metric():
    from haghighatshoarmuir2024_amd.sweep import track_errors

    rng = np.random.RandomState(1)
    G, B, T = 97, 3, 400
    doa_list = np.linspace(-np.pi, np.pi, G)
    truth = rng.uniform(-1.5, 1.5, size=(B, T))
    index = rng.randint(0, G, size=(B, T))
    for lag, settle in ((0, 0), (7, 0), (7, 50), (60, 20), (399, 0)):
        mean, med = track_errors(doa_list, index, truth, lag, settle)
        t0 = max(lag, settle)
        for b in range(B):
            e = [np.arcsin(abs(np.sin(doa_list[index[b, t]] - truth[b, t - lag]))) for t in range(t0, T)]
            assert mean[b] == np.mean(np.asarray(e)) and med[b] == np.median(np.asarray(e)), (lag, settle, b)
    # an estimate that IS the delayed truth on the grid scores zero; pi-periodic: the back lobe scores zero as well
    path = doa_list[rng.randint(0, G, size=(1, T))]
    idx = np.searchsorted(doa_list, np.roll(path, 5, axis=1))
    mean, med = track_errors(doa_list, idx, path, 5, 5)
    assert mean[0] < 1e-12 and med[0] < 1e-12
    with pytest.raises(ValueError):
        track_errors(doa_list, index, truth, 400, 0)


def _fake_localizer(G, calls=None):
    """index[b, t] from the signal itself (deterministic, no device): the column of the frame's largest |sample| scaled onto the grid."""

    def run(sig_batch, time_vec):
        if calls is not None:
            calls.append(len(sig_batch))
        s = np.asarray(sig_batch)
        return (np.abs(s).argmax(axis=2) * 13 + (np.abs(s).sum(axis=2) * 1000).astype(np.int64)) % G

    return run


def test_sweep_against_a_numpy_restatement():
    from haghighatshoarmuir2024_amd.snn_beamformer import synthesize_array_signal
    from haghighatshoarmuir2024_amd.sweep import moving_target_sweep

    beamf, env = _beamf(), _env()
    G = 57
    doa_list = np.linspace(-np.pi, np.pi, G)
    kw = dict(snr_db_vec=[0.0, 10.0], num_sim=3, seed=11, mode="parity", test_duration=20e-3, batch_trials=2, localizer=_fake_localizer(G))
    res = moving_target_sweep(beamf, None, doa_list, env, doa_max=1.0, num_period=1.5, **kw)
    assert res["lag_frames"] == 480 and res["settle_frames"] == 240  # int(kernel_duration * fs), int(fs * fall_time)
    assert res["err"].shape == (2, 3) and res["track_mae_deg"].shape == (2,) and res["track_median_deg"].shape == (2,)
    # the restatement: the draw order rand(1), randn(T, M) of the global stream
    time_test = np.arange(0, 20e-3, 1 / FS)
    sig_test = np.sin(2 * np.pi * 2000.0 * time_test)
    snr = np.repeat(np.asarray([0.0, 10.0]) - 10 * np.log10((FS / 2) / 1000.0), 3)
    np.random.seed(11)
    err, med, phase = [], [], []
    for trial in range(6):
        ph = np.random.rand(1)[0] * 2 * np.pi
        doa_t = 1.0 * np.sin(1.5 * np.pi * time_test / 20e-3 + ph)
        time_in, sig = synthesize_array_signal(beamf.geometry, FS, time_test, sig_test, doa_t)
        sig += np.sqrt(np.mean(sig**2)) / np.sqrt(10 ** (snr[trial] / 10)) * np.random.randn(*sig.shape)
        idx = _fake_localizer(G)(sig[None], time_in)[0]
        truth = 1.0 * np.sin(1.5 * np.pi * time_in / 20e-3 + ph)
        e = np.asarray([np.arcsin(abs(np.sin(doa_list[idx[t]] - truth[t - 480]))) for t in range(480, len(time_in))])
        err.append(e.mean())
        med.append(np.median(e))
        phase.append(ph)
    np.testing.assert_array_equal(res["phase"].ravel(), phase)
    np.testing.assert_array_equal(res["err"].ravel(), err)
    np.testing.assert_array_equal(res["med"].ravel(), med)
    np.testing.assert_array_equal(res["track_mae_deg"], np.mean(np.reshape(err, (2, 3)), axis=1) * 180 / np.pi)
    np.testing.assert_array_equal(res["track_median_deg"], np.median(np.reshape(med, (2, 3)), axis=1) * 180 / np.pi)
    # explicit lag / settle
    res2 = moving_target_sweep(beamf, None, doa_list, env, doa_max=1.0, num_period=1.5, lag_frames=3, settle_frames=700, **kw)
    assert res2["lag_frames"] == 3 and res2["settle_frames"] == 700 and not np.array_equal(res2["err"], res["err"])
    with pytest.raises(ValueError):
        moving_target_sweep(beamf, None, doa_list, env, settle_frames=959, **kw)
    with pytest.raises(ValueError):
        moving_target_sweep(beamf, None, doa_list, env, **dict(kw, mode="fast"))


def test_store_key_changes_with_every_keyed_parameter(tmp_path):
    from haghighatshoarmuir2024_amd.sweep import moving_target_sweep

    G = 33
    doa_list = np.linspace(-np.pi, np.pi, G)
    base = dict(doa_max=1.0, num_period=0.5, lag_frames=100, settle_frames=200)

    def run(beamf=None, env=None, store_key=None, **over):
        calls = []
        kw = dict(base, **over)
        res = moving_target_sweep(beamf or _beamf(), None, doa_list, env or _env(), snr_db_vec=[5.0], num_sim=2, seed=3, test_duration=10e-3,
                                  localizer=_fake_localizer(G, calls), out_dir=tmp_path, store_key=store_key or dict(localizer="fake"), **kw)
        return res, calls

    ref, calls = run()
    assert calls == [2] and len(os.listdir(tmp_path)) == 1
    again, calls = run()
    assert calls == [] and again["persistence"]["trials_loaded"] == 2  # the same key: everything is found
    for k in ("err", "med", "phase", "track_mae_deg", "track_median_deg"):
        np.testing.assert_array_equal(again[k], ref[k])
    (sub,) = os.listdir(tmp_path)
    meta = json.load(open(tmp_path / sub / "meta.json"))
    assert sub.startswith("moving-noisy-") and meta["method"] == "SNNBeamformer" and "tau_vec" in meta and "kernel" in meta
    assert (meta["doa_max"], meta["num_period"], meta["lag_frames"], meta["settle_frames"], meta["win_fall"], meta["win_rise"]) == (1.0, 0.5, 100, 200, 240, 48)
    n = 1
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer
    from micloc.snn_beamformer import SNNBeamformer

    tau = 1.0 / (2 * np.pi * 1500)
    others = [dict(doa_max=1.1), dict(num_period=0.75), dict(lag_frames=101), dict(settle_frames=201), dict(env=_env(fall=6e-3)),
              dict(env=_env(rise=2e-3)), dict(store_key=dict(localizer="other")),
              dict(beamf=Beamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], fs=FS)),  # the class
              dict(beamf=SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=FS)),  # tau_vec
              dict(beamf=SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [900.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=FS))]  # plan key
    for o in others:
        _, calls = run(**o)
        n += 1
        assert calls == [2] and len(os.listdir(tmp_path)) == n, o


def test_header_declares_and_lib_binds_the_tracking_symbols():
    from haghighatshoarmuir2024_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "micloc_hip.h")).read(), flags=re.S)
    names = ("micloc_track_workspace_bytes", "micloc_track_is_fused", "micloc_lif_beamform_track_f64", "micloc_beamform_c128_track_f64",
             "micloc_snn_pipeline_track_f64", "micloc_beamformer_pipeline_track_f64")
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert re.search(rf"\b{n}\s*\(", text), f"{n} is not declared in the header"
        assert n in _lib.SYMBOLS and hasattr(raw, n), n
    lib = _lib.load()
    assert lib.micloc_abi_version() == 1
    # argument validation before any device call
    one = ctypes.c_void_p(256)
    assert lib.micloc_track_workspace_bytes(None, 2, 100) == 0
    assert lib.micloc_track_is_fused(None) == _lib.MICLOC_ERR_INVALID
    for fn in (lib.micloc_lif_beamform_track_f64, lib.micloc_snn_pipeline_track_f64, lib.micloc_beamformer_pipeline_track_f64):
        assert fn(None, one, 1, 10, 0.9, 0.1, 0.99, one, None, None, one, 1 << 20, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_beamform_c128_track_f64(None, one, 1, 10, 16, 0.9, 0.1, 0.99, one, None, None, one, 1 << 20, None) == _lib.MICLOC_ERR_INVALID
    src = open(os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc", "track.hip")).read()
    assert "atomic" not in src.lower() and "hipStreamSynchronize" not in src and "hipDeviceSynchronize" not in src
    assert "track.hip" in csrc_build.built_sources()


# ---- moving_target_sweep over gloo ----------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys, json
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
rank, world, port, res_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
import torch.distributed as dist
from haghighatshoarmuir2024_amd.sweep import moving_target_sweep
from test_track_cpu import _beamf, _env, _fake_localizer

if world > 1:
    dist.init_process_group("gloo", rank=rank, world_size=world)
G = 57
res = moving_target_sweep(_beamf(), None, np.linspace(-np.pi, np.pi, G), _env(), snr_db_vec=[0.0, 10.0], num_sim=5, seed=5, mode="parity", rank=rank,
                          world_size=world, localizer=_fake_localizer(G), batch_trials=2, test_duration=20e-3)
np.savez(os.path.join(res_dir, f"w{world}_r{rank}.npz"), **{k: v for k, v in res.items() if isinstance(v, np.ndarray)})
json.dump({"exchange": res["exchange"]}, open(os.path.join(res_dir, f"w{world}_r{rank}.json"), "w"))
if world > 1:
    dist.barrier()
    dist.destroy_process_group()
""" % {"root": ROOT}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_moving_sweep_world2_equals_world1(tmp_path):
    outs = {}
    for world in (1, 2):
        d = tmp_path / f"w{world}"
        d.mkdir()
        port = str(_free_port())
        procs = [subprocess.Popen([sys.executable, "-c", CHILD, str(r), str(world), port, str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                 for r in range(world)]
        for p in procs:
            assert p.wait(timeout=240) == 0, p.stderr.read().decode(errors="replace")[-3000:]
        outs[world] = d
    ref = np.load(outs[1] / "w1_r0.npz")
    assert ref["err"].shape == (2, 5)
    for r in range(2):
        got = np.load(outs[2] / f"w2_r{r}.npz")
        for k in ("phase", "err", "med", "track_mae_deg", "track_median_deg", "mae_deg"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"rank {r} {k}")
        assert json.load(open(outs[2] / f"w2_r{r}.json"))["exchange"]["collectives"] == 1


def test_envelope_consts_are_numpys_own_arithmetic():
    """runtime.envelope_consts -> (a_rise, i_rise, a_fall): `1 - 1 / wl` and `1 / wl` of NumPy on the int array [fall, rise], element for
    element, and the refusal of a window below one sample.  Needs no device."""
    from haghighatshoarmuir2024_amd.runtime import envelope_consts

    for wf, wr in [(1, 1), (624, 96), (96, 624), (4800, 480), (3, 7), (2**31 - 1, 1)]:
        wl = np.asarray([wf, wr])
        a, inv = 1 - 1 / wl, 1 / wl
        got = envelope_consts(wf, wr)
        assert all(type(v) is float for v in got)
        assert got == (a[1], inv[1], a[0]), (wf, wr)
    assert envelope_consts(1, 1) == (0.0, 1.0, 0.0)
    assert envelope_consts(np.int64(5), 5.9) == envelope_consts(5, 5)  # int() of what Envelope.win_lens holds
    for wf, wr in [(0, 5), (5, 0), (0, 0), (-1, 3)]:
        with pytest.raises(ValueError, match="at least one sample"):
            envelope_consts(wf, wr)
