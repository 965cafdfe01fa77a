"""The on-disk format of a resumable sweep store (`out_dir=`, sweep.ShardStore): the entry names of `meta.json` (they are what is
hashed into the directory name), the values of its scalar entries, shape and dtype of its hashed arrays, and the record dtype and
file names of the `trials_*.npy` batches.  A sweep whose key entries or record changed would still compute the same results -- and
silently stop resuming the directories that earlier versions wrote.  Every sweep that runs on the CPU with an injected localizer;
the expected values are what the sweeps wrote before they shared one trial loop.  (No directory hash is pinned: it depends on libm
bits of the hashed arrays.)"""
import json
import os

import numpy as np
import pytest

FS, G = 48_000, 33

F8 = "float64"
ARRAYS = {"doa_list": ((G,), F8), "r_vec": ((7,), F8), "theta_vec": ((7,), F8), "snr_db_trial": ((4,), F8)}
SCALARS = {"format": 1, "fs": 48000.0, "mode": "parity", "num_mic": 7, "seed": 3, "total": 4}
BF_MAT = {"bf_mat": ((14, G), F8)}
# what _method_key adds for the SNN beamformer, and the tag the tests give an injected localizer
METHOD_ARRAYS = {"iir_a": ((5,), F8), "iir_b": ((5,), F8), "kernel": ((480,), F8), "tau_vec": ((2,), F8)}
METHOD_SCALARS = {"bipolar": True, "method": "SNNBeamformer", "robust_width": 12, "localizer": "fake"}

EXPECTED = {
    "noisy": dict(
        scalars={**SCALARS, "sweep": "noisy"},
        arrays={**ARRAYS, **BF_MAT, "sig_test": ((480,), F8), "time_test": ((480,), F8)},
        record=[("trial", "<i8"), ("doa", "<f8"), ("index", "<i8"), ("pmax", "<f8")]),
    "speech": dict(
        scalars={**SCALARS, "sweep": "speech"},
        arrays={**ARRAYS, **BF_MAT, "sig_test": ((331,), F8), "time_test": ((331,), F8)},
        record=[("trial", "<i8"), ("doa", "<f8"), ("index", "<i8"), ("pmax", "<f8")]),
    "multi-noisy": dict(
        scalars={**SCALARS, **METHOD_SCALARS, "sweep": "multi-noisy", "num_targets": 2, "min_separation": 0.7853981633974483,
                 "peak_separation": 0.39269908169872414, "tol": 0.39269908169872414, "rel_threshold": 0.0},
        arrays={**ARRAYS, **BF_MAT, **METHOD_ARRAYS, "gains": ((2,), F8), "sig_test": ((480,), F8), "time_test": ((480,), F8)},
        record=[("trial", "<i8"), ("doa", "<f8", (2,)), ("index", "<i8", (2,)), ("pmax", "<f8", (2,))]),
    "windowed-noisy": dict(
        scalars={**SCALARS, **METHOD_SCALARS, "sweep": "windowed-noisy", "record_width": 4, "window": 1024, "hop": 512},
        arrays={**ARRAYS, **BF_MAT, **METHOD_ARRAYS, "sig_test": ((2400,), F8), "time_test": ((2400,), F8)},
        record=[("trial", "<i8"), ("doa", "<f8"), ("index", "<i8", (4,)), ("pmax", "<f8", (4,))]),
    "moving-noisy": dict(  # (bf_mat=None: no such entry)
        scalars={**SCALARS, **METHOD_SCALARS, "sweep": "moving-noisy", "doa_max": 1.5707963267948966, "num_period": 0.5, "lag_frames": 100,
                 "settle_frames": 96, "win_fall": 96, "win_rise": 48},
        arrays={**ARRAYS, **METHOD_ARRAYS, "sig_test": ((480,), F8), "time_test": ((480,), F8)},
        record=[("trial", "<i8"), ("doa", "<f8"), ("index", "<i8"), ("pmax", "<f8"), ("med", "<f8")]),
}
# 4 trials in batches of 3: the name carries first trial, last + 1, count and the CRC-32 of the trial numbers (int64, little endian)
FILES = ["trials_00000000_00000003_3_4f8c5ccc.npy", "trials_00000003_00000004_1_ebadd88a.npy"]


def _beamf():
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    tau = 1.0 / (2 * np.pi * 2000)
    return SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=FS)


def _fake(width=None, frames=False):
    """A localizer that is a function of the batch alone: per-trial (index, value), [B, width] of them, or an index per frame."""

    def run(sig_batch, time_vec):
        s = np.abs(np.asarray(sig_batch))
        if frames:
            return (s.argmax(axis=2) * 13) % G
        v = np.stack([s[:, k :: (width or 1)].sum(axis=(1, 2)) for k in range(width or 1)], axis=1)
        a = (v * 1000).astype(np.int64) % G
        return (a[:, 0], v[:, 0]) if width is None else (a, v)

    return run


def _run(name, out_dir):
    from micloc.utils import Envelope

    from haghighatshoarmuir2024_amd import sweep

    beamf, doa_list = _beamf(), np.linspace(-np.pi, np.pi, G)
    W = np.random.RandomState(1).randn(14, G)
    kw = dict(snr_db_vec=[0.0, 10.0], num_sim=2, seed=3, mode="parity", batch_trials=3, out_dir=out_dir)
    tag = dict(store_key=dict(localizer="fake"))
    if name == "noisy":
        return sweep.noisy_target_sweep(beamf, W, doa_list, test_duration=10e-3, localizer=_fake(), **kw)
    if name == "speech":
        t = np.linspace(0.0, 10e-3, 331)
        return sweep.speech_target_sweep(beamf, W, doa_list, (t, np.sin(2 * np.pi * 1500 * t)), localizer=_fake(), **kw)
    if name == "multi-noisy":
        return sweep.multi_target_sweep(beamf, W, doa_list, num_targets=2, test_duration=10e-3, localizer=_fake(2), **tag, **kw)
    if name == "windowed-noisy":
        return sweep.windowed_target_sweep(beamf, W, doa_list, 1024, hop=512, test_duration=50e-3, localizer=_fake(4), **tag, **kw)
    return sweep.moving_target_sweep(beamf, None, doa_list, Envelope(rise_time=1e-3, fall_time=2e-3, fs=FS), test_duration=10e-3, lag_frames=100,
                                     localizer=_fake(frames=True), **tag, **kw)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_store_format(name, tmp_path):
    want = EXPECTED[name]
    res = _run(name, tmp_path)
    assert res["persistence"]["files_written"] == 2 and res["persistence"]["trials_loaded"] == 0
    (sub,) = os.listdir(tmp_path)
    assert sub.startswith(name + "-") and len(sub) == len(name) + 1 + 16
    meta = json.load(open(tmp_path / sub / "meta.json"))
    assert set(meta) == set(want["scalars"]) | set(want["arrays"])
    for k, v in want["scalars"].items():
        assert meta[k] == v and type(meta[k]) is type(v), k
    for k, (shape, dtype) in want["arrays"].items():
        assert set(meta[k]) == {"sha256", "shape", "dtype"} and len(meta[k]["sha256"]) == 64, k
        assert (tuple(meta[k]["shape"]), meta[k]["dtype"]) == (shape, dtype), k
    assert sorted(f for f in os.listdir(tmp_path / sub) if f != "meta.json") == FILES
    for f, trials in zip(FILES, ([0, 1, 2], [3])):
        rec = np.load(tmp_path / sub / f)
        assert [tuple(d) for d in rec.dtype.descr] == want["record"] and rec.dtype.itemsize == sum(np.dtype([d]).itemsize for d in want["record"])
        assert rec["trial"].tolist() == trials
    # the store of a second run reads these files back: nothing is computed, nothing written
    again = _run(name, tmp_path)
    assert again["persistence"]["trials_loaded"] == 4 and again["persistence"]["files_written"] == 0 and os.listdir(tmp_path) == [sub]
    for k, v in res.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(again[k], v, err_msg=k)
