"""CPU checks of the multi-source read-out and of multi_target_sweep: the NumPy restatement of the peak rule on hand cases, the
C-ABI's argument checks without a device, the sweep's argument checks, store key and trial generator, and -- with the C oracle
injected as the localizer -- sharding over a gloo world of 2, resume after an interrupted run, and num_targets = 1 against
noisy_target_sweep."""
import ctypes
import os
import socket

import numpy as np
import pytest

import multisource_ref as R
from conftest import ROOT

CLOSED = np.linspace(-np.pi, np.pi, 9)  # step pi / 4
LINEAR = np.linspace(0.0, 1.0, 9)
CIRC = np.arange(8) * (2 * np.pi / 8)


def pk(p, doa, K, sep=None, rel=0.0, kind=None):
    i, v = R.peaks(np.asarray(p, dtype=np.float64), doa, K, sep, rel, kind)
    return list(i[0]), v[0]


# ---- the rule, by hand ---------------------------------------------------------------------------------------------------------

def test_grid_kinds_from_the_doa_list():
    from haghighatshoarmuir2024_amd.utils import doa_grid_kind

    for doa, kind, name in ((CLOSED, R.CIRCULAR_CLOSED, "circular_closed"), (CIRC, R.CIRCULAR, "circular"), (LINEAR, R.LINEAR, "linear"),
                            (np.linspace(-np.pi, np.pi, 449), R.CIRCULAR_CLOSED, "circular_closed"), (np.zeros(1), R.LINEAR, "linear"),
                            (np.linspace(-np.pi / 2, np.pi / 2, 50), R.LINEAR, "linear")):
        assert R.grid_kind(doa) == kind and doa_grid_kind(doa) == name
    assert doa_grid_kind(np.linspace(-np.pi, np.pi + 2e-9, 9)) == "linear"


def test_plateau_gives_one_peak():
    p = [0, 1, 3, 3, 1, 0, 0, 2, 0]
    assert pk(p, LINEAR, 3)[0] == [2, 7, -1]  # the first plateau point; its plateau neighbour is within two steps
    assert pk(p, LINEAR, 3, sep=0.0)[0] == [2, 3, 7]  # without separation every plateau point is a local maximum
    # a plateau of three: its far end lies exactly two steps away (distance >= min_separation), a third step suppresses it
    q = [0, 1, 3, 3, 3, 1, 0, 2, 0]
    assert pk(q, LINEAR, 3)[0] == [2, 4, 7]
    assert pk(q, LINEAR, 3, sep=0.3)[0] == [2, 7, -1]


def test_closed_seam():
    # max at G-1: the merged ring point reports G-1; its ring neighbours are 1 and G-2
    p = np.array([1.0, 0, 0, 0, 2, 0, 0, 0.5, 3.0])
    i, v = pk(p, CLOSED, 2)
    assert i == [8, 4] and v[0] == 3.0
    # max at 0
    p2 = p.copy()
    p2[0], p2[8] = 3.0, 1.0
    assert pk(p2, CLOSED, 2)[0] == [0, 4]
    # tied: index 0
    p3 = p.copy()
    p3[0] = 3.0
    assert pk(p3, CLOSED, 2)[0] == [0, 4]
    # the seam blocks a neighbour: G-2 = 7 is below the merged value, so 7 is no peak even though p[7] > p[6]
    p4 = np.array([1.0, 0.5, 0.4, 0.3, 0.2, 0.3, 0.5, 0.9, 0.0])
    assert pk(p4, CLOSED, 2, sep=0.0)[0] == [0, -1]
    # on a linear reading of the same numbers, 0 and 7 are both peaks
    assert pk(p4, CLOSED, 2, sep=0.0, kind=R.LINEAR)[0] == [0, 7]


def test_circular_wrap_and_linear_edges():
    p = np.array([3.0, 1, 0, 0, 2, 0, 0, 3.5])
    assert pk(p, CIRC, 3, sep=0.0)[0] == [7, 4, -1]  # 0 neighbours 7 on the ring: no peak
    assert pk(p, CIRC, 3, sep=0.0, kind=R.LINEAR)[0] == [7, 0, 4]  # linear: both ends have one neighbour
    # circular distance: 7 and 0 are one step apart on the ring
    assert pk([3.0, 0, 0, 0, 0, 0, 2, 0], CIRC, 2, sep=2 * np.pi / 8 * 1.5)[0] == [0, 6]
    assert pk([3.0, 0, 0, 0, 0, 0, 0, 2.0], CIRC, 2, sep=0.0, kind=R.LINEAR)[0] == [0, 7]


def test_nan_rows():
    p = np.array([0, 1, np.nan, 2, 0, 5, np.nan, 0, 0.5])
    i, v = pk(p, LINEAR, 4, sep=0.0)
    assert i == [5, 3, 1, 8] and np.array_equal(v, [5, 2, 1, 0.5])  # a NaN neighbour counts as lower
    i, v = pk(np.full(9, np.nan), LINEAR, 2)
    assert i == [-1, -1] and np.isnan(v).all()
    # closed seam with a NaN end: the other end's value, index 0 if p[G-1] is NaN
    q = np.zeros(9)
    q[0], q[8] = 2.0, np.nan
    assert pk(q, CLOSED, 1)[0] == [0]
    q[0], q[8] = np.nan, 2.0
    assert pk(q, CLOSED, 1)[0] == [8]


def test_rel_threshold_and_fewer_than_k():
    p = np.array([0, 1.0, 0, 0.49, 0, 0.5, 0, 0, 0])
    assert pk(p, LINEAR, 3)[0] == [1, 5, 3]  # 3 is exactly two steps from 5
    assert pk(p, LINEAR, 5)[0] == [1, 5, 3, 7, -1]  # the zero plateau 6..8 is a local maximum; 8 lies one step from 7
    assert pk(p, LINEAR, 4, rel=0.5)[0] == [1, 5, -1, -1]
    assert pk(p, LINEAR, 4, rel=0.51)[0] == [1, -1, -1, -1]


def test_k1_is_argmax_on_every_grid():
    rng = np.random.RandomState(3)
    for doa in (CLOSED, CIRC, LINEAR, np.linspace(-np.pi, np.pi, 57)):
        for _ in range(200):
            p = rng.randint(0, 4, size=len(doa)).astype(np.float64)  # many exact ties
            assert pk(p, doa, 1)[0][0] == int(np.argmax(p))


def test_match_errors_restated():
    from haghighatshoarmuir2024_amd.sweep import match_errors

    rng = np.random.RandomState(0)
    doa_list = np.linspace(-np.pi, np.pi, 449)
    for K in (1, 2, 3):
        truth = rng.rand(50, K) * 2 * np.pi
        index = rng.randint(-1, 449, size=(50, K))
        got = match_errors(truth, doa_list, index)
        for n in range(50):
            np.testing.assert_array_equal(got[n], R.match(truth[n], doa_list, index[n]))


# ---- the C-ABI without a device ---------------------------------------------------------------------------------------------------

def test_doa_peaks_abi_rejects_without_a_device():
    from haghighatshoarmuir2024_amd import _lib

    lib = _lib.load()
    p, d, i, v = (ctypes.c_void_p(64) for _ in range(4))  # never dereferenced: the checks come first
    f = lib.micloc_doa_peaks_f64
    ok = dict(power=p, B=4, G=449, doa=d, kind=2, K=2, sep=0.1, rel=0.0, index=i, value=v)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["power"], a["B"], a["G"], a["doa"], a["kind"], a["K"], a["sep"], a["rel"], a["index"], a["value"], None)

    for bad in (dict(K=0), dict(K=17), dict(G=4097), dict(G=0), dict(B=0), dict(kind=3), dict(kind=-1), dict(power=None), dict(doa=None),
                dict(index=None), dict(sep=-1.0), dict(sep=float("nan")), dict(rel=-0.5), dict(rel=float("inf"))):
        assert call(**bad) == _lib.MICLOC_ERR_INVALID, bad


# ---- multi_target_sweep on the host ------------------------------------------------------------------------------------------------

def _snn():
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    tau = 1.0 / (2 * np.pi * 2000)
    return SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=48_000)


def _oracle_localizer(beamf, bf_mat, doa_list, K, sep, calls=None, fail_after=None):
    from micloc.snn_beamformer import neuron_impulse_response
    from oracle import oracle as O

    def run(sig_batch, time_vec):
        if calls is not None:
            if fail_after is not None and len(calls) == fail_after:
                raise KeyboardInterrupt("interrupted")
            calls.append(len(sig_batch))
        nir = neuron_impulse_response(time_vec, beamf.tau_vec)
        b, a = beamf.bandpass_filter
        pw, _ = O.snn_chain_batch(sig_batch, beamf.kernel, b, a, beamf.spk_encoder.robust_width, True, nir, bf_mat)
        return R.peaks(pw, doa_list, K, sep)

    return run


def test_sweep_argument_errors():
    from haghighatshoarmuir2024_amd.sweep import multi_target_sweep

    beamf = _snn()
    doa = np.linspace(-np.pi, np.pi, 9)
    W = np.zeros((14, 9))
    with pytest.raises(ValueError, match="pi"):
        multi_target_sweep(beamf, W, doa, num_targets=4, min_separation=np.pi / 4)  # 4 * 45 deg = pi
    with pytest.raises(ValueError, match="pi"):
        multi_target_sweep(beamf, W, doa, num_targets=2, min_separation=-0.1)
    with pytest.raises(ValueError, match="num_targets"):
        multi_target_sweep(beamf, W, doa, num_targets=5, min_separation=0.1)
    with pytest.raises(ValueError, match="num_targets"):
        multi_target_sweep(beamf, W, doa, num_targets=0)
    with pytest.raises(ValueError, match="gains"):
        multi_target_sweep(beamf, W, doa, num_targets=2, gains=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="mode"):
        multi_target_sweep(beamf, W, doa, num_targets=2, mode="fast")
    with pytest.raises(ValueError, match="redraws"):
        multi_target_sweep(beamf, W, doa, num_targets=3, min_separation=1.04, max_redraws=2, localizer=lambda s, t: None)


def test_trial_generator_restated():
    """Draw order, redraws and the host synthesis of the sweep against the restatement (parity mode's building blocks)."""
    from haghighatshoarmuir2024_amd.sweep import _draw_doas, synthesize_targets

    beamf = _snn()
    a, b = np.random.RandomState(11), np.random.RandomState(11)
    for _ in range(40):
        x = _draw_doas(a.rand, 3, np.deg2rad(50), 10_000)
        y = R.draw_doas(b.rand, 3, np.deg2rad(50))
        np.testing.assert_array_equal(x, y)
        assert not R.too_close(x, np.deg2rad(50))
    t = np.arange(0, 20e-3, 1 / 48_000)
    s = np.sin(2 * np.pi * 2000 * t)
    doas, gains = np.array([0.3, 2.5, 4.4]), np.array([1.0, 0.5, 2.0])
    t1, x1 = synthesize_targets(beamf.geometry, 48_000, t, s, doas, gains)
    t2, x2 = R.synth_targets_host(beamf.geometry, 48_000, t, s, doas, gains)
    np.testing.assert_array_equal(t1, t2)
    np.testing.assert_array_equal(x1, x2)
    # one target, gain 1: apply_to_template's noise-free signal
    from haghighatshoarmuir2024_amd.snn_beamformer import synthesize_array_signal

    _, x3 = synthesize_targets(beamf.geometry, 48_000, t, s, doas[:1], [1.0])
    _, x4 = synthesize_array_signal(beamf.geometry, 48_000, t, s, float(doas[0]))
    np.testing.assert_array_equal(x3, x4)


def test_store_key_follows_the_multi_target_arguments(tmp_path):
    from haghighatshoarmuir2024_amd.sweep import multi_target_sweep

    bfz = np.load(os.path.join(ROOT, "tests", "golden", "bf_mat_chirp449_bipolar.npz"))
    W, doa = bfz["bf_mat"], bfz["doa_list"]
    never = lambda s, t: (np.full((len(s), 2), -1), np.full((len(s), 2), np.nan))  # noqa: E731
    base = dict(num_targets=2, min_separation=np.deg2rad(45), snr_db_vec=[0.0], num_sim=2, test_duration=5e-3, out_dir=tmp_path)

    def store_dir(beamf=None, **kw):
        a = dict(base, **kw)
        K = a["num_targets"]
        loc = never if K == 2 else (lambda s, t: (np.full((len(s), K), -1), np.full((len(s), K), np.nan)))
        return multi_target_sweep(beamf or _snn(), W, doa, localizer=loc, **a)["persistence"]["dir"]

    d0 = store_dir()
    assert store_dir() == d0
    other = _snn()
    other.tau_vec = other.tau_vec * 2
    dirs = {d0, store_dir(num_targets=3, min_separation=np.deg2rad(40)), store_dir(min_separation=np.deg2rad(44)),
            store_dir(peak_separation=0.2), store_dir(tol=0.1), store_dir(gains=[1.0, 0.5]), store_dir(rel_threshold=0.1), store_dir(beamf=other)}
    assert len(dirs) == 8
    assert all(os.path.basename(d).startswith("multi-noisy-") for d in dirs)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SWEEP = dict(num_targets=2, min_separation=np.deg2rad(40), snr_db_vec=[0.0, 20.0], num_sim=5, seed=3, mode="parity", batch_trials=2,
             test_duration=20e-3)


def _world2_worker(rank, world, port, out_dir):
    import sys

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    from haghighatshoarmuir2024_amd.sweep import multi_target_sweep

    dist.init_process_group("gloo", rank=rank, world_size=world)
    bfz = np.load(os.path.join(ROOT, "tests", "golden", "bf_mat_chirp449_bipolar.npz"))
    beamf = _snn()
    loc = _oracle_localizer(beamf, bfz["bf_mat"], bfz["doa_list"], 2, SWEEP["min_separation"] / 2)
    res = multi_target_sweep(beamf, bfz["bf_mat"], bfz["doa_list"], rank=rank, world_size=world, localizer=loc, **SWEEP)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **{k: v for k, v in res.items() if isinstance(v, np.ndarray)})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_sweep_world2_and_resume_equal_the_plain_run(tmp_path):
    import torch.multiprocessing as mp

    from haghighatshoarmuir2024_amd.sweep import multi_target_sweep
    from oracle import oracle as O

    O.build()
    bfz = np.load(os.path.join(ROOT, "tests", "golden", "bf_mat_chirp449_bipolar.npz"))
    W, doa = bfz["bf_mat"], bfz["doa_list"]
    beamf = _snn()
    sep = SWEEP["min_separation"] / 2
    ref = multi_target_sweep(beamf, W, doa, localizer=_oracle_localizer(beamf, W, doa, 2, sep), **SWEEP)
    assert ref["peaks"].shape == (2, 5, 2) and ref["err"].shape == (2, 5, 2) and ref["resolved_rate"].shape == (2,)
    # the restated trial generator: the same DoAs from the global stream
    np.random.seed(3)
    M, T = 7, len(np.arange(0, 20e-3 - 1 / 48_000, 1 / 48_000))
    for n in range(10):
        d = R.draw_doas(np.random.rand, 2, SWEEP["min_separation"])
        np.testing.assert_array_equal(ref["doa"].reshape(10, 2)[n], d)
        np.random.randn(T, M)
    # matched errors, MAE and resolution rate from their definitions
    e = np.stack([R.match(ref["doa"].reshape(10, 2)[n], doa, ref["peaks"].reshape(10, 2)[n]) for n in range(10)])
    np.testing.assert_array_equal(ref["err"].reshape(10, 2), e)
    np.testing.assert_array_equal(ref["mae_deg"], np.mean(e.reshape(2, 10), axis=1) * 180 / np.pi)
    ok = np.all((ref["peaks"] >= 0) & (ref["err"] <= sep), axis=2)
    np.testing.assert_array_equal(ref["resolved_rate"], ok.mean(axis=1))

    # gloo world of 2: every rank ends with the single-process result
    mp.spawn(_world2_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("doa", "peaks", "peak_power", "err", "mae_deg", "resolved_rate"):
            np.testing.assert_array_equal(got[key], ref[key], err_msg=f"rank {r} {key}")

    # interrupted after two batches, then resumed from out_dir: the uninterrupted result, only the missing batches recomputed
    store = tmp_path / "store"
    calls = []
    with pytest.raises(KeyboardInterrupt):
        multi_target_sweep(beamf, W, doa, localizer=_oracle_localizer(beamf, W, doa, 2, sep, calls, fail_after=2), out_dir=store, **SWEEP)
    assert calls == [2, 2]
    calls2 = []
    res = multi_target_sweep(beamf, W, doa, localizer=_oracle_localizer(beamf, W, doa, 2, sep, calls2), out_dir=store, **SWEEP)
    assert calls2 == [2, 2, 2] and res["persistence"]["trials_loaded"] == 4
    for key in ("doa", "peaks", "peak_power", "err", "mae_deg", "resolved_rate"):
        np.testing.assert_array_equal(res[key], ref[key], err_msg=key)


@pytest.mark.timeout(600)
def test_one_target_is_the_noisy_sweep():
    """num_targets = 1 in parity mode: noisy_target_sweep's draws, signals, arg-max, power, errors and MAE, bit for bit."""
    from haghighatshoarmuir2024_amd.sweep import multi_target_sweep, noisy_target_sweep
    from micloc.snn_beamformer import neuron_impulse_response
    from oracle import oracle as O

    O.build()
    bfz = np.load(os.path.join(ROOT, "tests", "golden", "bf_mat_chirp449_bipolar.npz"))
    W, doa = bfz["bf_mat"], bfz["doa_list"]
    beamf = _snn()
    seen = {"noisy": [], "multi": []}

    def loc(tag, multi):
        def run(sig_batch, time_vec):
            seen[tag].append(np.array(sig_batch))
            nir = neuron_impulse_response(time_vec, beamf.tau_vec)
            b, a = beamf.bandpass_filter
            pw, am = O.snn_chain_batch(sig_batch, beamf.kernel, b, a, beamf.spk_encoder.robust_width, True, nir, W)
            if multi:
                return R.peaks(pw, doa, 1, np.pi / 8)
            return am.astype(np.int64), pw[np.arange(len(am)), am]

        return run

    kw = dict(snr_db_vec=[-5.0, 5.0, 15.0], num_sim=4, seed=7, batch_trials=3, test_duration=20e-3)
    a = noisy_target_sweep(beamf, W, doa, localizer=loc("noisy", False), **kw)
    b = multi_target_sweep(beamf, W, doa, num_targets=1, localizer=loc("multi", True), **kw)
    for x, y in zip(seen["noisy"], seen["multi"]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(b["doa"][..., 0], a["doa"])
    np.testing.assert_array_equal(b["peaks"][..., 0], a["argmax"])
    np.testing.assert_array_equal(b["peak_power"][..., 0], a["pmax"])
    np.testing.assert_array_equal(b["err"][..., 0], a["err"])
    np.testing.assert_array_equal(b["mae_deg"], a["mae_deg"])


def test_music_store_key_covers_the_music_parameters(tmp_path):
    """Without store_key, the MUSIC object's band, frame duration and grid still reach the key (an injected localizer)."""
    from haghighatshoarmuir2024_amd.sweep import multi_target_sweep
    from micloc.array_geometry import CenterCircularArray
    from micloc.music_beamformer import MUSIC

    doa = np.linspace(-np.pi, np.pi, 57)
    never = lambda s, t: (np.full((len(s), 2), -1), np.full((len(s), 2), np.nan))  # noqa: E731

    def store_dir(**kw):
        a = dict(geometry=CenterCircularArray(4.5e-2, 7), freq_range=[1600.0, 2400.0], doa_list=doa, frame_duration=1.0, fs=48_000)
        a.update(kw)
        m = MUSIC(**a)
        return multi_target_sweep(m, None, doa, localizer=never, snr_db_vec=[0.0], num_sim=2, test_duration=5e-3, out_dir=tmp_path)["persistence"]["dir"]

    d0 = store_dir()
    assert store_dir() == d0
    assert len({d0, store_dir(freq_range=[1500.0, 2400.0]), store_dir(frame_duration=0.5)}) == 3
