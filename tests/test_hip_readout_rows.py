"""The read-out rules of csrc/readout_rows.h on the MI355X, with the ties where the reductions can go wrong.  The random campaigns of the
other test files meet two equal maxima only by luck; here a beamforming matrix that is zero except for two identical columns gives
exactly two DoA columns the same positive power (or envelope), placed in one thread on two passes, in two threads with the winner in the
higher one, in neighbours, in two lanes and in one lane of a wave.  Expected values are np.argmax restated below -- the first maximum, a
NaN never wins, a row without a number gives 0 -- on the power or envelope rows the read-out kernel itself was given, never another
arg-max entry of the library; the streams must return the one-shot call's bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 48_000
PAIRS = [(5, 261), (297, 300), (40, 41)]  # one thread on two passes of 256 columns; two threads, the winner in the higher; neighbours


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def first_max(rows):
    """np.argmax over the last axis with NaN as "never wins"; a row without a number gives 0."""
    rows = np.asarray(rows, dtype=np.float64)
    idx = np.argmax(np.where(np.isnan(rows), -np.inf, rows), axis=-1)
    return np.where(np.all(np.isnan(rows), axis=-1), 0, idx).astype(np.int32)


def two_columns(C, G, pair, seed=0):
    """bf_mat [C, G]: zero except for the two columns of `pair`, which hold the same vector."""
    W = np.zeros((C, G))
    v = np.random.RandomState(seed).randn(C)
    W[:, pair[0]] = W[:, pair[1]] = v / np.linalg.norm(v)
    return W


def _plan(cfg2, M=7):
    from haghighatshoarmuir2024_amd.runtime import Plan

    p = Plan(M, cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True)
    p.set_neuron_kernel(cfg2["nir"])
    return p


def _raster(B, T, C, seed):
    rng = np.random.RandomState(seed)
    return (np.where(rng.rand(B, T, C) < 0.08, 1, 0) * rng.choice([-1, 1], size=(B, T, C))).astype(np.int8)


def _tied(power, pair):
    """The precondition: the two columns carry the same positive number and every other column is below it."""
    a, b = power[..., pair[0]], power[..., pair[1]]
    rest = np.delete(power, pair, axis=-1)
    return np.array_equal(a, b) and (a > 0).all() and (rest.size == 0 or (rest.max(axis=-1) < a).all())


# ---- the windowed SNN read-out (window_power_kernel) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
def test_windowed_power_gives_the_lower_of_two_equal_columns(cfg2, torch, pair):
    B, G, CH = 2, 360, 256
    T = 2 * CH + 100  # three chunks, the last one ragged: three windows
    p = _plan(cfg2)
    p.set_bf_mat(two_columns(14, G, pair))
    assert p.window_quantum() == CH
    out = p.lif_beamform(torch.from_numpy(_raster(B, T, 14, 7)).cuda(), window=CH, hop=CH)
    pw, am = out["window_power"].cpu().numpy(), out["window_argmax"].cpu().numpy()
    assert pw.shape == (B, 3, G) and _tied(pw, pair)
    np.testing.assert_array_equal(am, first_max(pw))
    assert (am == pair[0]).all()
    assert _tied(out["power"].cpu().numpy(), pair) and (out["argmax"].cpu().numpy() == pair[0]).all()


def test_all_zero_raster_ties_every_column_and_gives_zero(cfg2, torch):
    B, G, CH = 2, 360, 256
    T = 2 * CH + 100
    p = _plan(cfg2)
    p.set_bf_mat(two_columns(14, G, PAIRS[0]))
    out = p.lif_beamform(torch.zeros((B, T, 14), dtype=torch.int8, device="cuda"), window=CH, hop=CH)
    assert tuple(out["window_argmax"].shape) == (B, 3)
    assert not out["window_power"].cpu().numpy().any() and not out["window_argmax"].cpu().numpy().any()


def test_long_window_form_gives_the_lower_of_two_equal_columns(cfg2, torch):
    """One window of 129 chunks: window_power_kernel<4>, where only the first 256 of 1024 threads hold a pair."""
    G, CH, pair = 5, 256, (1, 3)
    T = 128 * CH + 1
    p = _plan(cfg2)
    p.set_bf_mat(two_columns(14, G, pair))
    out = p.lif_beamform(torch.from_numpy(_raster(1, T, 14, 9)).cuda(), window=129 * CH, hop=129 * CH)
    pw, am = out["window_power"].cpu().numpy(), out["window_argmax"].cpu().numpy()
    assert pw.shape == (1, 1, G) and _tied(pw, pair)
    np.testing.assert_array_equal(am, first_max(pw))
    assert am[0, 0] == pair[0]
    np.testing.assert_array_equal(pw[:, 0], out["power"].cpu().numpy())  # a single window >= T: the unwindowed bits


# ---- the streams -----------------------------------------------------------------------------------------------------------------------
def _wrap(x, L2):
    w = np.roll(x, L2, axis=1)[:, :L2, :]
    return np.concatenate([w, np.zeros((x.shape[0], L2 - w.shape[1], x.shape[2]))], axis=1) if w.shape[1] < L2 else w


@pytest.mark.parametrize("pair", PAIRS)
def test_streamed_windows_equal_the_one_shot_rows_on_tied_columns(torch, pair):
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    from haghighatshoarmuir2024_amd.streaming import StreamingLocalizer

    tau = 1 / (2 * np.pi * 2000)
    bf = SNNBeamformer(CenterCircularArray(4.5e-2, 7), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=FS)
    B, G, CH = 2, 360, 256
    T = 2 * CH + 100
    W = two_columns(14, G, pair)
    x = np.random.RandomState(11).randn(B, T, 7)
    one = bf.localize_batch(W, x, window=CH, hop=CH)
    pw, am = one["window_power"].cpu().numpy(), one["window_argmax"].cpu().numpy()
    assert pw.shape == (B, 3, G) and _tied(pw, pair)
    np.testing.assert_array_equal(am, first_max(pw))
    assert (am == pair[0]).all()
    cut = 304  # inside window 1
    s = StreamingLocalizer(bf, W, B, T, wrap_tail=_wrap(x, len(bf.kernel) // 2), max_tile=max(cut, T - cut), window=CH, hop=CH)
    s.push(x[:, :cut, :], final=False)
    s.push(x[:, cut:, :], final=True)
    out = s.finish()
    assert out["window_count"] == 3
    np.testing.assert_array_equal(out["window_power"].cpu().numpy(), pw)
    np.testing.assert_array_equal(out["window_argmax"].cpu().numpy(), am)
    np.testing.assert_array_equal(out["power"].cpu().numpy(), one["power"].cpu().numpy())
    np.testing.assert_array_equal(out["argmax"].cpu().numpy(), one["argmax"].cpu().numpy())
    assert (out["argmax"].cpu().numpy() == pair[0]).all()


def test_complex_stream_on_zero_input_equals_the_one_shot_rows(torch):
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer

    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

    M, B, G = 4, 2, 300
    bf = Beamformer(CenterCircularArray(4.5e-2, M), 10e-3, [1000.0, 2000.0], fs=FS)
    rng = np.random.RandomState(12)
    W = rng.randn(M, G) + 1j * rng.randn(M, G)
    bf.plan().set_bf_mat(W)
    CH = bf.plan().window_quantum()
    T = 2 * CH + 100
    x = np.zeros((B, T, M))
    one = bf.localize_batch(W, x, window=CH, hop=CH)
    pw, am = one["window_power"].cpu().numpy(), one["window_argmax"].cpu().numpy()
    assert pw.shape == (B, 3, G) and not pw.any() and not am.any()  # every column ties at 0
    cut = CH + 100  # inside window 1
    loc = bf.streaming_localizer(W, batch=B, total_frames=T, wrap_tail=ComplexStreamingLocalizer.wrap_rows(x, len(bf.kernel)),
                                 max_tile=max(cut, T - cut), window=CH, hop=CH)
    loc.push(x[:, :cut, :])
    loc.push(x[:, cut:, :])
    out = loc.finish()
    assert out["window_count"] == 3
    assert torch.equal(out["window_power"], one["window_power"]) and torch.equal(out["window_argmax"], one["window_argmax"])
    assert torch.equal(out["power"], one["power"]) and torch.equal(out["argmax"], one["argmax"]) and not out["argmax"].cpu().numpy().any()


# ---- the covariance route (cov_power_kernel) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
def test_covariance_route_gives_the_lower_of_two_equal_columns(cfg2, torch, pair):
    B, T, G = 2, 612, 360
    p = _plan(cfg2)
    p.set_bf_mat(two_columns(14, G, pair))
    x = np.random.RandomState(13).randn(B, T, 7)
    out = p.snn_pipeline_cov(p.to_device(x), want_power=True)
    power, am = out["power"].cpu().numpy(), out["argmax"].cpu().numpy()
    assert _tied(power, pair)
    np.testing.assert_array_equal(am, first_max(power))
    assert (am == pair[0]).all()


# ---- the row read-outs (rows_argmax_kernel, track_rows_kernel) ---------------------------------------------------------------------------
def _row_pairs(G):
    """(adjacent columns: different lanes; columns 64 apart: the same lane of the wave), where the row is wide enough."""
    return [pr for pr in ((G - 2, G - 1), (G - 65, G - 1)) if pr[0] >= 0]


@pytest.mark.parametrize("G", [1, 63, 64, 65, 130])
def test_envelope_rows_give_the_first_of_two_equal_maxima(torch, G):
    from haghighatshoarmuir2024_amd import runtime

    T = 6
    s = 1.0 + np.random.RandomState(G).rand(T)
    trials = []
    for pr in _row_pairs(G):
        y = np.outer(s, np.full(G, 0.25))  # every other column: a quarter of the series, so a quarter of the envelope
        y[:, pr[0]] = y[:, pr[1]] = s
        trials.append(y)
    trials.append(np.outer(s, np.ones(G)))  # every column ties
    trials.append(np.full((T, G), np.nan))  # rows without a number
    env, idx = runtime.envelope_track(torch.from_numpy(np.stack(trials)).cuda(), 3, 2)
    env, idx = env.cpu().numpy(), idx.cpu().numpy()
    np.testing.assert_array_equal(idx, first_max(env))
    for b, pr in enumerate(_row_pairs(G)):
        assert _tied(env[b], pr) and (idx[b] == pr[0]).all(), pr
    assert np.isnan(env[-1]).all() and not idx[-2:].any()


@pytest.mark.parametrize("G", [1, 63, 64, 65, 130])
def test_two_step_track_rows_give_the_first_of_two_equal_maxima(cfg2, torch, G):
    from haghighatshoarmuir2024_amd import runtime

    M, T = 20, 150  # forty channels: no fused kernel serves the plan, Plan.track takes the two-step route (track_rows_kernel)
    p = _plan(cfg2, M)
    spikes = torch.from_numpy(_raster(2, T, 2 * M, 15)).cuda()
    for pr in _row_pairs(G) or [(0, 0)]:
        p.set_bf_mat(two_columns(2 * M, G, pr, seed=G))
        assert not p.track_is_fused()
        out = p.track(spikes, 5, 3, kind="spikes")
        idx, peak = out["index"].cpu().numpy(), out["peak_envelope"].cpu().numpy()
        env, _ = runtime.envelope_track(p.lif_beamform(spikes, want_y=True, want_power=False)["y"], 5, 3, want_index=False)
        env = env.cpu().numpy()
        np.testing.assert_array_equal(env[..., pr[0]], env[..., pr[1]])
        np.testing.assert_array_equal(idx, first_max(env))
        np.testing.assert_array_equal(peak, env.max(axis=-1))
        live = peak > 0
        assert live.any() and (idx[live] == pr[0]).all() and not idx[~live].any()
    # a matrix of NaN: every row is without a number -> index 0, peak NaN
    p.set_bf_mat(np.full((2 * M, G), np.nan))
    out = p.track(spikes, 5, 3, kind="spikes")
    assert not out["index"].cpu().numpy().any() and np.isnan(out["peak_envelope"].cpu().numpy()).all()


# ---- the Xylo stream (sx_peak on integer counts) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("win_size", [1, 5])
def test_xylo_stream_on_a_silent_recording_ties_every_count(torch, win_size):
    """(The stream takes odd box-cars only and refuses win_size = 4; 5 has the same win_size // 2 = 2, so the same expected peak G - 2.)"""
    from micloc.array_geometry import CenterCircularArray

    from haghighatshoarmuir2024_amd.xylo_snn_localization import Demo, xylo_specification

    G = 33
    demo = Demo(CenterCircularArray(0.045, 7), [[1000, 2000]], doa_list=np.linspace(-np.pi, np.pi, G), recording_duration=0.05)
    demo.spec = xylo_specification(demo.bf_mats, demo.tau_vecs, demo.fs, 1e-3, demo.bipolar_spikes, w_rec_coef=0.0)  # (a stream has no recurrent weight)
    T, CH = 700, 256
    x = np.zeros((2, T, 7))
    L2 = len(demo.beamfs[0].kernel) // 2
    kw = dict(total_frames=T, wrap_tail=x[:, T - L2 :, :], max_tile=400, lag_frames=2048, window=CH, hop=CH)
    with pytest.raises(ValueError, match="win_size"):
        demo.streaming_localizer(2, win_size=4, **kw)
    s = demo.streaming_localizer(2, win_size=win_size, **kw)
    s.push(x[:, :400, :])
    s.push(x[:, 400:, :])
    out = s.finish()
    want = (0 - win_size // 2) % G  # all counts tie at 0: the first maximum of the box-car sums is sample 0
    assert not out["counts"].cpu().numpy().any() and not out["window_counts"].cpu().numpy().any()
    assert out["window_count"] == 3
    assert (out["peak"].cpu().numpy() == want).all() and (out["window_peak"].cpu().numpy() == want).all()
