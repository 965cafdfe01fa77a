"""Wideband moving-target tracking on the device (csrc/track.hip: track_bands_ws_kernel / track_bands_wsc_kernel; the rule: include/micloc_hip.h,
"wideband moving-target tracking").  Every comparison is bit for bit -- there is no tolerance in this file:
  1. one band: WidebandLocalizer.track_batch = the single-plan track_batch on the filterbank's output;
  2. two and three bands against the two-step rule, built from the device's own per-band y (the existing calls that store it), the band
     sum in NumPy in band order, oracle.envelope and np.argmax.  The complex bands run the whole call from x.  The SNN bands run the
     read-out on seeded random rasters at every shape: an encoder fed 2 or 63 frames emits no spike, and a sum of zeros checks nothing;
     from x they run where the encoder does spike (T = 209, 1001);
  3. the stage entries at every channel count the kernels treat differently;
  4. sets the fused kernels do not serve (20 microphones): the two-step route inside the call, with the minimum workspace, that of two
     trials out of three, and ten times the minimum;
  5. the footprint, from the size function, and the measured rise of the peak allocation across a call;
  6. graph capture; 7. the sweep; and the refusals that compare plans, in front of any launch.
Both routes take the first maximum by one rule, so the two-step reference is exact in every case and no case is skipped for ties."""
import ctypes
import warnings

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FS = 48_000
BANDS = [[1000.0, 1600.0], [1600.0, 2400.0], [2400.0, 3400.0]]
WF, WR = 624, 96  # envelope windows (frames): int(fs * 13 ms), int(fs * 2 ms)
KERNEL_AXIS = np.arange(4800) / FS  # the time axis the stage tests build the neuron kernels on: every band's kernel has all its taps


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _env():
    from haghighatshoarmuir2024_amd.utils import Envelope

    return Envelope(rise_time=2e-3, fall_time=13e-3, fs=FS)


def _loc(kind, F, G, M=7, seed=0):
    """A wideband localizer of F bands with seeded random matrices; the SNN bands have tau = 1 / (2 pi f_mid): NK differs band by band."""
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.beamformer import Beamformer
    from haghighatshoarmuir2024_amd.filterbank import ButterworthFilterbank
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer
    from haghighatshoarmuir2024_amd.wideband import WidebandBeamformerLocalizer, WidebandSNNLocalizer

    geo = CenterCircularArray(4.5e-2, M)
    bands = BANDS[:F]
    rng = np.random.RandomState(1000 * F + G + 17 * M + seed)
    if kind == "snn":
        beamfs = [SNNBeamformer(geo, 10e-3, fr, np.asarray([1 / (2 * np.pi * np.mean(fr))] * 2), bipolar_spikes=True, fs=FS) for fr in bands]
        Ws = []
        for _ in bands:
            W = rng.randn(2 * M, G)
            Ws.append(W / np.linalg.norm(W, axis=0, keepdims=True))
        loc = WidebandSNNLocalizer(beamfs, Ws, ButterworthFilterbank(freq_bands=np.asarray(bands), order=1, fs=FS))
    else:
        beamfs = [Beamformer(geo, 10e-3, fr, fs=FS) for fr in bands]
        Ws = [(rng.randn(M, G) + 1j * rng.randn(M, G)) / np.sqrt(2 * M) for _ in bands]
        loc = WidebandBeamformerLocalizer(beamfs, Ws, ButterworthFilterbank(freq_bands=np.asarray(bands), order=2, fs=FS))
    loc.doa_list = np.linspace(-np.pi, np.pi, G)
    return loc


def _plans(loc, time_vec=KERNEL_AXIS):
    return loc.plans(time_vec) if hasattr(loc.beamfs[0], "tau_vec") else loc.plans()


def _signal(rng, B, T, M):
    """B trials [T, M]: a tone inside every band plus noise, each microphone with its own phase."""
    t = np.arange(T) / FS
    x = 0.5 * rng.randn(B, T, M)
    for fr in BANDS:
        x += np.sin(2 * np.pi * np.mean(fr) * t[None, :, None] + rng.uniform(0, 2 * np.pi, size=(B, 1, M)))
    return x


def _magnitudes(torch, y):
    """|y| of a device tensor [B, T, G] as the rule names it: fabs, or the device library's hypot -- the envelope kernel's own magnitude of
    every value taken as a one-frame trial (Envelope state_0 = |y_0|)."""
    from haghighatshoarmuir2024_amd import runtime

    if not y.is_complex():
        return np.abs(y.cpu().numpy())
    B, T, G = y.shape
    return runtime.envelope_track(y.reshape(B * T, 1, G).contiguous(), 1, 1, want_index=False)[0].reshape(B, T, G).cpu().numpy()


def _reference(mags):
    """The two-step rule on the bands' magnitudes [F][B, T, G] -> (index [B, T], peak [B, T], last [B, G]); asserts the sum is not vacuous."""
    assert sum(bool(np.any(m != 0)) for m in mags) >= min(2, len(mags)), "fewer than two bands contribute a nonzero magnitude"
    m = mags[0].copy()
    for a in mags[1:]:
        m = m + a  # one IEEE addition per band, ascending
    idx, peak, last = [], [], []
    for b in range(m.shape[0]):
        e = O.envelope(m[b], WF, WR)
        idx.append(np.argmax(e, axis=1))
        peak.append(e.max(axis=1))
        last.append(e[-1])
    return np.asarray(idx), np.asarray(peak), np.asarray(last)


def _assert_equal(out, want, tag):
    idx, peak, last = want
    got = out["index"].cpu().numpy()
    assert got.dtype == np.int32 and got.shape == idx.shape, tag
    np.testing.assert_array_equal(got, idx, err_msg=f"index {tag}")
    np.testing.assert_array_equal(out["peak_envelope"].cpu().numpy(), peak, err_msg=f"peak {tag}")
    np.testing.assert_array_equal(out["envelope_last"].cpu().numpy(), last, err_msg=f"last {tag}")


def _rasters(torch, rng, F, B, T, C):
    u = rng.rand(F, B, T, C)
    return torch.from_numpy(((u < 0.1).astype(np.int8) - (u > 0.9).astype(np.int8))).cuda()


def _snn_stage_case(torch, plans, rng, B, T, tag):
    from haghighatshoarmuir2024_amd import runtime

    F, C = len(plans), plans[0].C
    spk = _rasters(torch, rng, F, B, T, C)
    mags = [_magnitudes(torch, plans[f].lif_beamform(spk[f], want_y=True, want_power=False)["y"]) for f in range(F)]
    out = runtime.snn_bands_track(plans, None, spk, WF, WR, kind="spikes", want_envelope_last=True)
    _assert_equal(out, _reference(mags), tag)


def _complex_stage_case(torch, plans, rng, B, T, tag):
    from haghighatshoarmuir2024_amd import runtime

    F, C = len(plans), plans[0].C
    Ts = plans[0].padded_T(T)
    pre = torch.from_numpy(rng.randn(F * B, C, Ts)).cuda()
    mags = [_magnitudes(torch, plans[f].beamform_c128(pre[f * B : (f + 1) * B], T, want_y=True, want_power=False)["y"]) for f in range(F)]
    out = runtime.beamformer_bands_track(plans, None, pre, WF, WR, kind="planar", T=T, want_envelope_last=True)
    _assert_equal(out, _reference(mags), tag)


def _pipeline_reference(torch, loc, x, time_vec=None):
    """The bands' magnitudes of x [B, T, M] by the calls a user has today: the filterbank, then every band's own pipeline with y stored."""
    from haghighatshoarmuir2024_amd import runtime

    snn = hasattr(loc.beamfs[0], "tau_vec")
    T = x.shape[1]
    plans = _plans(loc, np.arange(T) / FS if time_vec is None else time_vec)
    xd = plans[0].to_device(x)
    xf = runtime.filterbank(loc.filterbank.ba_list, xd)
    mags = []
    for f, p in enumerate(plans):
        y = (p.snn_pipeline(xf[f], want_y=True, want_power=False) if snn else p.beamformer_pipeline(xf[f], want_y=True, want_power=False))["y"]
        mags.append(_magnitudes(torch, y))
    return mags


# ---- 1. one band: the single-plan tracking entry on the filterbank's output ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["snn", "complex"])
def test_one_band_equals_the_single_plan_track_batch(torch, kind):
    from haghighatshoarmuir2024_amd import runtime

    loc = _loc(kind, 1, 65)
    rng = np.random.RandomState(11)
    for T in (209, 1001):
        x = _signal(rng, 2, T, 7)
        got = loc.track_batch(x, _env(), want_envelope_last=True)
        xf = runtime.filterbank(loc.filterbank.ba_list, torch.from_numpy(x).cuda())[0]
        want = loc.beamfs[0].track_batch(loc.bf_mats[0], xf, _env(), want_envelope_last=True)
        for k in ("index", "peak_envelope", "envelope_last"):
            assert torch.equal(got[k], want[k]), (kind, T, k)
        assert got["index"].dtype == torch.int32 and tuple(got["index"].shape) == (2, T)
    assert runtime.bands_track_is_fused(_plans(loc, np.arange(T) / FS), kind == "complex")


# ---- 2. two and three bands against the two-step rule ------------------------------------------------------------------------------------
SHAPES_T = (2, 63, 64, 65, 209, 1001)


@pytest.mark.parametrize("G", [33, 64, 65, 130, 449])
def test_snn_bands_equal_the_two_step_rule(torch, G):
    from haghighatshoarmuir2024_amd import runtime

    for F in (2, 3):
        loc = _loc("snn", F, G)
        plans = _plans(loc)
        assert runtime.bands_track_is_fused(plans)
        rng = np.random.RandomState(100 * G + F)
        for T in SHAPES_T:
            for B in (1, 3):
                _snn_stage_case(torch, plans, rng, B, T, f"snn rasters F={F} G={G} T={T} B={B}")
        for T in (209, 1001):  # the whole call from x, where the encoder spikes
            x = _signal(rng, 3, T, 7)
            out = loc.track_batch(x, _env(), want_envelope_last=True)
            _assert_equal(out, _reference(_pipeline_reference(torch, loc, x)), f"snn pipeline F={F} G={G} T={T}")


def test_snn_bands_have_different_neuron_kernel_lengths(torch):
    from haghighatshoarmuir2024_amd.snn_beamformer import neuron_impulse_response

    loc = _loc("snn", 3, 33)
    nk = [(len(neuron_impulse_response(KERNEL_AXIS, b.tau_vec)) + 15 + 3) // 4 for b in loc.beamfs]
    assert len(set(nk)) == 3, nk  # the LDS regions of the band kernel are sized for the largest, every band stages its own


@pytest.mark.parametrize("G", [33, 64, 65, 130, 449])
def test_complex_bands_equal_the_two_step_rule(torch, G):
    from haghighatshoarmuir2024_amd import runtime

    for F in (2, 3):
        loc = _loc("complex", F, G)
        assert runtime.bands_track_is_fused(loc.plans(), True)
        rng = np.random.RandomState(200 * G + F)
        for T in SHAPES_T:
            for B in (1, 3):
                x = _signal(rng, B, T, 7)
                out = loc.track_batch(x, _env(), want_envelope_last=True)
                _assert_equal(out, _reference(_pipeline_reference(torch, loc, x)), f"complex F={F} G={G} T={T} B={B}")


# ---- 3. the stage entries on chosen inputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 7, 8])
def test_snn_stage_entry_at_every_channel_count(torch, M):
    """2, 10, 14 and 16 channels (at 16 the channel padding of the spike tile vanishes); G = 65 is two column groups, the second of one
    column; 15 frames are less than a tile, 130 two chunks and a ragged one."""
    for F in (2, 3):
        plans = _plans(_loc("snn", F, 65, M=M))
        rng = np.random.RandomState(300 + 10 * M + F)
        for T in (15, 130):
            _snn_stage_case(torch, plans, rng, 2, T, f"snn stage M={M} F={F} T={T}")


@pytest.mark.parametrize("M", range(1, 9))
def test_complex_stage_entry_at_every_row_of_the_channel_table(torch, M):
    plans = _loc("complex", 2, 65, M=M).plans()
    rng = np.random.RandomState(400 + M)
    for T in (15, 130):
        _complex_stage_case(torch, plans, rng, 2, T, f"complex stage M={M} T={T}")


# ---- 4. the two-step route inside the call ---------------------------------------------------------------------------------------------
def _call_pipeline(torch, name, plans, ba_list, x, nbytes, want_rc=0):
    """The pipeline entry itself with a workspace of exactly nbytes."""
    from haghighatshoarmuir2024_amd import _lib, runtime

    lib = _lib.load()
    F, handles = runtime._band_handles(plans)
    bb, aa, n = runtime.pad_ba_list(ba_list)
    B, T, _ = x.shape
    G = plans[0].G
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=x.device)
    out = dict(index=torch.empty((B, T), dtype=torch.int32, device=x.device), peak_envelope=torch.empty((B, T), dtype=torch.float64, device=x.device),
               envelope_last=torch.empty((B, G), dtype=torch.float64, device=x.device))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    rc = getattr(lib, f"micloc_{name}_pipeline_bands_track_f64")(
        handles, F, dp(bb), dp(aa), n, x.data_ptr(), B, T, 1 - 1 / WR, 1 / WR, 1 - 1 / WF, out["index"].data_ptr(), out["peak_envelope"].data_ptr(),
        out["envelope_last"].data_ptr(), ws.data_ptr(), int(nbytes), torch.cuda.current_stream().cuda_stream)
    assert rc == want_rc, rc
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", ["snn", "complex"])
def test_twenty_microphones_take_the_two_step_route_inside_the_call(torch, kind):
    from haghighatshoarmuir2024_amd import _lib, runtime

    loc = _loc(kind, 2, 97, M=20)
    B, T = 3, 300
    x = _signal(np.random.RandomState(5), B, T, 20)
    plans = _plans(loc, np.arange(T) / FS)
    name = "snn" if kind == "snn" else "beamformer"
    F, handles = runtime._band_handles(plans)
    assert getattr(_lib.load(), f"micloc_{name}_bands_track_is_fused")(handles, F) == 0
    want = _reference(_pipeline_reference(torch, loc, x))
    _assert_equal(loc.track_batch(x, _env(), want_envelope_last=True), want, f"{kind} M=20")
    need = getattr(_lib.load(), f"micloc_{name}_bands_track_workspace_bytes")(handles, F, B, T)
    assert need > 0
    xd = plans[0].to_device(x)
    al = lambda v: (v + 255) // 256 * 256  # noqa: E731
    # one trial of the two-step route: y (complex: two cells of T x G doubles in one aligned block), the band sum, its envelope
    per_trial = al((16 if kind == "complex" else 8) * T * 97) + 2 * al(8 * T * 97)
    for nbytes in (need, need + per_trial, 10 * need):  # one trial per sub-batch; two, then one; all three at once
        _assert_equal(_call_pipeline(torch, name, plans, loc.filterbank.ba_list, xd, nbytes), want, f"{kind} M=20 ws={nbytes}")
    _call_pipeline(torch, name, plans, loc.filterbank.ba_list, xd, need - 256, want_rc=_lib.MICLOC_ERR_WORKSPACE)


# ---- 5. the footprint --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["snn", "complex"])
def test_fused_workspace_depends_on_the_grid_through_the_pairs_alone(torch, kind):
    from haghighatshoarmuir2024_amd import _lib, runtime

    lib = _lib.load()
    F, B, T = 3, 2, 24_000
    name = "snn" if kind == "snn" else "beamformer"
    size = {}
    for G in (64, 449):
        loc = _loc(kind, F, G)
        plans = _plans(loc)
        _, handles = runtime._band_handles(plans)
        assert getattr(lib, f"micloc_{name}_bands_track_is_fused")(handles, F) == 1
        size[G] = getattr(lib, f"micloc_{name}_bands_track_workspace_bytes")(handles, F, B, T)
        assert size[G] > 0
    assert 0 < size[449] - size[64] <= 12 * B * T * -(-449 // 64) + 4096, size
    # measured: the rise of the peak allocation across the call (workspace + results; inputs and plans exist before)
    x = plans[0].to_device(_signal(np.random.RandomState(6), B, T, 7))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = loc.track_batch(x, _env(), want_envelope_last=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"{kind}: workspace {size[449]} B at G = 449, {size[64]} B at G = 64; peak allocation rose by {rise} B; one trial's y is {8 * T * 449} B")
    assert tuple(out["index"].shape) == (B, T)


# ---- 6. graph capture --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["snn", "complex"])
def test_captured_call_replays_to_the_same_bits(torch, kind):
    from haghighatshoarmuir2024_amd import runtime

    loc = _loc(kind, 3, 130)
    B, T = 2, 1001
    rng = np.random.RandomState(7)
    xa, xb = _signal(rng, B, T, 7), _signal(rng, B, T, 7)
    plans = _plans(loc, np.arange(T) / FS)
    fn = runtime.snn_bands_track if kind == "snn" else runtime.beamformer_bands_track
    call = lambda x: fn(plans, loc.filterbank.ba_list, x, WF, WR, want_envelope_last=True)  # noqa: E731
    eager = {k: v.clone() for k, v in call(plans[0].to_device(xb)).items()}
    static_x = plans[0].to_device(xa)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(static_x)  # warm-up: the workspace is allocated here
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(static_x)
    static_x.copy_(torch.from_numpy(xb).cuda())
    g.replay()
    torch.cuda.synchronize()
    for k in ("index", "peak_envelope", "envelope_last"):
        assert torch.equal(out[k], eager[k]), (kind, k)


# ---- 7. the sweep ------------------------------------------------------------------------------------------------------------------------
def _composed_localizer(torch, loc, env):
    """What a user composes today: per band the pipeline with y stored, the device sum of the magnitudes, Envelope.track."""
    from haghighatshoarmuir2024_amd import runtime

    snn = hasattr(loc.beamfs[0], "tau_vec")

    def run(sig_batch, time_vec):
        plans = loc.plans(time_vec) if snn else loc.plans()
        x = plans[0].to_device(sig_batch)
        B, T, _ = x.shape
        xf = runtime.filterbank(loc.filterbank.ba_list, x)
        m = None
        for f, p in enumerate(plans):
            y = (p.snn_pipeline(xf[f], want_y=True, want_power=False) if snn else p.beamformer_pipeline(xf[f], want_y=True, want_power=False))["y"]
            a = y.abs() if snn else runtime.envelope_track(y.reshape(B * T, 1, -1).contiguous(), 1, 1, want_index=False)[0].reshape(B, T, -1)
            m = a.clone() if m is None else m + a
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return env.track(m)

    return run


@pytest.mark.parametrize("mode", ["parity", "throughput"])
@pytest.mark.parametrize("kind", ["snn", "complex"])
def test_sweep_equals_the_sweep_over_the_two_step_composition(torch, tmp_path, kind, mode):
    from haghighatshoarmuir2024_amd.sweep import wideband_moving_target_sweep

    loc, env = _loc(kind, 3, 65), _env()
    kw = dict(snr_db_vec=[0.0, 10.0], num_sim=2, seed=3, mode=mode, test_duration=50e-3, batch_trials=4)  # 4 trials of 2399 frames
    fused = wideband_moving_target_sweep(loc, env, out_dir=tmp_path, **kw)
    composed = wideband_moving_target_sweep(loc, env, localizer=_composed_localizer(torch, loc, env), store_key=dict(localizer="composed"), **kw)
    resumed = wideband_moving_target_sweep(loc, env, out_dir=tmp_path, **kw)
    assert resumed["persistence"]["trials_loaded"] == 4
    assert fused["err"].shape == (2, 2) and np.all(np.isfinite(fused["err"]))
    for k in ("phase", "err", "med", "track_mae_deg", "track_median_deg"):
        np.testing.assert_array_equal(fused[k], composed[k], err_msg=f"{kind} {mode} {k}")
        np.testing.assert_array_equal(resumed[k], fused[k], err_msg=f"{kind} {mode} resumed {k}")


# ---- the refusals that compare plans: status codes in front of any launch ------------------------------------------------------------------
def test_refusals_that_compare_plans(torch):
    from haghighatshoarmuir2024_amd import _lib, runtime

    lib = _lib.load()
    SHAPE, NOT_SET, WS = _lib.MICLOC_ERR_SHAPE, _lib.MICLOC_ERR_NOT_SET, _lib.MICLOC_ERR_WORKSPACE
    snn, cpx = _plans(_loc("snn", 2, 33)), _loc("complex", 2, 33).plans()
    other_g, other_m = _plans(_loc("snn", 1, 65)), _plans(_loc("snn", 1, 33, M=5))
    bare_snn = _loc("snn", 1, 33, seed=9).beamfs[0].new_plan()   # neither neuron kernel nor bf_mat
    bare_cpx = _loc("complex", 1, 33, seed=9).beamfs[0].new_plan()
    no_kernel = _loc("snn", 1, 33, seed=8).beamfs[0].new_plan()
    no_kernel.set_bf_mat(np.random.RandomState(0).randn(14, 33))

    def handles(*plans):
        return (ctypes.c_void_p * len(plans))(*[p.handle.value for p in plans])

    ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")  # the input of either kind: 2 bands x 1 trial x 10 frames
    idx = torch.empty(10, dtype=torch.int32, device="cuda")
    c = (0.9, 0.1, 0.99)
    st = torch.cuda.current_stream().cuda_stream

    def stage(name, hs, F, wsp=None, nbytes=1 << 24, Ts=16):
        wsp = ws.data_ptr() if wsp is None else wsp
        if name == "snn":
            return lib.micloc_lif_beamform_bands_track_f64(hs, F, buf.data_ptr(), 1, 10, *c, idx.data_ptr(), None, None, wsp, nbytes, st)
        return lib.micloc_beamform_c128_bands_track_f64(hs, F, buf.data_ptr(), 1, 10, Ts, *c, idx.data_ptr(), None, None, wsp, nbytes, st)

    cases = [("snn", handles(snn[0], other_g[0]), SHAPE), ("snn", handles(snn[0], other_m[0]), SHAPE), ("snn", handles(snn[0], cpx[0]), SHAPE),
             ("beamformer", handles(cpx[0], snn[0]), SHAPE), ("snn", handles(snn[0], bare_snn), NOT_SET), ("snn", handles(snn[0], no_kernel), NOT_SET),
             ("beamformer", handles(cpx[0], bare_cpx), NOT_SET)]
    for name, hs, want in cases:
        assert stage(name, hs, 2) == want, (name, want)
        assert getattr(lib, f"micloc_{name}_bands_track_workspace_bytes")(hs, 2, 1, 10) == 0
        assert getattr(lib, f"micloc_{name}_bands_track_is_fused")(hs, 2) == want
    good_snn, good_cpx = handles(*snn), handles(*cpx)
    need = lib.micloc_snn_bands_track_workspace_bytes(good_snn, 2, 1, 10)
    assert need > 0 and stage("snn", good_snn, 2, nbytes=need - 1) == WS and stage("snn", good_snn, 2, wsp=ws.data_ptr() + 8) == WS
    assert stage("snn", good_snn, 2, wsp=0) == WS
    assert stage("beamformer", good_cpx, 2, Ts=24) == SHAPE  # Ts is not micloc_padded_T(10)
    assert stage("snn", good_snn, 2) == 0 and stage("beamformer", good_cpx, 2) == 0  # the same arguments, accepted
    torch.cuda.synchronize()
    assert runtime.bands_track_is_fused(snn) and runtime.bands_track_is_fused(cpx, True)
