"""The contract of the one-shot plan entries of csrc/api_plan.hip and csrc/api_track.hip, entry by entry: which status code each refusal gives and in which order the
checks run (nothing is launched by a refused call), and that every pipeline entry computes, bit for bit, what the chain
micloc_stht_f64 -> micloc_bandpass_rzcc_f64 -> the stage entry of the same read-out computes.

  read-out     from spikes              from planar rows          SNN pipeline                    Beamformer pipeline
  power / y    lif_beamform             beamform_c128             snn_pipeline(_stages)           beamformer_pipeline
  windows      lif_beamform_windows     beamform_c128_windows     snn_pipeline_windows            beamformer_pipeline_windows
  track        lif_beamform_track       beamform_c128_track       snn_pipeline_track              beamformer_pipeline_track
  covariance   lif_covariance           -                         snn_pipeline_cov                -
  fp32 tail    lif_beamform_f32         -                         -                               -
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NULL = ctypes.c_void_p(0)
F64_SENTINEL, I32_SENTINEL, I8_SENTINEL = -7.25, -7, 77
TRACK_CONSTS = (1 - 1 / 48, 1 / 48, 1 - 1 / 480)  # a_rise, i_rise, a_fall of a 48 / 480 frame envelope
G_COMPLEX = 57

# src: what the entry reads ("spikes" int8 [B][T][2M], "planar" float64 [B][2M][Ts], "x" float64 [B][T][M])
Entry = namedtuple("Entry", "name kind src readout")
ENTRIES = [
    Entry("micloc_lif_beamform_f64", "real", "spikes", "power"),
    Entry("micloc_lif_beamform_windows_f64", "real", "spikes", "windows"),
    Entry("micloc_lif_beamform_track_f64", "real", "spikes", "track"),
    Entry("micloc_lif_covariance_f64", "real", "spikes", "cov"),
    Entry("micloc_lif_beamform_f32", "real", "spikes", "f32"),
    Entry("micloc_snn_pipeline_stages_f64", "real", "x", "power"),
    Entry("micloc_snn_pipeline_f64", "real", "x", "power"),
    Entry("micloc_snn_pipeline_windows_f64", "real", "x", "windows"),
    Entry("micloc_snn_pipeline_track_f64", "real", "x", "track"),
    Entry("micloc_snn_pipeline_cov_f64", "real", "x", "cov"),
    Entry("micloc_beamform_c128_f64", "complex", "planar", "power"),
    Entry("micloc_beamform_c128_windows_f64", "complex", "planar", "windows"),
    Entry("micloc_beamform_c128_track_f64", "complex", "planar", "track"),
    Entry("micloc_beamformer_pipeline_f64", "complex", "x", "power"),
    Entry("micloc_beamformer_pipeline_windows_f64", "complex", "x", "windows"),
    Entry("micloc_beamformer_pipeline_track_f64", "complex", "x", "track"),
]
BY_NAME = {e.name: e for e in ENTRIES}


def _takes_spikes_out(e):
    return e.kind == "real" and e.src == "x" and e.readout != "track"


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def plans(cfg2, torch):
    """real: config 2 (7 microphones, 14 channels, real bf_mat, G = 449); complex: the same front end with a complex bf_mat, G = 57 (and
    the neuron kernel, so that the covariance entries reach their bf_mat rule); bare: no table set."""
    from haghighatshoarmuir2024_amd.runtime import Plan

    def make():
        return Plan(7, cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True)

    real = make()
    real.set_neuron_kernel(cfg2["nir"])
    real.set_bf_mat(cfg2["bf_mat"])
    rng = np.random.RandomState(57)
    cpx = make()
    cpx.set_neuron_kernel(cfg2["nir"])
    cpx.set_bf_mat((rng.randn(7, G_COMPLEX) + 1j * rng.randn(7, G_COMPLEX)) / np.sqrt(14))
    return dict(real=real, complex=cpx, bare=make())


def _outputs(torch, e, B, T, G, nW, with_y=True):
    """The entry's output tensors in argument order (complex y as [.., 2] float64), filled with the sentinels."""
    f64 = lambda *s: torch.full(s, F64_SENTINEL, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda *s: torch.full(s, I32_SENTINEL, dtype=torch.int32, device="cuda")  # noqa: E731
    if e.readout == "power":
        y = (f64(B, T, G, 2) if e.kind == "complex" else f64(B, T, G)) if with_y else None
        return [y, f64(B, G), i32(B)]
    if e.readout == "windows":
        return [f64(B, nW, G), i32(B, nW), f64(B, G), i32(B)]
    if e.readout == "track":
        return [i32(B, T), f64(B, T), f64(B, G)]
    if e.readout == "cov":
        return [f64(B, 14, 14), f64(B, G), i32(B)]
    return [f64(B, G), i32(B)]  # f32


def _untouched(torch, tensors):
    torch.cuda.synchronize()
    for t in tensors:
        if t is None:
            continue
        want = F64_SENTINEL if t.dtype == torch.float64 else (I32_SENTINEL if t.dtype == torch.int32 else I8_SENTINEL)
        if int((t != want).sum()) != 0:
            return False
    return True


def _call(lib, e, plan, src, B, T, outs, ws, nbytes, Ts=0, window=0, hop=0, spikes_out=None, stages=7, t_start=0):
    from haghighatshoarmuir2024_amd.runtime import _ptr, _stream

    p = lambda t: t if isinstance(t, ctypes.c_void_p) else _ptr(t)  # noqa: E731
    a = [plan.handle, p(src), B, T]
    if e.src == "planar":
        a.append(Ts)
    if e.readout == "windows":
        a += [window, hop]
    if e.readout == "track":
        a += list(TRACK_CONSTS)
    if e.readout == "cov":
        a.append(t_start)
    if _takes_spikes_out(e):
        a.append(p(spikes_out))
    a += [p(o) for o in outs]
    a += [p(ws), nbytes, _stream(plan.device)]
    if e.name == "micloc_snn_pipeline_stages_f64":
        a.append(stages)
    return getattr(lib, e.name)(*a)


def _need(lib, e, plan, B, T, window, hop):
    """The exact number of workspace bytes the entry asks for."""
    if e.readout == "track":
        return lib.micloc_track_workspace_bytes(plan.handle, B, T)
    if e.src == "x":
        return lib.micloc_workspace_bytes(plan.handle, B, T)
    if e.readout == "cov":  # cov_partial_bytes of csrc/covariance.hip for one channel tile: a 16 x 16 tile per 512-frame chunk
        return B * ((T + 511) // 512) * 256 * 8
    if e.readout == "windows":
        return lib.micloc_window_workspace_bytes(plan.handle, B, T, window, hop, 0)
    return lib.micloc_lif_beamform_workspace_bytes(plan.handle, B, T)


def _source(torch, e, B, T, Ts, seed=0):
    rng = np.random.RandomState(seed)
    if e.src == "spikes":
        return torch.from_numpy(rng.randint(-1, 2, size=(B, T, 14)).astype(np.int8)).cuda()
    if e.src == "planar":
        return torch.from_numpy(rng.randn(B, 14, Ts)).cuda()
    return torch.from_numpy(rng.randn(B, T, 7)).cuda()


# ---- 1. the status table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [e.name for e in ENTRIES])
def test_status_codes_in_the_order_of_the_checks(plans, torch, name):
    from haghighatshoarmuir2024_amd import _lib

    lib = _lib.load()
    e = BY_NAME[name]
    B, T = 2, 300
    right, wrong, bare = plans[e.kind], plans["complex" if e.kind == "real" else "real"], plans["bare"]
    Ts = lib.micloc_padded_T(T)
    q = lib.micloc_window_quantum(right.handle)
    assert q > 0
    nW = lib.micloc_window_count(T, q, q, q)
    assert nW > 0
    src = _source(torch, e, B, T, Ts)
    outs = _outputs(torch, e, B, T, right.G, nW)
    spikes_out = torch.full((B, T, 14), I8_SENTINEL, dtype=torch.int8, device="cuda") if _takes_spikes_out(e) else None
    n = _need(lib, e, right, B, T, q, q)
    assert n > 0
    ws = torch.full((n + 256,), I8_SENTINEL, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    watched = outs + [spikes_out, ws]

    def call(plan=right, src=src, B=B, T=T, outs=outs, ws=ws, nbytes=n, Ts=Ts, window=q, spikes_out=spikes_out, stages=7):
        rc = _call(lib, e, plan, src, B, T, outs, ws, nbytes, Ts=Ts, window=window, hop=q, spikes_out=spikes_out, stages=stages)
        if rc != _lib.MICLOC_OK:
            assert _untouched(torch, watched), f"{name}: a call refused with status {rc} wrote to its buffers"
        return rc

    assert call(plan=bare, ws=NULL) == _lib.MICLOC_ERR_NOT_SET
    assert call(plan=wrong, ws=NULL) == _lib.MICLOC_ERR_SHAPE
    if e.src == "planar":
        assert call(plan=bare, Ts=Ts + 8) == _lib.MICLOC_ERR_SHAPE  # the row stride is checked before the tables
    if e.readout == "windows":
        assert call(window=q + 1, ws=NULL) == _lib.MICLOC_ERR_SHAPE  # the window rule is checked before the workspace
    if e.readout == "track":
        assert call(T=0) == _lib.MICLOC_ERR_SHAPE
        assert call(B=65536) == _lib.MICLOC_ERR_INVALID
    assert call(nbytes=n - 1) == _lib.MICLOC_ERR_WORKSPACE
    assert call(ws=NULL) == _lib.MICLOC_ERR_WORKSPACE
    assert call(ws=ctypes.c_void_p(ws.data_ptr() + 8)) == _lib.MICLOC_ERR_WORKSPACE
    assert call(B=0) == _lib.MICLOC_ERR_INVALID
    assert call(src=NULL) == _lib.MICLOC_ERR_INVALID
    assert call(outs=[None] * len(outs), spikes_out=None) == _lib.MICLOC_ERR_INVALID
    if name == "micloc_snn_pipeline_stages_f64":
        assert call(stages=0) == _lib.MICLOC_ERR_INVALID
        assert call(stages=32) == _lib.MICLOC_ERR_INVALID
    if name == "micloc_lif_beamform_f64":  # the workspace holds the sums of the power read-out: y alone needs none
        assert call(outs=[outs[0], None, None], ws=NULL, nbytes=0) == _lib.MICLOC_OK
        torch.cuda.synchronize()
        assert int((outs[0] == F64_SENTINEL).sum()) == 0 and _untouched(torch, outs[1:])


# ---- 2. pipeline entry == STHT -> band-pass / RZCC -> stage entry ----------------------------------------------------------------------
def _run(torch, lib, e, plan, src, B, T, Ts, window=0, hop=0, with_y=True, want_spikes=False):
    from haghighatshoarmuir2024_amd import _lib

    nW = lib.micloc_window_count(T, window, hop, lib.micloc_window_quantum(plan.handle)) if e.readout == "windows" else 0
    outs = _outputs(torch, e, B, T, plan.G, nW, with_y=with_y)
    n = _need(lib, e, plan, B, T, window, hop)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    spikes_out = torch.full((B, T, 14), I8_SENTINEL, dtype=torch.int8, device="cuda") if want_spikes else None
    assert _call(lib, e, plan, src, B, T, outs, ws, n, Ts=Ts, window=window, hop=hop, spikes_out=spikes_out, t_start=T // 4) == _lib.MICLOC_OK, e.name
    return outs + [spikes_out]


@pytest.mark.parametrize("shape", ["one-chunk", "ragged-chunks"])
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_pipeline_entries_equal_the_chain_of_stage_entries(plans, torch, kind, shape):
    from haghighatshoarmuir2024_amd import _lib
    from haghighatshoarmuir2024_amd.runtime import _ptr, _stream

    lib = _lib.load()
    plan = plans[kind]
    q = lib.micloc_window_quantum(plan.handle)
    assert q > 0
    B, T = (3, 300) if shape == "one-chunk" else (2, 2 * q + 5)  # the second: several chunks, the last one and the last window ragged
    Ts = lib.micloc_padded_T(T)
    st = _stream(plan.device)
    x = torch.from_numpy(np.random.RandomState(B * T).randn(B, T, 7)).cuda()
    h = torch.empty((B, 14, Ts), dtype=torch.float64, device="cuda")
    assert lib.micloc_stht_f64(plan.handle, _ptr(x), B, T, _ptr(h), Ts, st) == _lib.MICLOC_OK
    # the band-pass stage writes the intermediate the plan's kind reads: the raster (real bf_mat) or the planar rows (complex)
    if kind == "real":
        mid = torch.empty((B, T, 14), dtype=torch.int8, device="cuda")
        n = lib.micloc_workspace_bytes(plan.handle, B, T)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        assert lib.micloc_bandpass_rzcc_f64(plan.handle, _ptr(h), B, T, Ts, None, _ptr(mid), _ptr(ws), n, st) == _lib.MICLOC_OK
        assert int((mid != 0).sum()) > 0
        rows = [("lif_beamform", "snn_pipeline", "power"), ("lif_beamform", "snn_pipeline_stages", "power"),
                ("lif_beamform_windows", "snn_pipeline_windows", "windows"), ("lif_beamform_track", "snn_pipeline_track", "track"),
                ("lif_covariance", "snn_pipeline_cov", "cov")]
    else:
        mid = torch.empty((B, 14, Ts), dtype=torch.float64, device="cuda")
        assert lib.micloc_bandpass_rzcc_f64(plan.handle, _ptr(h), B, T, Ts, _ptr(mid), None, None, 0, st) == _lib.MICLOC_OK
        rows = [("beamform_c128", "beamformer_pipeline", "power"), ("beamform_c128_windows", "beamformer_pipeline_windows", "windows"),
                ("beamform_c128_track", "beamformer_pipeline_track", "track")]
    for stage, pipeline, readout in rows:
        es, ep = BY_NAME[f"micloc_{stage}_f64"], BY_NAME[f"micloc_{pipeline}_f64"]
        variants = dict(power=[dict(with_y=False), dict(with_y=True)], windows=[dict(window=q, hop=q), dict(window=2 * q, hop=q)]).get(readout, [{}])
        for kw in variants:
            want = _run(torch, lib, es, plan, mid, B, T, Ts, **kw)
            got = _run(torch, lib, ep, plan, x, B, T, Ts, want_spikes=_takes_spikes_out(ep), **kw)
            tag = f"{pipeline} vs {stage} {kw} B={B} T={T}"
            if got[-1] is not None:
                assert torch.equal(got[-1], mid), f"{tag}: spikes"
            for i, (g, w) in enumerate(zip(got[:-1], want[:-1])):
                if w is None:
                    assert g is None
                    continue
                assert torch.equal(g, w), f"{tag}: output {i}"
                assert int((g == (F64_SENTINEL if g.dtype == torch.float64 else I32_SENTINEL)).sum()) == 0, f"{tag}: output {i} not written"
