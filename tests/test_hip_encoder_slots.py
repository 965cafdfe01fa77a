"""The three-slot sweep encoder (csrc/rzcc_sweep.hip: bandpass_rzcc_sweep_kernel with a 32-entry candidate ring and the loader's LDS
table of stream bases, taken by unchunked spikes-only launches with the order-2 band-pass, through the pipeline entries and
micloc_bandpass_rzcc_f64 alike) against the oracle and against the chunked route (rzcc.hip's 64-entry form with writer and resolver
waves), and the exact ring-space check of its detect wave on inputs that need more ring than the sweep: predicted overflows
(tools/dev/ring_demand.py) must be the units the fallback kernel redid.

Which kernel served a launch is not visible through the C-ABI.  What would fail if rzcc_sweep.hip's launcher quietly declined is
the w = 36 case of test_ring_overflow_is_predicted_and_exact: the 32-entry form sends 11 of the 28 streams to the fallback,
rzcc.hip's 64-entry form (whole-tile check) would send 4."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as O

pytestmark = pytest.mark.gpu

try:
    O.lib()
except Exception as e:  # the whole file needs the oracle: no single case is skipped
    pytest.skip(f"the CPU oracle cannot be built: {e}", allow_module_level=True)

_spec = importlib.util.spec_from_file_location("ring_demand", os.path.join(ROOT, "tools", "dev", "ring_demand.py"))
ring_demand = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ring_demand)

RING = 32  # entries of the form under test


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def plan(cfg2, torch):
    from haghighatshoarmuir2024_amd.runtime import Plan

    assert len(np.trim_zeros(np.asarray(cfg2["b"]), "b")) == 5, "the three-slot form serves the order-2 band-pass"
    p = Plan(7, cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True)
    p.set_neuron_kernel(cfg2["nir"])
    p.set_bf_mat(cfg2["bf_mat"])
    return p


# B = 1, 5, 10: 14, 70 and 140 streams -- one partial workgroup, two with a partial one, three with a stream group that straddles a
# trial.  T: ragged last tiles, fewer tiles than the pipeline is deep, step counts that are no multiple of four (the loader's tail).
@pytest.mark.parametrize("snr_db", [-10.0, 20.0])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 47, 48, 49, 255, 1000])
@pytest.mark.parametrize("B", [1, 5, 10])
def test_sweep_form_equals_oracle_and_chunked_route(cfg2, plan, torch, B, T, snr_db):
    """Spikes bit for bit, arg-max and power.  Power: bit-identical between the two encoder routes (same spikes into the same
    beamformer); against the oracle it is held to the 1e-12 relative of the suite's other pipeline tests (tests/test_hip_parity.py:
    the device sums the products in another order) -- the encoder reaches the power only through the spikes, which are bit-checked.
    Up to T = 32 a chunk of 32 frames is the whole stream, so both launches are the 32-entry form there and only the oracle is an
    independent reference; from T = 47 on the second launch is the chunked 64-entry form."""
    x = ring_demand.headline_input(B, 1000 * B + T, snr_db=snr_db, T=T)
    xd = plan.to_device(x)
    plan.set_encoder_chunk(0)
    assert plan.encoder_chunks(B, T) == 1
    one = plan.snn_pipeline(xd, want_spikes=True, want_power=True)
    spikes, power, argmax = one["spikes"].cpu().numpy(), one["power"].cpu().numpy(), one["argmax"].cpu().numpy()
    plan.set_encoder_chunk(32)  # two-tile chunks: the writer / resolver form with the 64-entry ring (one chunk up to T = 32)
    try:
        assert plan.encoder_chunks(B, T) == max(1, -(-(-(-T // 16)) // 2))
        chk = plan.snn_pipeline(xd, want_spikes=True, want_power=True)
        np.testing.assert_array_equal(chk["spikes"].cpu().numpy(), spikes)
        np.testing.assert_array_equal(chk["power"].cpu().numpy(), power)
        np.testing.assert_array_equal(chk["argmax"].cpu().numpy(), argmax)
    finally:
        plan.set_encoder_chunk(0)
    for i in range(B):
        ref = O.snn_chain(x[i], cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True, cfg2["nir"], cfg2["bf_mat"], want=("spikes", "power"))
        np.testing.assert_array_equal(spikes[i], ref["spikes"], err_msg=f"trial {i}")
        np.testing.assert_allclose(power[i], ref["power"], rtol=1e-12, atol=0, err_msg=f"trial {i}")
        assert int(argmax[i]) == ref["argmax"], f"trial {i}"


def _wide_plan(cfg2, b, a, w):
    from haghighatshoarmuir2024_amd.runtime import Plan

    return Plan(7, cfg2["kernel"], b, a, w, True)


def _flagged(plan, xd, T):
    """Spikes of the single encoder stage and the number of units it sent to the fallback kernel (the first word of the stage's
    scratch, which is the start of the plan's workspace)."""
    import torch

    B = xd.shape[0]
    plan.set_encoder_chunk(0)
    assert plan.encoder_chunks(B, T) == 1
    _, spk = plan.bandpass_rzcc(plan.stht(xd), T, want_pre=False, want_spikes=True)
    torch.cuda.synchronize()
    ws, _ = plan.workspace(B, T)
    return spk.cpu().numpy(), int(ws[:4].cpu().numpy().view(np.int32)[0])


# band-passed white noise, 28 streams x 1000 frames.  w = 48 behind a 2 - 4 kHz band-pass (the sweep's 1 - 2 kHz band completes only
# 31 candidates of a polarity in 1000 frames): every cluster chains on, more than 32 candidates of one polarity -- all streams
# overflow.  The sweep's band with w = 36: some do.  With w = 28: up to 19 entries outstanding, which the whole-tile check (16
# reserved: 15 usable of 32) would have flagged, and which the exact check lets through.
@pytest.mark.parametrize("w", [48, 36, 28])
def test_ring_overflow_is_predicted_and_exact(cfg2, torch, w):
    B, T = 2, 1000
    x = np.random.RandomState(7).randn(B, T, 7)
    bb, aa = O.bandpass(48_000, [2000.0, 4000.0]) if w == 48 else (cfg2["b"], cfg2["a"])
    refs = [O.snn_chain(x[i], cfg2["kernel"], bb, aa, w, True, cfg2["nir"], cfg2["bf_mat"], want=("pre_enc", "spikes")) for i in range(B)]
    sums = [np.cumsum(r["pre_enc"][:, c]) for r in refs for c in range(14)]
    worst, late = [ring_demand.ring_demand(c, w, True, 2) for c in sums], [ring_demand.ring_demand(c, w, True, 1) for c in sums]
    over = [v["demand"] > RING for v in worst]
    assert over == [v["demand"] > RING for v in late], "an input for this test overflows whichever publication the detect wave reads"
    if w == 48:
        for c in sums:  # the oracle's clusters: a chain of same-polarity candidates less than w apart, more than the ring holds
            _, pos, pol = ring_demand.candidates(c)
            assert max(np.diff(np.nonzero(np.r_[True, np.diff(pos[pol == q]) >= w, True])[0]).max() for q in (0, 1)) > RING
        assert all(over)
    if w == 36:
        assert 0 < sum(over) < len(over)
    if w == 28:
        assert not any(over) and max(v["outstanding"] for v in worst) > RING - 17, "needs the exact check, not the fallback"
    plan = _wide_plan(cfg2, bb, aa, w)
    spikes, flagged = _flagged(plan, plan.to_device(x), T)
    assert flagged == sum(over), f"fallback units taken {flagged}, predicted {sum(over)} of {len(over)} streams"
    for i in range(B):
        np.testing.assert_array_equal(spikes[i], refs[i]["spikes"], err_msg=f"w={w} trial {i}")
