"""Stage 1 of beamform_ws_kernel_lean at 35 taps (csrc/beamform_lean.hip): the LIF as a sliding-window FIR on the vector ALU, a lane per
(channel, block of 8 frames), instead of the padded Toeplitz product on the matrix cores -- at the smallest shapes at which it can go wrong.

The calls are those of tests/test_hip_beamform_lean.py: `Plan.lif_beamform(spikes)` is the one-shot call the fixed-shape kernel serves,
the same call with `window=256` keeps the general beamform_ws_kernel (matrix-core LIF) on the same 256-frame chunks and reduces the same
per-chunk partial sums.  Every case asks: total power and arg-max equal to the last bit between the two, power within 1e-12 relative of
oracle.lif_fir + oracle.beamform (the project's bar for power), arg-max equal to the oracle's.

  impulses   one spike of +1 or -1 in one channel and nothing else: every tap's position and every hand-over of the window is seen on its
             own -- block of 8 frames, tile of 16, wave of 32, chunk of 256 and the 36-row halo in front of it, the end of the trial;
  dense      every entry +-1, so all 35 taps of every output carry a product; T from one frame to two chunks and a ragged third;
  int8       the full range, staging converts whatever it finds;
  B          8 / 9 (the XCD chunk order treats the last B mod 8 trials differently) and 1;
  36 taps    a tap count the FIR form does not serve (NK = 13 all the same): the matrix-core stage 1 still answers;
  golden     the three golden trials of config 2 through the whole pipeline against oracle.snn_chain_batch.
As in test_hip_beamform_lean.py, which kernel answered is the profiler's to say (profiles/ws_lean_fir/RECORD.json)."""
import numpy as np
import pytest

from conftest import golden
from oracle import oracle as O

pytestmark = pytest.mark.gpu

C = 14
T_IMP = 600
IMPULSE_FRAMES = [0, 7, 8, 31, 32, 220, 221, 222, 255, 256, 257, 290, 291, 292, T_IMP - 36, T_IMP - 35, T_IMP - 1]
DENSE_TS = [1, 8, 9, 35, 36, 257, 292, 513, 600]
DENSE_GS = [257, 360, 384]


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def plans(cfg2, torch):
    """One plan per (DoA count, neuron kernel): the first G columns of config 2's bf_mat."""
    from haghighatshoarmuir2024_amd.runtime import Plan

    made = {}

    def get(G, nir=None):
        key = (G, None if nir is None else len(nir))
        if key not in made:
            p = Plan(7, cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True)
            p.set_neuron_kernel(cfg2["nir"] if nir is None else nir)
            p.set_bf_mat(np.ascontiguousarray(cfg2["bf_mat"][:, :G]))
            made[key] = p
        return made[key]

    return get


def check(torch, p, s, nir, W):
    """s: int8 [B][T][14].  One-shot against windowed to the last bit, both against the oracle's LIF + beamforming."""
    spikes = torch.from_numpy(s).cuda()
    one = p.lif_beamform(spikes, want_power=True)
    win = p.lif_beamform(spikes, want_power=True, window=256)
    power, argmax = one["power"].cpu().numpy(), one["argmax"].cpu().numpy()
    ref = np.empty((s.shape[0], W.shape[1]))
    for i in range(s.shape[0]):
        y = O.beamform(O.lif_fir(s[i], nir), W)
        ref[i] = np.mean(y * y, axis=0)
    print("max relative deviation from the oracle: %.3e" % np.max(np.abs(power - ref) / np.where(ref > 0, ref, 1.0)))
    np.testing.assert_array_equal(power, win["power"].cpu().numpy())
    np.testing.assert_array_equal(argmax, win["argmax"].cpu().numpy())
    np.testing.assert_allclose(power, ref, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(argmax, np.argmax(ref, axis=1))


def ternary(seed, B, T):
    rng = np.random.RandomState(seed)
    return (np.where(rng.rand(B, T, C) < 0.08, 1, 0) * rng.choice([-1, 1], size=(B, T, C))).astype(np.int8)


@pytest.mark.parametrize("c", [0, 12, 13])
def test_impulses(plans, cfg2, torch, c):
    """A trial per (frame, sign): 34 trials of one spike each."""
    s = np.zeros((2 * len(IMPULSE_FRAMES), T_IMP, C), dtype=np.int8)
    for i, f in enumerate(IMPULSE_FRAMES):
        s[2 * i, f, c] = 1
        s[2 * i + 1, f, c] = -1
    check(torch, plans(360), s, cfg2["nir"], np.ascontiguousarray(cfg2["bf_mat"][:, :360]))


@pytest.mark.parametrize("G", DENSE_GS)
@pytest.mark.parametrize("T", DENSE_TS)
def test_dense_rasters(plans, cfg2, torch, T, G):
    """Trial 0: random signs; trial 1: all -1."""
    s = np.empty((2, T, C), dtype=np.int8)
    s[0] = np.random.RandomState(2000 + T).choice([-1, 1], size=(T, C))
    s[1] = -1
    check(torch, plans(G), s, cfg2["nir"], np.ascontiguousarray(cfg2["bf_mat"][:, :G]))


def test_full_int8_range(plans, cfg2, torch):
    """Trial 0: random -128 .. 127; trial 1: only -128 and 127."""
    rng = np.random.RandomState(6)
    s = np.empty((2, 513, C), dtype=np.int8)
    s[0] = rng.randint(-128, 128, size=(513, C))
    s[1] = rng.choice([-128, 127], size=(513, C))
    check(torch, plans(360), s, cfg2["nir"], np.ascontiguousarray(cfg2["bf_mat"][:, :360]))


@pytest.mark.parametrize("B", [1, 8, 9])
def test_batch_sizes(plans, cfg2, torch, B):
    check(torch, plans(360), ternary(3000 + B, B, 513), cfg2["nir"], np.ascontiguousarray(cfg2["bf_mat"][:, :360]))


def test_a_tap_count_the_fir_form_does_not_serve(plans, cfg2, torch):
    """34 taps of nir, a zero, a non-zero 36th tap: 13 k-steps as for 35 taps, through the matrix-core stage 1."""
    nir = np.concatenate([cfg2["nir"][:34], [0.0, 0.25 * cfg2["nir"][33]]])
    assert len(cfg2["nir"]) == 35 and len(nir) == 36 and nir[35] != 0.0 and (len(nir) + 15 + 3) // 4 == 13
    check(torch, plans(360, nir), ternary(4000, 3, 513), nir, np.ascontiguousarray(cfg2["bf_mat"][:, :360]))


def test_pipeline_on_the_golden_trials_against_the_oracle_chain(plans, cfg2):
    x = golden("trials_cfg2.npz")["sig_in"]
    p = plans(360)
    W = np.ascontiguousarray(cfg2["bf_mat"][:, :360])
    out = p.snn_pipeline(p.to_device(x), want_power=True)
    ref_power, ref_argmax = O.snn_chain_batch(x, cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True, cfg2["nir"], W)
    np.testing.assert_allclose(out["power"].cpu().numpy(), ref_power, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(out["argmax"].cpu().numpy(), ref_argmax)
