"""The fixed-shape beamformer of csrc/beamform_lean.hip (14 channels, three DoA tiles per wave, power only: the sweep's launch) against
the general beamform_ws_kernel and against the oracle.

(a) bit-equality: `Plan.lif_beamform(spikes)` is the one-shot call that the fixed-shape kernel serves; `Plan.lif_beamform(spikes,
    window=256)` keeps the general kernel (the windowed read-out needs its launch) on the same raster with the same 256-frame chunks and
    reduces the same per-chunk partial sums with the same power_argmax_kernel -- so total power and arg-max must agree to the last bit.
(b) the oracle: a raster has no signal to give oracle.snn_chain_batch, so the rasters are checked against the oracle's own LIF and
    beamforming stages (what snn_chain_batch runs behind the encoder) and the golden trials of config 2 go through the whole pipeline
    against oracle.snn_chain_batch itself; power within 1e-12 relative (tests/test_hip_parity.py's bar for power), arg-max equal.

What these tests cannot show is WHICH kernel answered the one-shot call: the library has no switch and no query for it (none was added:
no new ABI), so if the dispatch declined everywhere they would pass as general against general.  That the eligible shapes run
beamform_ws_kernel_lean is recorded by the profiler instead: the kernel name and its counters in profiles/ws_lean/RECORD.json, and
tests/test_bench_gpu.py finds the dominant kernel by the `beamform_ws_kernel` substring.

T: one tile, the chunk edge (255 / 256 / 257), the length of a chunk plus its LIF halo (291 / 292 spike rows: still two edge chunks, staged
element-wise with clamps), two whole chunks and one frame more (a chunk is interior -- the wide staging path -- iff it starts at frame
256 or later and ends inside the trial, so 512 is the first length with one), the sweep's 4799 (17 interior chunks and a ragged last
one).  G: 257 / 360 / 368 / 384 = 17 / 23 / 23 / 24 DoA tiles
(one wave with three tiles, a light last wave, padded and unpadded columns)."""
import numpy as np
import pytest

from conftest import golden
from oracle import oracle as O

pytestmark = pytest.mark.gpu

B = 3
TS = [1, 15, 16, 17, 255, 256, 257, 291, 292, 512, 513, 4799]
GS = [257, 360, 368, 384]


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def plans(cfg2, torch):
    """One plan per DoA count: the first G columns of config 2's bf_mat."""
    from haghighatshoarmuir2024_amd.runtime import Plan

    made = {}

    def get(G):
        if G not in made:
            p = Plan(7, cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True)
            p.set_neuron_kernel(cfg2["nir"])
            p.set_bf_mat(np.ascontiguousarray(cfg2["bf_mat"][:, :G]))
            made[G] = p
        return made[G]

    return get


_RASTERS = {}


def raster(T, C=14):
    """Random ternary raster at about 8 % density and the oracle's membrane signal for it (computed once per length)."""
    if (T, C) not in _RASTERS:
        rng = np.random.RandomState(1000 + T + C)
        s = (np.where(rng.rand(B, T, C) < 0.08, 1, 0) * rng.choice([-1, 1], size=(B, T, C))).astype(np.int8)
        _RASTERS[(T, C)] = s
    return _RASTERS[(T, C)]


_VMEM = {}


def vmem(T, nir, C=14):
    if (T, C) not in _VMEM:
        _VMEM[(T, C)] = [O.lif_fir(raster(T, C)[i], nir) for i in range(B)]
    return _VMEM[(T, C)]


def oracle_power(T, nir, W):
    out = np.empty((B, W.shape[1]))
    for i, v in enumerate(vmem(T, nir, W.shape[0])):
        y = O.beamform(v, W)
        out[i] = np.mean(y * y, axis=0)
    return out


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("T", TS)
def test_lean_kernel_bit_equal_to_general_and_within_oracle_bar(plans, cfg2, torch, T, G):
    p = plans(G)
    spikes = torch.from_numpy(raster(T)).cuda()
    lean = p.lif_beamform(spikes, want_power=True)                # fixed-shape kernel
    gen = p.lif_beamform(spikes, want_power=True, window=256)     # general kernel, same chunks, same time reduction
    power, argmax = lean["power"].cpu().numpy(), lean["argmax"].cpu().numpy()
    np.testing.assert_array_equal(power, gen["power"].cpu().numpy())
    np.testing.assert_array_equal(argmax, gen["argmax"].cpu().numpy())
    ref = oracle_power(T, cfg2["nir"], np.ascontiguousarray(cfg2["bf_mat"][:, :G]))
    np.testing.assert_allclose(power, ref, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(argmax, np.argmax(ref, axis=1))


@pytest.mark.parametrize("G", GS)
def test_pipeline_on_the_golden_trials_against_the_oracle_chain(plans, cfg2, G):
    x = golden("trials_cfg2.npz")["sig_in"]
    p = plans(G)
    W = np.ascontiguousarray(cfg2["bf_mat"][:, :G])
    out = p.snn_pipeline(p.to_device(x), want_power=True)
    ref_power, ref_argmax = O.snn_chain_batch(x, cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True, cfg2["nir"], W)
    np.testing.assert_allclose(out["power"].cpu().numpy(), ref_power, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(out["argmax"].cpu().numpy(), ref_argmax)


def test_raster_that_is_not_ternary(plans, cfg2, torch):
    """The staging converts int8 values, whatever they are: -128 .. 127 in an interior chunk."""
    rng = np.random.RandomState(5)
    s = rng.randint(-128, 128, size=(B, 1000, 14)).astype(np.int8)
    p = plans(360)
    spikes = torch.from_numpy(s).cuda()
    lean = p.lif_beamform(spikes, want_power=True)
    gen = p.lif_beamform(spikes, want_power=True, window=256)
    np.testing.assert_array_equal(lean["power"].cpu().numpy(), gen["power"].cpu().numpy())
    np.testing.assert_array_equal(lean["argmax"].cpu().numpy(), gen["argmax"].cpu().numpy())
    W = np.ascontiguousarray(cfg2["bf_mat"][:, :360])
    for i in range(B):
        y = O.beamform(O.lif_fir(s[i], cfg2["nir"]), W)
        np.testing.assert_allclose(lean["power"][i].cpu().numpy(), np.mean(y * y, axis=0), rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", ["G449", "C8"])
def test_other_shapes_fall_through_to_the_general_kernel(cfg2, torch, shape):
    """449 DoAs (four DoA tiles per wave) and 8 channels are not the fixed-shape kernel's: the one-shot call still answers."""
    from haghighatshoarmuir2024_amd.runtime import Plan

    T = 513
    if shape == "G449":
        M, W = 7, cfg2["bf_mat"]
    else:
        M, W = 4, np.random.RandomState(8).randn(8, 360)
    p = Plan(M, cfg2["kernel"], cfg2["b"], cfg2["a"], cfg2["robust_width"], True)
    p.set_neuron_kernel(cfg2["nir"])
    p.set_bf_mat(W)
    spikes = torch.from_numpy(raster(T, 2 * M)).cuda()
    one = p.lif_beamform(spikes, want_power=True)
    win = p.lif_beamform(spikes, want_power=True, window=256)
    np.testing.assert_array_equal(one["power"].cpu().numpy(), win["power"].cpu().numpy())
    ref = oracle_power(T, cfg2["nir"], np.ascontiguousarray(W))
    np.testing.assert_allclose(one["power"].cpu().numpy(), ref, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(one["argmax"].cpu().numpy(), np.argmax(ref, axis=1))
