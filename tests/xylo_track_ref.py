"""Reference and inputs of the Xylo tracking tests (no tests here): the oracle's integer LIF for the spike raster, then the host
Envelope.evolve and np.argmax -- the script's read-out (paper_plots/target_xylo_localization.py:757-789) on the host.

The input recipe makes ties and moving winners.  A random network does not: a random 449-neuron network has two or three distinct
winners in 700 frames and ties in 0.3 % of them, and a wrong reduction order would pass.  Here P = N // 4 random columns (weights,
decays, threshold) are dealt to the neurons at random, so equal envelopes sit at scattered indices across lanes, halves, waves and
blocks, and the raster changes its active channels every 37 frames, so the winner moves.  tests/test_xylo_track_cpu.py asserts on the
reference that the recipe does what it is for."""
import functools

import numpy as np

from haghighatshoarmuir2024_amd.utils import Envelope
from oracle import oracle as O

WINDOWS = ((1, 1), (2, 5), (48, 480))  # (w_rise, w_fall) in frames
C_RECIPE = 14
BLOCK_FRAMES = 37


def envelope(w_rise, w_fall):
    """A utils.Envelope whose windows are exactly (w_rise, w_fall) frames."""
    return Envelope(rise_time=int(w_rise), fall_time=int(w_fall), fs=1)


def random_spec(rng, Cin, N, thr_lo, thr_hi, dash_hi, w_rec=0):
    return dict(W_in=rng.randint(-127, 128, size=(Cin, N)).astype(np.int8), w_rec=w_rec,
                dash_syn=rng.randint(0, dash_hi + 1, size=N).astype(np.uint8), dash_mem=rng.randint(0, dash_hi + 1, size=N).astype(np.uint8),
                threshold=rng.randint(thr_lo, thr_hi + 1, size=N).astype(np.int16))


def grouped_spec(rng, Cin, N):
    """P = N // 4 random columns dealt to the N neurons at random."""
    P = max(N // 4, 1)
    col = dict(W=rng.randint(-127, 128, size=(Cin, P)), ds=rng.randint(0, 4, size=P), dm=rng.randint(0, 4, size=P), th=rng.randint(40, 401, size=P))
    gid = rng.randint(P, size=N)
    return dict(W_in=col["W"][:, gid].astype(np.int8), w_rec=0, dash_syn=col["ds"][gid].astype(np.uint8), dash_mem=col["dm"][gid].astype(np.uint8),
                threshold=col["th"][gid].astype(np.int16))


def blocked_raster(rng, B, T, C):
    """Ternary raster [B, T, C]: per block of 37 frames a fresh random half of the channels is active, with p(0) = 0.7."""
    raster = np.zeros((B, T, C), np.int8)
    for b in range(B):
        for t0 in range(0, T, BLOCK_FRAMES):
            act = rng.permutation(C)[: max(C // 2, 1)]
            n = min(BLOCK_FRAMES, T - t0)
            blk = raster[b, t0 : t0 + n]  # (a view)
            blk[:, act] = rng.choice([-1, 0, 1], size=(n, len(act)), p=[0.15, 0.7, 0.15])
    return raster


def all_fire(rng, raster, b=1):
    """trial b fires every channel at every step: the largest input currents"""
    if raster.shape[0] > b:
        raster[b] = rng.choice([-1, 1], size=raster.shape[1:])
    return raster


def events_of(raster):
    return np.concatenate([raster > 0, raster < 0], axis=2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def recipe(N, T, B=3):
    """(spec, raster int8 [B, T, 14]) of the recipe at (N, T); trial 1 fires every channel at every step."""
    rng = np.random.RandomState(N + T)
    spec = grouped_spec(rng, 2 * C_RECIPE, N)
    raster = all_fire(rng, blocked_raster(rng, B, T, C_RECIPE))
    raster.setflags(write=False)
    return spec, raster


def lif_reference(spec, events, max_spikes=31):
    """events uint8 [B, T, Cin] -> (spikes_out uint8 [B, T, N], rate int32 [B, N]) of the oracle"""
    outs, rates = [], []
    for ev in events:
        o, r = O.xylo_lif(ev, spec["W_in"], spec["w_rec"], spec["dash_syn"], spec["dash_mem"], spec["threshold"], max_spikes)
        outs.append(o)
        rates.append(r)
    return np.stack(outs), np.stack(rates)


def track_reference(spikes_out, rate, w_rise, w_fall):
    """The script's read-out per trial: dict(index int64 [B, T], peak_env [B, T], env_last [B, N], rate [B, N], env [B, T, N])."""
    env = np.stack([envelope(w_rise, w_fall).evolve(s) for s in spikes_out])
    index = np.argmax(env, axis=2)
    peak = np.take_along_axis(env, index[..., None], axis=2)[..., 0]
    return dict(index=index, peak_env=peak, env_last=env[:, -1, :].copy(), rate=rate, env=env)


@functools.lru_cache(maxsize=None)
def recipe_spikes(N, T):
    spec, raster = recipe(N, T)
    return lif_reference(spec, events_of(raster))


@functools.lru_cache(maxsize=None)
def recipe_reference(N, T, w_rise, w_fall):
    out, rate = recipe_spikes(N, T)
    return track_reference(out, rate, w_rise, w_fall)


def assert_equal_bits(got, ref, what=""):
    """got: XyloNetwork.track's dict of device tensors (or arrays); ref: track_reference's dict (or another got)."""
    def host(v):
        return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)

    for k in ("index", "peak_env", "env_last", "rate"):
        if k in got and got[k] is not None and k in ref and ref[k] is not None:
            g, r = host(got[k]), host(ref[k])
            if k in ("index", "rate"):
                np.testing.assert_array_equal(g.astype(np.int64), r.astype(np.int64), err_msg=f"{what} {k}")
            else:
                np.testing.assert_array_equal(g.view(np.int64), np.ascontiguousarray(r, dtype=np.float64).view(np.int64), err_msg=f"{what} {k}")
