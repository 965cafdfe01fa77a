#!/usr/bin/env python3
"""CPU model of the candidate ring of the encoder kernels (csrc/rzcc_sweep.hip, csrc/rzcc.hip): how many ring entries a stream needs.

    python tools/dev/ring_demand.py [trials] [seed]      headline-like streams at the lowest SNR of the sweep

The kernel's rules, as modelled (unchunked form: no resolver wave):

* Candidates.  The detect wave walks the running sum c of the band-passed stream.  Every reversal of the direction of the last
  strict change completes one candidate at the step t of the reversal: a maximum when c falls after a rise, a minimum (bipolar
  encoders only) when it rises after a fall.  Its position is the plateau midpoint (left + t - 1) >> 1, `left` being the time of the
  previous strict change.  The first strict change of a stream completes nothing.  Maxima and minima alternate, so polarity q owns
  every second list index from its first one on (unipolar: every index is a maximum).
* Tiles and barriers.  Time is cut into tiles of 16 steps, one barrier per tile.  Between two barriers the detect wave appends the
  candidates of tile m (those with t // 16 == m) while the select waves examine what the detect wave had published at the last barrier:
  the candidates of the tiles <= m - 1.  The detect wave reads the select waves' `oldest` without ordering inside the step, so what it
  sees is their publication of this step or of the one before: at worst the state after the tiles <= m - 2 (`select_lag` = 2, the
  default; 1 is the other end of the race).
* oldest.  A select wave examines its own candidates in order.  One that lies >= w behind the previous own candidate closes the open
  cluster and opens the next.  It publishes the first list index of its open cluster, or its next unexamined index while it has none;
  `oldest` is the minimum over the polarities.
* Space check, per tile and before its appends, with n candidates appended so far and ne events in the tile:
      exact (rzcc_sweep.hip, RING = 32):  n + max(ne, 3) - oldest > RING   (the three unconditional stores need their slots too)
      whole tile (rzcc.hip, RING = 64):   n + 16 - oldest > RING - 1
  A stream that fails it stops appending; its unit is redone by rzcc_unit_fallback_kernel.

`ring_demand` returns the largest left-hand sides: `demand` = max(n + max(ne, 3) - oldest) and `outstanding` = max(n - oldest).
The exact check overflows iff demand > RING, the whole-tile check iff outstanding > RING - 17."""
import sys

import numpy as np

MT = 16      # steps per tile
DET_PF = 3   # unconditional stores per tile


def candidates(c, bipolar=True):
    """Running sum c [T] -> (event step, position, polarity: 0 maximum / 1 minimum) of every candidate, in list order."""
    d = np.sign(np.diff(np.asarray(c, dtype=np.float64)))
    ts = np.nonzero(d)[0] + 1  # steps with a strict change
    ds = d[ts - 1]
    rev = np.nonzero(ds[1:] != ds[:-1])[0] + 1
    t = ts[rev]
    pos = (ts[rev - 1] + t - 1) >> 1
    pol = (ds[rev] > 0).astype(np.int64)
    if not bipolar:
        keep = pol == 0
        t, pos, pol = t[keep], pos[keep], pol[keep]
    return t, pos, pol


def ring_demand(c, w, bipolar=True, select_lag=2):
    """-> dict(demand, outstanding, candidates) of one stream (see the module docstring)."""
    T = len(c)
    NM = (T + MT - 1) // MT
    t, pos, pol = candidates(c, bipolar)
    n_all = len(t)
    ne = np.bincount(t // MT, minlength=NM)[:NM] if n_all else np.zeros(NM, dtype=np.int64)
    n_after = np.cumsum(ne)                       # candidates appended after tile m
    n_before = n_after - ne
    m = np.arange(NM)
    seen = np.where(m - select_lag >= 0, n_after[np.maximum(m - select_lag, 0)], 0)  # what the select waves have examined
    oldest = np.full(NM, np.iinfo(np.int64).max)
    for q in ((0, 1) if bipolar else (0,)):
        g = np.nonzero(pol == q)[0]               # list indices of this polarity
        first = g[0] if len(g) else 1             # (a polarity without a candidate waits at list index 1)
        if len(g):
            p = pos[g]
            start = np.ones(len(g), dtype=bool)
            start[1:] = p[1:] - p[:-1] >= w
            open_ = np.maximum.accumulate(np.where(start, np.arange(len(g)), 0))  # own index of the open cluster's first candidate
            done = np.searchsorted(g, seen, side="left")                           # own candidates examined
            keep = np.where(done > 0, g[open_[np.maximum(done - 1, 0)]], np.where(seen > 0, first, 0))
        else:
            keep = np.where(seen > 0, first, 0)
        oldest = np.minimum(oldest, keep)
    out = n_before - oldest
    return dict(demand=int((out + np.maximum(ne, DET_PF)).max()), outstanding=int(out.max()), candidates=int(n_all))


def overflows(c, w, ring, bipolar=True, exact=True, select_lag=2):
    r = ring_demand(c, w, bipolar, select_lag)
    return r["demand"] > ring if exact else r["outstanding"] > ring - MT - 1


def stht_kernel(fs=48_000, duration=10e-3):
    from scipy.signal import hilbert

    L = int(fs * duration)
    imp = np.zeros(L)
    imp[0] = 1
    return np.fft.fftshift(np.imag(hilbert(imp)))


def running_sums(x, b, a, kernel):
    """x [B, T, M] -> running sums [B * 2M, T] of the band-passed in-phase and quadrature (Hilbert kernel) channels."""
    from scipy.signal import fftconvolve, lfilter

    q = fftconvolve(x, kernel[None, :, None], mode="full")[:, len(kernel) // 2: len(kernel) // 2 + x.shape[1]]
    h = np.concatenate([x, q], axis=2)
    return np.cumsum(lfilter(b, a, h, axis=1), axis=1).transpose(0, 2, 1).reshape(-1, x.shape[1])


def headline_input(trials, seed, snr_db=-10.0, fs=48_000, T=4799, M=7, f0=2000.0, radius=4.5e-2):
    """The sweep's test signal: a 2 kHz tone on a 7-microphone circle from a random direction plus white noise at
    snr_db - 10 log10((fs / 2) / 1 kHz) -- the bandwidth gain of the sweep -- per microphone.  -> x [trials, T, M]"""
    rng = np.random.RandomState(seed)
    tt = np.arange(T) / fs
    doa = rng.rand(trials) * 2 * np.pi
    ang = np.concatenate([[0.0], np.arange(M - 1) * 2 * np.pi / (M - 1)])
    rad = np.concatenate([[0.0], np.full(M - 1, radius)])
    delay = rad[None, :] * np.cos(doa[:, None] - ang[None, :]) / 340.0
    x = np.sin(2 * np.pi * f0 * (tt[None, :, None] - delay[:, None, :]))
    snr = snr_db - 10 * np.log10((fs / 2) / 1000.0)
    return x + np.sqrt(0.5 / 10 ** (snr / 10)) * rng.randn(trials, T, M)


def headline_demand(trials=143, seed=0, w=12, select_lag=2, kernel=None):
    """Ring demand of trials x 14 headline-like streams at the lowest SNR -> (demand, outstanding) arrays.
    kernel: the Hilbert kernel of the quadrature channels (default: scipy's, rebuilt here; a plan's own may be passed)."""
    from scipy.signal import butter

    b, a = butter(2, [1000.0, 2000.0], btype="bandpass", fs=48_000)
    cs = running_sums(headline_input(trials, seed), b, a, stht_kernel() if kernel is None else np.asarray(kernel, dtype=np.float64))
    r = [ring_demand(c, w, True, select_lag) for c in cs]
    return np.array([v["demand"] for v in r]), np.array([v["outstanding"] for v in r])


if __name__ == "__main__":
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 286
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    dem, out = headline_demand(trials, seed)
    print(f"{len(dem)} streams: outstanding entries mean {out.mean():.1f}, 99th percentile {np.percentile(out, 99):.0f}, max {out.max()}; "
          f"exact-check demand max {dem.max()} of 32")
