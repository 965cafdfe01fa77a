"""NumPy restatement of the multi-source read-out (include/micloc_hip.h, micloc_doa_peaks_f64) and of the K-target trial generator
of `sweep.multi_target_sweep`.  Written from the stated rule, not from the kernel: the tests hold the two against each other."""
import itertools

import numpy as np

LINEAR, CIRCULAR, CIRCULAR_CLOSED = 0, 1, 2
TWO_PI = 2 * np.pi


def grid_kind(doa_list, tol=1e-9):
    doa = np.asarray(doa_list, dtype=np.float64)
    G = len(doa)
    if G < 2:
        return LINEAR
    span = doa[-1] - doa[0]
    if abs(span - TWO_PI) <= tol:
        return CIRCULAR_CLOSED
    if abs(span * G / (G - 1) - TWO_PI) <= tol:
        return CIRCULAR
    return LINEAR


def _dist(a, b, circular):
    r = abs(a - b)
    return min(r, TWO_PI - r) if circular else r


def _lower(x, v):
    """a neighbour x does not block v: NaN counts as lower"""
    return np.isnan(x) or v >= x


def peaks_row(p, doa, K, min_sep, rel=0.0, kind=None):
    p = np.asarray(p, dtype=np.float64)
    doa = np.asarray(doa, dtype=np.float64)
    G = len(p)
    kind = grid_kind(doa) if kind is None else kind
    closed = kind == CIRCULAR_CLOSED and G >= 2
    circular = kind != LINEAR
    R = G - 1 if closed else G
    vals = [float(p[r]) for r in range(R)]
    ids = list(range(R))
    if closed:
        if np.isnan(p[G - 1]) or p[0] >= p[G - 1]:
            vals[0], ids[0] = float(p[0]), 0
        else:
            vals[0], ids[0] = float(p[G - 1]), G - 1
    finite = [v for v in vals if not np.isnan(v)]
    thr = rel * (max(finite) if finite else -np.inf)
    cand = []
    for r in range(R):
        v = vals[r]
        if np.isnan(v):
            continue
        ok = True
        if r > 0 or circular:
            ok = ok and _lower(vals[r - 1 if r > 0 else R - 1], v)
        if r < R - 1 or circular:
            ok = ok and _lower(vals[r + 1 if r < R - 1 else 0], v)
        if rel > 0:
            ok = ok and v >= thr
        if ok:
            cand.append((v, ids[r]))
    cand.sort(key=lambda c: (-c[0], c[1]))
    idx = np.full(K, -1, dtype=np.int32)
    val = np.full(K, np.nan)
    n = 0
    for v, i in cand:
        if n == K:
            break
        if all(_dist(doa[i], doa[j], circular) >= min_sep for j in idx[:n]):
            idx[n], val[n] = i, v
            n += 1
    return idx, val


def peaks(power, doa, K, min_sep=None, rel=0.0, kind=None):
    """[G] or [B, G] -> (index [B, K] int32, value [B, K]); min_sep defaults to two grid steps (utils.find_doa_peaks)."""
    power = np.atleast_2d(np.asarray(power, dtype=np.float64))
    doa = np.asarray(doa, dtype=np.float64)
    if min_sep is None:
        min_sep = default_separation(doa)
    out = [peaks_row(r, doa, K, min_sep, rel, kind) for r in power]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def default_separation(doa):
    doa = np.asarray(doa, dtype=np.float64)
    return 2 * abs(doa[-1] - doa[0]) / (len(doa) - 1) if len(doa) > 1 else 0.0


# ---- the K-target trial generator of multi_target_sweep -------------------------------------------------------------------

def pi_error(a, b):
    return np.arcsin(np.abs(np.sin(a - b)))


def too_close(doa, min_sep):
    return any(pi_error(doa[i], doa[j]) < min_sep for i, j in itertools.combinations(range(len(doa)), 2))


def draw_doas(draw, K, min_sep, max_redraws=10_000):
    doa = draw(K) * 2 * np.pi
    n = 0
    while too_close(doa, min_sep):
        n += 1
        if n > max_redraws:
            raise RuntimeError("redraw cap")
        doa = draw(K) * 2 * np.pi
    return doa


def synth_targets_host(geometry, fs, time_test, sig_test, doas, gains):
    """sum_k g_k * apply_to_template's delayed copy of target k (one shift = the min over all targets' delays), sig = 0; sig += ..."""
    time_test = np.asarray(time_test, dtype=np.float64)
    time_in = np.arange(time_test.min(), time_test.max(), step=1 / fs)
    sig_in = np.interp(time_in, time_test, sig_test)
    delays = np.stack([geometry.delays(d, normalized=False) for d in doas])  # [K, M]
    delays = delays - delays.min()
    sig = np.zeros((len(time_in), delays.shape[1]))
    for k in range(len(doas)):
        t = time_in.reshape(-1, 1) - delays[k].reshape(1, -1)
        t = np.maximum(t, time_in.min())
        sig += gains[k] * np.interp(t, time_in, sig_in)
    return time_in, sig


def match(doa_true, doa_grid, index):
    """Matched pi-periodic errors [K]: the permutation of the estimates with the least summed error (first in lexicographic order
    on ties); a missing estimate (-1) costs pi / 2."""
    K = len(doa_true)
    best, best_sum = None, None
    for perm in itertools.permutations(range(K)):
        e = np.array([pi_error(doa_grid[index[j]], doa_true[k]) if index[j] >= 0 else np.pi / 2 for k, j in enumerate(perm)])
        s = 0.0
        for v in e:
            s += v
        if best_sum is None or s < best_sum:
            best, best_sum = e, s
    return best


# ---- hand cases of the rule: (power, doa_list, K, min_sep or None, rel, grid kind or None, expected indices) ----------------------
# run against the restatement (test_multisource_cpu.py) and against the device (test_hip_multisource.py)

_CLOSED9 = np.linspace(-np.pi, np.pi, 9)
_LINEAR9 = np.linspace(0.0, 1.0, 9)
_CIRC8 = np.arange(8) * (2 * np.pi / 8)
HAND_CASES = [
    # plateaus: a two-point plateau gives one peak; a three-point one its far end, two steps away
    ([0, 1, 3, 3, 1, 0, 0, 2, 0], _LINEAR9, 3, None, 0.0, None, [2, 7, -1]),
    ([0, 1, 3, 3, 1, 0, 0, 2, 0], _LINEAR9, 3, 0.0, 0.0, None, [2, 3, 7]),
    ([0, 1, 3, 3, 3, 1, 0, 2, 0], _LINEAR9, 3, None, 0.0, None, [2, 4, 7]),
    ([0, 1, 3, 3, 3, 1, 0, 2, 0], _LINEAR9, 3, 0.3, 0.0, None, [2, 7, -1]),
    # the closed seam: maximum at G-1, at 0, tied; the merged point blocks its neighbour G-2
    ([1.0, 0, 0, 0, 2, 0, 0, 0.5, 3.0], _CLOSED9, 2, None, 0.0, None, [8, 4]),
    ([3.0, 0, 0, 0, 2, 0, 0, 0.5, 1.0], _CLOSED9, 2, None, 0.0, None, [0, 4]),
    ([3.0, 0, 0, 0, 2, 0, 0, 0.5, 3.0], _CLOSED9, 2, None, 0.0, None, [0, 4]),
    ([1.0, 0.5, 0.4, 0.3, 0.2, 0.3, 0.5, 0.9, 0.0], _CLOSED9, 2, 0.0, 0.0, None, [0, -1]),
    ([1.0, 0.5, 0.4, 0.3, 0.2, 0.3, 0.5, 0.9, 0.0], _CLOSED9, 2, 0.0, 0.0, LINEAR, [0, 7]),
    # circular wrap and linear edges
    ([3.0, 1, 0, 0, 2, 0, 0, 3.5], _CIRC8, 3, 0.0, 0.0, None, [7, 4, -1]),
    ([3.0, 1, 0, 0, 2, 0, 0, 3.5], _CIRC8, 3, 0.0, 0.0, LINEAR, [7, 0, 4]),
    ([3.0, 0, 0, 0, 0, 0, 2, 0], _CIRC8, 2, 2 * np.pi / 8 * 1.5, 0.0, None, [0, 6]),
    ([3.0, 0, 0, 0, 0, 0, 0, 2.0], _CIRC8, 2, 0.0, 0.0, LINEAR, [0, 7]),
    # NaN: a NaN neighbour counts as lower, an all-NaN row has no peak, the seam takes the non-NaN end
    ([0, 1, np.nan, 2, 0, 5, np.nan, 0, 0.5], _LINEAR9, 4, 0.0, 0.0, None, [5, 3, 1, 8]),
    ([np.nan] * 9, _LINEAR9, 2, None, 0.0, None, [-1, -1]),
    ([2.0, 0, 0, 0, 0, 0, 0, 0, np.nan], _CLOSED9, 1, None, 0.0, None, [0]),
    ([np.nan, 0, 0, 0, 0, 0, 0, 0, 2.0], _CLOSED9, 1, None, 0.0, None, [8]),
    # rel_threshold and fewer peaks than K
    ([0, 1.0, 0, 0.49, 0, 0.5, 0, 0, 0], _LINEAR9, 3, None, 0.0, None, [1, 5, 3]),
    ([0, 1.0, 0, 0.49, 0, 0.5, 0, 0, 0], _LINEAR9, 5, None, 0.0, None, [1, 5, 3, 7, -1]),
    ([0, 1.0, 0, 0.49, 0, 0.5, 0, 0, 0], _LINEAR9, 4, None, 0.5, None, [1, 5, -1, -1]),
    ([0, 1.0, 0, 0.49, 0, 0.5, 0, 0, 0], _LINEAR9, 4, None, 0.51, None, [1, -1, -1, -1]),
]
