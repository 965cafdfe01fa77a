"""MUSIC restated from its definition, twice, for the stage tests of csrc/music.hip and csrc/stream_music.hip (whose arithmetic is
csrc/music_rows.h's).  One chain: per slice `lfilter(b, a)` from zero state, frames of N samples, X = frames . W, bin power, stable
top-k, steering power, read-out.  Nothing here is written from the kernels' method: the filter is the difference equation (direct form,
the kernels run DF2T), the products are plain matrix products, the rank is the definition of a stable sort.

  slices(T, L, hop)            MUSIC.apply_to_signal's slices in integers: the full ones and the leftover one of more than L / 2 samples
  stable_rank, select          THE RANK RULE: ascending power, a NaN behind every number, equal powers and NaNs by bin index -- counted
                               pair by pair, and np.argsort(kind="stable")'s order (tests/test_music_ref_cpu.py)
  exact_music                  THE EXACT TIER.  Data, filter, W and steering tables are integers and the chain runs in int64.  Every value
                               the device forms is then an integer below 2^53, so its result depends neither on the order of a sum nor on
                               how a matrix instruction adds its four k-steps: device and reference agree bit for bit.  Every sum is guarded
                               by the sum of the absolute values of its terms (which bounds every partial sum in every order, and every
                               word of the DF2T state): ExactRangeError at 2^53, the read-out's P^2 included.  The only divisions are
                               correctly rounded ones of exact integers (bin power / (M F), which only orders the bins; / F; / S): exact for
                               F, S in {1, 2, 4}, one rounding each otherwise -- the sum over the selected bins then rounds per addition,
                               which the tests allow 1 ulp for.
  INTEGER_FILTERS              integer filters that stay bounded: products of cyclotomic polynomials as denominator
  ld_music and the *_bound     THE ROUNDING TIER.  The same chain in np.longdouble (eps <= 2^-63 asserted) on real data, and beside every
                               value a first-order forward error bound for the float64 device of the form
                                   2 x (roundings on the path of a term) x 2^-53 x (sum of the absolute values of the terms)
                               plus the first-order image of the bound of the stage before.  The factor 2 covers the second order and the
                               reference's own error.  The counts, read off music_rows.h (built with -ffp-contract=off: a product and a sum
                               round apart unless written as fma):
    filter   DF2T, per step y = fma(b0, x, z0): 1 rounding of |b0 x| + |z0|; z_k = fma(-a, y, fma(b, x, z_k+1)): 2 roundings, each of at
             most |b x| + |z_k+1| + |a y|.  A local error put into z_k reaches y k + 1 samples later, and every error of y comes back
             through the recursion: |dy| <= |h| * eta, h the impulse response of 1 / a(z), eta the local errors (filter_bound).  The
             recurrence has no closed bound beyond this one.
    DFT      music_dft_rows: one chain of Np fused multiply-adds per (row, column), whatever the order: Np roundings,
             2 Np 2^-53 sum_n |xf[n]| |W[n, c]|  (dft_bound)
    steering music_steer_sum, per (bin, frame): zr = sum_m (ar re + ai im) -- each product 1, their sum 1, the running sum over M mics
             <= M: M + 2 roundings of Ar = sum_m (|ar re| + |ai im|), and zi alike with Ai.  v = zr zr + zi zi: every term of the expanded
             square carries both factors' roundings, 2 (M + 2), the square 1, the sum of the two squares 1; acc over F frames: F;
             acc / F: 1; P over ksel bins: ksel.  Together R = 2 (M + 2) + 3 + F + ksel roundings of sum_i mean_f (Ar^2 + Ai^2)
             (steer_bound; an error dX of X adds 2 Ar sum_m (|ar| dre + |ai| dim), and alike for Ai).
    read-out music_power_add: P P: 1, the sum over S slices: S, / S: 1: S + 2 roundings of mean_s P^2, and 2 |P| dP / S from the
             spectrum (power_bound)
  filter_probe, delta_steering the probe tables that isolate one stage through the public call (see tests/test_hip_music_stages.py)
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0**-63, "np.longdouble is no wider than float64 here: the rounding tier has no reference"
U = 2.0**-53
LIMIT = 2**53


class ExactRangeError(ValueError):
    """An intermediate of the exact tier reaches 2^53: the device's float64 would round."""


# ---- the slices ------------------------------------------------------------------------------------------------------------------
def slices(T, L, hop):
    """[(start, length)] of MUSIC.apply_to_signal on T samples: full slices while they fit, then the rest if longer than L / 2."""
    out = []
    s = 0
    while s * hop + L <= T:
        out.append((s * hop, L))
        s += 1
    if 2 * (T - s * hop) > L:
        out.append((s * hop, T - s * hop))
    return out


# ---- the rank rule ---------------------------------------------------------------------------------------------------------------
def sorts_before(pi, i, pj, j):
    """Does bin i (power pi) stand before bin j in the selection's order?"""
    if pj != pj:
        return pi == pi or i < j
    return pi < pj or (pi == pj and i < j)


def stable_rank(pw):
    """rank[j] = the number of bins that stand before bin j: a permutation of 0 .. len(pw) - 1, whatever pw holds."""
    pw = np.asarray(pw, dtype=np.float64)
    if len(pw) <= 8:  # the definition, pair by pair
        return np.asarray([sum(sorts_before(pi, i, pj, j) for i, pi in enumerate(pw) if i != j) for j, pj in enumerate(pw)], dtype=np.int64)
    # the same for all pairs at once: before[i, j] = sorts_before(pw[i], i, pw[j], j)
    pi, pj = pw[:, None], pw[None, :]
    earlier = np.arange(len(pw))[:, None] < np.arange(len(pw))[None, :]
    with np.errstate(invalid="ignore"):
        before = np.where(np.isnan(pj), ~np.isnan(pi) | earlier, (pi < pj) | ((pi == pj) & earlier))
    return before.sum(axis=0).astype(np.int64)


def select(pw, ksel):
    """The ksel strongest bins in the rule's order (ascending): sel[rank - (nbin - ksel)] = bin."""
    rank = stable_rank(pw)
    sel = np.full(ksel, -1, dtype=np.int32)
    for j, r in enumerate(rank):
        if r >= len(rank) - ksel:
            sel[r - (len(rank) - ksel)] = j
    return sel


def ksel_of(k, nbin):
    return nbin if (k == 0 or k > nbin) else k


# ---- the exact tier --------------------------------------------------------------------------------------------------------------
def _poly(*factors):
    p = np.asarray([1], dtype=np.int64)
    for f in factors:
        p = np.convolve(p, np.asarray(f, dtype=np.int64))
    return [int(v) for v in p]


PHI = {2: [1, 1], 3: [1, 1, 1], 4: [1, 0, 1], 5: [1, 1, 1, 1, 1], 6: [1, -1, 1], 12: [1, 0, -1, 0, 1]}

# name -> (b, a): numerator entries in -3 .. 3, the denominator a product of cyclotomic polynomials (simple roots on the unit circle: the
# response to a bounded input grows at most linearly).  "n3_a0=2" doubles both, for the entry's normalisation by a[0].
INTEGER_FILTERS = {
    "n1": ([3], [1]),
    "n2": ([2, -1], _poly(PHI[2])),
    "n3": ([1, 0, -1], _poly(PHI[6])),
    "n4": ([1, -2, 3, 1], _poly(PHI[2], PHI[3])),
    "n5": ([2, 1, -3, 1, -1], _poly(PHI[3], PHI[4])),
    "n7": ([1, -1, 2, 3, -2, 1, -1], _poly(PHI[3], PHI[4], PHI[6])),
    "n9a": ([1, 2, -1, 3, -3, 1, -2, 1, 1], _poly(PHI[3], PHI[4], PHI[5])),
    "n9b": ([-1, 1, 3, -2, 1, 2, -3, 1, -1], _poly(PHI[5], PHI[12])),
    "n3_a0=2": ([2, 0, -2], [2 * v for v in _poly(PHI[6])]),
}


def _guard(abs_sum, what):
    """abs_sum: the float64 sum of the absolute values of a sum's terms (exact below 2^53, and never rounded to below it)."""
    worst = float(np.max(abs_sum)) if np.size(abs_sum) else 0.0
    if not worst < LIMIT:
        raise ExactRangeError(f"{what}: an intermediate may reach {worst:.4g} >= 2^53")


def _as_int(a, what):
    a = np.asarray(a)
    i = a.astype(np.int64)
    if not np.array_equal(i, a):
        raise ValueError(f"{what} is not integer")
    _guard(np.abs(i).astype(np.float64), what)
    return i


def exact_lfilter(b, a, x):
    """lfilter(b, a, x, axis=0) from zero state in integers, from the difference equation; b, a are divided by a[0] first (exactly, or
    ValueError).  Guard: sum |b_k x| + sum |a_k y| per sample, which bounds y, every partial sum and every DF2T state word."""
    b, a, x = _as_int(b, "b"), _as_int(a, "a"), _as_int(x, "x")
    if a[0] == 0 or np.any(b % a[0]) or np.any(a % a[0]):
        raise ValueError("a[0] does not divide the coefficients")
    b, a = b // a[0], a // a[0]
    y = np.zeros_like(x)
    for n in range(len(x)):
        acc = np.zeros(x.shape[1:], dtype=np.int64)
        mag = np.zeros(x.shape[1:], dtype=np.float64)
        for k in range(min(len(b), n + 1)):
            acc += b[k] * x[n - k]
            mag += np.abs(b[k] * x[n - k])
        for k in range(1, min(len(a), n + 1)):
            acc -= a[k] * y[n - k]
            mag += np.abs(a[k] * y[n - k])
        _guard(mag, f"filter at sample {n}")
        y[n] = acc
    return y


def _matmul_guarded(A, B, what):
    _guard(np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64), what)
    return A @ B


def exact_music(x, b, a, L, hop, N, W, sre, sim, k, readout=True):
    """x [B, T, M], W [N, 2 nbin], sre / sim [nbin, M, G]: integers.  -> dict(S, sel [B, S, ksel] int32, spectrum [B, S, G], power [B, G],
    argmax [B] int32, pw [B, S, nbin]) in float64, every entry the exact value (but for a division by an F or S that is no power of two:
    module docstring)."""
    x, W, sre, sim = _as_int(x, "x"), _as_int(W, "W"), _as_int(sre, "steer_re"), _as_int(sim, "steer_im")
    B, T, M = x.shape
    nbin, G = sre.shape[0], sre.shape[2]
    assert W.shape == (N, 2 * nbin) and sre.shape == sim.shape == (nbin, M, G)
    ksel = ksel_of(k, nbin)
    sl = slices(T, L, hop)
    S = len(sl)
    sel = np.zeros((B, S, ksel), dtype=np.int32)
    spec = np.zeros((B, S, G))
    pws = np.zeros((B, S, nbin))
    for s, (start, length) in enumerate(sl):
        F = length // N
        if F < 1:
            raise ValueError("a slice shorter than N")
        y = exact_lfilter(b, a, np.moveaxis(x[:, start : start + F * N, :], 1, 0))  # [F N, B, M]
        fr = np.moveaxis(y, 0, -1).reshape(B, M, F, N)
        X = _matmul_guarded(fr, W, "DFT")  # [B, M, F, 2 nbin]
        re, im = X[..., 0::2], X[..., 1::2]
        _guard(np.sum(np.abs(re).astype(np.float64) ** 2 + np.abs(im).astype(np.float64) ** 2, axis=(1, 2)), "bin power")
        psum = np.sum(re * re + im * im, axis=(1, 2))  # [B, nbin]
        pw = psum.astype(np.float64) / float(M * F)
        pws[:, s] = pw
        ar, ai = np.abs(sre).astype(np.float64), np.abs(sim).astype(np.float64)
        for i in range(B):
            sel[i, s] = select(pw[i], ksel)
            P = np.zeros(G)
            mag = np.zeros(G)
            for j in sel[i, s]:
                # conj(a) x = (ar re + ai im) + 1j (ar im - ai re), summed over the mics: [F, G]
                rj, ij = re[i, :, :, j].T, im[i, :, :, j].T  # [F, M]
                zmag = np.abs(rj).astype(np.float64) @ (ar[j] + ai[j]) + np.abs(ij).astype(np.float64) @ (ar[j] + ai[j])
                _guard(zmag, "steering sum")
                zr = rj @ sre[j] + ij @ sim[j]
                zi = ij @ sre[j] - rj @ sim[j]
                mag += np.sum(zmag**2, axis=0)
                acc = np.sum(zr * zr + zi * zi, axis=0)
                P = P + acc.astype(np.float64) / float(F)
            _guard(mag, "steering power")
            spec[i, s] = P
    out = dict(S=S, sel=sel, spectrum=spec, pw=pws)
    if readout:
        _guard(np.sum(spec**2, axis=1), "read-out (sum_s P^2)")
        p = np.zeros((B, G))
        for s in range(S):
            p = p + spec[:, s] * spec[:, s]
        out["power"] = p / float(S)
        out["argmax"] = np.argmax(out["power"], axis=1).astype(np.int32)
    return out


# ---- the probe tables ------------------------------------------------------------------------------------------------------------
def filter_probe(N, samples):
    """W [N, 2 nbin]: column 2 j is the unit vector at sample samples[j], column 2 j + 1 is zero -- X[.., bin j] = y[samples[j]] + 0j."""
    W = np.zeros((N, 2 * len(samples)))
    W[np.asarray(samples), 2 * np.arange(len(samples))] = 1.0
    return W


def delta_steering(nbin, M):
    """sre[j, m, g] = 1 iff g == j M + m, sim = 0, G = nbin M: with one frame and every bin selected P[j M + m] = |X[m, 0, bin j]|^2,
    the square of one entry of X with nothing but zeros added to it."""
    sre = np.zeros((nbin, M, nbin * M))
    for j in range(nbin):
        for m in range(M):
            sre[j, m, j * M + m] = 1.0
    return sre, np.zeros_like(sre)


def pad_W(W, N):
    """[N, 2 nbin] -> the device table [Np, Cp] (Np = N rounded up to 64, Cp = 2 nbin rounded up to 16; zero elsewhere)."""
    Np, Cp = (N + 63) // 64 * 64, (W.shape[1] + 15) // 16 * 16
    out = np.zeros((Np, Cp))
    out[:N, : W.shape[1]] = W
    return out


def ld_dft_table(N, bins):
    """W [N, 2 nbin] in long double: cos and -sin of 2 pi ((k n) mod N) / N."""
    n = np.arange(N, dtype=np.int64)
    two_pi = 2 * LD("3.14159265358979323846264338327950288")
    ang = two_pi * ((np.asarray(bins, dtype=np.int64)[None, :] * n[:, None]) % N).astype(LD) / LD(N)
    W = np.zeros((N, 2 * len(bins)), dtype=LD)
    W[:, 0::2] = np.cos(ang)
    W[:, 1::2] = -np.sin(ang)
    return W


# ---- the rounding tier -----------------------------------------------------------------------------------------------------------
def ld_lfilter(b, a, x):
    """lfilter(b, a, x, axis=0) from zero state in long double (the difference equation), and the local rounding errors eta [T, ...] of
    the float64 DF2T chain beside it (first order, not doubled): module docstring, "filter"."""
    b, a = np.asarray(b, dtype=np.float64).astype(LD), np.asarray(a, dtype=np.float64).astype(LD)
    b, a = b / a[0], a / a[0]
    n = max(len(b), len(a))
    b, a = np.concatenate([b, np.zeros(n - len(b), dtype=LD)]), np.concatenate([a, np.zeros(n - len(a), dtype=LD)])
    x = np.asarray(x, dtype=np.float64).astype(LD)
    y = np.zeros_like(x)
    eta = np.zeros_like(x)
    z = np.zeros((max(n - 1, 1),) + x.shape[1:], dtype=LD)  # the DF2T state, for the magnitudes of the local errors only
    for t in range(len(x)):
        acc = b[0] * x[t]
        for k in range(1, min(n, t + 1)):
            acc = acc + (b[k] * x[t - k] - a[k] * y[t - k])
        y[t] = acc
        eta[t] += U * (np.abs(b[0] * x[t]) + (np.abs(z[0]) if n > 1 else 0))
        for k in range(n - 1):
            nxt = z[k + 1] if k + 1 < n - 1 else 0 * z[0]
            inner = np.abs(b[k + 1] * x[t]) + np.abs(nxt)
            if t + k + 1 < len(x):
                eta[t + k + 1] += U * (inner + (inner + np.abs(a[k + 1] * y[t])))
            z[k] = b[k + 1] * x[t] + nxt - a[k + 1] * y[t]
    return y, eta


def filter_bound(a, eta):
    """2 |h| * eta along axis 0, h the impulse response of 1 / a(z) (long double) over the length of eta."""
    a = np.asarray(a, dtype=np.float64).astype(LD)
    a = a / a[0]
    T = len(eta)
    h = np.zeros(T, dtype=LD)
    for t in range(T):
        h[t] = (1 if t == 0 else 0) - sum(a[k] * h[t - k] for k in range(1, min(len(a), t + 1)))
    h = np.abs(h)
    out = np.zeros_like(eta)
    for t in range(T):
        out[t] = 2 * np.tensordot(h[: t + 1][::-1], eta[: t + 1], axes=(0, 0))
    return out


def dft_bound(fr_abs, W, Np, dfr=None):
    """fr_abs [.., N] = |frames|, W [N, C] -> 2 Np 2^-53 sum_n |xf[n]| |W[n, c]|  (+ sum_n dxf[n] |W[n, c]| for a bound dfr of the frames)."""
    Wa = np.abs(np.asarray(W)).astype(LD)
    out = 2 * Np * LD(U) * (fr_abs @ Wa)
    return out if dfr is None else out + dfr @ Wa


def steer_roundings(M, F, ksel):
    return 2 * (M + 2) + 3 + F + ksel


def ld_steer(re, im, sre, sim, sel, dre=None, dim=None):
    """re, im [M, F, nbin] (long double), sre / sim [nbin, M, G], sel: the bins in order -> (P [G], its bound [G]); dre / dim: bounds of
    re / im (the stage before), or None for exact entries."""
    M, F, _ = re.shape
    G = sre.shape[2]
    P = np.zeros(G, dtype=LD)
    mag = np.zeros(G, dtype=LD)
    prop = np.zeros(G, dtype=LD)
    for j in sel:
        ar, ai = np.asarray(sre[j]).astype(LD), np.asarray(sim[j]).astype(LD)  # [M, G]
        rj, ij = re[:, :, j].T, im[:, :, j].T  # [F, M]
        zr = rj @ ar + ij @ ai
        zi = ij @ ar - rj @ ai
        Ar = np.abs(rj) @ np.abs(ar) + np.abs(ij) @ np.abs(ai)  # [F, G]
        Ai = np.abs(ij) @ np.abs(ar) + np.abs(rj) @ np.abs(ai)
        P = P + np.sum(zr * zr + zi * zi, axis=0) / F
        mag = mag + np.sum(Ar * Ar + Ai * Ai, axis=0) / F
        if dre is not None:
            dr, di = dre[:, :, j].T, dim[:, :, j].T
            prop = prop + np.sum(2 * Ar * (dr @ np.abs(ar) + di @ np.abs(ai)) + 2 * Ai * (di @ np.abs(ar) + dr @ np.abs(ai)), axis=0) / F
    return P, 2 * steer_roundings(M, F, len(sel)) * LD(U) * mag + prop


def power_bound(spec, dspec):
    """spec, dspec [S, G] -> (power [G] = mean_s P^2, its bound)."""
    S = spec.shape[0]
    p = np.sum(spec * spec, axis=0) / S
    return p, 2 * (S + 2) * LD(U) * p + np.sum(2 * np.abs(spec) * dspec, axis=0) / S


def ld_music(x, b, a, L, hop, N, W, sre, sim, k, Np=None):
    """One trial x [T, M] through the chain in long double with the bounds beside it: W [N, 2 nbin] (the float64 table the device is
    given, or a long-double one), sre / sim [nbin, M, G].  -> dict(S, sel [S, ksel], pw [S, nbin], gap [S] (the relative distance of the
    weakest selected bin from the strongest one left out, inf when all are taken), spectrum, spectrum_bound [S, G], power, power_bound
    [G], X_err [S]: the largest bound of an entry of X relative to the largest |X| of the slice)."""
    x = np.asarray(x, dtype=np.float64)
    T, M = x.shape
    nbin, G = np.asarray(sre).shape[0], np.asarray(sre).shape[2]
    Np = (N + 63) // 64 * 64 if Np is None else Np
    ksel = ksel_of(k, nbin)
    Wl = np.asarray(W).astype(LD)
    sl = slices(T, L, hop)
    out = dict(S=len(sl), sel=[], pw=[], gap=[], spectrum=[], spectrum_bound=[], X_err=[])
    for start, length in sl:
        F = length // N
        y, eta = ld_lfilter(b, a, x[start : start + F * N])
        dy = filter_bound(a, eta)
        fr, dfr = y.T.reshape(M, F, N), dy.T.reshape(M, F, N)
        X = fr @ Wl
        dX = dft_bound(np.abs(fr), Wl, Np, dfr)
        re, im = X[..., 0::2], X[..., 1::2]
        pw = np.sum(re * re + im * im, axis=(0, 1)) / (M * F)
        order = np.argsort(pw.astype(np.float64), kind="stable")
        sel = order[nbin - ksel :]
        srt = pw[order]
        out["gap"].append(float((srt[nbin - ksel] - srt[nbin - ksel - 1]) / srt[nbin - ksel]) if ksel < nbin else np.inf)
        P, dP = ld_steer(re, im, sre, sim, sel, dX[..., 0::2], dX[..., 1::2])
        out["sel"].append(sel), out["pw"].append(pw), out["spectrum"].append(P), out["spectrum_bound"].append(dP)
        out["X_err"].append(float(np.max(dX) / np.max(np.abs(X))))
    for key in ("sel", "pw", "spectrum", "spectrum_bound"):
        out[key] = np.asarray(out[key])
    out["power"], out["power_bound"] = power_bound(out["spectrum"], out["spectrum_bound"])
    return out
