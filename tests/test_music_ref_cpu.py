"""tests/music_ref.py, the reference of the MUSIC stage tests (tests/test_hip_music_stages.py), checked on the CPU: its two tiers against
float64 restatements, its rank rule against np.argsort and against the text of csrc/music_rows.h, its integer filters against its guard."""
import itertools
import os
import re

import numpy as np
import pytest
from scipy.signal import butter, lfilter

import music_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ---- the rank rule ---------------------------------------------------------------------------------------------------------------
def _vectors(max_len=6, values=(0.0, 1.0, NAN)):
    for n in range(1, max_len + 1):
        yield from itertools.product(values, repeat=n)


def test_rank_rule_is_numpys_stable_argsort_with_nans_and_ties():
    count = 0
    for pw in _vectors():
        order = np.argsort(np.asarray(pw), kind="stable")
        rank = R.stable_rank(pw)
        assert sorted(rank) == list(range(len(pw))), pw  # a permutation: every position of sel has one writer
        assert np.array_equal(order[rank], np.arange(len(pw))), pw
        for ksel in range(1, len(pw) + 1):
            assert np.array_equal(R.select(pw, ksel), order[len(pw) - ksel :]), (pw, ksel)
        count += 1
    assert count == sum(3**n for n in range(1, 7))
    rng = np.random.RandomState(0)
    for n in range(9, 40):  # (longer vectors are counted for all pairs at once)
        pw = rng.choice([0.0, 1.0, 2.0, NAN, np.inf], size=n)
        order = np.argsort(pw, kind="stable")
        assert np.array_equal(order[R.stable_rank(pw)], np.arange(n)) and np.array_equal(R.select(pw, n // 2), order[n - n // 2 :])
    # +Inf is a number: it ties with itself by index and stands before a NaN
    assert np.array_equal(R.select([np.inf, NAN, np.inf, 1.0], 4), [3, 0, 2, 1])


def _device_rank_rule():
    """music_bin_rank's counting expression (csrc/music_rows.h) as a Python function of (pi, i, p, j)."""
    text = open(os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc", "music_rows.h")).read()
    body = text[text.index("int music_bin_rank(") :]
    body = body[: body.index("return rank;")]
    assert re.search(r"const bool pnan = p != p;", body)
    m = re.search(r"rank \+= pnan \? (.*) : (.*);", body)
    assert m, "the rank count is no longer `rank += pnan ? <NaN rule> : <number rule>;`"
    py = [s.replace("||", " or ").replace("&&", " and ") for s in m.groups()]
    assert all(re.fullmatch(r"[\sa-z()<>=]+", s) for s in py), py  # names, comparisons and brackets only
    return lambda pi, i, p, j: bool(eval(py[0] if p != p else py[1], {}, dict(pi=pi, i=i, p=p, j=j)))


def test_the_header_counts_by_the_same_rule():
    before = _device_rank_rule()
    for pw in _vectors(max_len=5, values=(0.0, 1.0, NAN, np.inf)):
        rank = [sum(before(pi, i, pw[j], j) for i, pi in enumerate(pw)) for j in range(len(pw))]  # (the kernel counts i == j as well)
        assert np.array_equal(rank, R.stable_rank(pw)), pw


# ---- the exact tier --------------------------------------------------------------------------------------------------------------
def test_integer_filters_stay_below_the_guard_and_lfilter_reproduces_them():
    rng = np.random.RandomState(1)
    x = rng.randint(-8, 9, size=(1100, 3))
    assert sorted(len(a) for _, a in R.INTEGER_FILTERS.values()) == [1, 2, 3, 3, 4, 5, 7, 9, 9]
    for name, (b, a) in R.INTEGER_FILTERS.items():
        assert max(abs(v) for v in b) <= 3 * abs(a[0]) and len(b) == len(a)
        y = R.exact_lfilter(b, a, x)  # (raises at 2^53)
        print(f"{name}: max |y| = {int(np.abs(y).max())} over 1100 samples of |x| <= 8")
        assert np.abs(y).max() < 2**20
        assert np.array_equal(lfilter(np.asarray(b, dtype=float), np.asarray(a, dtype=float), x.astype(float), axis=0), y), name
    with pytest.raises(ValueError):
        R.exact_lfilter([1, 1], [2, 2], x)
    with pytest.raises(R.ExactRangeError):
        R.exact_lfilter([1], [1, -2], np.ones((60, 1), dtype=np.int64))  # y doubles every sample


def _float64_chain(x, b, a, L, hop, N, W, sre, sim, k):
    """The chain in float64 with SciPy and NumPy: one trial x [T, M] -> (sel, spectrum, power, argmax)."""
    nbin = sre.shape[0]
    ksel = R.ksel_of(k, nbin)
    sels, spec = [], []
    for start, length in R.slices(len(x), L, hop):
        F = length // N
        y = lfilter(np.asarray(b, dtype=float), np.asarray(a, dtype=float), x[start : start + F * N].astype(float), axis=0)
        X = y.T.reshape(x.shape[1], F, N) @ W.astype(float)
        Xc = X[..., 0::2] + 1j * X[..., 1::2]  # [M, F, nbin]
        pw = np.mean(Xc.real**2 + Xc.imag**2, axis=(0, 1))
        sel = np.argsort(pw, kind="stable")[nbin - ksel :]
        P = np.zeros(sre.shape[2])
        for j in sel:
            z = np.conj(sre[j] + 1j * sim[j]).T @ Xc[:, :, j]  # [G, F]
            P = P + np.mean(z.real**2 + z.imag**2, axis=-1)
        sels.append(sel), spec.append(P)
    spec = np.asarray(spec)
    power = np.mean(spec**2, axis=0)
    return np.asarray(sels), spec, power, int(np.argmax(power))


@pytest.mark.parametrize("name", ["n1", "n3", "n4", "n9b", "n3_a0=2"])
def test_exact_tier_equals_float64_scipy_and_numpy_bit_for_bit(name):
    rng = np.random.RandomState(7)
    B, T, M, L, hop, N, nbin, G, k = 2, 150, 3, 64, 40, 16, 5, 9, 2  # F = 4, S = 3 full slices + no leftover (30 <= 32) -> S = 3
    b, a = R.INTEGER_FILTERS[name]
    x = rng.randint(-2, 3, size=(B, T, M))
    W = rng.randint(-1, 2, size=(N, 2 * nbin))
    sre, sim = rng.randint(-1, 2, size=(nbin, M, G)), rng.randint(-1, 2, size=(nbin, M, G))
    ref = R.exact_music(x, b, a, L, hop, N, W, sre, sim, k)
    assert ref["S"] == 3 and ref["sel"].shape == (B, 3, k)
    for i in range(B):
        sel, spec, power, am = _float64_chain(x[i], b, a, L, hop, N, W, sre, sim, k)
        assert np.array_equal(sel, ref["sel"][i]) and np.array_equal(spec, ref["spectrum"][i])
        # S = 3: one rounding per addition in either chain
        assert np.allclose(power, ref["power"][i], rtol=2.0**-51, atol=0) and am == ref["argmax"][i]
    with pytest.raises(R.ExactRangeError):
        R.exact_music(x * 2**18, b, a, L, hop, N, W, sre, sim, k)
    ok = R.exact_music(x, b, a, L, hop, N, W, 4 * sre, 4 * sim, k, readout=False)
    assert np.array_equal(ok["spectrum"], 16 * ref["spectrum"])


def test_exact_tier_guards_the_read_out_square():
    # one frame of two samples, one bin, one direction: P = 2 (3 * 2^12)^2 = 18 * 2^24 < 2^53, P^2 is not
    x = np.full((1, 2, 1), 3)
    W = np.full((2, 2), 2**11)
    one = np.ones((1, 1, 1), dtype=np.int64)
    assert R.exact_music(x, [1], [1], 2, 2, 2, W, one, 0 * one, 0, readout=False)["spectrum"][0, 0, 0] == 2.0 * (3 * 2**12) ** 2
    with pytest.raises(R.ExactRangeError, match="read-out"):
        R.exact_music(x, [1], [1], 2, 2, 2, W, one, 0 * one, 0)


def test_slices_are_the_packages():
    from haghighatshoarmuir2024_amd.streaming import MusicStreamingLocalizer as Loc

    for T, L, hop in itertools.product((1, 31, 32, 33, 64, 100, 161, 950), (32, 64, 71), (1, 17, 32, 64)):
        if hop > L:
            continue
        full, left = Loc.slices_of(T, L, hop)
        assert R.slices(T, L, hop) == [(s * hop, L) for s in range(full)] + ([left] if left else []), (T, L, hop)


# ---- the rounding tier -----------------------------------------------------------------------------------------------------------
def test_long_double_chain_agrees_with_the_float64_restatement_within_its_own_bound():
    from test_hip_music import _numpy_music

    fs, M, N, L, hop, G, k = 8000, 3, 64, 200, 150, 7, 2
    rng = np.random.RandomState(3)
    T = 2 * hop + L - 20  # two full slices and a leftover of 130 > 100 samples with 2 frames (< 3)
    t = np.arange(T) / fs
    x = 0.3 * rng.randn(T, M) + np.sin(2 * np.pi * 1300.0 * t[:, None] + rng.uniform(0, 6, M)[None, :])
    band = (1000.0, 1500.0)
    b, a = butter(1, band, btype="bandpass", fs=fs)
    fv = np.linspace(0, fs, N)
    bins = np.nonzero((band[0] <= fv) & (fv <= band[1]))[0]
    assert len(bins) == 4
    steer = np.exp(-1j * 2 * np.pi * fv[bins][:, None, None] * rng.uniform(-2e-4, 2e-4, (1, M, G)))
    ref = R.ld_music(x, b, a, L, hop, N, R.ld_dft_table(N, bins), steer.real, steer.imag, k)
    assert ref["S"] == 3 and min(ref["gap"]) > 1e-6
    spec, sels, _ = _numpy_music(x, b, a, L, hop, 3, N, k, fs, band, steer)
    assert np.array_equal(np.asarray(sels), ref["sel"])
    err = np.abs(spec - ref["spectrum"])
    print(f"float64 restatement: worst spectrum error / bound {float(np.max(err / ref['spectrum_bound'])):.3f}, worst error relative to the "
          f"maximum {float(err.max() / ref['spectrum'].max()):.2e}, worst bound {float((ref['spectrum_bound'] / ref['spectrum'].max()).max()):.2e}")
    assert np.all(err <= ref["spectrum_bound"]) and err.max() > 0
    perr = np.abs(np.mean(spec**2, axis=0) - ref["power"])
    assert np.all(perr <= ref["power_bound"])
    # the bound is a bound of rounding, not a tolerance: a relative slip of 1e-9 anywhere is far outside it
    assert np.all(ref["spectrum_bound"] < 1e-11 * ref["spectrum"].max())


def test_long_double_filter_bound_holds_for_float64_lfilter():
    rng = np.random.RandomState(4)
    x = rng.randn(256, 2)
    for order in (1, 2, 3, 4):
        b, a = butter(order, (1000.0, 2000.0), btype="bandpass", fs=8000)
        assert len(a) == 2 * order + 1
        y, eta = R.ld_lfilter(b, a, x)
        bound = R.filter_bound(a, eta)
        err = np.abs(lfilter(b, a, x, axis=0) - y)
        print(f"order {order}: float64 lfilter error / bound {float(np.max(err[1:] / bound[1:])):.3f}, max error {float(err.max()):.2e}")
        assert np.all(err <= bound)


def test_dft_table_and_bound():
    N, bins = 96, np.asarray([5, 17, 40])
    Wl = R.ld_dft_table(N, bins)
    n = np.arange(N)
    ang = 2 * np.pi * ((bins[None, :] * n[:, None]) % N) / N
    assert np.max(np.abs(Wl[:, 0::2] - np.cos(ang))) <= 20 * R.U and np.max(np.abs(Wl[:, 1::2] + np.sin(ang))) <= 20 * R.U
    assert Wl[0, 0] == 1 and Wl[0, 1] == 0 and Wl[24, 1::2][2] == 0  # 40 * 24 = 10 N: the index is reduced before the angle
    x = np.random.RandomState(5).randn(4, N)
    err = np.abs(x @ Wl.astype(float) - x.astype(R.LD) @ Wl)
    assert np.all(err <= R.dft_bound(np.abs(x).astype(R.LD), Wl, 128))
    P = R.pad_W(np.ones((N, 6)), N)
    assert P.shape == (128, 16) and P[:N, :6].all() and P.sum() == 6 * N
