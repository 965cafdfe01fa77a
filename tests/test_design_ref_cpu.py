"""tests/design_ref.py against the package's host route (CPU only): the high-precision references of the two design vectors agree with
LAPACK + bisection (`_find_dc_removed_sing_vec`, svd="host") and with `np.linalg.svd` on every covariance family, the generators deliver
the gaps they promise, and the host constants K_HOST / K_LAPACK that the device tolerances of tests/test_hip_design.py are built on are
measured here."""
import numpy as np
import pytest

import design_ref as R

SIZES = {False: R.SMALL_UNIPOLAR + R.WIDE, True: R.SMALL_BIPOLAR + R.WIDE}
MODE = {False: "unipolar", True: "bipolar"}


def _families(bipolar):
    return [pytest.param(f, bipolar, id=f"{f}-{MODE[bipolar]}") for f in (R.BIPOLAR_FAMILIES if bipolar else R.UNIPOLAR_FAMILIES)]


@pytest.mark.parametrize("family,bipolar", _families(False) + _families(True))
def test_reference_equals_the_host_route(family, bipolar):
    """max(n eps, rel_prec) / gap_rel bounds the distance of the LAPACK route (bisection to 1e-13) from the reference on every column;
    gap_rel = gap / lambda_max with the gap of design_ref's docstring."""
    for C in SIZES[bipolar]:
        if not R.defined(family, C, bipolar):
            continue
        cs = R.case(family, C, bipolar)
        assert np.all(cs.gap_abs > 0) and np.all(np.abs(np.linalg.norm(cs.ref, axis=1) - 1.0) < 1e-14)
        dist = R.host_distance(family, C, bipolar)
        tol = np.maximum(C * R.EPS, R.REL_PREC) / cs.gap_rel
        print(f"{family} C={C} {MODE[bipolar]}: gap_rel {cs.gap_rel.min():.2e}  host distance {dist.max():.2e}  / tol {np.max(dist / tol):.3f}")
        assert np.all(dist <= tol), (family, C, bipolar, dist, tol)
        if bipolar:
            for u in cs.ref:
                assert R.kref_of(u)[1], "phase-convention component too close to the kernels' thresholds"
            if family in ("first0", "permdiag") and C > 2:
                assert all(R.kref_of(u)[0] != 0 for u in cs.ref)  # the fallback of the convention is really exercised


@pytest.mark.parametrize("bipolar", [False, True], ids=["unipolar", "bipolar"])
def test_host_constants(bipolar):
    """K_HOST and K_LAPACK (design_ref.py) cover the measured worst ratios and are not slack by more than 2x: the worst distance of the
    LAPACK route from the mpmath vector in units of n eps lambda_max / gap, the bisection to 1e-13 (K_HOST) and to 1e-15 (K_LAPACK)."""
    for name, pinned, rel_prec in (("K_host", R.K_HOST[bipolar], R.REL_PREC), ("K_lapack", R.K_LAPACK[bipolar], R.REL_PREC_FINE)):
        worst = {}
        for family, C in R.all_cases(bipolar, sizes=[c for c in SIZES[bipolar] if c <= 32]):
            cs = R.case(family, C, bipolar)
            ratio = R.host_distance(family, C, bipolar, rel_prec) / cs.unit(small_kernel=False)  # LAPACK decomposes C_comp itself
            worst[family] = max(worst.get(family, 0.0), float(ratio[cs.is_mp].max()))
        for family in worst:
            print(f"{name} {MODE[bipolar]} {family}: {worst[family]:.3f}")
        k = max(worst.values())
        print(f"{name} {MODE[bipolar]} = {k:.3f} (pinned: {pinned})")
        assert pinned / 2 <= k <= pinned


@pytest.mark.parametrize("bipolar", [False, True], ids=["unipolar", "bipolar"])
def test_generators_deliver_what_they_promise(bipolar):
    for C in SIZES[bipolar]:
        n_free = C // 2 if bipolar else C - 1  # order of the problem the two leading values belong to
        for family, g in R.PROMISED_GAP.items():
            cs = R.case(family, C, bipolar)
            if n_free < 2:
                assert np.all(cs.lam_second == 0.0)
                continue
            got = cs.gap_proj / cs.lam_top
            # building Q diag Q^T in float64 moves every eigenvalue by a few n eps lambda_max
            assert np.all(np.abs(got - g) <= 16 * C * R.EPS * cs.lam_max / cs.lam_top), (family, C, got)
        # rank deficiency: exact zero eigenvalues up to rounding
        M = R.covariances("rankdef", C, bipolar)[0]
        s = np.linalg.svd(R.fold(M) if bipolar else M, compute_uv=False)
        assert np.sum(s > 1e-12 * s[0]) == (max(1, (C // 2) // 2) if bipolar else max(1, C // 2))
        # near rank one: condition number about 1e12 on the leading pair
        if n_free >= 2:
            M = R.covariances("rank1", C, bipolar)[0]
            s = np.linalg.svd(R.fold(M) if bipolar else M, compute_uv=False)
            assert 1e-14 < s[1] / s[0] < 1e-10
        # DC-dominant: the rank-one term is 1e2 ... 1e6 times the rest
        f = np.array([c[0, 1] / np.mean(np.diag(c) - c[0, 1]) for c in R.covariances("dc", C, bipolar)])
        assert 30 < f[0] < 300 and 3e5 < f[-1] < 3e6
        # diagonal: the secular bisection's first midpoint is exactly 1.0
        for fam in ("diag", "permdiag"):
            for c in R.covariances(fam, C, bipolar):
                dg = np.sort(np.diag(c))[::-1]
                assert np.count_nonzero(c - np.diag(np.diag(c))) == 0 and (dg[0] + dg[1]) / 2 == 1.0
        # scaling by a power of two changes nothing but the scale
        assert R.case("wide_up", C, bipolar).ref is R.case("wide", C, bipolar).ref
        assert np.array_equal(R.covariances("dc_dn", C, bipolar) * 2.0**40, R.covariances("dc", C, bipolar))


def test_non_symmetric_fold_is_told_apart():
    """Family 7: with C21 in place of C21^T the leading vector moves by far more than any tolerance."""
    for C in (4, 14, 64):
        cs = R.case("nonsym", C, True)
        d = C // 2
        for i in range(R.N_DOA):
            c = cs.cov[i]
            wrong = (c[:d, :d] + c[d:, d:]) / 2 + 1j * ((c[:d, d:] + c[d:, :d]) / 2)
            assert R.phase_distance(np.linalg.svd(wrong)[0][:, 0], cs.ref[i]) > 1e-3


def test_residual_bounds_hold_for_the_reference():
    """The long-double residual bounds are small on the reference vectors themselves and see a perturbation of 1e-6."""
    for C in (34, 128):
        cs = R.case("wide", C, False)
        assert R.unipolar_residual(cs.cov[0], cs.ref[0], cs.gap_proj[0]) <= R.K_LAPACK[False] * cs.unit()[0]
        e = np.zeros(C)
        e[0], e[1] = 1e-6, -1e-6
        assert R.unipolar_residual(cs.cov[0], cs.ref[0] + e, cs.gap_proj[0]) > 1e-8
        cb = R.case("wide", C, True)
        assert R.bipolar_residual(cb.cov[0], cb.ref[0], cb.gap2_abs[0]) <= R.K_LAPACK[True] * cb.unit()[0]
        eb = np.zeros(C // 2, dtype=complex)
        eb[1] = 1e-6
        assert R.bipolar_residual(cb.cov[0], cb.ref[0] + eb, cb.gap2_abs[0]) > 1e-8
