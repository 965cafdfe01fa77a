"""The design kernels of csrc/design.hip (micloc_design_vectors_f64: `design_vec_kernel`, two-sided Jacobi, C <= 32; `design_vec_wide_kernel`,
one-sided Jacobi, 32 < C <= 128) handed matrices directly, against the high-precision references of tests/design_ref.py: mpmath at 40
digits up to C = 32, float64 LAPACK on a long-double projection plus a long-double residual bound beyond.

Tolerance per column: 8 K_host n eps lambda_max / gap (the small bipolar kernel, which decomposes C_comp C_comp^H: sigma0^2 / (sigma0^2 -
sigma1^2) in place of lambda_max / gap), gap as design_ref's docstring defines it.  K_host is measured by tests/test_design_ref_cpu.py on the
host route (LAPACK, the bisection to the 1e-13 these tests use) against mpmath:

    K_host   unipolar 61.1 (n = 2, where the bisection's 1e-13 is 225 n eps; 8 or less from n = 14 on)    bipolar 0.60
    K_lapack unipolar 1.72 (the host's bisection run to 1e-15: LAPACK's own error)                         bipolar 0.60

The 8 allows for Jacobi's other rotation order and the kernels' unfused sums.  K_lapack is the base of the rel_prec tests: there the
tolerance is 8 K_lapack n eps lambda_max / gap + 4 rel_prec lam_top / gap, which at rel_prec = 1e-15 pins the eigen-solvers themselves."""
import functools

import numpy as np
import pytest

import design_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 8.0
MODE = {False: "unipolar", True: "bipolar"}
SIZES = {("small", False): R.SMALL_UNIPOLAR, ("small", True): R.SMALL_BIPOLAR, ("wide", False): R.WIDE, ("wide", True): R.WIDE}


def launch(cov, bipolar, rel_prec=R.REL_PREC):
    """One launch; columns written at g0 = 1 of a [C, n + 2] tensor whose outer columns have to stay zero."""
    import torch

    from haghighatshoarmuir2024_amd import runtime

    n, C, _ = cov.shape
    out = torch.zeros((C, n + 2), dtype=torch.float64, device="cuda")
    runtime.design_vectors(torch.from_numpy(np.ascontiguousarray(cov)).cuda(), bipolar, out, 1, rel_prec=rel_prec)
    W = out.cpu().numpy()
    assert not W[:, 0].any() and not W[:, -1].any(), "a column outside g0 .. g0 + n was written"
    return W[:, 1:-1]


@functools.lru_cache(maxsize=None)
def device(family, C, bipolar, rel_prec=R.REL_PREC):
    return launch(R.covariances(family, C, bipolar), bipolar, rel_prec)


def check(cs, W, tol, columns=None, residual=True):
    """Every assertion on the columns W [C, N_DOA] of one case -> (failures, worst distance / (n eps lambda_max / gap)).  The residual
    bound overstates a distance that lies along well separated directions by up to lam_top / gap, which is what a coarse bisection
    produces: it is asserted where the decomposition dominates the error (rel_prec <= 1e-13), not in the coarse rel_prec tests."""
    C, d = cs.C, cs.C // 2
    fails, worst = [], 0.0
    ok = R.compared(cs.family, C, cs.bipolar)
    unit = cs.unit()
    for i in range(R.N_DOA) if columns is None else columns:
        if not ok[i]:
            continue
        w, tag = W[:, i], f"{cs.family} C={C} {MODE[cs.bipolar]} column {i}"
        if not np.all(np.isfinite(w)):
            fails.append(f"{tag}: not finite")
            continue
        nrm = float(np.linalg.norm(w))
        if abs(nrm - 1.0) > 1e-12:
            fails.append(f"{tag}: norm - 1 = {nrm - 1.0:.2e}")
        if not cs.bipolar:
            dist = float(np.linalg.norm(w - cs.ref[i]))  # sign included: the conditional vector has no sign freedom
            if abs(np.sum(w)) > tol[i] * np.sqrt(C):
                fails.append(f"{tag}: |sum w| = {abs(np.sum(w)):.2e} > {tol[i] * np.sqrt(C):.2e}")
            res = R.unipolar_residual(cs.cov[i], w, cs.gap_proj[i]) if C > 32 and residual else 0.0
        else:
            wc = w[:d] + 1j * w[d:]
            dist = R.phase_distance(wc, cs.ref[i])
            k = R.kref_of(cs.ref[i])[0]
            if not (wc[k].real < 0 and abs(wc[k].imag) <= 1e-12):
                fails.append(f"{tag}: phase convention, component {k} = {wc[k]}")
            res = R.bipolar_residual(cs.cov[i], wc, cs.gap2_abs[i]) if C > 32 and residual else 0.0
        worst = max(worst, dist / unit[i])
        if dist > tol[i]:
            fails.append(f"{tag}: distance {dist:.3e} > tol {tol[i]:.3e} ({dist / unit[i]:.1f} units, gap_rel {cs.gap_rel[i]:.1e})")
        if res > tol[i]:
            fails.append(f"{tag}: long-double residual bound {res:.3e} > tol {tol[i]:.3e}")
    return fails, worst


def _params(families_of):
    return [pytest.param(f, b, k, id=f"{f}-{MODE[b]}-{k}") for b in (False, True) for k in ("small", "wide") for f in families_of(b)]


@pytest.mark.parametrize("family,bipolar,kernel", _params(lambda b: R.BIPOLAR_FAMILIES if b else R.UNIPOLAR_FAMILIES))
def test_design_vectors_against_reference(family, bipolar, kernel):
    """Every family at every size of one kernel and mode, six columns a launch: unit norm, distance from the reference (unipolar: sign
    included; bipolar: up to the phase, whose convention is checked on the component the reference names), |sum w|, residual bound."""
    fails, worst = [], 0.0
    for C in SIZES[kernel, bipolar]:
        if not R.defined(family, C, bipolar):
            continue
        cs = R.case(family, C, bipolar)
        f, w = check(cs, device(family, C, bipolar), FACTOR * R.K_HOST[bipolar] * cs.unit())
        fails += f
        worst = max(worst, w)
    print(f"device/host {family} {MODE[bipolar]} {kernel}: worst distance = {worst:.3f} units = {worst / R.K_HOST[bipolar]:.3f} K_host (limit {FACTOR:g})")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rel_prec,families", [(1e-15, R.UNIPOLAR_FAMILIES), (1e-8, ("wide", "dc")), (1e-4, ("wide", "dc"))],
                         ids=["1e-15", "1e-8-default", "1e-4-reference-default"])
@pytest.mark.parametrize("kernel", ["small", "wide"])
def test_rel_prec(rel_prec, families, kernel):
    """The bisection's stopping rule: the distance grows by no more than 4 rel_prec lam_top / gap.  At 1e-15 (every family) that term is a
    few n eps: what is left is the eigen-solver, held to 8 times LAPACK's own error."""
    fails, worst = [], 0.0
    for family in families:
        for C in SIZES[kernel, False]:
            cs = R.case(family, C, False)
            tol = FACTOR * R.K_LAPACK[False] * cs.unit() + 4 * rel_prec * cs.lam_top / cs.gap_abs
            f, w = check(cs, device(family, C, False, rel_prec), tol, residual=rel_prec <= R.REL_PREC)
            fails += f
            worst = max(worst, w)
    print(f"rel_prec {rel_prec:g} {kernel}: worst distance = {worst:.3f} units = {worst / R.K_LAPACK[False]:.3f} K_lapack")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("bipolar", [False, True], ids=["unipolar", "bipolar"])
@pytest.mark.parametrize("C", [14, 64])
def test_mixed_launch(C, bipolar):
    """70 workgroups of different families in one launch: every column has the bits of its own family's launch of six (a workgroup's LDS
    state does not leak into its neighbour) and passes the same checks."""
    fams = [f for f in (R.BIPOLAR_FAMILIES if bipolar else R.UNIPOLAR_FAMILIES) if R.defined(f, C, bipolar)]
    picks = [(f, i) for i in range(R.N_DOA) for f in fams][:70]  # interleaved: neighbours are of different families
    assert len(picks) == 70
    W = launch(np.stack([R.covariances(f, C, bipolar)[i] for f, i in picks]), bipolar)
    fails = []
    for col, (f, i) in enumerate(picks):
        if not np.array_equal(W[:, col], device(f, C, bipolar)[:, i]):
            fails.append(f"{f} column {i} (workgroup {col}): differs from its own launch by {np.max(np.abs(W[:, col] - device(f, C, bipolar)[:, i])):.2e}")
        cs = R.case(f, C, bipolar)
        Wf = np.zeros((C, R.N_DOA))
        Wf[:, i] = W[:, col]
        fails += check(cs, Wf, FACTOR * R.K_HOST[bipolar] * cs.unit(), columns=[i])[0]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("C", [3, 14, 32, 34, 64, 128])
def test_diagonal_bisection_midpoint_one(C):
    """diag(1.5, 0.5, 0.25, ...), in place and permuted: no rotation at all, and the first midpoint of the secular bisection is exactly
    1.0 -- where a thread past n that divides 0 by (1.0 - u_mid) turns the sum into NaN and the bisection the wrong way (the wide kernel
    before its padding threads added zero: |sum w| = 5.07 and distance 1.03 from the reference at C = 34, 7.28 and 1.13 at C = 62)."""
    fails = []
    for family in ("diag", "permdiag"):
        cs = R.case(family, C, False)
        W = device(family, C, False)
        fails += check(cs, W, FACTOR * R.K_HOST[False] * cs.unit())[0]
        overlap = np.abs(np.sum(W * cs.ref.T, axis=0))
        print(f"{family} C={C}: |sum w| {np.max(np.abs(W.sum(axis=0))):.2e}  overlap with the reference {overlap.min():.6f}")
    assert not fails, "\n".join(fails)


def test_power_of_two_scaling():
    """Families 1 and 2 times 2^-40 and 2^40: the expected vector does not change (checked with every other family above); says whether
    the device result is bit-identical to the unscaled one."""
    for bipolar in (False, True):
        same = total = 0
        for base in ("wide", "dc"):
            for C in SIZES["small", bipolar] + R.WIDE:
                for tag in ("_dn", "_up"):
                    eq = np.all(device(base + tag, C, bipolar) == device(base, C, bipolar), axis=0)
                    same, total = same + int(eq.sum()), total + eq.size
        print(f"power-of-two scaling, {MODE[bipolar]}: {same} of {total} columns bit-identical to the unscaled result")
        assert total > 0


def test_coverage():
    """Only gap = 1e-5 columns on which the LAPACK route itself is further than 1e-6 from the reference may be left out: at least 95 %
    of all generated columns are compared."""
    total = done = 0
    for bipolar in (False, True):
        for family, C in R.all_cases(bipolar):
            ok = R.compared(family, C, bipolar)
            total, done = total + ok.size, done + int(ok.sum())
    print(f"{done} of {total} generated columns compared")
    assert done >= 0.95 * total
