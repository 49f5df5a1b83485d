"""The exact problems of tests/spectral_problem.py are exact: the float64 NumPy evaluation of the spectral draw equals the one in
rationals (fractions.Fraction) and the one in np.longdouble with every contraction reversed, and every sqrt(d) squares back to d
as a rational.  That is what lets tests/test_spectral_gpu.py hold the kernels to np.array_equal; a later change of the inputs
cannot quietly make them inexact.  No GPU."""

from fractions import Fraction

import numpy as np
import pytest

import spectral_problem as sp


@pytest.mark.parametrize("p", sp.FRACTION_P)
def test_exact_case_equals_the_rational_evaluation(p):
    C = 1 if p == 1 else 3
    case = sp.exact_case(p, C, 0)
    sp.assert_exact(case, fractions=True)
    for c in range(C):
        _, _, d, rt = sp.fraction_reference(case, c)
        assert all(r * r == di for r, di in zip(rt, d))
        assert all(Fraction(1) / di == Fraction(1.0 / float(di)) for di in d)  # the kernel's 1 / d is exact as well
    # the data is what the docstring says: one +-1 per row and column of V, one cycle; the grains of the vectors
    P = np.abs(case.V)
    assert np.array_equal(P.sum(axis=0), np.ones(p)) and np.array_equal(P.sum(axis=1), np.ones(p))
    if p > 2:
        assert not np.array_equal(case.V, case.V.T)
        assert np.array_equal(np.linalg.matrix_power(P.astype(np.int64), p), np.eye(p, dtype=np.int64))
        assert all(np.trace(np.linalg.matrix_power(P.astype(np.int64), k)) == 0 for k in range(1, min(p, 6)))
    assert set(np.unique(case.ev)) <= set(sp.EV_EXACT)
    for a, grain, bound in ((case.terms[0]["rhs"], 4, 2), (case.terms[1]["rhs"], 8, 2), (case.rhs_chain, 16, 1), (case.z, 16, 2)):
        assert np.array_equal(a * grain, np.rint(a * grain)) and np.abs(a).max() <= bound
    assert case.terms[2]["rhs"] is None and case.k_mat == 1


@pytest.mark.parametrize("p,C", sp.GPU_SHAPES)
def test_every_gpu_shape_is_exact(p, C):
    case = sp.get_exact(p, C)
    sp.assert_exact(case, fractions=p <= 33)
    assert sp.logdet_is_well_conditioned(case)  # the 1e-12 relative bar on the log-determinant means something


@pytest.mark.parametrize("name", list(sp.LAYOUTS))
def test_every_layout_is_exact(name):
    case = sp.get_exact(*sp.LAYOUT_SHAPE, name=name)
    sp.assert_exact(case, fractions=True)
    assert sp.logdet_is_well_conditioned(case)
    kinds = [t["kind"] for t in case.terms]
    assert kinds.index("M") == case.k_mat and kinds.count("M") == 1


def test_layouts_cover_what_they_are_named_for():
    get = lambda name: sp.get_exact(*sp.LAYOUT_SHAPE, name=name)  # noqa: E731
    assert [get(f"k_mat={k}").k_mat for k in range(4)] == [0, 1, 2, 3]
    assert all(len(get(f"k_mat={k}").terms) == 4 for k in range(4))
    assert sorted(len(get(n).terms) - 1 for n in ("one-identity", "two-identities", "k_mat=0")) == [1, 2, 3]
    assert get("identity-scale-absent").terms[0]["scale"] is None and get("matrix-scale-absent").terms[1]["scale"] is None
    assert get("rhs_chain-absent").rhs_chain is None
    # the chains differ in their scales, also where one scale is absent
    for name in sp.LAYOUTS:
        case = get(name)
        assert any(t["scale"] is not None and len(set(t["scale"])) > 1 for t in case.terms), name


def test_reference_solves_the_system_it_is_named_for():
    """The reference against a dense solve: mean = Q^-1 b, (x - mean)'Q(x - mean) = |z|^2, logdet = log det Q."""
    p, C = 33, 3
    case = sp.random_case(p, C, 0)
    E = case.V.T
    M = E @ np.diag(case.ev) @ E.T
    for c in range(C):
        x, mean, logdet = (np.asarray(v, dtype=np.float64) for v in sp.reference(case, c))
        s = [t["scale"][c] for t in case.terms]
        Q = (s[0] + s[2]) * np.eye(p) + s[1] * M
        b = s[0] * case.terms[0]["rhs"] + s[1] * case.terms[1]["rhs"] + case.rhs_chain[c]
        assert np.allclose(mean, np.linalg.solve(Q, b), rtol=0, atol=1e-12 * np.abs(mean).max())
        assert abs((x - mean) @ Q @ (x - mean) - case.z[c] @ case.z[c]) < 1e-10 * (case.z[c] @ case.z[c])
        assert abs(logdet - np.linalg.slogdet(Q)[1]) < 1e-12 * abs(logdet)
        # path-wise: the draw's whitened coordinates are z itself, in order
        w = np.sqrt((s[0] + s[2]) + s[1] * case.ev) * (E.T @ (x - mean))
        assert np.allclose(w, case.z[c], rtol=0, atol=1e-12)
