"""The guard of tests/test_mh_exact_gpu.py: every case that file holds to np.array_equal is shown here, on the host, to be exact
in float64 (mh_exact_problem.assert_exact), to contain both outcomes of the decision, and to keep every decision a margin away
from its uniform.  A GPU case can therefore never run on data where bit equality would be unjustified."""

import numpy as np
import pytest

import mh_exact_problem as P


def _id(c):
    kind, d, C, step, steps, with_mu = c
    return f"{kind}-d{d}-C{C}-step{step:g}-n{steps}-{'mu' if with_mu else 'nomu'}"


@pytest.mark.parametrize("d", [1, 2, 33, 130, 513, 1025])
def test_factor_is_dyadic_dense_and_inverts_exactly(d):
    prob = P.build(d, 0)
    L, Linv = prob.L, prob.Linv
    assert np.array_equal(L * 2, np.rint(L * 2)) and np.array_equal(Linv * 2, np.rint(Linv * 2))
    assert np.all(np.diag(L) > 0) and np.abs(L).max() <= 4 and np.abs(Linv).max() <= 4
    assert prob.sumlogL == pytest.approx(np.log(np.diag(L)).sum(), abs=1e-9)
    assert np.array_equal(prob.mu * 4, np.rint(prob.mu * 4)) and np.abs(prob.mu).max() <= 2
    if d >= 33:
        fill = np.count_nonzero(L) / (d * (d + 1) / 2)
        assert 0.35 < fill < 0.65, fill
        assert np.count_nonzero(Linv) / (d * (d + 1) / 2) > 0.35


@pytest.mark.parametrize("case", P.step_cases() + P.run_cases(), ids=_id)
def test_case_is_exact_and_decided_with_margin(case):
    c = P.get_case(*case)
    c.check_decisions()
    P.assert_exact(c)


def test_pick_uniforms_forces_what_it_can():
    la = np.array([5.0, -5.0, -2000.0, 0.0, -1e-2])
    u = P.pick_uniforms(la, np.array([False, True, True, False, False]))
    ok = np.log(u) < la
    assert ok.tolist() == [True, True, False, True, False]
    assert np.abs(np.log(u) - la).min() > 1e-3


def test_routes_agree_on_exact_data():
    """The products route and the whitened route form the same sums on exact data: same odds, same states."""
    for kind_a, kind_b, step in (("mala", "mala_white", 2.0), ("rw", "rw_white", 0.5)):
        a = P.get_case(kind_a, 33, 33, step, 4)
        b = P.get_case(kind_b, 33, 33, step, 4)
        assert np.array_equal(a.u, b.u)
        for ra, rb in zip(a.trace, b.trace):
            assert np.array_equal(ra["x"], rb["x"]) and np.array_equal(ra["log_alpha"], rb["log_alpha"])


@pytest.mark.parametrize("d", [137, 500])
@pytest.mark.parametrize("kind", ["mala_white", "mala", "rw", "rw_white"])
def test_float_case_decides_alike_in_both_precisions(kind, d):
    """The float-data cases of the GPU file: both outcomes at every step, the margin on the np.longdouble reference, the float64
    restatement deciding alike and staying within rounding of the reference."""
    c = P.get_float_case(kind, d)
    c.check_decisions()
    for rl, r64 in zip(c.trace_ld, c.trace_64):
        err = np.abs(r64["x"] - rl["x"]).max()
        assert err < 1e-9 * np.abs(r64["x"]).max(), err
