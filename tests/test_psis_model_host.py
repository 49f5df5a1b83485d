"""The numpy restatement of omc_store_psis (tests/psis_model.py) against itself at two precisions, on the columns the GPU tests
run on (no GPU needed).  The fp64 and the np.longdouble runs must agree to 1e-12 in elpd and k -- four orders inside the 1e-10 the
device is held to --, and no candidate weight of the generalised-Pareto fit may lie within 1e-6 (relative) of the 10 * 2^-52 cut
below which a candidate is dropped: on that branch a rounding could move a result, so no test case sits on it."""

import numpy as np
import pytest
from psis_model import PSIS_S_HOST, PSIS_SHAPES, column_summaries, loglik, psis, psis_inputs, tail_max_of

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).nmant <= 52, reason="np.longdouble is no wider than fp64 here")


@pytest.fixture(scope="module")
def runs():
    out = {}
    for S in PSIS_S_HOST:
        mu, y, tau = psis_inputs(S)
        ll = loglik(mu, y, tau)
        out[S] = (ll, psis(ll, tail_max_of(S), np.float64), psis(ll, tail_max_of(S), np.longdouble))
    return out


def test_every_gpu_shape_is_covered():
    assert {n * c for n, c in PSIS_SHAPES} <= set(PSIS_S_HOST)


@pytest.mark.parametrize("S", PSIS_S_HOST)
def test_fp64_agrees_with_longdouble(runs, S):
    ll, (e64, k64, t64, m64), (e80, k80, t80, m80) = runs[S]
    fin = np.isfinite(k80)
    print(S, "elpd", np.max(np.abs(e64 - e80)), "k", np.max(np.abs(k64[fin] - k80[fin]), initial=0.0), "margin", m64.min())
    assert np.array_equal(t64, t80)
    assert np.all(np.abs(e64 - e80) <= 1e-12 * np.maximum(1, np.abs(e80)))
    assert np.array_equal(np.isinf(k64), np.isinf(k80)) and np.array_equal(np.isinf(k64), t64 <= 4)
    assert np.all(np.abs(k64[fin] - k80[fin]) <= 1e-12 * np.maximum(1, np.abs(k80[fin])))
    assert min(m64.min(), m80.min()) >= 1e-6


def test_regimes_are_mixed(runs):
    """both sides of k = 0.7, tails of 4 draws or fewer at S = 5 and 6, and ties at the cut that shorten the last column's tail"""
    ks = np.concatenate([runs[S][2][1] for S in PSIS_S_HOST if S >= 25])
    assert ks.min() < 0.7 < ks[np.isfinite(ks)].max()
    for S in (5, 6):
        assert np.all(runs[S][2][2] <= 4) and np.all(np.isinf(runs[S][2][1]))
    for S in PSIS_S_HOST:
        if S >= 25:
            t = runs[S][2][2]
            assert t[8] < tail_max_of(S) and np.all(t[:8] == tail_max_of(S)), (S, t)


def test_summaries_of_a_non_finite_column():
    ll = np.array([[0.0, -1.0], [-2.0, np.inf], [-1.0, -3.0]])
    lse, mean, var = column_summaries(ll)
    assert np.isfinite(lse[0]) and np.isnan([lse[1], mean[1], var[1]]).all()
    e, k, t, _ = psis(ll, 1)
    assert np.isnan(e[1]) and np.isnan(k[1]) and t[1] == -1 and t[0] >= 0
