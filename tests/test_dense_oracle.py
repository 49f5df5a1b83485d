"""oracle.longdouble_ref.dense_draw, the extended-precision yardstick of tests/test_dense_edges_gpu.py: pinned against
a factorisation small enough to check by hand, against the fp64 oracle on well-conditioned matrices, and against the exact
index of the first failing pivot on constructed failures.  CPU only."""

import numpy as np
import pytest

from oracle import gmrf_ref
from oracle.longdouble_ref import dense_draw


def test_longdouble_is_wider_than_double():
    """The yardstick is only one if longdouble carries more than 53 bits (x87: 64)."""
    assert np.finfo(np.longdouble).eps < 2.0**-60


def test_three_by_three_with_an_integer_factor_is_exact():
    """Q = L L' with L = [[2,0,0],[6,1,0],[-8,5,3]] (Q = [[4,12,-16],[12,37,-43],[-16,-43,98]]): every intermediate of
    the factorisation and of the solves below is a small integer or a dyadic fraction, so every output is exact."""
    L0 = np.array([[2.0, 0.0, 0.0], [6.0, 1.0, 0.0], [-8.0, 5.0, 3.0]])
    Q = np.array([[4.0, 12.0, -16.0], [12.0, 37.0, -43.0], [-16.0, -43.0, 98.0]])
    assert np.array_equal(L0 @ L0.T, Q)
    mu0 = np.array([1.0, -2.0, 3.0])
    b = Q @ mu0                      # [-68, -191, 364]
    z = np.array([2.0, -4.0, 6.0])   # L' d = z: d3 = 2, d2 = -4 - 5*2 = -14, d1 = (2 - 6*(-14) + 8*2) / 2 = 51
    x, mu, logdet, L = dense_draw(Q, b, z)
    assert L.dtype == np.longdouble
    assert np.array_equal(L.astype(np.float64), L0)
    assert np.array_equal(mu, mu0)
    assert np.array_equal(x, mu0 + np.array([51.0, -14.0, 2.0]))
    assert logdet == pytest.approx(2 * np.log(6.0), rel=1e-15)
    # only the lower triangle is read
    Qlow = np.tril(Q) + np.triu(np.full((3, 3), np.nan), 1)
    x2, mu2, logdet2, _ = dense_draw(Qlow, b, z)
    assert np.array_equal(x2, x) and np.array_equal(mu2, mu) and logdet2 == logdet


@pytest.mark.parametrize("p", [1, 2, 17, 64, 65, 200])
def test_agrees_with_the_fp64_oracle_on_well_conditioned_matrices(p):
    """Condition number below 10: the fp64 route is good to a few p * 2^-53, and so must the agreement be."""
    rng = np.random.default_rng(p)
    A = rng.standard_normal((p, p))
    Q = A @ A.T + p * np.eye(p)
    b, z = rng.standard_normal(p), rng.standard_normal(p)
    x, mu, logdet, L = dense_draw(Q, b, z)
    xo, mo, Lo = gmrf_ref.draw_canonical(b.reshape(p, 1), Q, z.reshape(p, 1))
    tol = 64 * p * 2.0**-53
    assert np.max(np.abs(x - xo.ravel())) <= tol * np.max(np.abs(xo))
    assert np.max(np.abs(mu - mo.ravel())) <= tol * np.max(np.abs(mo))
    assert abs(logdet - 2 * np.sum(np.log(np.diag(Lo)))) <= tol * max(1.0, abs(logdet))
    assert np.max(np.abs(L.astype(np.float64) - Lo)) <= tol * np.max(np.abs(Lo))
    assert np.array_equal(np.triu(L, 1), np.zeros((p, p), dtype=np.longdouble))
    # the factor reproduces Q to longdouble rounding (far below fp64's)
    R = L @ L.T - Q.astype(np.longdouble)
    assert float(np.max(np.abs(R))) <= p * 2.0**-60 * np.max(np.abs(Q))


@pytest.mark.parametrize("p,k", [(1, 0), (5, 0), (5, 4), (70, 1), (70, 63), (70, 64), (70, 65), (70, 69), (300, 200)])
def test_first_failing_pivot_is_reported_under_its_index(p, k):
    """Q = L0 L0' with 2 L0[k,k]^2 taken off Q[k,k]: the leading k x k block is untouched and positive definite, pivot k
    comes out as -L0[k,k]^2 < 0 and is the first to fail."""
    rng = np.random.default_rng(100 * p + k)
    L0 = np.tril(rng.standard_normal((p, p))) / np.sqrt(p)
    L0[np.diag_indices(p)] = 1.0 + rng.random(p)
    Q = L0 @ L0.T
    dense_draw(Q, np.ones(p), np.zeros(p))  # healthy as built
    Q[k, k] -= 2 * L0[k, k] ** 2
    with pytest.raises(np.linalg.LinAlgError, match=f"pivot {k}\\b") as info:
        dense_draw(Q, np.ones(p), np.zeros(p))
    assert info.value.pivot == k
    if k > 0:  # and the block above it still factorises
        dense_draw(Q[:k, :k], np.ones(k), np.zeros(k))


def test_nan_and_zero_pivots_fail_and_shapes_are_checked():
    Q = np.eye(4)
    Q[2, 2] = 0.0
    with pytest.raises(np.linalg.LinAlgError) as info:
        dense_draw(Q, np.ones(4), np.zeros(4))
    assert info.value.pivot == 2
    Q[1, 1] = np.nan
    with pytest.raises(np.linalg.LinAlgError) as info:
        dense_draw(Q, np.ones(4), np.zeros(4))
    assert info.value.pivot == 1
    with pytest.raises(ValueError):
        dense_draw(np.eye(4), np.ones(3), np.zeros(4))
