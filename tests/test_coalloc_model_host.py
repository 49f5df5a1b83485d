"""CPU only: the numpy restatement of the co-allocation summaries (coalloc_model.py) held to Python loops, to the floating-point
definition of the least-squares score in exact fractions, and to its own identities.  The GPU tests hold the kernels to it."""

from fractions import Fraction

import numpy as np
from coalloc_model import canonical, coalloc, first_argmin, flags_of, labels_of, scores


def tiny():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 3, size=(7, 5)).astype(np.float64)
    x[1, 2] = np.nan
    x[4, 0] = 0.5
    x[5, 3] = -0.0
    x[6, 1] = 3.0
    return x


def test_label_rule():
    v = np.array([0.0, -0.0, 1.0, 2.0, 3.0, 0.5, -1.0, np.nan, np.inf, -np.inf, 5e-324, 2.0 + 2.0 ** -51])
    assert labels_of(v, 3).tolist() == [0, 0, 1, 2, -2, -2, -2, -1, -2, -2, -2, -2]
    assert flags_of(labels_of(v, 3).reshape(-1, 1)).tolist() == [[1, 7]]


def test_restatement_against_a_triple_loop():
    x, K = tiny(), 3
    Z = labels_of(x, K)
    R, n = Z.shape
    plain = np.zeros((n, n), dtype=np.int64)
    per = np.zeros((K, n, n), dtype=np.int64)
    for r in range(R):
        for i in range(n):
            for j in range(n):
                if Z[r, i] >= 0 and Z[r, i] == Z[r, j]:
                    plain[i, j] += 1
                    per[Z[r, i], i, j] += 1
    assert np.array_equal(coalloc(Z, K, chunk=3), plain)
    assert np.array_equal(coalloc(Z, K, per_label=True, chunk=2), per)
    assert plain[2, 2] == R - 1 and plain[0, 0] == R - 1 and plain[1, 1] == R - 1 and plain[3, 3] == R


def test_per_label_sums_to_plain_and_its_diagonal_is_bincount():
    rng = np.random.default_rng(1)
    K = 5
    Z = rng.integers(-2, K, size=(300, 9))
    per = coalloc(Z, K, per_label=True)
    assert np.array_equal(per.sum(axis=0), coalloc(Z, K))
    for i in range(Z.shape[1]):
        col = Z[:, i]
        assert np.array_equal(per[:, i, i], np.bincount(col[col >= 0], minlength=K))


def test_score_orders_the_rows_as_the_squared_distance_does():
    rng = np.random.default_rng(2)
    K, n = 3, 6
    Z = rng.integers(0, K, size=(12, n))
    Z[3, 1] = -1
    Z = np.concatenate([Z, Z[[5, 2, 5]]])  # duplicated rows: tied scores, the minimum among them or not
    R = Z.shape[0]
    counts = coalloc(Z, K)
    sc = scores(Z, counts, R)
    dist = []
    for z in Z:  # sum over i < j of (c_ij - pi_ij)^2, exactly
        d = Fraction(0)
        for i in range(n):
            for j in range(i + 1, n):
                c = 1 if (z[i] >= 0 and z[i] == z[j]) else 0
                d += (c - Fraction(int(counts[i, j]), R)) ** 2
        dist.append(d)
    # R * distance = score + a constant: the same order, ties included
    const = {R * d - int(s) for d, s in zip(dist, sc)}
    assert len(const) == 1
    assert first_argmin(sc)[0] == first_argmin(dist)[0] == int(np.argmin(sc))
    assert sc[5] == sc[12] == sc[14] and sc[2] == sc[13]
    # a tie at the minimum: the first of equals
    Zc = np.array([[0, 0, 1, 1], [0, 1, 0, 1], [0, 0, 1, 1], [1, 1, 0, 0], [0, 0, 1, 1]])  # rows 0, 2, 3, 4: one partition
    sc = scores(Zc, coalloc(Zc, 2), 5)
    assert sc[0] == sc[2] == sc[3] == sc[4] < sc[1] and first_argmin(sc) == (0, sc[0])
    Zc = Zc[[1, 0, 2, 3, 4]]
    sc = scores(Zc, coalloc(Zc, 2), 5)
    assert first_argmin(sc) == (1, sc[1]) and int(np.argmin(sc)) == 1


def test_canonical():
    assert canonical(np.array([2, 2, 0, -1, 1, 0])).tolist() == [0, 0, 1, -1, 2, 1]
