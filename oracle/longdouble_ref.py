"""Extended-precision restatements of the tridiagonal and the dense canonical draw (test infrastructure, never shipped).

The same recurrences as gmrf.sample_normal_canonical on a tridiagonal Q (factor gmrf.py:489-520, solves
gmrf.py:414-462, draw gmrf.py:29-61), carried in numpy.longdouble (x87 80-bit on the x86 hosts here and on the GPU
box: 64-bit mantissa, eps 1.1e-19).  It is the yardstick for weakly contractive chains (lambda/tau >> 1), where the
fp64 oracle itself is only good to eps * cond(Q): with it the tests can say how far the fp64 sequential algorithm
and the GPU kernel each are from the exact-arithmetic answer, instead of loosening a tolerance on faith.
"""

import numpy as np


def tridiag_draw(a, b, r, z):
    """a (n,) diagonal, b (n-1,) off-diagonal of Q; r (n,) right-hand side; z (n,) N(0,1) draws.
    Returns x = Q^-1 r + L^-T z, mu = Q^-1 r, log det Q as float64 values computed in longdouble."""
    ld = np.longdouble
    a, b, r, z = (np.asarray(v, dtype=ld) for v in (a, b, r, z))
    n = a.size
    D = np.empty(n, dtype=ld)
    l = np.zeros(n, dtype=ld)
    u = np.empty(n, dtype=ld)
    D[0], u[0] = a[0], r[0]
    for i in range(1, n):
        l[i - 1] = b[i - 1] / D[i - 1]
        D[i] = a[i] - l[i - 1] * b[i - 1]
        u[i] = r[i] - l[i - 1] * u[i - 1]
    if np.any(D <= 0):
        raise np.linalg.LinAlgError("not positive definite")
    g = u / D + z / np.sqrt(D)
    m = u / D
    x = np.empty(n, dtype=ld)
    mu = np.empty(n, dtype=ld)
    x[-1], mu[-1] = g[-1], m[-1]
    for i in range(n - 2, -1, -1):
        x[i] = g[i] - l[i] * x[i + 1]
        mu[i] = m[i] - l[i] * mu[i + 1]
    return x.astype(np.float64), mu.astype(np.float64), float(np.sum(np.log(D)))


def dense_draw(Q, b, z):
    """Q (p, p) symmetric (only the lower triangle is read), b (p,) right-hand side, z (p,) N(0,1) draws.

    The dense branch of gmrf.sample_normal_canonical (factor gmrf.py:481: np.linalg.cholesky, natural order, no
    pivoting; solves gmrf.py:437-462; draw gmrf.py:29-61) in longdouble: Cholesky column by column (the inner products of
    a column in one vectorised product), forward and backward substitution.  Returns
        x = Q^-1 b + L^-T z, mu = Q^-1 b   (float64, rounded once from the longdouble result),
        log det Q = 2 sum log L_ii         (float),
        L                                  (p, p) lower factor, kept in longdouble.
    A non-positive (or NaN) pivot raises numpy.linalg.LinAlgError whose attribute `pivot` is the 0-based index of the
    first such pivot: the leading pivot x pivot block is positive definite, the one a row larger is not."""
    ld = np.longdouble
    A = np.asarray(Q, dtype=ld)
    b, z = np.asarray(b, dtype=ld).ravel(), np.asarray(z, dtype=ld).ravel()
    p = A.shape[0]
    if A.shape != (p, p) or b.size != p or z.size != p:
        raise ValueError("dense_draw: Q must be (p, p), b and z (p,)")
    L = np.zeros((p, p), dtype=ld)
    for j in range(p):
        row = L[j, :j]
        d = A[j, j] - row @ row
        if not d > 0:
            err = np.linalg.LinAlgError(f"Matrix is not positive definite (pivot {j})")
            err.pivot = j
            raise err
        ljj = np.sqrt(d)
        L[j, j] = ljj
        if j + 1 < p:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ row) / ljj
    w = np.empty(p, dtype=ld)  # L w = b
    for i in range(p):
        w[i] = (b[i] - L[i, :i] @ w[:i]) / L[i, i]
    t = np.stack([w, w + z], axis=1)  # L' [mu, x] = [w, w + z], by columns of L' (= rows of L)
    for i in range(p - 1, -1, -1):
        t[i] /= L[i, i]
        t[:i] -= np.outer(L[i, :i], t[i])
    logdet = 2 * np.sum(np.log(np.diag(L)))
    return t[:, 1].astype(np.float64), t[:, 0].astype(np.float64), float(logdet), L
