"""numpy restatement of omc_store_loo_expect (include/omcmc_hip.h), written from the definitions there and parametrised by dtype:
np.float64 follows the device's formulas at the device's precision, np.longdouble is the reference the GPU tests hold the device
to.  The fit is psis_model's, restated here only as far as it must hand out what psis_column keeps to itself (sigma and the
smoothed column); test_loo_expect_model_host.py holds the two to each other.  Also the inputs of the tests: psis_inputs with ties
INSIDE the tail and a matrix of posterior-predictive replicates."""

import numpy as np
from psis_model import LOG_DBL_MIN, WEIGHT_CUT, logsumexp, psis_inputs, tail_max_of  # noqa: F401  (tail_max_of: for the tests)
from scipy.special import erfc


def smoothed_column(ll, tail_max, dtype=np.float64):
    """(v sorted ascending, the smoothed x' at the sorted positions, k, T, smoothed?) of one column of finite log-likelihoods:
    steps 1 - 5 of the omc_store_psis contract, as psis_model.psis_column takes them"""
    ll = np.asarray(ll, dtype=np.float64).astype(dtype)
    S, M = ll.size, int(tail_max)
    v = np.sort(-ll)
    x = v - v[-1]
    xc = max(x[S - M - 1], dtype(LOG_DBL_MIN))
    T = int(np.sum(x > xc))
    k, sigma, exc = dtype(np.inf), dtype(0), np.exp(xc)
    xs = x.copy()
    with np.errstate(all="ignore"):
        if T > 4:
            a = np.exp(x[S - T:]) - exc
            n = T
            m = 30 + int(np.floor(np.sqrt(n)))
            q = int(np.floor(n / 4 + 0.5)) - 1
            i = np.arange(1, m + 1).astype(dtype)
            b = 1 / a[n - 1] + (1 - np.sqrt(dtype(m) / (i - dtype(0.5)))) / (3 * a[q])
            ki = np.log1p(-b[:, None] * a[None, :]).sum(axis=1) / dtype(n)
            L = dtype(n) * (np.log(-b / ki) - ki - 1)
            w = 1 / np.exp(L[None, :] - L[:, None]).sum(axis=1)
            keep = w >= dtype(WEIGHT_CUT)
            w = w[keep] / w[keep].sum()
            bb = (b[keep] * w).sum()
            kp = np.log1p(-bb * a).sum() / dtype(n)
            sigma = -kp / bb
            k = (dtype(n) * kp + 5) / (dtype(n) + 10)
        smooth = bool(np.isfinite(k))
        if smooth:
            p = (np.arange(T).astype(dtype) + dtype(0.5)) / dtype(T)
            g = -sigma * np.log1p(-p) if abs(k) < 2.0 ** -52 else sigma * np.expm1(-k * np.log1p(-p)) / k
            xs[S - T:] = np.log(g + exc) if sigma > 0 else np.nan
        xs = np.where(xs > 0, dtype(0), xs)
    return v, xs, k, T, smooth


def draw_weights(ll, tail_max, dtype=np.float64):
    """(w (S,), lw (S,), k, T) of one column: every draw's smoothed weight and its normalised logarithm, in draw order.  A draw
    outside the tail (or of a column that was not smoothed) has w = exp(min(x, 0)); a tail draw the mean of exp(x') over the
    sorted positions its value occupies, so tied tail draws share theirs evenly.  NaN and T = -1 for a column that is not finite."""
    ll = np.asarray(ll, dtype=np.float64).astype(dtype)
    S = ll.size
    if not np.all(np.isfinite(ll)):
        return np.full(S, np.nan, dtype), np.full(S, np.nan, dtype), np.nan, -1
    v, xs, k, T, smooth = smoothed_column(ll, tail_max, dtype)
    with np.errstate(all="ignore"):
        lse_x = logsumexp(xs)
        mine = -ll
        lo, hi = np.searchsorted(v, mine, side="left"), np.searchsorted(v, mine, side="right")
        x = np.minimum(mine - v[-1], dtype(0))
        w, lw = np.exp(x), x - lse_x
        if smooth:
            for s in np.nonzero(lo >= S - T)[0]:
                if hi[s] - lo[s] == 1:
                    w[s], lw[s] = np.exp(xs[lo[s]]), xs[lo[s]] - lse_x
                else:
                    w[s] = np.exp(xs[lo[s]: hi[s]]).sum() / dtype(hi[s] - lo[s])
                    lw[s] = np.log(w[s]) - lse_x
    return w, lw, k, T


def loo_expect_column(ll, tail_max, f, thr=None, tau=None, dtype=np.float64):
    """dict mean, var, below, ess, invprec, k, tail, lw of one column: the sums of the contract, plainly"""
    f = np.asarray(f, dtype=np.float64).astype(dtype)
    w, lw, k, T = draw_weights(ll, tail_max, dtype)
    out = {"k": k, "tail": T, "lw": lw}
    with np.errstate(all="ignore"):
        W = w.sum()
        mean = (w * f).sum() / W
        out["mean"], out["var"], out["ess"] = mean, (w * (f - mean) ** 2).sum() / W, W * W / (w * w).sum()
        out["below"] = np.nan if thr is None else np.where(f <= dtype(thr), w, dtype(0)).sum() / W
        out["invprec"] = np.nan if tau is None else (w / np.asarray(tau, dtype=np.float64).astype(dtype)).sum() / W
    return out


def loo_expect(ll, tail_max, f, thr=None, tau=None, dtype=np.float64):
    """the same over the columns of ll (S, n): f (S, n), thr (n,) or None, tau (S, 1), (S, n) or None; fp64 arrays, lw (S, n)"""
    ll, f = np.asarray(ll), np.asarray(f)
    n = ll.shape[1]
    tm = np.broadcast_to(np.asarray(tail_max), (n,))
    if tau is not None:
        tau = np.broadcast_to(np.asarray(tau), ll.shape)
    cols = [loo_expect_column(ll[:, j], tm[j], f[:, j], None if thr is None else thr[j], None if tau is None else tau[:, j], dtype)
            for j in range(n)]
    out = {name: np.array([float(c[name]) for c in cols]) for name in ("mean", "var", "below", "ess", "invprec", "k")}
    out["tail"] = np.array([c["tail"] for c in cols], dtype=np.int64)
    out["lw"] = np.stack([c["lw"] for c in cols], axis=1).astype(np.float64)
    return out


def normal_cdf(x, y, tau):
    """f of f_kind CDF: 0.5 erfc(-z / sqrt(2)), z = sqrt(tau) (y - x), at fp64 (erfc has no wider form; its rounding is 1e-16)"""
    z = np.sqrt(tau) * (y[None, :] - x)
    return 0.5 * erfc(-z * 0.70710678118654752440)


def loo_inputs(S, seed=0):
    """(mu (S, 9), y (9,), tau (S, 9), y_rep (S, 9)): psis_inputs(S) with, in column 8, the three draws with the largest -ll sharing
    one mean -- ties INSIDE the tail, whose f differ in y_rep --, and the replicates mu + eps / sqrt(tau) of a seeded generator"""
    mu, y, tau = psis_inputs(S, seed)
    order = np.argsort(np.abs(y[8] - mu[:, 8]), kind="stable")  # ascending -ll at tau = 1
    mu[order[-3:], 8] = mu[order[-1], 8]
    rng = np.random.default_rng(77000 + 1000 * S + seed)
    return mu, y, tau, mu + rng.standard_normal(mu.shape) / np.sqrt(tau)
