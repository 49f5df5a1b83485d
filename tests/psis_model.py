"""numpy restatement of omc_store_loglik and omc_store_psis (include/omcmc_hip.h), written from the definitions there and
parametrised by dtype: np.float64 follows the device's formulas at the device's precision, np.longdouble is the reference the
GPU tests hold the device to.  Also the columns the PSIS tests run on (test_psis_model_host.py, test_store_psis_gpu.py)."""

import numpy as np

HALF_LOG_2PI = 0.91893853320467274178  # 0.5 log(2 pi), rounded to fp64
LOG_DBL_MIN = -708.3964185322641
WEIGHT_CUT = 10.0 * 2.0 ** -52

# (n_iter, C) of the GPU tests; S = n_iter * C
PSIS_SHAPES = [(5, 1), (3, 2), (5, 5), (13, 2), (16, 4), (25, 4), (125, 8), (4099, 1)]
PSIS_S_HOST = [5, 6, 25, 26, 64, 100, 1000, 4099, 20000]
SD_Y = [(0.1, 0.0), (0.5, 0.0), (1.0, 3.0), (2.0, 6.0)]


def loglik(x, y, tau, dtype=np.float64):
    """ll (S, n) of rows x (S, n) under observations y (n,) and precisions tau (S, 1) or (S, n)"""
    x, y, tau = (np.asarray(a, dtype=np.float64).astype(dtype) for a in (x, y, tau))
    with np.errstate(all="ignore"):
        h = dtype(0.5) * np.log(tau) - dtype(HALF_LOG_2PI)
        r = y[None, :] - x
        return h - dtype(0.5) * tau * r * r


def logsumexp(a, axis=None):
    a = np.asarray(a)
    with np.errstate(all="ignore"):
        m = np.max(a, axis=axis, keepdims=True)
        out = np.log(np.sum(np.exp(a - m), axis=axis, keepdims=True)) + m
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def column_summaries(ll):
    """(lse, mean, var) down the columns of ll (S, n); NaN where a column holds a value that is not finite"""
    ll = np.asarray(ll)
    bad = ~np.all(np.isfinite(ll), axis=0)
    safe = np.where(bad[None, :], ll.dtype.type(0), ll)
    out = [logsumexp(safe, axis=0), safe.mean(axis=0), safe.var(axis=0, ddof=1)]
    return tuple(np.where(bad, np.nan, o) for o in out)


def tail_max_of(S, reff=1.0):
    return int(min(S - 1, np.ceil(min(S / 5.0, 3.0 * np.sqrt(S / reff)))))


def psis_column(ll, tail_max, dtype=np.float64):
    """(elpd, k, T, margin) of one column of log-likelihoods; margin is the smallest relative distance of a candidate weight
    from the 10 * 2^-52 cut (inf where nothing was fitted)"""
    ll = np.asarray(ll, dtype=np.float64).astype(dtype)
    S, M = ll.size, int(tail_max)
    if not np.all(np.isfinite(ll)):
        return np.nan, np.nan, -1, np.inf
    v = np.sort(-ll)
    x = v - v[-1]
    xc = max(x[S - M - 1], dtype(LOG_DBL_MIN))
    T = int(np.sum(x > xc))
    k, sigma, margin, exc = dtype(np.inf), dtype(0), np.inf, np.exp(xc)
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
            margin = float(np.min(np.abs(w - dtype(WEIGHT_CUT)) / dtype(WEIGHT_CUT)))
            keep = w >= dtype(WEIGHT_CUT)
            w = w[keep] / w[keep].sum()
            bb = (b[keep] * w).sum()
            kp = np.log1p(-bb * a).sum() / dtype(n)
            sigma = -kp / bb
            k = (dtype(n) * kp + 5) / (dtype(n) + 10)
        xs = x.copy()
        if np.isfinite(k):
            p = (np.arange(T).astype(dtype) + dtype(0.5)) / dtype(T)
            g = -sigma * np.log1p(-p) if abs(k) < 2.0 ** -52 else sigma * np.expm1(-k * np.log1p(-p)) / k
            xs[S - T:] = np.log(g + exc) if sigma > 0 else np.nan
            xs = np.where(xs > 0, dtype(0), xs)
        lse_x = logsumexp(xs)
        terms = xs - lse_x - v          # w + ll, ll = -v
        terms[: S - T] = -v[-1] - lse_x  # a draw outside the tail
        elpd = logsumexp(terms)
    return elpd, k, T, margin


def psis(ll, tail_max, dtype=np.float64):
    """(elpd, k, T, margin) arrays over the columns of ll (S, n); tail_max a number or (n,)"""
    ll = np.asarray(ll)
    tm = np.broadcast_to(np.asarray(tail_max), (ll.shape[1],))
    cols = [psis_column(ll[:, j], tm[j], dtype) for j in range(ll.shape[1])]
    return (np.array([float(c[0]) for c in cols]), np.array([float(c[1]) for c in cols]),
            np.array([c[2] for c in cols], dtype=np.int64), np.array([c[3] for c in cols]))


def psis_inputs(S, seed=0):
    """(mu (S, 9), y (9,), tau (S, 9)) of fp64: the four (sd, y) columns mu ~ N(0, sd) with tau = 1, the same four regimes with
    tau ~ Gamma(50, scale 0.02) per draw, and a column (tau = 1) whose draws around the cut of tail_max_of(S) are tied"""
    rng = np.random.default_rng(1000 * S + seed)
    mu = rng.standard_normal((S, 9)) * np.array([sd for sd, _ in SD_Y] * 2 + [1.0])
    y = np.array([yy for _, yy in SD_Y] * 2 + [3.0])
    tau = np.ones((S, 9))
    tau[:, 4:8] = rng.gamma(50.0, 0.02, size=(S, 1))
    # ties at the cut: the draws at sorted positions S - M - 2 .. S - M + 1 of the last column share one mean, hence one ll
    M = tail_max_of(S)
    order = np.argsort(np.abs(y[8] - mu[:, 8]))  # ascending -ll at tau = 1
    lo, hi = max(0, S - M - 2), min(S - 1, S - M + 1)
    mu[order[lo: hi + 1], 8] = mu[order[lo], 8]
    return mu, y, tau
