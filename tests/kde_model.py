"""The binned kernel density estimate of omc_kde_binned (include/omcmc_hip.h), restated in numpy at a chosen precision (default
np.longdouble): the bandwidth rules from (counts, lo, hi) alone -- binned moments, binned quantiles with Python-integer prefix sums,
the improved Sheather-Jones rule with its cosine taken from a table by the exact integer k (2 j + 1) mod 4 G, the scan over
t_i = 2^(-(6 + i) / 2) and exactly 60 bisection steps --, the Gaussian convolution over the bin centres with reflection at a bound,
and the mode.  Written from the definitions, column by column, with no thought for speed.

Beside the results it reports what a test needs to know that rounding cannot change the root ISJ picks: `bracket`, the index i of
the scan pair (t_i, t_(i+1)) taken (-1: none, the rule fell back), and `margin`, the smallest |Phi(t_i)| / t_i over the scan
points up to and including that pair (all of them without a pair)."""

import numpy as np

RULES = ("given", "scott", "silverman", "isj", "experimental")
N_SCAN, N_BISECT = 47, 60


def _quantile(c, N, lo, delta, u_num, ft):
    """q(u_num / 4) = lo + delta (j + (u N - C_j) / c_j), j the first non-empty bin with C_j + c_j >= u N: integers throughout"""
    C = 0
    for j, cj in enumerate(c):
        if cj > 0 and 4 * (C + cj) >= u_num * N:
            return lo + delta * (ft(j) + ft(u_num * N - 4 * C) / ft(4 * cj))
        C += cj
    raise AssertionError("no bin reaches the quantile")


def isj_phi(p, N, ft):
    """Phi of the ISJ rule for bin probabilities p (G,) and N draws: a function of t"""
    G = len(p)
    pi = 4 * np.arctan(ft(1))
    table = np.cos(pi * np.arange(G + 1).astype(ft) / ft(2 * G))
    k = np.arange(1, G, dtype=np.int64)[:, None]
    idx = (k * (2 * np.arange(G, dtype=np.int64)[None, :] + 1)) % (4 * G)
    q = np.where(idx <= 2 * G, idx, 4 * G - idx)
    cs = np.where(q <= G, table[np.minimum(q, G)], -table[np.clip(2 * G - q, 0, G)])
    a = (cs * p[None, :]).sum(axis=1)
    A2 = a * a
    K = (np.arange(1, G, dtype=np.int64) ** 2).astype(ft)

    def f(s, t):
        return 2 * pi ** (2 * s) * np.sum(K**s * A2 * np.exp(-K * pi * pi * t))

    def phi(t):
        fs = f(7, t)
        for s in range(6, 1, -1):
            c_s = (1 + ft(2) ** (-(ft(s) + ft(1) / 2))) / 3
            kappa = ft(int(np.prod(np.arange(1, 2 * s, 2)))) / np.sqrt(2 * pi)
            t_s = (2 * c_s * kappa / (ft(N) * fs)) ** (ft(2) / ft(3 + 2 * s))
            fs = f(s, t_s)
        return t - (2 * ft(N) * np.sqrt(pi) * fs) ** (-ft(2) / ft(5))

    return phi


def isj_root(p, N, ft):
    """(t* or None, bracket index, margin) by the pinned root rule"""
    phi = isj_phi(p, N, ft)
    ts = [ft(2) ** (-(ft(6) + i) / 2) for i in range(N_SCAN)]
    with np.errstate(all="ignore"):
        vals = [phi(ts[0])]
        bracket = -1
        for i in range(1, N_SCAN):
            vals.append(phi(ts[i]))
            if np.isfinite(vals[i - 1]) and np.isfinite(vals[i]) and (vals[i - 1] >= 0) != (vals[i] >= 0):
                bracket = i - 1
                break
        ratios = [abs(v) / t for v, t in zip(vals, ts) if not np.isnan(v)]
        margin = float(min(ratios)) if ratios else float("inf")
        if bracket < 0:
            return None, -1, margin
        t_hi, t_lo, lo_pos = ts[bracket], ts[bracket + 1], vals[bracket + 1] >= 0
        for _ in range(N_BISECT):
            mid = (t_lo + t_hi) / 2
            if (phi(mid) >= 0) == lo_pos:
                t_lo = mid
            else:
                t_hi = mid
        return (t_lo + t_hi) / 2, bracket, margin


def kde_column(counts, lo, hi, rule="experimental", bw=None, bw_fct=1.0, reflect=(False, False), dtype=np.longdouble):
    """One column: dict(density (G,), bw, mode, flag, n, bracket, margin) at `dtype`"""
    ft = dtype
    c = [int(v) for v in counts]
    if min(c) < 0:
        raise ValueError("negative count")
    G, N = len(c), sum(c)
    nan = ft("nan")
    out = dict(density=np.full(G, nan, dtype=ft), bw=nan, mode=nan, flag=2, n=N, bracket=-1, margin=float("inf"))
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        return out
    if rule == "given":
        if N < 1 or not (np.isfinite(bw) and bw > 0):
            return out
    elif N < 2 or sum(v > 0 for v in c) < 2:
        return out
    lo, hi = ft(lo), ft(hi)
    pi = 4 * np.arctan(ft(1))
    delta = (hi - lo) / G
    g = lo + (np.arange(G).astype(ft) + ft(1) / 2) * delta
    cf = np.array(c, dtype=ft)
    flag = 0
    if rule == "given":
        h = ft(bw)
    else:
        p = cf / ft(N)
        m = np.sum(p * g)
        sd = np.sqrt(ft(N) / ft(N - 1) * np.sum(p * (g - m) ** 2))
        n15 = ft(N) ** (-ft(1) / ft(5))
        scott = ft(106) / ft(100) * sd * n15
        iqr = _quantile(c, N, lo, delta, 3, ft) - _quantile(c, N, lo, delta, 1, ft)
        spread = sd if iqr == 0 else min(sd, iqr / (ft(134) / ft(100)))
        silver = ft(9) / ft(10) * spread * n15
        h = scott if rule == "scott" else silver
        if rule in ("isj", "experimental"):
            t_star, out["bracket"], out["margin"] = isj_root(p, N, ft)
            if t_star is None:
                isj, flag = silver, 1
            else:
                isj = np.sqrt(t_star) * (hi - lo)
            h = isj if rule == "isj" else (silver + isj) / 2
    h = h * ft(bw_fct)
    d = np.arange(2 * G).astype(ft) * delta / h
    T = np.exp(-d * d / 2)
    k, j = np.arange(G)[:, None], np.arange(G)[None, :]
    w = T[np.abs(k - j)]
    if reflect[0]:
        w = w + T[k + j + 1]
    if reflect[1]:
        w = w + T[2 * G - 1 - k - j]
    dens = (w * cf[None, :]).sum(axis=1) / (ft(N) * h * np.sqrt(2 * pi))
    out.update(density=dens, bw=h, mode=g[int(np.argmax(dens))], flag=flag)
    return out


def kde_model(counts, lo, hi, rule="experimental", bw=None, bw_fct=1.0, reflect=(False, False), dtype=np.longdouble):
    """Every column of counts (.., G) with lo, hi (and bw under rule "given") of the leading shape: dict of arrays of that shape,
    "density" with G behind it"""
    counts = np.asarray(counts)
    lead, G = counts.shape[:-1], counts.shape[-1]
    c2 = counts.reshape(-1, G)
    lo1, hi1 = np.broadcast_to(lo, lead).reshape(-1), np.broadcast_to(hi, lead).reshape(-1)
    bw1 = None if bw is None else np.broadcast_to(bw, lead).reshape(-1)
    cols = [kde_column(c2[i], lo1[i], hi1[i], rule, None if bw1 is None else bw1[i], bw_fct, reflect, dtype) for i in range(len(c2))]
    res = {"density": np.stack([c["density"] for c in cols]).reshape(lead + (G,))}
    for key, dt in (("bw", dtype), ("mode", dtype), ("flag", np.int32), ("n", np.int64), ("bracket", np.int64), ("margin", np.float64)):
        res[key] = np.array([c[key] for c in cols], dtype=dt).reshape(lead)
    return res
