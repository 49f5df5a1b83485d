"""A numpy restatement of omc_kde2d_binned's definition (include/omcmc_hip.h), at np.longdouble unless told otherwise: the binned
moments, the kernel covariance H (given, or Scott's rule H = N^(-1/3) S), the full-covariance binned Gaussian convolution -- a loop
over the non-empty cells only --, the joint mode and the levels of the highest-density regions by a plain sort and running sum.
Shared by the host and the GPU tests of the joint density; nothing here calls the library."""

import numpy as np

NEARLY_ONE = 1.0 - 2.0**-20


def _one(c, lox, hix, loy, hiy, rule, h_in, bw_fct, probs, dtype):
    f = dtype
    nx, ny = c.shape
    n_probs = len(probs)
    nan = np.nan
    out = dict(density=np.full((nx, ny), nan, dtype=f), bw=np.full(3, nan, dtype=f), mode=np.full(2, nan), mode_index=np.full(2, -1),
               level=np.full(n_probs, nan, dtype=f), level_pos=np.full(n_probs, -1, dtype=np.int64), flag=np.int32(2),
               margin=np.full(n_probs, np.inf), gap=np.inf)
    N = int(c.sum())
    if not (np.isfinite([lox, hix, loy, hiy]).all() and hix > lox and hiy > loy):
        return out
    rows, cols = c.sum(axis=1), c.sum(axis=0)
    if rule == "given":
        if N < 1:
            return out
    elif N < 2 or (rows > 0).sum() < 2 or (cols > 0).sum() < 2:
        return out
    lox, hix, loy, hiy = f(lox), f(hix), f(loy), f(hiy)
    dx, dy = (hix - lox) / f(nx), (hiy - loy) / f(ny)
    X, Y = lox + (np.arange(nx).astype(f) + f(0.5)) * dx, loy + (np.arange(ny).astype(f) + f(0.5)) * dy
    Nf = f(N)
    if rule == "given":
        hxx, hxy, hyy = (f(v) for v in h_in)
    else:
        px, py = rows.astype(f) / Nf, cols.astype(f) / Nf
        mx, my = (px * X).sum(), (py * Y).sum()
        corr = Nf / (Nf - f(1))
        sxx, syy = corr * (px * (X - mx) ** 2).sum(), corr * (py * (Y - my) ** 2).sum()
        sxy = corr * ((c.astype(f) / Nf) * np.outer(X - mx, Y - my)).sum()
        fac = Nf ** (-f(1) / f(3))
        hxx, hxy, hyy = fac * sxx, fac * sxy, fac * syy
    f2 = f(bw_fct) * f(bw_fct)
    hxx, hxy, hyy = hxx * f2, hxy * f2, hyy * f2
    if not (hxx > 0 and hyy > 0 and np.isfinite(float(hxx)) and np.isfinite(float(hyy)) and np.isfinite(float(hxy))):
        return out
    if not hxy * hxy < f(NEARLY_ONE) * (hxx * hyy):
        return out
    det = hxx * hyy - hxy * hxy
    A, beta = hyy / det, -hxy / hyy  # q = A u^2 + 2 B u v + C v^2 = A (u + (B / A) v)^2 + v^2 / h_yy: nothing cancels between the two
    acc = np.zeros((nx, ny), dtype=f)
    K, Lc = np.arange(nx)[:, None], np.arange(ny)[None, :]
    for i, j in zip(*np.nonzero(c)):  # the non-empty cells only
        u, v = (K - i).astype(f) * dx, (Lc - j).astype(f) * dy
        acc += f(int(c[i, j])) * np.exp(-(A * (u + beta * v) ** 2 + v * v / hyy) / f(2))
    dens = acc / (Nf * f(2) * f(np.pi if f is np.float64 else np.arccos(f(-1))) * np.sqrt(det))
    flat = dens.ravel()
    best = int(np.argmax(flat))  # (the first of equals: the lowest flat index)
    top = np.sort(flat)[-2:]
    k, l = divmod(best, ny)
    lo64, d64 = (np.float64(lox), np.float64(loy)), ((np.float64(hix) - np.float64(lox)) / nx, (np.float64(hiy) - np.float64(loy)) / ny)
    out.update(density=dens, bw=np.array([hxx, hxy, hyy], dtype=f), mode_index=np.array([k, l]), flag=np.int32(0),
               mode=np.array([lo64[0] + (k + 0.5) * d64[0], lo64[1] + (l + 0.5) * d64[1]]),  # fp64, both roundings, as the kernel
               gap=float((top[1] - top[0]) / top[1]))
    if n_probs:
        D = np.sort(flat)[::-1]
        S_r = np.cumsum(D, dtype=f)
        S = S_r[-1]
        for q, p in enumerate(probs):
            r = int(np.argmax(S_r >= f(p) * S))
            out["level_pos"][q], out["level"][q] = r, D[r]
            near = [abs(S_r[r] - f(p) * S) / S] + ([abs(S_r[r - 1] - f(p) * S) / S] if r else [])
            out["margin"][q] = float(min(near))
    return out


def kde2d_model(counts, lo_x, hi_x, lo_y, hi_y, rule="scott", bw=None, bw_fct=1.0, probs=(), dtype=np.longdouble):
    """counts int64 (.., nx, ny), the ends of the leading shape, bw (.., 3) with rule "given" -> dict of arrays of the leading
    shape: density (.., nx, ny), bw (.., 3), level, level_pos (.., n_probs), flag as omc_kde2d_binned defines them, at dtype;
    mode_index (.., 2) the cell of the largest density and mode (.., 2) its centre formed in fp64 as the kernel forms it; margin
    (.., n_probs) = min |S_r - prob S| / S over r = level_pos and level_pos - 1; gap = the relative distance of the two largest
    densities."""
    counts = np.asarray(counts)
    lead = counts.shape[:-2]
    n = int(np.prod(lead, dtype=np.int64))
    c = counts.reshape((n,) + counts.shape[-2:])
    ends = [np.broadcast_to(np.asarray(v, dtype=np.float64), lead).reshape(n) for v in (lo_x, hi_x, lo_y, hi_y)]
    h = None if bw is None else np.broadcast_to(np.asarray(bw, dtype=np.float64), lead + (3,)).reshape(n, 3)
    rule = "scott" if rule == "silverman" else rule
    probs = tuple(np.atleast_1d(np.asarray(probs, dtype=np.float64)))
    res = [_one(c[g], ends[0][g], ends[1][g], ends[2][g], ends[3][g], rule, None if h is None else h[g], bw_fct, probs, dtype)
           for g in range(n)]
    return {k: np.stack([r[k] for r in res]).reshape(lead + np.shape(res[0][k])) for k in res[0]}
