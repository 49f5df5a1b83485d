"""Numpy restatement of omc_store_first_failure (include/omcmc_hip.h) and of the rules of MCMC.excursion and MCMC.contour_map
(openmcmc_amd/summary/excursion.py), written from their documentation.  Everything is an integer or one IEEE division of two
integers, so the tests that use it compare with np.array_equal.  tests/test_excursion_model_host.py ties it to the definition by
brute force."""

import numpy as np

KINDS = (">", "<", "!=", "=")


def agree(sel, lo, hi):
    """(R, n) bool: the draws sel (R, n) on the side (lo[k], hi[k]) of their element -- a NaN draw is on no side, +-inf draws are
    ordinary values, an infinite bound is no bound, bounds are strict"""
    with np.errstate(invalid="ignore"):
        return ~np.isnan(sel) & (np.isneginf(lo)[None, :] | (sel > lo[None, :])) & (np.isposinf(hi)[None, :] | (sel < hi[None, :]))


def first_failure(rows, lo, hi, pos, idx=None):
    """(h (n + 1,) int64, r (R,) int32) of rows (R, size) for ONE slot lo, hi, pos (n,)"""
    sel = rows if idx is None else rows[:, idx]
    n = sel.shape[1]
    r = np.where(~agree(sel, lo, hi), pos[None, :], n).min(axis=1)
    return np.bincount(r, minlength=n + 1).astype(np.int64), r.astype(np.int32)


def first_failure_slots(rows, lo, hi, pos, idx=None):
    """(h (L, n + 1), r (L, R)) of tables (L, n)"""
    out = [first_failure(rows, a, b, p, idx) for a, b, p in zip(lo, hi, pos)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def joint_counts(h):
    """J (n,): J[j] = R - sum_{i <= j} h[i], the rows that agree at all of the first j + 1 elements of the order"""
    return h.sum() - np.cumsum(h)[:-1]


def excursion_function(h, pos):
    """F (n,) = J[pos] / R"""
    return joint_counts(h)[pos] / float(h.sum())


def order_of(count):
    """(order, pos): the elements by agreeing count, descending, ties by ascending element; pos[order[j]] = j"""
    order = np.argsort(-np.asarray(count, dtype=np.int64), kind="stable")
    pos = np.empty_like(order)
    pos[order] = np.arange(order.size)
    return order, pos


def sides(sel, u, kind):
    """(lo, hi, agreeing count) per element of the side of `kind` at the levels u (n,)"""
    n = sel.shape[1]
    with np.errstate(invalid="ignore"):
        above, below = (sel > u[None, :]).sum(axis=0), (sel < u[None, :]).sum(axis=0)
    if kind == ">":
        up = np.ones(n, dtype=bool)
    elif kind == "<":
        up = np.zeros(n, dtype=bool)
    else:
        up = above >= below  # the side on which more of the element's draws lie; a tie takes the upper side
    return np.where(up, u, -np.inf), np.where(up, np.inf, u), np.where(up, above, below)


def excursion(store, level, kind=">", alpha=0.05, index=None, offset=None, order=None):
    """MCMC.excursion on a host store (n_iter, C, size), one level"""
    rows = store.reshape(-1, store.shape[2])
    sel = rows if index is None else rows[:, np.asarray(index)]
    R, n = sel.shape
    u = np.full(n, float(level)) + (0.0 if offset is None else np.asarray(offset, dtype=np.float64))
    lo, hi, count = sides(sel, u, kind)
    if order is None:
        order, pos = order_of(count)
    else:
        order = np.asarray(order)
        pos = np.empty_like(order)
        pos[order] = np.arange(n)
    h, _ = first_failure(sel, lo, hi, pos)
    F, marginal = excursion_function(h, pos), count / float(R)
    inside = F >= 1 - alpha
    if kind == "=":
        F, marginal, inside = 1.0 - F, 1.0 - marginal, ~inside
    return {"marginal": marginal, "F": F, "set": inside, "order": order, "counts": h}


def bands_of(mean, levels):
    """band (n,) of K sorted levels: the number of levels <= the mean (a mean on a level belongs to the band above it)"""
    return np.searchsorted(np.asarray(levels, dtype=np.float64), mean, side="right")


def band_sides(band, levels, widen):
    """(lo, hi) of every element's band, widened by `widen` neighbouring bands either way"""
    edges = np.concatenate([[-np.inf], np.asarray(levels, dtype=np.float64), [np.inf]])
    return edges[np.maximum(band - widen, 0)], edges[np.minimum(band + 1 + widen, edges.size - 1)]


def contour_map(store, levels, index=None, mean=None):
    """MCMC.contour_map on a host store (n_iter, C, size); mean: the pooled means of the selected elements, else numpy's"""
    rows = store.reshape(-1, store.shape[2])
    sel = rows if index is None else rows[:, np.asarray(index)]
    R, n = sel.shape
    levels = np.sort(np.asarray(levels, dtype=np.float64))
    with np.errstate(invalid="ignore"):  # (inf - inf: a NaN mean sorts above every level)
        band = bands_of(sel.mean(axis=0) if mean is None else mean, levels)
    out = {"band": band}
    for w in (0, 1):
        lo, hi = band_sides(band, levels, w)
        count = agree(sel, lo, hi).sum(axis=0)
        _, pos = order_of(count)
        h, _ = first_failure(sel, lo, hi, pos)
        out[f"P{w}"] = joint_counts(h)[n - 1] / float(R)
        out[f"F{w}"] = excursion_function(h, pos)
    return out
