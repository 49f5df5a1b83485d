"""The range rule of `histogram` / `histogram2d` (bin_edges) and of `kde` / `kde2d` (auto_range, widen, linspace_edges): numpy only."""

import numpy as np


def auto_range(mn, mx, cnt, pool=False):
    """(lo, hi) per element, (0, 1) for one without a draw; pool: one range, that of the flattened draws, as arrays of one element"""
    lo, hi = np.where(cnt > 0, mn, 0.0), np.where(cnt > 0, mx, 1.0)
    if pool:
        have = cnt > 0
        lo, hi = (np.array([lo[have].min()]), np.array([hi[have].max()])) if have.any() else (np.zeros(1), np.ones(1))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("autodetected range is not finite")
    return lo, hi


def widen(lo, hi, extend=None):
    """0.5 either way where lo == hi, elsewhere extend (hi - lo); None forms no product (0 * inf is NaN near the ends of fp64)"""
    same = lo == hi
    if extend is None:  # (not lo - 0.0, hi + 0.0 either: an end of -0.0 keeps its sign)
        return np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)
    pad = extend * (hi - lo)
    return np.where(same, lo - 0.5, lo - pad), np.where(same, hi + 0.5, hi + pad)


def grid_lengths(lens, most, message, extend):
    if any(int(n) != n for n in lens) or not all(8 <= n <= most for n in lens):
        raise ValueError(message)
    if not (np.ndim(extend) == 0 and extend >= 0 and np.isfinite(extend)):
        raise ValueError("extend must be a finite non-negative number")
    return [int(n) for n in lens]


def linspace_edges(a, b, n):
    return np.stack([np.linspace(x, y, n + 1) for x, y in zip(a, b)])


def bin_edges(bins, rng, minmax, messages, pool=False):
    """Edges of one axis by np.histogram's rules: bins an array of edges, (n + 1,) or unless pool (n_elements, n + 1), or an int n: then
    np.linspace over rng = (lo, hi), one row, or over auto_range(*minmax()).  messages: the caller's words for a bad int and a bad shape."""
    if np.ndim(bins) != 0:
        edges = np.array(bins, dtype=np.float64)
        if edges.ndim not in ((1,) if pool else (1, 2)) or edges.shape[-1] < 2:
            raise ValueError(messages[1])
        if np.isnan(edges).any() or (np.diff(edges, axis=-1) < 0).any():
            raise ValueError("`bins` must increase monotonically, when an array")
        return edges
    n = int(bins)
    if n != bins or not 1 <= n <= 1024:
        raise ValueError(messages[0])
    if rng is None:
        lo, hi = auto_range(*minmax(), pool=pool)
    else:
        lo, hi = (float(v) for v in rng)
        if lo > hi:
            raise ValueError("max must be larger than min in range parameter.")
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"supplied range of [{lo}, {hi}] is not finite")
        lo, hi = np.array([lo]), np.array([hi])
    edges = linspace_edges(*widen(lo, hi), n)
    return edges[0] if (rng is not None or pool) else edges
