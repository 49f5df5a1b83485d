"""The stores and intervals on which omc_store_ess_indicator is held to its exact model (tests/essq_model.py): shared by
test_essq_model_host.py (which checks, without a GPU, the condition on these inputs that makes the comparison meaningful: no Geyer
decision closer to zero than 1e-9) and test_store_essq_gpu.py."""

import functools

import numpy as np
from essq_model import ar1, indicator_exact, split_series

QUANT = ([-1.0, -1.0, -1.0], [0.05, 0.5, 0.9])


def _case(name, x, lo, hi, n_cnt, idx=None):
    return {"name": name, "x": np.ascontiguousarray(x, dtype=np.float64), "lo": np.asarray(lo, dtype=np.float64),
            "hi": np.asarray(hi, dtype=np.float64), "n_cnt": int(n_cnt), "idx": None if idx is None else np.asarray(idx, dtype=np.int64)}


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # the word edges: M = 63, 64, 65, 127, 128, 129, N even and odd; quantile intervals, a local one, lo == hi
    for N in (126, 129, 131, 254, 257, 259):
        out.append(_case(f"edge-N{N}", ar1(N, 3, np.linspace(0.3, 0.9, 5), seed=N), QUANT[0] + [0.2, 0.3], QUANT[1] + [0.4, 0.3], min(N // 2, 70)))
    # one chain
    out.append(_case("one-chain", ar1(200, 1, [0.3, 0.6, 0.8, 0.9], seed=7), QUANT[0] + [0.45], QUANT[1] + [0.55], 40))
    # slow columns: the sequence runs past lag 128 (the host test asserts it)
    out.append(_case("slow", ar1(1200, 2, [0.99, 0.985, 0.98], seed=11), [-1.0, -1.0], [0.5, 0.1], 200))
    # the largest store, four probabilities across the range
    out.append(_case("large", ar1(1200, 8, np.linspace(0.3, 0.99, 40), seed=3), [-1.0] * 4, [0.05, 0.35, 0.65, 0.95], 0))
    # a trend: the sequence reaches the M - 3 limit (at p = 0.5 with W == 0 < B_M)
    n = np.arange(100.0)
    out.append(_case("trend", (n[:, None] + 0.01 * np.arange(2.0)[None, :])[:, :, None], [-1.0, -1.0, 0.1], [0.25, 0.5, 0.3], 50))
    # prob 0 and 1 and the whole range: the all-ones indicator gives ess = J M
    out.append(_case("ends", ar1(90, 2, [0.5, 0.9], seed=5), [-1.0, -1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0, 1.0], 45))
    # two chains at separate levels, p = 0.5: every series constant, W == 0 < B_M
    rng = np.random.default_rng(13)
    lev = rng.standard_normal((40, 2, 2))
    lev[:, 1, :] += 10.0
    out.append(_case("levels", lev, [-1.0, -1.0], [0.5, 0.3], 20))
    # integer-valued draws: many ties at the thresholds
    out.append(_case("ties", np.floor(3.0 * ar1(300, 4, [0.5, 0.8, 0.95], seed=17)), QUANT[0] + [0.3, 0.5], QUANT[1] + [0.7, 0.5], 64))
    # one interval; thirty-two (quantile and local mixed)
    x = ar1(150, 4, np.linspace(0.3, 0.95, 6), seed=19)
    out.append(_case("one-interval", x, [-1.0], [0.3], 75))
    lo32 = np.where(np.arange(32) % 2 == 0, -1.0, np.linspace(0.0, 0.6, 32))
    out.append(_case("32-intervals", x, lo32, np.where(lo32 < 0, np.linspace(0.02, 0.98, 32), lo32 + 0.3), 10))
    # repeated and permuted selection
    out.append(_case("selection", x, QUANT[0], QUANT[1], 30, idx=[3, 0, 3, 5, 1, 0, 4]))
    # an element with a NaN and one with an infinity (one of them in the dropped middle row) beside clean ones
    bad = ar1(131, 3, np.linspace(0.3, 0.9, 5), seed=23)
    bad[65, 1, 1] = np.nan
    bad[7, 2, 3] = np.inf
    out.append(_case("non-finite", bad, QUANT[0] + [0.2], QUANT[1] + [0.6], 20))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def model(name):
    """the exact model of a case: ess, lags (n_p, n_idx), q (n_p, n_idx, 2), counts (n_p, n_idx, 2 + 2 n_cnt), dead (n_idx,), and
    the smallest decision margin"""
    c = case(name)
    x, n_cnt = c["x"], c["n_cnt"]
    idx = np.arange(x.shape[2]) if c["idx"] is None else c["idx"]
    n_p, n = c["hi"].size, idx.size
    ess, lags = np.full((n_p, n), np.nan), np.zeros((n_p, n), dtype=np.int32)
    q, counts = np.full((n_p, n, 2), np.nan), np.zeros((n_p, n, 2 + 2 * n_cnt), dtype=np.int64)
    dead = np.zeros(n, dtype=bool)
    margin = np.inf
    done = {}
    for k, col in enumerate(idx):
        if not np.all(np.isfinite(x[:, :, col])):
            dead[k] = True
            continue
        xs = split_series(x[:, :, col])
        for p in range(n_p):
            key = (int(col), p)
            if key not in done:
                done[key] = indicator_exact(xs, c["lo"][p], c["hi"][p], n_cnt)
            r = done[key]
            ess[p, k], lags[p, k], q[p, k], counts[p, k] = r["ess"], r["lags"], r["q"], r["counts"]
            margin = min(margin, r["margin"])
    return {"ess": ess, "lags": lags, "q": q, "counts": counts, "dead": dead, "margin": margin}
