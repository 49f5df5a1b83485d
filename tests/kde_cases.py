"""The made-up bin counts that tests/test_store_kde_gpu.py hands to Engine.kde_binned, and their restatement (tests/kde_model.py) at
np.longdouble and np.float64, computed once per process.  tests/test_kde_model_host.py holds the two precisions together on the same
cases without a GPU.

Columns: unimodal, bimodal (unequal components: no exact ties between two peaks for rounding to break), heavily tied (draws on a
coarse lattice: most bins empty), skewed at a lower bound, the unimodal counts scaled so that single bins reach 2^40 (with that many
draws ISJ's Phi keeps one sign over the whole scan and the rule falls back), nearly flat counts that rise in small steps (exactly
flat ones would leave the mode to rounding), and the degenerate ones -- all-zero, a single draw, a single non-empty bin,
hi <= lo.  No grid is symmetric about zero, so that no mode sits where a + (k + 1/2) delta cancels."""

import functools

import numpy as np
from kde_model import kde_model

GRIDS = (8, 64, 65, 100, 512, 1024)
GOOD = ("unimodal", "bimodal", "tied", "skewed", "big", "flat")
DEGENERATE = ("zeros", "one_draw", "one_bin", "empty_range")
MIXED = GOOD + DEGENERATE


def column(kind, G, rng):
    """(counts (G,), lo, hi) of one column"""
    lo, hi = -3.1, 4.3
    n = 40 * G + 37
    if kind in ("unimodal", "big"):
        x = 0.4 + 0.9 * rng.standard_normal(n)
    elif kind == "bimodal":
        x = np.where(rng.random(n) < 0.35, -1.4 + 0.35 * rng.standard_normal(n), 1.9 + 0.6 * rng.standard_normal(n))
    elif kind == "tied":
        x = np.round((0.2 + 1.1 * rng.standard_normal(n)) * 2.0) / 2.0 + 0.013
    elif kind == "skewed":
        lo, hi = 0.0, 6.5
        x = rng.exponential(0.8, n)
    elif kind == "flat":
        return 7 + np.arange(G, dtype=np.int64) // 3, lo, hi
    elif kind == "zeros":
        return np.zeros(G, dtype=np.int64), lo, hi
    elif kind == "one_draw":
        c = np.zeros(G, dtype=np.int64)
        c[G // 3] = 1
        return c, lo, hi
    elif kind == "one_bin":
        c = np.zeros(G, dtype=np.int64)
        c[2 * G // 3] = 12345
        return c, lo, hi
    elif kind == "empty_range":
        return np.histogram(rng.standard_normal(n), G, (lo, hi))[0].astype(np.int64), 1.5, 1.5
    else:
        raise ValueError(kind)
    c = np.histogram(x, G, (lo, hi))[0].astype(np.int64)
    if kind == "big":
        c = c * (2**40 // int(c.max()))
        assert c.max() > 2**39
    return c, lo, hi


def columns(kinds, G, seed):
    rng = np.random.default_rng(seed)
    cols = [column(k, G, rng) for k in kinds]
    return (np.stack([c[0] for c in cols]), np.array([c[1] for c in cols]), np.array([c[2] for c in cols]))


def _case(name, kinds, G, seed, rule, reflect=(False, False), bw_fct=1.0):
    counts, lo, hi = columns(kinds, G, seed)
    bw = None
    if rule == "given":  # a bandwidth of a few bins, another for every column; one that is no bandwidth where the test wants a flag
        bw = (hi - lo) / G * (1.5 + np.arange(len(kinds)) % 5)
        bw[[k == "flat" for k in kinds]] = np.inf
    return dict(name=name, kinds=tuple(kinds), G=G, counts=counts, lo=lo, hi=hi, rule=rule, bw=bw, bw_fct=bw_fct, reflect=reflect)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for G in GRIDS:
        rules = ("experimental", "given") if G >= 512 else ("experimental", "isj", "silverman", "scott", "given")
        for rule in rules:
            out.append(_case(f"mixed-G{G}-{rule}", MIXED, G, 100 + G, rule, bw_fct=1.0 if rule != "scott" else 0.7))
    out.append(_case("one-column", ("bimodal",), 64, 7, "isj"))
    out.append(_case("three-columns", ("skewed", "zeros", "unimodal"), 100, 8, "experimental", reflect=(True, False)))
    many = [MIXED[i % len(MIXED)] for i in range(257)]
    out.append(_case("many-silverman", many, 65, 9, "silverman"))
    out.append(_case("many-isj", many, 8, 13, "isj"))
    for lower in (False, True):
        for upper in (False, True):
            for rule in ("given", "silverman"):
                out.append(_case(f"reflect-{int(lower)}{int(upper)}-{rule}", ("skewed", "unimodal", "one_bin"), 64, 11, rule,
                                 reflect=(lower, upper)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(i, dtype=np.longdouble):
    """kde_model of cases()[i] at dtype"""
    c = cases()[i]
    return kde_model(c["counts"], c["lo"], c["hi"], c["rule"], c["bw"], c["bw_fct"], c["reflect"], dtype=dtype)
