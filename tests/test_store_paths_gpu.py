"""omc_store_quantiles, omc_store_moments and omc_store_thin on the paths that tests/test_store_gpu.py and
tests/test_round4_edges_gpu.py do not reach, called through Engine.store_quantiles / store_moments / store_thin.

Quantiles: bit-equal (same(): up to the sign of zero and the payload of NaN) to np.nanquantile / np.quantile.  A store
(n_iter, C, size) is seen per chain as R = n_iter rows and K = C size columns, pooled as R = n_iter C rows and K = size columns;
route() restates the dispatch of omc_store_quantiles.  The route each store takes:

    store             per chain                                           pooled
    (2050, 5, 1639)   R 2050, K 8195: k_q_owned, 8195 mod 8 = 3           R 10250, K 1639: row-sliced, 1639 mod 16 = 7
    (2048, 3, 2731)   R 2048, K 8193: k_q_owned4 (largest R), mod 16 = 1  R 6144,  K 2731: row-sliced, 2731 mod 16 = 11
    (41, 65, 127)     R 41,   K 8255: k_q_owned4, 8255 mod 16 = 15        R 2665,  K 127:  row-sliced, 127 mod 16 = 15
    (1, 1, 8200)      R 1,    K 8200: k_q_owned4, valid counts 0 and 1    the same view
    (2, 1, 8200)      R 2,    K 8200: k_q_owned4, valid counts 0, 1, 2    the same view

Every store is NaN-padded to a random live length per (chain, element) -- none, one and all iterations live among them --, with
NaNs of either sign and with payloads, and carries hard columns in the first column tile and in the last, partial one of the
per-chain view: values that differ in their last bits only (the late digit passes choose among many candidates), subnormals and
both zeros, and +-DBL_MAX and +-inf, whose leading key digit is the NaN key's.

Moments: against exact rational arithmetic (the doubles as integers on their common binary grid, rounded once at the end),
inside the first-order bound of Chan, Golub & LeVeque for updating algorithms, which the one-pass textbook formula misses by
two orders of magnitude on the offset columns; constant columns exactly; non-finite draws as numpy treats them.  The slices
omc_col_moments cuts (no more than ceil(R / 256) of them):

    store           pooled                                    per chain
    (549, 1, 37)    R 549: three slices of 183 rows           the same view
    (183, 3, 37)    R 549, K 37: three slices of 183 rows     R 183, K 111: one slice
    (1030, 2, 40)   R 2060: nine slices of 229 rows, last 228  R 1030, K 80: five slices of 206 rows
    (7, 2, 5)       R 14 < 16: idle row lanes                 R 7: idle row lanes (the nb == 0 branch of omc_chan)
    (1, 3, 4)       R 3                                       R 1: the variance is defined as 0

Thinning: more than 65 535 output rows, so that omc_store_thin's second and third launch run.

Out of reach of a test-sized store: the column-chunk loop of the row-sliced quantile route (K above about 31 000 columns
together with R > 2^22 rows) and that route's clamp of the row slices to 65 535.

Measured on the MI355X (the moments tests print these): the worst |error| / bound over all stores and both views is 0.26 for the
variance (R = 7) and 0.30 for the mean (R = 3), and with R >= 183 rows 0.015 and 0.014.  (The textbook formula, run on the host over the same data,
lies between 5.7e5 (R = 3) and 1.5e10 times the variance bound.)
"""

import functools
import warnings
from fractions import Fraction

import numpy as np
import pytest

from test_store_gpu import make_engine, same

# (the shared stores are read-only arrays; Engine.to_device copies them and writes to nothing)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

# ------------------------------------------------------------------------------------------------------------------ quantiles
Q11 = [0.0, 0.025, 0.1, 0.2, 0.25, 0.3, 0.5, 0.7, 0.9, 0.975, 1.0]  # three launches of the four-level kernels
Q5 = [0.0, 0.3, 0.5, 0.975, 1.0]                                    # two
LARGE = [(2050, 5, 1639), (2048, 3, 2731)]
SMALL = [(41, 65, 127), (1, 1, 8200), (2, 1, 8200)]
TILE = {"k_q_owned": 8, "k_q_owned4": 16, "row-sliced": 16}         # columns of a workgroup


def route(R, K):
    """the kernel omc_store_quantiles picks for a view of R rows and K columns"""
    if K >= 8192 and R <= 2048:
        return "k_q_owned4"
    if K >= 8192 and R <= 2 ** 22:
        return "k_q_owned"
    return "row-sliced"


def view_shape(shape, pooled):
    n_iter, C, size = shape
    return (n_iter * C, size) if pooled else (n_iter, C * size)


# (store, pooled, omit_nan, levels): the large stores leave out omit_nan=False on the pooled view (numpy's time, not the GPU's)
Q_CASES = [(s, False, True, Q5) for s in LARGE] + [(s, False, False, Q5) for s in LARGE] + [(s, True, True, Q5) for s in LARGE] + \
          [(s, pooled, omit, Q11) for s in SMALL for pooled in (False, True) for omit in (True, False)]
# every route with a partial column tile (every store below is NaN-padded): if the thresholds of the library move, this table moves
_partial = {route(*view_shape(s, p)) for s, p, _, _ in Q_CASES if view_shape(s, p)[1] % TILE[route(*view_shape(s, p))]}
assert _partial == {"k_q_owned", "k_q_owned4", "row-sliced"}, _partial
assert route(*view_shape(LARGE[0], False)) == "k_q_owned" and route(*view_shape(LARGE[1], False)) == "k_q_owned4"

DBL_MAX = np.finfo(float).max
NAN_BITS = np.array([0xFFF8000000000000, 0x7FF8000000000001, 0xFFF0000000000001, 0x7FF4000000ABCDEF, 0xFFFFFFFFFFFFFFFF,
                     0x7FF0000000000001, 0xFFF8DEADBEEF0000], dtype=np.uint64)  # -nan, payloads, signalling, all ones


def hard_values(rng, family, shape):
    if family == 0:    # positive, equal but for the last 12 bits
        return 1.0 + rng.integers(0, 4096, size=shape) * 2.0 ** -52
    if family == 1:    # negative, equal but for the last 4 bits
        return -(1.0 + rng.integers(0, 16, size=shape) * 2.0 ** -52)
    if family == 2:    # subnormals and both zeros
        return rng.integers(-3, 4, size=shape) * 5e-324 * np.where(rng.random(shape) < 0.5, 1.0, -1.0)
    big = rng.standard_normal(shape) * 1e307  # most of these share the leading key digit of +-DBL_MAX, +-inf and (positive) NaN
    u = rng.random(shape)
    if family == 3:
        return np.where(u < 0.3, DBL_MAX, np.where(u < 0.6, -DBL_MAX, big))
    if family == 4:
        return np.where(u < 0.2, np.inf, np.where(u < 0.4, -np.inf, big))
    pick = rng.integers(0, 5, size=shape)  # family 5: all of them in one column
    out = np.empty(shape)
    for f in range(5):
        out = np.where(pick == f, hard_values(rng, f, shape), out)
    return out


N_FAMILIES = 6


@functools.lru_cache(maxsize=2)
def hard_store(shape):
    """(n_iter, C, size): normals over many binades; the hard families at elements 0 .. 5 and size - 6 .. size - 1 of every chain
    (the first column tile of chain 0 and the last, partial one of the last chain in the per-chain view; element size - 1 is the
    mixture); every (chain, element) live at a random set of iterations of random length, the rest NaN of assorted bit patterns"""
    n_iter, C, size = shape
    rng = np.random.default_rng(sum(shape))
    a = rng.standard_normal(shape) * np.exp(rng.uniform(-30, 30, size=(1, 1, size)))
    for f in range(N_FAMILIES):
        a[:, :, f] = hard_values(rng, f, (n_iter, C))
        a[:, :, size - 1 - (N_FAMILIES - 1 - f)] = hard_values(rng, f, (n_iter, C))
    live = rng.integers(0, n_iter + 1, size=(C, size))
    live[rng.random((C, size)) < 0.25] = n_iter      # a quarter of the columns whole (what omit_nan=False can be checked on)
    live[0::2, :N_FAMILIES] = n_iter                 # ... the hard columns of the even chains at the front among them
    live[1::2, size - N_FAMILIES:] = n_iter          # ... and of the odd chains at the back
    e = N_FAMILIES
    live[:, [e, e + 1, size - e - 1]] = 0            # elements no chain ever had,
    live[:, [e + 2, e + 3, size - e - 2]] = min(1, n_iter)  # that every chain had once,
    live[:, [e + 4, e + 5, size - e - 3]] = n_iter   # and that every chain always had
    # exactly live[c, e] iterations, at scattered places that differ from column to column
    place = (rng.permutation(n_iter).astype(np.int32).reshape(-1, 1, 1) + rng.integers(0, n_iter, size=(1, C, size), dtype=np.int32)) % n_iter
    dead = place >= live[None]
    bits = a.view(np.uint64)
    bits[dead] = NAN_BITS[rng.integers(0, len(NAN_BITS), size=int(dead.sum()))]
    assert np.array_equal(np.isnan(a), dead) and (n_iter - dead.sum(axis=0) == live).all()
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("shape,pooled,omit_nan,levels", Q_CASES,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}-{'pooled' if p else 'chain'}-{'nan' if o else 'prop'}" for s, p, o, _ in Q_CASES])
def test_store_quantiles_of_hard_padded_stores_are_numpys(shape, pooled, omit_nan, levels):
    n_iter, C, size = shape
    a = hard_store(shape)
    view = a.reshape(-1, size) if pooled else a
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "All-NaN slice encountered", inf - inf inside numpy's interpolation
        want = (np.nanquantile if omit_nan else np.quantile)(view, levels, axis=0)
    eng = make_engine(C)
    got = eng.store_quantiles(eng.to_device(a), levels, pooled=pooled, omit_nan=omit_nan).cpu().numpy()
    eng.check_status()
    eng.close()
    print(route(*view_shape(shape, pooled)), "columns NaN at every level:", int(np.isnan(want).all(axis=0).sum()), "of", want[0].size)
    assert same(got, want)


# -------------------------------------------------------------------------------------------------------------------- moments
M_STORES = [(549, 1, 37), (183, 3, 37), (1030, 2, 40), (7, 2, 5), (1, 3, 4)]
FAMILIES = [(0.0, 1.0), (-3e4, 5.0), (1e6, 1.0), (1e8, 1e-2)]  # (mean, sd) of column j: family j mod 4 -- every tile holds each
CONSTANTS = [1.5, 0.1, 1e300, -5e-324, -0.0]
U = 2.0 ** -53
_worst = {"var": 0.0, "mean": 0.0}


@functools.lru_cache(maxsize=None)
def moments_store(shape):
    n_iter, C, size = shape
    rng = np.random.default_rng(sum(shape) + 1)
    mu, sd = (np.array([FAMILIES[j % 4][i] for j in range(size)]) for i in (0, 1))
    a = mu + sd * rng.standard_normal(shape)
    a.setflags(write=False)
    return a


def exact_moments(x):
    """exact mean and unbiased variance of the columns of a finite (R, K) array, as Fractions: every double is an integer multiple
    of the column's smallest unit 2^s, and the sums of those integers and of their squares are Python integers"""
    R, K = x.shape
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)  # exact: 53 bits
    e = e.astype(np.int64) - 53
    s = e.min(axis=0)
    means, variances = [], []
    for k in range(K):
        col = [v << sh for v, sh in zip(mi[:, k].tolist(), (e[:, k] - s[k]).tolist())]
        s1, s2 = sum(col), sum(v * v for v in col)
        unit = Fraction(2) ** int(s[k])
        means.append(Fraction(s1, R) * unit)
        variances.append(Fraction(R * s2 - s1 * s1, R * (R - 1)) * unit * unit if R > 1 else Fraction(0))
    return means, variances


@functools.lru_cache(maxsize=None)
def exact_reference(shape, pooled):
    a = moments_store(shape)
    return exact_moments(a.reshape(-1, shape[2]) if pooled else a.reshape(shape[0], -1))


def device_moments(a, pooled):
    eng = make_engine(a.shape[1])
    t = eng.to_device(a)
    first = [v.cpu().numpy() for v in eng.store_moments(t, pooled=pooled)]
    again = [v.cpu().numpy() for v in eng.store_moments(t, pooled=pooled)]
    eng.check_status()
    eng.close()
    # the combination order is a function of the shape alone: a second call gives the same bits
    assert all(np.array_equal(f, g, equal_nan=True) and np.array_equal(np.signbit(f), np.signbit(g)) for f, g in zip(first, again))
    return first


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "chain"])
@pytest.mark.parametrize("shape", M_STORES, ids=lambda s: "x".join(map(str, s)))
def test_store_moments_within_the_bound_of_an_updating_algorithm(shape, pooled):
    """u = 2^-53, kappa = sqrt(1 + mean^2 / var) of the exact values: |var - exact| <= R kappa u exact (Chan, Golub & LeVeque's
    first-order bound for updating algorithms) and |mean - exact| <= R u max|x|."""
    a = moments_store(shape)
    x = a.reshape(-1, shape[2]) if pooled else a.reshape(shape[0], -1)
    R = x.shape[0]
    mean, var = (v.reshape(-1) for v in device_moments(a, pooled))
    want_mean, want_var = exact_reference(shape, pooled)
    assert mean.shape == var.shape == (x.shape[1],)
    if R == 1:
        assert np.array_equal(mean, x[0]) and np.all(var == 0.0)
        return
    r_var = r_mean = 0.0
    for k in range(x.shape[1]):
        kappa = float(1 + want_mean[k] ** 2 / want_var[k]) ** 0.5
        r_var = max(r_var, float(abs(Fraction(float(var[k])) - want_var[k])) / (R * kappa * U * float(want_var[k])))
        r_mean = max(r_mean, float(abs(Fraction(float(mean[k])) - want_mean[k])) / (R * U * np.max(np.abs(x[:, k]))))
    _worst["var"], _worst["mean"] = max(_worst["var"], r_var), max(_worst["mean"], r_mean)
    print(f"R = {R}: worst |error| / bound: variance {r_var:.3g}, mean {r_mean:.3g}; so far {_worst['var']:.3g}, {_worst['mean']:.3g}")
    assert r_var <= 1.0 and r_mean <= 1.0


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "chain"])
@pytest.mark.parametrize("shape", M_STORES, ids=lambda s: "x".join(map(str, s)))
def test_store_moments_of_constant_columns_are_exact(shape, pooled):
    """omc_moments.h: equal values give the mean exactly and m2 = 0 -- through the row lanes, the idle lanes and up to nine slices"""
    n_iter, C, size = shape
    value = np.array([CONSTANTS[j % len(CONSTANTS)] for j in range(size)])
    a = np.broadcast_to(value, shape).copy()
    mean, var = device_moments(a, pooled)
    assert np.array_equal(mean, np.broadcast_to(value, mean.shape))
    assert np.all(var == 0.0), var


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "chain"])
@pytest.mark.parametrize("shape", M_STORES, ids=lambda s: "x".join(map(str, s)))
def test_store_moments_with_non_finite_draws(shape, pooled):
    """One NaN in element 0, one +inf in element 1, +inf and -inf in element 2 (in different chains where there is one iteration
    only): NaN where numpy's mean and variance are NaN, numpy's infinite means, the other columns bit for bit what they were."""
    n_iter, C, size = shape
    clean = moments_store(shape)
    a = clean.copy()
    a[n_iter // 2, 0, 0] = np.nan
    a[n_iter - 1, C - 1, 1] = np.inf
    a[0, 0, 2], a[n_iter // 3, C - 1, 2] = np.inf, -np.inf
    touched = a != clean
    mean, var = device_moments(a, pooled)
    mean0, var0 = device_moments(clean, pooled)
    x = a.reshape(-1, size) if pooled else a
    hit = touched.reshape(x.shape).any(axis=0)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_mean = x.mean(axis=0)
        want_var = x.var(axis=0, ddof=1) if x.shape[0] > 1 else np.zeros(x.shape[1:])  # one draw: the variance is defined as 0
    assert hit.sum() >= 3 and np.isinf(want_mean).any() and np.isnan(want_mean).any()
    assert np.array_equal(np.isnan(mean), np.isnan(want_mean)), (mean[hit], want_mean[hit])
    assert np.array_equal(np.isnan(var), np.isnan(want_var)), (var[hit], want_var[hit])
    assert np.array_equal(mean[np.isinf(want_mean)], want_mean[np.isinf(want_mean)])
    assert np.array_equal(mean[~hit], mean0[~hit]) and np.array_equal(var[~hit], var0[~hit])


# ------------------------------------------------------------------------------------------------------------------- thinning
@pytest.mark.parametrize("shape,every,first", [((140001, 1, 3), 2, 0), ((140001, 1, 3), 1, 5), ((140001, 1, 3), 70000, 1), ((65536, 2, 1), 1, 0)],
                         ids=["140001x1x3-every2", "140001x1x3-every1-first5", "140001x1x3-every70000-first1", "65536x2x1-every1"])
def test_store_thin_beyond_one_launch(shape, every, first):
    """omc_store_thin walks its output in launches of 65 535 rows: 70 001 rows are two, 139 996 three, 65 536 one and one row"""
    a = np.random.default_rng(shape[0]).standard_normal(shape)
    eng = make_engine(shape[1])
    got = eng.store_thin(eng.to_device(a), every, first=first).cpu().numpy()
    eng.check_status()
    eng.close()
    assert got.shape == a[first::every].shape and np.array_equal(got, a[first::every])
