"""Column summaries of the pointwise Normal log-density of the device store (omc_store_loglik, Engine.store_loglik) against numpy.

Exact data.  y and the elements are integers in [-2^10, 2^10] times 2^-3 and tau = 1: log(1) = 0, r = y - x and 0.5 r are exact, and
ll = fma(-0.5 r, r, -c) is the one rounding of -c - 0.5 r^2 that numpy's `-c - 0.5 * r * r` makes: ll_out must be np.array_equal.

Rounded data, against np.longdouble from the same fp64 inputs, with u = 2^-53 and E = |0.5 log tau| + c + 0.5 tau r^2 per element:
  ll    within 4 u E: the device log at 1 ulp = 2 u relative (the figure of the HIP math API's table for fp64 log and exp; the ROCm
        documentation installed beside the compiler does not state one) gives 2 u |0.5 log tau|, the fused h = 0.5 log tau - c another
        u (|0.5 log tau| + c); r, the rounded product and the last fused multiply-add 3 u (0.5 tau r^2) + u E.
  lse   within 4 u E_max + (K + 4) u + u |lse|: the terms' own error moves the sum by at most 4 u E_max relative to it; a term then
        passes through K roundings -- additions and rescalings -- on its way into the sum, the 4 are its own exp (2 u), the final
        log of the sum (2 u of a number >= 1, as an absolute error of the logarithm no more), and u |lse| is the final addition.
        K = 2 ((L - 1) + (min(16, rows) - 1) + (slices - 1)) as omc_loglik.hip derives it from the shape; asserted <= 3 S.
  mean, var   the tolerances tests/test_store_gpu.py holds omc_store_moments to: 1e-12 of max |ll|, 1e-10 of the largest variance.

The kernel's tile is LL_COLS = 32 selection positions; slices are cut from 257 rows on (65 x 8 = 520 rows: three slices)."""

import ctypes as C

import numpy as np
import pytest
from psis_model import HALF_LOG_2PI, column_summaries, loglik

pytestmark = pytest.mark.gpu

TILE = 32
SHAPES = [(2, 1), (3, 5), (17, 7), (33, 8), (65, 8)]
N_IDX = [1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
GUARD = -12345.0
U = 2.0 ** -53


@pytest.fixture(scope="module")
def engines():
    from openmcmc_amd.engine import Engine

    made = {}

    def get(C):
        if C not in made:
            made[C] = Engine(C)
        return made[C]

    yield get
    for e in made.values():
        e.close()


def roundings(S, n):
    """(K, slices) of omc_loglik.hip for S rows and n selection positions"""
    tiles = -(-n // TILE)
    slices = max(1, min(-(-2048 // tiles), -(-S // 256), 1024))
    rows = -(-S // slices)
    return 2 * ((-(-rows // 16) - 1) + (min(16, rows) - 1) + (slices - 1)), slices


def make_index(rng, size, n):
    """unsorted, with repeats; n may exceed size"""
    return rng.integers(0, size, size=n).astype(np.int64)


def raw_call(eng, store, idx, y, prec, want="lmvp", n_iter=None, size=None, n_idx=None, prec_size=None, ctx=True):
    """omc_store_loglik itself on guarded outputs: (status, {name: host array}, guards intact)"""
    import torch

    from openmcmc_amd._abi import lib

    N, Cc, sz = store.shape
    n = sz if idx is None else idx.numel()
    n = n if n_idx is None else n_idx
    bufs = {}
    for name, length in (("l", max(n, 1)), ("m", max(n, 1)), ("v", max(n, 1)), ("p", N * Cc * max(n, 1))):
        bufs[name] = eng.full((length + 64,), GUARD) if name in want else None
    ptr = lambda t: None if t is None else t.data_ptr()
    st = lib.omc_store_loglik(eng._ctx if ctx else None, N if n_iter is None else n_iter, sz if size is None else size, ptr(store),
                              ptr(idx), n, ptr(y), ptr(prec), (0 if prec is None else prec.shape[2]) if prec_size is None else prec_size,
                              ptr(bufs["l"]), ptr(bufs["m"]), ptr(bufs["v"]), ptr(bufs["p"]))
    torch.cuda.synchronize()
    host = {k: (None if b is None else b.cpu().numpy()) for k, b in bufs.items()}
    return st, host


def run_case(eng, x, y, tau, idx, exact):
    """x (N, C, size), y (n,), tau (N, C, 1 or n), idx or None: every output against the restatement"""
    N, Cc, size = x.shape
    S = N * Cc
    sel = x.reshape(S, size) if idx is None else x.reshape(S, size)[:, idx]
    n = sel.shape[1]
    st, host = raw_call(eng, eng.to_device(x), None if idx is None else eng._store_index(idx, size)[0], eng.to_device(y), eng.to_device(tau))
    assert st == 0
    for name, length in (("l", n), ("m", n), ("v", n), ("p", S * n)):
        assert np.all(host[name][length:] == GUARD), name
    ll = host["p"][: S * n].reshape(S, n)
    t2 = tau.reshape(S, -1)
    ref = loglik(sel, y, t2, np.longdouble)
    r = y[None, :] - sel
    E = np.abs(0.5 * np.log(t2)) + HALF_LOG_2PI + 0.5 * t2 * r * r
    if exact:
        assert np.array_equal(ll, -HALF_LOG_2PI - 0.5 * r * r), (N, Cc, size, n)
    err = np.abs(ll - ref).astype(np.float64)
    print("ll", (N, Cc, size, n), "worst error / (u E)", float(np.max(err / (U * E))))
    assert np.all(err <= 4 * U * E)
    lse, mean, var = (a.astype(np.float64) for a in column_summaries(ref))
    K, _ = roundings(S, n)
    assert K <= 3 * S
    bound = 4 * U * E.max(axis=0) + (K + 4) * U + U * np.abs(lse)
    print("lse worst error / bound", float(np.max(np.abs(host["l"][:n] - lse) / bound)), "K", K)
    assert np.all(np.abs(host["l"][:n] - lse) <= bound)
    assert np.all(np.abs(host["m"][:n] - mean) <= 1e-12 * np.abs(ll).max())
    assert np.all(np.abs(host["v"][:n] - var) <= 1e-10 * max(var.max(), np.finfo(float).tiny))
    return host


@pytest.mark.parametrize("n_iter,C", SHAPES)
def test_exact_dyadic_grid(engines, n_iter, C):
    """every n_idx at the tile's and a pair's edges: without an index (size = n_idx, odd and even: the even ones take the 16-byte
    loads) and with one over an odd and an even size; a scalar and a vector precision"""
    eng = engines(C)
    rng = np.random.default_rng(100 * n_iter + C)
    for j, n in enumerate(N_IDX):
        for with_index in (False, True):
            size = (7 if j % 2 else 10) if with_index else n
            x = rng.integers(-1024, 1025, size=(n_iter, C, size)) / 8.0
            y = rng.integers(-1024, 1025, size=n) / 8.0
            idx = make_index(rng, size, n) if with_index else None
            for prec_cols in (1, n):
                run_case(eng, x, y, np.ones((n_iter, C, prec_cols)), idx, exact=True)


@pytest.mark.parametrize("n_iter,C", SHAPES)
def test_rounded_data_within_the_derived_bounds(engines, n_iter, C):
    eng = engines(C)
    rng = np.random.default_rng(7 * n_iter + C)
    for j, n in enumerate(N_IDX):
        for with_index in (False, True):
            size = (9 if j % 2 else 12) if with_index else n
            x = rng.standard_normal((n_iter, C, size)) * rng.choice([0.1, 1.0, 5.0], size=size)
            y = rng.standard_normal(n) * 3
            idx = make_index(rng, size, n) if with_index else None
            for prec_cols in (1, n):
                run_case(eng, x, y, rng.gamma(2.0, 2.0, size=(n_iter, C, prec_cols)) + 1e-3, idx, exact=False)


def test_constant_column(engines):
    """var == 0, mean == ll, lse within 2 ulp of ll + log(S): the exact sum is the integer S in any order"""
    for n_iter, C in SHAPES:
        eng = engines(C)
        S = n_iter * C
        x = np.tile(np.array([16.0, -20.5, 3.125]), (n_iter, C, 1))
        y = np.array([0.0, 0.5, -12.0])
        st, host = raw_call(eng, eng.to_device(x), None, eng.to_device(y), eng.to_device(np.ones((n_iter, C, 1))))
        assert st == 0
        r = y - x[0, 0]
        ll = -HALF_LOG_2PI - 0.5 * r * r
        assert np.array_equal(host["v"][:3], np.zeros(3)) and np.array_equal(host["m"][:3], ll)
        want = ll + np.log(S)
        assert np.all(np.abs(host["l"][:3] - want) <= 2 * np.spacing(np.abs(want))), (host["l"][:3], want)


def test_two_load_forms_and_repeated_calls_give_the_same_bits(engines):
    """the same rows 16-byte aligned (16-byte loads) and 8 bytes off (8-byte loads), and the same call twice"""
    n_iter, C, size = 65, 8, 34
    eng = engines(C)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n_iter, C, size))
    y, tau = eng.to_device(rng.standard_normal(size)), eng.to_device(rng.gamma(3.0, 1.0, size=(n_iter, C, 1)))
    flat = eng.empty(x.size + 1)
    outs = []
    for off in (0, 1, 0):
        store = flat[off: off + x.size].view(n_iter, C, size)
        store.copy_(eng.to_device(x))
        assert store.data_ptr() % 16 == 8 * off
        outs.append([t.cpu().numpy() for t in eng.store_loglik(store, y, tau, ll=True)])
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    for a, b in zip(outs[0], outs[2]):
        assert np.array_equal(a, b)
    idx = np.arange(size)  # the identity selection through the index path: the same bits again
    for a, b in zip(outs[0], eng.store_loglik(flat[:x.size].view(n_iter, C, size), y, tau, index=idx, ll=True)):
        assert np.array_equal(a, b.cpu().numpy())


@pytest.mark.parametrize("prec_cols", [1, 5])
def test_non_finite_terms_touch_their_own_columns_only(engines, prec_cols):
    n_iter, C, size = 33, 8, 5
    eng = engines(C)
    S = n_iter * C
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n_iter, C, size))
    y = rng.standard_normal(size)
    tau = rng.gamma(3.0, 1.0, size=(n_iter, C, prec_cols))
    clean = run_case(eng, x, y, tau, None, exact=False)
    for kind, value in (("x", np.nan), ("x", np.inf), ("x", -np.inf), ("tau", 0.0), ("tau", -1.0), ("tau", np.nan)):
        xb, tb = x.copy(), tau.copy()
        if kind == "x":
            xb[n_iter // 2, C - 1, 2] = value
            hit = [2]
        else:
            tb[n_iter - 1, 0, prec_cols // 2] = value
            hit = [0, 1, 2, 3, 4] if prec_cols == 1 else [prec_cols // 2]
        st, host = raw_call(eng, eng.to_device(xb), None, eng.to_device(y), eng.to_device(tb))
        assert st == 0
        keep = [k for k in range(size) if k not in hit]
        for name in "lmv":
            assert np.all(np.isnan(host[name][hit])), (kind, value, name)
            assert np.array_equal(host[name][keep], clean[name][keep]), (kind, value, name)
            assert np.all(host[name][size:] == GUARD)
        with np.errstate(all="ignore"):
            want = loglik(xb.reshape(S, size), y, tb.reshape(S, -1))
        got = host["p"][: S * size].reshape(S, size)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), (kind, value)
        assert np.array_equal(np.sign(got[np.isinf(got)]), np.sign(want[np.isinf(want)]))
        fin = np.isfinite(want)
        assert np.array_equal(got[fin], clean["p"][: S * size].reshape(S, size)[fin])


def test_invalid_arguments_leave_the_outputs_untouched(engines):
    from openmcmc_amd._abi import INVALID_ARG, lib

    eng = engines(5)
    rng = np.random.default_rng(1)
    store = eng.to_device(rng.standard_normal((3, 5, 4)))
    y, prec = eng.to_device(rng.standard_normal(4)), eng.to_device(np.ones((3, 5, 1)))
    bad_idx = eng._store_index([0, 4, 1, 2], 4)[0]
    low_idx = eng._store_index([0, -1, 1, 2], 4)[0]
    one = engines(1)
    cases = {
        "no context": dict(ctx=False),
        "fewer than 2": dict(eng=one, store=one.to_device(np.zeros((1, 1, 4))), prec=one.to_device(np.ones((1, 1, 1)))),
        "size < 1": dict(size=0),
        "n_idx < 1": dict(n_idx=0),
        "n_idx != size": dict(n_idx=3),
        "prec_size": dict(prec_size=2),
        "NULL:store": dict(store_null=True),
        "NULL:y": dict(y=None),
        "NULL:prec": dict(prec=None, prec_size=1),
        "every output": dict(want=""),
        "index outside": dict(idx=bad_idx),
        "index outside (negative)": dict(idx=low_idx),
    }
    for what, kw in cases.items():
        e = kw.pop("eng", eng)
        s = kw.pop("store", store)
        args = dict(idx=None, y=y if e is eng else e.to_device(np.zeros(4)), prec=prec, want="lmvp")
        args.update(kw)
        null = args.pop("store_null", False)
        if null:
            class Null:  # a store whose pointer is NULL
                shape = s.shape

                @staticmethod
                def data_ptr():
                    return None
            s = Null
        st, host = raw_call(e, s, args.pop("idx"), args.pop("y"), args.pop("prec"), **args)
        assert st == INVALID_ARG, what
        assert lib.omc_last_error(), what
        for name, h in host.items():
            assert h is None or np.all(h == GUARD), (what, name)
    with pytest.raises(ValueError, match="index outside"):
        eng.store_loglik(store, y, prec, index=[0, 4, 1, 2])
    with pytest.raises(ValueError):
        eng.store_loglik(store, y, prec, lse=False, mean=False, var=False)
    assert C.c_char_p(lib.omc_last_error()).value
