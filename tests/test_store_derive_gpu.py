"""Per-draw reductions of the device store (omc_store_reduce, Engine.store_reduce, MCMC.derive, MCMC.simultaneous_band) against
the numpy restatement of the table in include/omcmc_hip.h written here.  MIN, MAX, ARGMIN, ARGMAX, COUNT_ABOVE, SUPNORM and the
count are compared with np.array_equal(..., equal_nan=True): every term is at most one rounded subtraction and one rounded
division on identical inputs.  SUM is held to |got - math.fsum(terms)| <= n_idx 2^-53 sum|terms| per row, the worst case of any
order of n_idx - 1 additions of rounded or fused products (each of the n_idx roundings is at most 2^-53 of a partial sum, and no
partial sum exceeds sum|terms| in magnitude to first order; the products' own roundings, where fused away, are within the same
2^-53 |term| each) -- derived, not measured."""

import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPS = {"sum": 0, "min": 1, "max": 2, "argmin": 3, "argmax": 4, "count_above": 5, "supnorm": 6}
EXACT = ("min", "max", "argmin", "argmax", "count_above", "supnorm")
SIZES = [1, 2, 3, 20, 63, 64, 65, 127, 257, 1001]
CHAINS = [1, 3, 70]
ALGOS = (0, 1, 2)


# ---------------------------------------------------------------------------------------------------------- restatement
def terms_of(sel, op, a=None, b=None):
    """(R, n) terms of the selected elements sel (R, n); a, b (n,)"""
    with np.errstate(all="ignore"):
        if op == "sum" and a is not None:
            return a[None, :] * sel
        if op == "supnorm":
            return np.abs(sel - a[None, :]) / b[None, :]
    return sel


def reduce_ref(x, op, idx=None, omit_nan=True, a=None, b=None):
    """(out, count) of rows x (R, size); "sum" gives (exact sums by math.fsum, sum|terms|) per row in out, NaN where a term is not
    finite -- those rows are in the third result: numpy's own sum of the terms"""
    sel = x if idx is None else x[:, idx]
    R, n = sel.shape
    term = terms_of(sel, op, a, b)
    nan = np.isnan(term)
    cnt = (~nan).sum(axis=1).astype(np.int64)
    if op == "count_above":
        return (sel > a[None, :]).sum(axis=1).astype(np.float64), cnt
    if op == "sum":
        exact, mag, plain = np.empty(R), np.empty(R), np.full(R, np.nan)
        for r in range(R):
            t = term[r][~nan[r]] if omit_nan else term[r]
            if np.isfinite(t).all():
                exact[r], mag[r] = math.fsum(t), math.fsum(np.abs(t))
            else:
                exact[r] = mag[r] = np.nan
                with np.errstate(all="ignore"):
                    plain[r] = np.sum(t)
        return (exact, mag, plain), cnt
    up = op in ("max", "argmax", "supnorm")
    masked = np.where(nan, -np.inf if up else np.inf, term)
    best = masked.max(axis=1) if up else masked.min(axis=1)
    hit = ~nan & (term == best[:, None])  # -0.0 == 0.0: the first of them
    pos = np.argmax(hit, axis=1)
    val = term[np.arange(R), pos]
    empty = cnt == 0  # by hand: np.nanargmax raises and np.nanmax warns on a row without a number
    if not omit_nan:
        has = nan.any(axis=1)
        pos = np.where(has, np.argmax(nan, axis=1), pos)  # numpy's rule: the first NaN
        val = np.where(has, np.nan, val)
        empty = np.zeros(R, dtype=bool)
    out = pos.astype(np.float64) if op in ("argmin", "argmax") else val
    return np.where(empty, np.nan, out), cnt


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def assert_sum(got, want, n, what):
    exact, mag, plain = want
    fin = ~np.isnan(exact)
    err, bound = np.abs(got[fin] - exact[fin]), n * 2.0 ** -53 * mag[fin]
    assert np.all(err <= bound), (what, float(np.max(err - bound)))
    assert same(got[~fin], plain[~fin]), what  # NaN and infinite rows: by isnan and equality


def engine(C, **options):
    from openmcmc_amd.engine import Engine

    eng = Engine(C, seed=1)
    for name, value in options.items():
        eng.set_option(name, value)
    return eng


def device(eng, x):
    return eng.to_device(np.ascontiguousarray(x))


def run(eng, d, op, **kw):
    out, cnt = eng.store_reduce(d, op, **kw)
    return out.cpu().numpy().ravel(), cnt.cpu().numpy().ravel()


# ---------------------------------------------------------------------------------------------------------- inputs
def stores(N, C, size, seed):
    """{kind: (N, C, size)}: normal draws; ragged rows (the first m slots valid, the rest NaN, m from 0 to size); rows with +-inf;
    rows of a few values with tied extremes, -0.0 beside 0.0, and a first column that never moves"""
    rng = np.random.default_rng(seed)
    R = N * C
    normal = rng.standard_normal((R, size))
    ms = np.arange(size + 1) if size + 1 <= R else np.unique(np.concatenate([[0, 1, size - 1, size], rng.integers(0, size + 1, R)]))
    ragged = rng.standard_normal((R, size))
    for r in range(R):
        ragged[r, ms[r % len(ms)]:] = np.nan
    inf = rng.standard_normal((R, size))
    inf[rng.random((R, size)) < 0.15] = np.inf
    inf[rng.random((R, size)) < 0.15] = -np.inf
    inf[rng.random((R, size)) < 0.05] = np.nan
    ties = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0]), size=(R, size))
    ties[::3] = rng.choice(np.array([-0.0, 0.0]), size=ties[::3].shape)  # the extreme is a zero of either sign
    ties[:, 0] = 1.0
    return {k: v.reshape(N, C, size) for k, v in (("normal", normal), ("ragged", ragged), ("inf", inf), ("ties", ties))}


def indices(size, rng):
    sub = rng.permutation(size)[: max(1, size // 2)]
    return [None, np.array([size // 2]), np.concatenate([sub, sub[:2], sub[:1]]), rng.integers(0, size, size + 7)]


def vectors(size, rng):
    """per element: weights, thresholds, centres, scales (one scale 0 under a centre the ties store sits on: 0 / 0)"""
    w, thr, cen, sc = rng.standard_normal(size), 0.3 * rng.standard_normal(size), 0.1 * rng.standard_normal(size), rng.uniform(0.5, 2.0, size)
    cen[0], sc[0] = 1.0, 0.0
    return w, thr, cen, sc


def variants(idx, size, vec):
    """(label, op, a, b) of every op, the vectors aligned with the selection"""
    w, thr, cen, sc = (v if idx is None else v[idx] for v in vec)
    return [("sum", "sum", None, None), ("sum weighted", "sum", w, None), ("min", "min", None, None), ("max", "max", None, None),
            ("argmin", "argmin", None, None), ("argmax", "argmax", None, None), ("count_above", "count_above", thr, None),
            ("supnorm", "supnorm", cen, sc)]


# ---------------------------------------------------------------------------------------------------------- 1. the table
@pytest.mark.parametrize("C", CHAINS)
@pytest.mark.parametrize("size", SIZES)
def test_every_op_matches_the_restatement(size, C):
    rng = np.random.default_rng(1000 * size + C)
    vec = vectors(size, rng)
    idxs = indices(size, rng)
    eng = engine(C)
    for N in (1, 5):
        for kind, x in stores(N, C, size, seed=7 * size + C + N).items():
            d = device(eng, x)
            rows = x.reshape(N * C, size)
            for idx in idxs:
                n = size if idx is None else len(idx)
                for label, op, a, b in variants(idx, size, vec):
                    for omit in (True, False):
                        want, want_cnt = reduce_ref(rows, op, idx, omit, a, b)
                        got = {}
                        for algo in ALGOS:
                            eng.set_option("reduce_algo", algo)
                            out, cnt = run(eng, d, op, index=idx, omit_nan=omit, a=a, b=b)
                            what = (kind, N, n, label, omit, algo)
                            assert same(cnt, want_cnt), what
                            if op == "sum":
                                assert_sum(out, want, n, what)
                                again, _ = run(eng, d, op, index=idx, omit_nan=omit, a=a, b=b)
                                assert out.tobytes() == again.tobytes(), what  # a repeated call is bit-equal under each form
                            else:
                                assert same(out, want), (what, out, want)
                            got[algo] = out
                        if op != "sum":
                            assert same(got[1], got[2]) and same(got[0], got[2]), (kind, N, n, label, omit)  # the two forms agree
    eng.set_option("reduce_algo", 0)
    eng.close()


def test_the_ragged_store_has_every_live_length():
    x = stores(5, 70, 20, seed=3)["ragged"].reshape(350, 20)
    live = (~np.isnan(x)).sum(axis=1)
    assert set(live.tolist()) == set(range(21))  # all-NaN rows included
    assert np.isnan(reduce_ref(x, "max")[0][live == 0]).all() and np.all(reduce_ref(x, "sum")[0][0][live == 0] == 0.0)


# ---------------------------------------------------------------------------------------------------------- 2. scale of the terms
@pytest.mark.parametrize("weighted", [False, True])
def test_sum_of_terms_over_sixteen_decades(weighted):
    N, C, size = 5, 3, 257
    rng = np.random.default_rng(21)
    x = (rng.standard_normal((N, C, size)) * 10.0 ** rng.uniform(-8, 8, (N, C, size)))
    a = rng.standard_normal(size) if weighted else None
    assert np.abs(x).max() / np.abs(x).min() > 1e14
    want, _ = reduce_ref(x.reshape(N * C, size), "sum", None, True, a)
    eng = engine(C)
    d = device(eng, x)
    for algo in ALGOS:
        eng.set_option("reduce_algo", algo)
        out, _ = run(eng, d, "sum", a=a)
        print("algo", algo, "largest error / bound", np.max(np.abs(out - want[0]) / (size * 2.0 ** -53 * want[1])))
        assert_sum(out, want, size, algo)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 3. rows cut over four waves
def test_a_row_long_enough_for_four_waves():
    """32768 selected elements and more: the long form cuts the row over the four waves of a workgroup (odd size: every second
    row starts 8 bytes off a 16-byte boundary)"""
    N, C, size = 2, 3, 32771
    rng = np.random.default_rng(22)
    x = rng.standard_normal((N, C, size))
    x[1, 1, 5] = x[1, 1, 30000] = 9.0  # a tie across two pieces
    x[0, 2, 40:50] = np.nan
    rows = x.reshape(N * C, size)
    eng = engine(C, reduce_algo=2)
    d = device(eng, x)
    for op in ("max", "argmax", "argmin", "min"):
        for omit in (True, False):
            want, want_cnt = reduce_ref(rows, op, None, omit)
            out, cnt = run(eng, d, op, omit_nan=omit)
            assert same(out, want) and same(cnt, want_cnt), (op, omit)
    want, _ = reduce_ref(rows, "sum")
    out, _ = run(eng, d, "sum")
    assert_sum(out, want, size, "sum")
    assert out.tobytes() == run(eng, d, "sum")[0].tobytes()
    idx = rng.integers(0, size, 40000)
    want, want_cnt = reduce_ref(rows, "argmax", idx)
    out, cnt = run(eng, d, "argmax", index=idx)
    assert same(out, want) and same(cnt, want_cnt)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 4. errors
def abi(eng, d, op, idx=None, a=None, b=None, out=None, cnt=None, n_iter=None, size=None):
    from openmcmc_amd import _abi

    N, _, sz = d.shape
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    st = _abi.lib.omc_store_reduce(eng._ctx, N if n_iter is None else n_iter, sz if size is None else size, d.data_ptr(), p(idx),
                                   sz if idx is None else idx.numel(), op, 1, p(a), p(b), p(out), p(cnt))
    return st, _abi.lib.omc_last_error().decode()


def test_invalid_calls_say_why_and_write_nothing():
    import torch

    from openmcmc_amd import _abi

    N, C, size = 4, 3, 5
    eng = engine(C)
    d = device(eng, np.random.default_rng(23).standard_normal((N, C, size)))
    vec = eng.to_device(np.ones(size))
    sentinel = lambda: (eng.full((N, C), -7.0), torch.full((N, C), -7, dtype=torch.int64, device=d.device))  # noqa: E731

    def untouched(out, cnt):
        eng.synchronize()
        return np.all(out.cpu().numpy() == -7.0) and np.all(cnt.cpu().numpy() == -7)

    for algo in ALGOS:
        eng.set_option("reduce_algo", algo)
        for bad in ([0, 1, size], [-1, 2, 3]):
            idx = torch.as_tensor(bad, dtype=torch.int64, device=d.device)
            out, cnt = sentinel()
            st, text = abi(eng, d, OPS["max"], idx=idx, out=out, cnt=cnt)
            assert st == _abi.INVALID_ARG and "index outside" in text and untouched(out, cnt)
            with pytest.raises(ValueError, match="index outside"):
                eng.store_reduce(d, "max", index=bad)
    eng.set_option("reduce_algo", 0)
    for op, kw, text_has in ((7, {}, "unknown op"), (-1, {}, "unknown op"), (OPS["supnorm"], {"a": vec}, "SUPNORM"),
                             (OPS["supnorm"], {"b": vec}, "SUPNORM"), (OPS["count_above"], {}, "COUNT_ABOVE"),
                             (OPS["max"], {"n_iter": 0}, "n_iter"), (OPS["max"], {"size": 0}, "size")):
        out, cnt = sentinel()
        st, text = abi(eng, d, op, out=out, cnt=cnt, **kw)
        assert st == _abi.INVALID_ARG and text_has in text and untouched(out, cnt), (op, kw, text)
    with pytest.raises(ValueError, match="unknown reduction"):
        eng.store_reduce(d, "median")
    with pytest.raises(ValueError, match="SUPNORM"):
        eng.store_reduce(d, "supnorm", a=0.0)  # no scale
    with pytest.raises(ValueError, match="COUNT_ABOVE"):
        eng.store_reduce(d, "count_above")  # no threshold
    with pytest.raises(ValueError, match="one value per selected element"):
        eng.store_reduce(d, "sum", index=[0, 1], a=np.ones(size))  # aligned with the selection, not with size
    with pytest.raises(ValueError):
        eng.set_option("reduce_algo", 3)
    # count_out may be NULL; scalars are broadcast; device tensors are taken as they are
    out = eng.full((N, C), -7.0)
    assert abi(eng, d, OPS["sum"], out=out)[0] == _abi.OK
    x = d.cpu().numpy().reshape(N * C, size)
    assert np.allclose(out.cpu().numpy().ravel(), x.sum(axis=1), rtol=1e-14)
    assert same(run(eng, d, "count_above", a=0.25)[0], (x > 0.25).sum(axis=1).astype(float))
    assert same(run(eng, d, "supnorm", a=vec, b=2.0)[0], (np.abs(x - 1.0) / 2.0).max(axis=1))
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 5. public API
def store_of(out, key):
    """(n_iter, C, size) host array of a collect() entry"""
    arr = out[key] if key != "log_post" else np.transpose(out[key], (0, 2, 1))  # (C, size, n_iter)
    return np.ascontiguousarray(np.transpose(arr, (2, 0, 1)))


def derive_ref(x, reduce, index=None, omit_nan=True, **vec):
    """(n_iter, C) of a host store x (n_iter, C, size): MCMC.derive in numpy"""
    N, C, size = x.shape
    rows = x.reshape(N * C, size)
    idx = None if index is None else np.asarray(index)
    n = size if idx is None else len(idx)
    full = lambda v: None if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))  # noqa: E731
    if reduce in ("sum", "mean", "count"):
        (exact, _, _), cnt = reduce_ref(rows, "sum", idx, omit_nan, full(vec.get("weights")))
        with np.errstate(all="ignore"):
            out = {"sum": exact, "mean": exact / cnt, "count": cnt.astype(np.float64)}[reduce]
    else:
        a = full(vec.get("threshold") if reduce == "count_above" else vec.get("center"))
        out, _ = reduce_ref(rows, reduce, idx, omit_nan, a, full(vec.get("scale")))
    return out.reshape(N, C)


@pytest.fixture(scope="module")
def gmrf_run(golden):
    from test_mcmc_api_gpu import build

    M, _ = build(golden("gmrf_chain"), "sparse_", True, 6, fuse=True, n_burn=5, n_iter=300, seed=5)
    M.run_mcmc()
    yield M, store_of(M.collect(), "b")
    M.engine.close()


def test_mcmc_derive_gmrf(gmrf_run):
    M, x = gmrf_run
    N, C, n = x.shape
    rng = np.random.default_rng(31)
    index = [n - 1, 0, 3, 0]
    mean, sd = x.reshape(N * C, n).mean(axis=0), x.reshape(N * C, n).std(axis=0, ddof=1)
    cases = [("max", None, {}), ("argmax", None, {}), ("min", index, {}), ("argmin", index, {}), ("count", None, {}),
             ("count_above", None, {"threshold": float(np.median(x))}), ("count_above", index, {"threshold": mean[index]}),
             ("supnorm", None, {"center": mean, "scale": sd}), ("supnorm", index, {"center": 0.0, "scale": sd[index]})]
    for reduce, idx, vec in cases:
        got = M.derive("b", reduce, index=idx, **vec)
        assert got.shape == (N, C) and same(got, derive_ref(x, reduce, idx, **vec)), reduce
    for reduce, idx, vec in (("sum", None, {}), ("sum", index, {"weights": rng.standard_normal(4)}), ("mean", None, {})):
        got, want = M.derive("b", reduce, index=idx, **vec), derive_ref(x, reduce, idx, **vec)
        k = n if idx is None else len(idx)
        w = np.broadcast_to(np.asarray(vec.get("weights", 1.0)), (k,))
        mag = np.abs((x if idx is None else x[:, :, idx]) * w).sum(axis=2)
        # the mean: the sum's bound over the count, and one rounding of the division on either side (each at most 2^-53 sum|terms| / k)
        bound = (k + 2) * 2.0 ** -53 * mag / k if reduce == "mean" else k * 2.0 ** -53 * mag
        assert np.all(np.abs(got - want) <= bound), reduce
    lp = store_of(M.collect(), "log_post")
    assert same(M.derive("log_post", "max"), lp[:, :, 0])  # a 2-D entry is one element
    for bad in ({"weights": 1.0}, {"scale": 1.0}, {"threshold": 0.0}):
        with pytest.raises(ValueError, match="does not apply"):
            M.derive("b", "max", **bad)
    with pytest.raises(ValueError, match="unknown reduce"):
        M.derive("b", "median")


def test_summaries_accept_a_derived_entry(gmrf_run):
    from test_store_diagnostics_gpu import RTOL, restate
    from test_store_hdi_gpu import hdi_want
    from test_store_rank_diagnostics_gpu import assert_diag, rank_restate

    M, x = gmrf_run
    N, C, n = x.shape
    before = set(M.store)
    got = M.derive("b", "max", name="b_max")
    want = derive_ref(x, "max")
    assert same(got, want) and set(M.store) == before | {"b_max"} and tuple(M.store["b_max"].shape) == (N, C, 1)
    d = want[:, :, None]  # the derived quantity as a store (n_iter, C, 1)
    flat = want.ravel()
    assert same(M.hdi("b_max"), hdi_want(d, [0.94])[0])
    assert same(M.hdi("b_max", pooled=False), hdi_want(d, [0.94], pooled=False)[0])
    q = [0.05, 0.5, 0.95]
    assert same(M.quantiles("b_max", q), np.quantile(flat, q)[:, None])
    assert same(M.quantiles("b_max", q, pooled=False), np.quantile(want, q, axis=0)[:, :, None])
    hist, edges = M.histogram("b_max", bins=12)
    wh, we = np.histogram(flat, bins=12)
    assert np.array_equal(hist[0], wh) and np.array_equal(edges[0], we)
    rhat, ess, _ = restate(d)
    diag = M.diagnostics("b_max")
    np.testing.assert_allclose(diag["rhat"], rhat, rtol=RTOL, atol=0)
    np.testing.assert_allclose(diag["ess"], ess, rtol=RTOL, atol=0)
    np.testing.assert_allclose(diag["mcse_mean"], flat.std(ddof=1) / np.sqrt(ess), rtol=1e-8, atol=0)
    rd = M.rank_diagnostics("b_max")
    assert_diag((rd["rhat"], rd["ess_bulk"], rd["ess_tail"]), rank_restate(d))
    mean, var = M.summary("b_max")
    np.testing.assert_allclose(mean, [flat.mean()], rtol=1e-12)
    np.testing.assert_allclose(var, [flat.var(ddof=1)], rtol=1e-10)
    out = M.collect()
    assert out["b_max"].shape == (C, 1, N) and same(out["b_max"][:, 0, :], want.T)  # a scalar parameter of the run
    # a derived name may be derived again; a name of the run may not be taken
    assert same(M.derive("b", "min", name="b_max"), derive_ref(x, "min")) and same(M.collect()["b_max"][:, 0, :], derive_ref(x, "min").T)
    for taken in ("b", "lambda", "log_post"):
        with pytest.raises(ValueError, match="store entry of the run"):
            M.derive("b", "max", name=taken)
    assert same(store_of(M.collect(), "b"), x)  # the store itself is untouched
    del M.store["b_max"]
    M._derived.discard("b_max")


def band_ref(x, mean, sd, prob):
    N, C, n = x.shape
    with np.errstate(all="ignore"):
        term = np.abs(x.reshape(N * C, n) - mean[None, :]) / sd[None, :]
    m = np.where(np.isnan(term).all(axis=1), np.nan, np.max(np.where(np.isnan(term), -np.inf, term), axis=1))
    critical = np.quantile(m[~np.isnan(m)], prob)
    return critical, mean - critical * sd, mean + critical * sd


def test_simultaneous_band(gmrf_run):
    M, x = gmrf_run
    N, C, n = x.shape
    t = M._store_3d("b")
    mean_d, var_d = (v.cpu().numpy() for v in M.engine.store_moments(t, pooled=True))  # the restatement's inputs
    for prob, index in ((0.95, None), (0.5, [n - 1, 0, 3, 0]), (0.99, list(range(1, n, 2)))):
        sel = x if index is None else x[:, :, index]
        mean, sd = (mean_d, np.sqrt(var_d)) if index is None else (mean_d[index], np.sqrt(var_d[index]))
        band = M.simultaneous_band("b", prob=prob, index=index)
        critical, lower, upper = band_ref(sel, mean, sd, prob)
        assert isinstance(band["critical"], float) and band["critical"] == critical
        assert same(band["lower"], lower) and same(band["upper"], upper) and same(band["mean"], mean) and same(band["sd"], sd)
        inside = np.all((sel >= lower) & (sel <= upper), axis=2).mean()
        pointwise = np.all((sel >= np.quantile(sel, (1 - prob) / 2, axis=(0, 1))) & (sel <= np.quantile(sel, (1 + prob) / 2, axis=(0, 1))), axis=2).mean()
        print("prob", prob, "critical", critical, "whole draws inside the band", inside, "inside the pointwise intervals", pointwise)
        # at least floor((R - 1) prob) + 1 of the R draws have m <= critical; one more may fall out where mean -/+ critical sd rounds
        assert inside >= prob - 2.0 / (N * C) and (len(mean) < 8 or pointwise < inside)
    for prob in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            M.simultaneous_band("b", prob=prob)
    with pytest.raises(ValueError):
        M.simultaneous_band("b", index=[n])


def test_band_ignores_elements_that_never_move_and_padding():
    """an element that never moves (sd = 0: 0 / 0) and a NaN-padded element do not change the critical value"""
    from openmcmc_amd.mcmc import MCMC

    N, C, n = 40, 3, 9
    x = np.random.default_rng(41).standard_normal((N, C, n + 2))
    x[:, :, n] = 2.5
    x[:, :, n + 1] = np.nan
    x[::2, :, n + 1] = 1.0
    M = MCMC.__new__(MCMC)  # the summaries need the engine, the store and the ring fields only
    M.engine = engine(C)
    M.store, M._derived, M.store_ring, M._n_dev, M.n_iter = {"f": device(M.engine, x)}, set(), 0, N, N
    plain = M.simultaneous_band("f", index=list(range(n)))
    both = M.simultaneous_band("f")
    assert both["critical"] == plain["critical"] and same(both["lower"][:n], plain["lower"]) and same(both["upper"][:n], plain["upper"])
    assert both["sd"][n] == 0.0 and both["lower"][n] == both["upper"][n] == 2.5 and np.isnan(both["lower"][n + 1])
    m = M.derive("f", "supnorm", center=both["mean"], scale=both["sd"], name="m")
    assert not np.isnan(m).any() and same(M.quantiles("m", [0.95]), np.quantile(m.ravel(), [0.95])[:, None])
    M.engine.close()


def test_mcmc_derive_of_a_reversible_jump_store(golden):
    from test_rj_chain_gpu import run_with_tape

    G = golden("rj_gmrf_chain")
    chains = np.arange(min(4, G["init_k"].shape[0]))
    n_iter = 40
    M, _, _ = run_with_tape(G, chains, n_iter)
    M.run_mcmc()
    out = M.collect()
    theta, beta, k = (store_of(out, key) for key in ("theta", "beta", "n_basis"))
    assert np.isnan(theta).any()
    live = M.derive("theta", "count", name="live")
    assert same(live, k[:, :, 0]) and same(live, derive_ref(theta, "count"))  # the stored count parameter, in every draw
    total, want = M.derive("beta", "sum", name="total"), derive_ref(beta, "sum")
    assert np.all(np.abs(total - want) <= beta.shape[2] * 2.0 ** -53 * np.nansum(np.abs(beta), axis=2))
    for reduce in ("max", "argmax", "min", "argmin"):
        for omit in (True, False):
            assert same(M.derive("theta", reduce, omit_nan=omit), derive_ref(theta, reduce, omit_nan=omit)), (reduce, omit)
    assert same(M.derive("beta", "count_above", threshold=0.0), derive_ref(beta, "count_above", threshold=0.0))
    assert same(M.quantiles("live", [0.25, 0.75]), np.quantile(k.ravel(), [0.25, 0.75])[:, None])
    out = M.collect()
    assert out["live"].shape == (len(chains), 1, n_iter) and same(out["live"], out["n_basis"].reshape(out["live"].shape))
    M.engine.close()


def test_a_ring_store_is_refused(golden):
    from test_mcmc_api_gpu import build_linreg

    M = build_linreg(golden("linreg_chain"), "ex3_", 3, store_ring=6)
    M.run_mcmc()
    with pytest.raises(ValueError, match="store_ring"):
        M.derive("beta", "max")
    with pytest.raises(ValueError, match="store_ring"):
        M.simultaneous_band("beta")
    M.engine.close()
