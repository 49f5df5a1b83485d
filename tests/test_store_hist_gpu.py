"""Marginal histograms, ranges and exceedance of the device store (omc_store_histogram / omc_store_minmax, Engine.store_histogram
/ store_minmax, MCMC.histogram / exceedance) against numpy on the host copy of the same store: np.histogram(col, bins=edges),
np.nanmin, np.nanmax, (col > t).sum().  Counts are integers: every comparison is np.array_equal; edges and densities are built
by the same numpy operations and compared with ==; min and max with == (the sign of a zero minimum is numpy's to choose).

Shapes sit at the edges of the tiling: TE elements of a workgroup's tile and RB rows of a slice, both a function of n_bins and
of the edge mode (Engine.hist_tile).  A pooled row count of exactly RB - 1, RB or 3 RB + 7 needs a chain count that divides
it: those cases run with C = 1, and with C = 3 where 3 divides RB - 1 (RB = 1024 and 16384; not 2048, where the C = 3 case
takes the next multiple of 3 above, 2049 = RB + 1 rows); C = 65 divides none of them and runs in the per-chain form and pooled
with the next multiple of 65 above 3 RB + 7."""

import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def engine(C):
    from openmcmc_amd.engine import Engine
    return Engine(C, seed=1)


def reference(x, edges, idx=None, pooled=True):
    """(counts, outside) of host store x (n_iter, C, size) by np.histogram per column; NaN draws counted apart"""
    n_iter, C, size = x.shape
    sel = np.arange(size) if idx is None else np.asarray(idx)
    nb = edges.shape[-1] - 1
    batches = [x.reshape(-1, size)] if pooled else [x[:, c, :] for c in range(C)]
    counts = np.zeros((len(batches), len(sel), nb), dtype=np.int64)
    outside = np.zeros((len(batches), len(sel), 3), dtype=np.int64)
    for b, rows in enumerate(batches):
        for k, i in enumerate(sel):
            col, e = rows[:, i], (edges if edges.ndim == 1 else edges[k])
            ok = col[~np.isnan(col)]
            counts[b, k] = np.histogram(ok, bins=e)[0]
            outside[b, k] = [(ok < e[0]).sum(), (ok > e[-1]).sum(), np.isnan(col).sum()]
    return (counts[0], outside[0]) if pooled else (counts, outside)


def check(eng, x, edges, idx=None, pooled=True, d=None):
    d = eng.to_device(x) if d is None else d
    counts, outside = (t.cpu().numpy() for t in eng.store_histogram(d, edges, index=idx, pooled=pooled))
    want_c, want_o = reference(x, np.asarray(edges), idx, pooled)
    assert counts.dtype == np.int64 and outside.dtype == np.int64
    assert np.array_equal(counts, want_c)
    assert np.array_equal(outside, want_o)
    draws = x.shape[0] * (x.shape[1] if pooled else 1)
    assert np.all(counts.sum(axis=-1) + outside.sum(axis=-1) == draws)
    return counts, outside


def make_edges(rng, nb, rows, uniform):
    """(nb + 1,) for rows None, else (rows, nb + 1): evenly spaced, or sorted normal deviates (with a repeated edge)"""
    n = 1 if rows is None else rows
    if uniform:
        lo, hi = rng.uniform(-2.5, -0.5, n), rng.uniform(0.5, 2.5, n)
        e = np.stack([np.linspace(a, b, nb + 1) for a, b in zip(lo, hi)])
    else:
        e = np.sort(rng.standard_normal((n, nb + 1)) * 1.3, axis=-1)
        if nb >= 3:
            e[:, nb // 2] = e[:, nb // 2 + 1]
    return e[0] if rows is None else e


# ---------------------------------------------------------------------------------------------------------- tile edges
SIZES = ("1", "TE-1", "TE", "TE+1", "2TE+3")
FORMS = ((1, "3RB+7", True), (3, "RB-1", True), (1, "RB", True), (65, "1", False), (3, "RB+1", False), (1, "1", True),
         (65, ">3RB+7", True), (1, "RB-1", True), (1, "RB+1", False))


def tile_cases():
    out, k = [], 0
    for i, (nb, per) in enumerate((nb, per) for nb in (1, 2, 63, 64, 65, 1024) for per in (False, True)):
        for f in (i, i + 2, i + 4):
            C, rows, pooled = FORMS[f % len(FORMS)]
            out.append(pytest.param(nb, per, SIZES[k % 5], C, rows, pooled, (k // 2) % 2 == 0,
                                    id=f"bins{nb}-{'per' if per else 'shared'}-size{SIZES[k % 5]}-C{C}-rows{rows}-{'pooled' if pooled else 'chain'}"))
            k += 1
    return out


@pytest.mark.parametrize("nb,per,size_kind,C,rows_kind,pooled,uniform", tile_cases())
def test_tile_edges(nb, per, size_kind, C, rows_kind, pooled, uniform):
    from openmcmc_amd.engine import Engine

    TE, RB = Engine.hist_tile(nb, per)
    size = max(1, {"1": 1, "TE-1": TE - 1, "TE": TE, "TE+1": TE + 1, "2TE+3": 2 * TE + 3}[size_kind])
    rows = {"1": 1, "RB-1": RB - 1, "RB": RB, "RB+1": RB + 1, "3RB+7": 3 * RB + 7, ">3RB+7": -(-(3 * RB + 7) // C) * C}[rows_kind]
    n_iter = -(-rows // C) if pooled else rows  # (pooled: the row count itself where C divides it, else the next multiple of C)
    rng = np.random.default_rng(1000 * nb + 10 * C + len(size_kind) + int(per))
    x = rng.standard_normal((n_iter, C, size)) * rng.uniform(0.5, 1.5, size) + rng.uniform(-0.5, 0.5, size)
    edges = make_edges(rng, nb, size if per else None, uniform)
    eng = engine(C)
    check(eng, x, edges, pooled=pooled)
    eng.close()


@pytest.mark.parametrize("pooled", (True, False))
@pytest.mark.parametrize("per", (False, True))
def test_index_with_repeats_and_in_reversed_order(pooled, per):
    from openmcmc_amd.engine import Engine

    nb, C = 17, 3
    TE, RB = Engine.hist_tile(nb, per)
    size, n_iter = 2 * TE + 3, (RB + 1 if not pooled else (RB + 2) // C * 2)
    rng = np.random.default_rng(7 + per)
    x = rng.standard_normal((n_iter, C, size)) + np.linspace(-1, 1, size)
    idx = np.concatenate([np.arange(size)[::-1], [5, 5, 0, size - 1, 5], rng.integers(0, size, TE)])
    eng = engine(C)
    d = eng.to_device(x)
    edges = make_edges(rng, nb, len(idx) if per else None, uniform=False)
    counts, _ = check(eng, x, edges, idx=idx, pooled=pooled, d=d)
    if not per:  # a repeated index repeats its row; the reversed part is the whole result upside down
        full, _ = check(eng, x, edges, pooled=pooled, d=d)
        assert np.array_equal(counts[..., :size, :], full[..., ::-1, :])
        assert np.array_equal(counts[..., size, :], counts[..., size + 1, :])
    mn, mx, cnt = (t.cpu().numpy() for t in eng.store_minmax(d, index=idx, pooled=pooled))
    rows = x.reshape(-1, size) if pooled else x
    assert np.all(mn == rows.min(axis=0)[..., idx]) and np.all(mx == rows.max(axis=0)[..., idx]) and np.all(cnt == rows.shape[0])
    eng.close()


# ---------------------------------------------------------------------------------------------------------- the bin rule
def rule(edges, v):
    """np.searchsorted(edges, v, 'right') - 1 with the last bin closed; -1 / -2 / -3 = below / above / NaN"""
    nb = len(edges) - 1
    j = np.searchsorted(edges, v, "right") - 1
    j = np.where((j == nb) & (v == edges[-1]), nb - 1, j)
    j = np.where(v < edges[0], -1, np.where(v > edges[-1], -2, j))
    return np.where(np.isnan(v), -3, j)


EDGE_SETS = {
    "equal-neighbours": [0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 3.0],
    "closed-last-bin": [0.0, 1.0, 2.0, 2.5],
    "equal-at-the-end": [0.0, 1.0, 2.0, 2.0],
    "all-equal": [1.0, 1.0, 1.0],
    "infinite-ends": [-np.inf, -1.0, 0.0, 1.0, np.inf],
    "infinite-left": [-np.inf, -np.inf, 0.0, 5.0],
    "one-bin": [-1.0, 1.0],
    "twelve-decades": list(np.logspace(-6, 6, 25)),
    "twelve-decades-signed": list(-np.logspace(6, -6, 13)) + [0.0] + list(np.logspace(-6, 6, 13)),
    "uniform": list(np.linspace(-1.0, 1.0, 11)),
    "uniform-thirds": list(np.linspace(0.1, 0.7, 4)),
}


@pytest.mark.parametrize("name", sorted(EDGE_SETS))
def test_bin_rule_on_and_beside_every_edge(name):
    edges = np.array(EDGE_SETS[name])
    fin = edges[np.isfinite(edges)]
    vals = np.concatenate([edges, np.nextafter(fin, np.inf), np.nextafter(fin, -np.inf), [np.inf, -np.inf, np.nan, 0.0, -0.0],
                           0.5 * (fin[:-1] + fin[1:])])
    x = np.tile(vals, 3).reshape(-1, 1, 1)
    nb = len(edges) - 1
    j = rule(edges, x[:, 0, 0])
    want = np.bincount(j[j >= 0], minlength=nb)
    eng = engine(1)
    for algo in (0, 1):
        eng.set_option("hist_algo", algo)
        counts, outside = check(eng, x, edges)
        assert np.array_equal(counts[0], want)
        assert list(outside[0]) == [(j == -1).sum(), (j == -2).sum(), (j == -3).sum()]
    eng.close()


@pytest.mark.parametrize("n", (7, 10, 100, 333))
def test_uniform_edges_where_the_arithmetic_guess_is_off_by_one(n):
    """np.histogram(x, bins=n, range=r), np.histogram(x, bins=np.linspace(*r, n + 1)) and the kernel agree, with ranges between
    the 0.1 and 0.9 quantiles of the sample and draws placed on every edge and beside it: 64 samples as the 64 elements of one
    store with their own edges, by the arithmetic guess and by the bisection."""
    rng = np.random.default_rng(n)
    size, m = 64, 400
    x = rng.standard_normal((m, 1, size)) * 10.0 ** rng.uniform(-3, 3, size) + rng.standard_normal(size) * 10.0 ** rng.uniform(-3, 3, size)
    r = np.quantile(x[:, 0, :], [0.1, 0.9], axis=0)
    edges = np.stack([np.linspace(r[0, i], r[1, i], n + 1) for i in range(size)])
    on = np.concatenate([edges, np.nextafter(edges, np.inf), np.nextafter(edges, -np.inf)], axis=1).T[:, None, :]
    x = np.concatenate([x, on], axis=0)
    want = np.stack([np.histogram(x[:, 0, i], bins=n, range=(r[0, i], r[1, i]))[0] for i in range(size)])
    eng = engine(1)
    for algo in (0, 1):
        eng.set_option("hist_algo", algo)
        counts, _ = check(eng, x, edges)
        assert np.array_equal(counts, want)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- NaN
def test_ragged_padding_and_an_all_nan_element():
    n_iter, C, size = 40, 3, 70
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n_iter, C, size))
    live = rng.integers(1, size, (n_iter, C))  # NaN beyond a live length per (iteration, chain)
    x[np.arange(size)[None, None, :] >= live[:, :, None]] = np.nan
    x[:, :, 11] = np.nan
    x[:, 1, 12] = np.nan
    x[3, 0, 0], x[4, 2, 0] = np.inf, -np.inf
    eng = engine(C)
    d = eng.to_device(x)
    for pooled in (True, False):
        for per in (False, True):
            edges = make_edges(rng, 9, size if per else None, uniform=not per)
            counts, outside = check(eng, x, edges, pooled=pooled, d=d)
            assert not counts[..., 11, :].any() and np.all(outside[..., 11, 2] == (n_iter * C if pooled else n_iter))
        mn, mx, cnt = (t.cpu().numpy() for t in eng.store_minmax(d, pooled=pooled))
        rows = x.reshape(-1, size) if pooled else x
        valid = (~np.isnan(rows)).sum(axis=0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (np.nanmin of an all-NaN column warns)
            want_mn, want_mx = np.nanmin(rows, axis=0), np.nanmax(rows, axis=0)
        assert cnt.dtype == np.int64 and np.array_equal(cnt, valid)
        assert np.array_equal(np.isnan(mn), valid == 0) and np.array_equal(np.isnan(mx), valid == 0)
        assert np.all((mn == want_mn) | (valid == 0)) and np.all((mx == want_mx) | (valid == 0))
        assert np.isnan(mn[..., 11]).all() and np.isnan(mx[..., 11]).all() and not cnt[..., 11].any()
        assert mn.reshape(-1, size)[0, 0] == -np.inf or not pooled
    eng.close()


def test_minmax_over_several_slices_and_signed_zero():
    n_iter, C, size = 700, 5, 67
    rng = np.random.default_rng(6)
    x = rng.standard_normal((n_iter, C, size))
    x[:, :, 1] = np.abs(x[:, :, 1])
    x[17, 2, 1], x[18, 3, 1] = 0.0, -0.0
    eng = engine(C)
    d = eng.to_device(x)
    for pooled in (True, False):
        mn, mx, cnt = (t.cpu().numpy() for t in eng.store_minmax(d, pooled=pooled))
        rows = x.reshape(-1, size) if pooled else x
        assert np.all(mn == rows.min(axis=0)) and np.all(mx == rows.max(axis=0)) and np.all(cnt == rows.shape[0])
    again = [t.cpu().numpy() for t in eng.store_minmax(d)]
    assert all(np.array_equal(a, b) for a, b in zip(again, [t.cpu().numpy() for t in eng.store_minmax(d)]))
    eng.close()


# ---------------------------------------------------------------------------------------------------------- contention
@pytest.mark.parametrize("nb,per", ((32, False), (32, True), (256, False)))
def test_constant_column_and_one_crowded_bin(nb, per):
    from openmcmc_amd.engine import Engine

    TE, RB = Engine.hist_tile(nb, per)
    C, size = 1, TE + 1
    n_iter = 3 * RB + 7
    rng = np.random.default_rng(nb)
    x = rng.standard_normal((n_iter, C, size))
    crowded = rng.random((n_iter, C, size)) < 0.99
    x = np.where(crowded, 0.25 + 1e-3 * x, x)  # 99 % of the draws in one bin
    x[:, :, 0] = 0.25                            # a constant column
    x[:, :, size - 1] = -0.0
    eng = engine(C)
    edges = make_edges(rng, nb, size if per else None, uniform=True)
    counts, _ = check(eng, x, edges)
    assert counts[0].max() == n_iter
    eng.close()


# ---------------------------------------------------------------------------------------------------------- contract
def test_rejections_leave_the_outputs_alone_and_null_outside_works():
    import torch

    from openmcmc_amd import _abi

    n_iter, C, size, nb = 16, 3, 40, 6
    rng = np.random.default_rng(9)
    x = rng.standard_normal((n_iter, C, size))
    eng = engine(C)
    d = eng.to_device(x)
    good = np.linspace(-2, 2, nb + 1)
    nan_edge, decreasing = good.copy(), good.copy()
    nan_edge[3] = np.nan
    decreasing[4] = decreasing[3] - 1e-9
    for bad in (nan_edge, decreasing, np.tile(decreasing, (size, 1))):
        with pytest.raises(ValueError, match="invalid argument"):
            eng.store_histogram(d, bad)
    for bad in ([0, -1], [size, 1], [2 ** 40]):
        with pytest.raises(ValueError, match="invalid argument"):
            eng.store_histogram(d, good, index=bad)
        with pytest.raises(ValueError, match="invalid argument"):
            eng.store_minmax(d, index=bad)
    with pytest.raises(ValueError):
        eng.store_histogram(d, np.zeros((3, nb + 1)))  # per-element edges of another count
    with pytest.raises(ValueError):
        eng.store_histogram(d, np.linspace(0, 1, 1026 + 1))

    def call(n_bins, edges, idx, n_idx, counts, outside, per=0):
        e = eng.to_device(edges)
        st = _abi.lib.omc_store_histogram(eng._ctx, n_iter, size, d.data_ptr(), None if idx is None else idx.data_ptr(), n_idx, 1, n_bins,
                                          e.data_ptr(), per, counts.data_ptr(), None if outside is None else outside.data_ptr())
        torch.cuda.synchronize()
        return st

    counts = torch.full((size, nb), -7, dtype=torch.int64, device=d.device)
    outside = torch.full((size, 3), -7, dtype=torch.int64, device=d.device)
    idx_bad = torch.as_tensor(np.array([3, size], dtype=np.int64), device=d.device)
    idx_neg = torch.as_tensor(np.array([-1, 3], dtype=np.int64), device=d.device)
    assert call(nb, nan_edge, None, size, counts, outside) == _abi.INVALID_ARG
    assert call(nb, decreasing, None, size, counts, outside) == _abi.INVALID_ARG
    assert call(0, good, None, size, counts, outside) == _abi.INVALID_ARG
    assert call(1025, np.linspace(0, 1, 1026), None, size, counts, outside) == _abi.INVALID_ARG
    assert call(nb, good, idx_bad, 2, counts, outside) == _abi.INVALID_ARG
    assert call(nb, good, idx_neg, 2, counts, outside) == _abi.INVALID_ARG
    assert call(nb, good, None, 2, counts, outside) == _abi.INVALID_ARG  # n_idx must equal size without an index
    assert np.all(counts.cpu().numpy() == -7) and np.all(outside.cpu().numpy() == -7)
    mn = eng.full((2,), -7.0)
    cnt = torch.full((2,), -7, dtype=torch.int64, device=d.device)
    st = _abi.lib.omc_store_minmax(eng._ctx, n_iter, size, d.data_ptr(), idx_bad.data_ptr(), 2, 1, mn.data_ptr(), None, cnt.data_ptr())
    torch.cuda.synchronize()
    assert st == _abi.INVALID_ARG and np.all(mn.cpu().numpy() == -7.0) and np.all(cnt.cpu().numpy() == -7)
    # NULL outside_out; the outputs are overwritten, not accumulated
    want, _ = reference(x, good)
    for _ in range(2):
        assert call(nb, good, None, size, counts, None) == _abi.OK
        assert np.array_equal(counts.cpu().numpy(), want)
    # any output of omc_store_minmax may be NULL
    mx = eng.full((size,), -7.0)
    st = _abi.lib.omc_store_minmax(eng._ctx, n_iter, size, d.data_ptr(), None, size, 1, None, mx.data_ptr(), None)
    torch.cuda.synchronize()
    assert st == _abi.OK and np.all(mx.cpu().numpy() == x.reshape(-1, size).max(axis=0))
    eng.close()


def test_repeated_calls_and_both_forms_are_bit_equal():
    n_iter, C, size, nb = 900, 3, 70, 50
    rng = np.random.default_rng(10)
    x = rng.standard_normal((n_iter, C, size))
    eng = engine(C)
    d = eng.to_device(x)
    shared = np.linspace(-3, 3, nb + 1)
    per = np.stack([np.linspace(-3 - 0.01 * i, 3 + 0.02 * i, nb + 1) for i in range(size)])
    for edges in (shared, per, eng.to_device(shared)):  # (a device tensor of edges is taken as it is)
        for pooled in (True, False):
            res = []
            for algo in (0, 0, 1):
                eng.set_option("hist_algo", algo)
                res.append([t.cpu().numpy() for t in eng.store_histogram(d, edges, pooled=pooled)])
            assert all(np.array_equal(res[0][k], r[k]) for r in res[1:] for k in (0, 1))
    eng.set_option("hist_algo", 0)
    check(eng, x, per, d=d)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- public API
def test_histogram_and_exceedance_through_mcmc(golden):
    """A short run of the linear-regression model: MCMC.histogram against np.histogram of the stored draws of every element,
    MCMC.exceedance against (col > t).sum() / len(col)."""
    from test_mcmc_api_gpu import build_linreg

    G = golden("linreg_chain")
    C = 3
    M = build_linreg(G, "ex3_", C)
    M.run_mcmc()
    M.store["beta"][:, :, 1] = 2.5  # a constant element
    beta = M.store["beta"].cpu().numpy()
    beta = beta.reshape(beta.shape[0], C, -1)
    logp = M.store["log_post"].cpu().numpy().reshape(beta.shape[0], C, 1)
    n_iter, p = beta.shape[0], beta.shape[2]
    for key, host in (("beta", beta), ("log_post", logp)):
        flat = host.reshape(-1, host.shape[2])
        for bins in (10, 1, 37):
            hist, edges = M.histogram(key, bins=bins)
            dens, edges_d = M.histogram(key, bins=bins, density=True)
            assert hist.shape == (host.shape[2], bins) and edges.shape == (host.shape[2], bins + 1) and hist.dtype == np.int64
            assert np.array_equal(edges, edges_d)
            for i in range(host.shape[2]):
                want, want_e = np.histogram(flat[:, i], bins)
                assert np.array_equal(hist[i], want) and np.all(edges[i] == want_e)
                assert np.all(dens[i] == np.histogram(flat[:, i], bins, density=True)[0])
            per, edges_p = M.histogram(key, bins=bins, pooled=False)  # the chains of an element share the pooled range's edges
            assert per.shape == (C, host.shape[2], bins) and np.array_equal(edges_p, edges)
            assert np.array_equal(per.sum(axis=0), hist)
            for c in range(C):
                for i in range(host.shape[2]):
                    assert np.array_equal(per[c, i], np.histogram(host[:, c, i], bins=edges[i])[0])
    # a range; array bins, shared and per element; an index
    lo, hi = np.quantile(beta, 0.2), np.quantile(beta, 0.9)
    hist, edges = M.histogram("beta", bins=12, range=(lo, hi))
    flat = beta.reshape(-1, p)
    assert edges.shape == (13,)
    for i in range(p):
        want, want_e = np.histogram(flat[:, i], 12, range=(lo, hi))
        assert np.array_equal(hist[i], want) and np.all(edges == want_e)
    dens, _ = M.histogram("beta", bins=12, range=(lo, hi), density=True)
    with np.errstate(all="ignore"):
        for i in range(p):
            want = np.histogram(flat[:, i], 12, range=(lo, hi), density=True)[0]
            assert np.array_equal(dens[i], want, equal_nan=True)
    mine = np.sort(np.random.default_rng(3).standard_normal(8)) * 3.0
    idx = [p - 1, 0, 0]
    hist, edges = M.histogram("beta", bins=mine, index=idx)
    assert np.array_equal(edges, mine) and hist.shape == (3, 7)
    for k, i in enumerate(idx):
        assert np.array_equal(hist[k], np.histogram(flat[:, i], bins=mine)[0])
    per_el = np.stack([mine + 0.1 * k for k in range(3)])
    hist, _ = M.histogram("beta", bins=per_el, index=idx, pooled=False)
    for c in range(C):
        for k, i in enumerate(idx):
            assert np.array_equal(hist[c, k], np.histogram(beta[:, c, i], bins=per_el[k])[0])
    with pytest.raises(ValueError):
        M.histogram("beta", bins=mine[::-1])
    with pytest.raises(ValueError):
        M.histogram("beta", bins=0)
    M.store["beta"][0, 0, 0] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        M.histogram("beta", bins=5)
    M.store["beta"][0, 0, 0] = float(beta[0, 0, 0])
    # exceedance: thresholds out of order, one of them a draw, one above and one below everything
    th = np.array([0.3, flat[5, 0], -1e300, 1e300, flat[7, p - 1], 0.3, 2.5])
    ex = M.exceedance("beta", th)
    assert ex.shape == (len(th), p)
    for j, t in enumerate(th):
        assert np.array_equal(ex[j], (flat > t).sum(axis=0) / flat.shape[0])
    ex = M.exceedance("beta", th, index=idx, pooled=False)
    assert ex.shape == (len(th), C, 3)
    for j, t in enumerate(th):
        assert np.array_equal(ex[j], ((beta > t).sum(axis=0) / n_iter)[:, idx])
    assert M.exceedance("log_post", float(logp[3, 1, 0])).shape == (1, 1)
    # NaN draws leave the denominator; an element without a draw gives NaN
    M.store["beta"][:, :, p - 1] = float("nan")
    M.store["beta"][: n_iter // 2, :, 0] = float("nan")
    ex = M.exceedance("beta", [0.0], index=[0, p - 1])
    col = beta[n_iter // 2:, :, 0].ravel()
    assert ex[0, 0] == (col > 0.0).sum() / col.size and np.isnan(ex[0, 1])
    hist, edges = M.histogram("beta", bins=4, index=[p - 1, 0])
    assert not hist[0].any() and np.all(edges[0] == np.linspace(0.0, 1.0, 5))
    assert np.array_equal(hist[1], np.histogram(col, 4)[0]) and np.all(edges[1] == np.histogram(col, 4)[1])
    M.engine.close()
    # a ring store holds the last iterations only: nothing to reduce on the device
    M = build_linreg(G, "ex3_", C, store_ring=6)
    M.run_mcmc()
    for call in (lambda: M.histogram("beta"), lambda: M.exceedance("beta", 0.0)):
        with pytest.raises(ValueError, match="store_ring"):
            call()
    M.engine.close()
