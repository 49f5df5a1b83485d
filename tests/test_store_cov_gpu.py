"""Posterior covariance / correlation of the device store (omc_store_cov, Engine.store_cov, MCMC.covariance /
MCMC.correlation) against a host restatement -- two-pass covariance in np.longdouble: means, centred products, divisor,
rounded to double -- and against np.cov / np.corrcoef themselves, at the tile edges (16 and 128 on both sides), in the
pooled and the per-chain form, with two tensors, under an index, at the edges of the contract, and through the public API.

Tolerance (README: fp64 quantities to 1e-10 relative): |out_ij - ref_ij| <= 1e-10 sqrt(ref_ii ref_jj) on data with
|mean| <= 1e3 sd per element (the scale is sqrt(c_ii c_jj), not |c_ij|: a covariance near zero has no relative accuracy in
any summation order); correlations to 1e-10 absolute."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-10


# ---------------------------------------------------------------------------------------------------------- restatement
def restate(a, b=None):
    """(cov (na, nb), var_a, var_b) of draws a (R, na), b (R, nb): two passes in long double, rounded to double"""
    def centred(x):
        x = x.astype(np.longdouble)
        return x - x.mean(axis=0)
    R = a.shape[0]
    da = centred(a)
    db = da if b is None else centred(b)
    div = np.longdouble(max(R - 1, 1))
    cov = np.zeros((da.shape[1], db.shape[1]), dtype=np.longdouble)
    for r0 in range(0, R, 4096):  # (keeps the long-double temporaries small)
        cov += da[r0:r0 + 4096].T @ db[r0:r0 + 4096]
    va, vb = (da * da).sum(axis=0) / div, (db * db).sum(axis=0) / div
    if R == 1:
        cov[:], va[:], vb[:] = 0, 0, 0
    return (cov / div).astype(np.float64), va.astype(np.float64), vb.astype(np.float64)


def restate_store(sa, sb=None, ia=None, ib=None, pooled=True):
    """the same for host stores (n_iter, C, size): (cov, var_a, var_b) pooled, or stacked over the chains"""
    def draws(s, idx, c):
        s = s if idx is None else s[:, :, np.asarray(idx)]
        return s.reshape(-1, s.shape[2]) if c is None else s[:, c, :]
    res = [restate(draws(sa, ia, c), None if sb is None else draws(sb, ib, c)) for c in ([None] if pooled else range(sa.shape[1]))]
    return res[0] if pooled else tuple(np.stack([r[k] for r in res]) for k in range(3))


def scaled_err(out, ref, va, vb):
    """max |out - ref| / sqrt(var_a_i var_b_j); an entry whose scale is zero must be exact"""
    scale = np.sqrt(va[..., :, None] * vb[..., None, :])
    d = np.abs(out - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale > 0, d / scale, np.where(d == 0, 0.0, np.inf))
    return float(e.max())


def make_store(seed, n_iter, C, size, mean_over_sd=1e3):
    """(n_iter, C, size) draws with neighbouring elements correlated, sd over four decades, |mean| <= mean_over_sd * sd for
    every element in the pooled sample and in every chain's own (the seed is advanced until the sample says so)"""
    while True:
        rng = np.random.default_rng(seed)
        z = rng.standard_normal((n_iter, C, size))
        x = (z + 0.6 * np.roll(z, 1, axis=-1)) * 10.0 ** rng.uniform(-2, 2, size)
        flat = x.reshape(-1, size)
        samples = ([flat] if n_iter * C > 1 else []) + ([x[:, c, :] for c in range(C)] if n_iter > 1 else [])
        if not samples:
            return x + rng.uniform(-1, 1, size) * 100.0
        x = x + rng.uniform(-1, 1, size) * 0.5 * mean_over_sd * np.min([m.std(axis=0, ddof=1) for m in samples], axis=0)
        flat = x.reshape(-1, size)
        samples = ([flat] if n_iter * C > 1 else []) + ([x[:, c, :] for c in range(C)] if n_iter > 1 else [])
        ratio = max(np.max(np.abs(m.mean(axis=0)) / m.std(axis=0, ddof=1)) for m in samples)
        if ratio <= mean_over_sd:
            return x
        seed += 1000


def engine(C):
    from openmcmc_amd.engine import Engine
    return Engine(C, seed=1)


def both_forms(eng, x, tol=TOL, correlation=True):
    """Engine.store_cov of host store x in the pooled and per-chain form against the restatement and numpy"""
    n_iter, C, size = x.shape
    d = eng.to_device(x)
    for pooled in (True, False):
        ref, va, _ = restate_store(x, pooled=pooled)
        out = eng.store_cov(d, pooled=pooled).cpu().numpy()
        assert out.shape == ((size, size) if pooled else (C, size, size))
        err = scaled_err(out, ref, va, va)
        print(f"cov n_iter={n_iter} C={C} size={size} pooled={pooled}: scaled error {err:.3g}")
        assert err <= tol
        assert np.array_equal(out, np.swapaxes(out, -1, -2))
        R = n_iter * C if pooled else n_iter
        if R < 2:
            assert not out.any()
            continue
        mats = [x.reshape(-1, size)] if pooled else [x[:, c, :] for c in range(C)]
        npc = np.stack([np.cov(m.T).reshape(size, size) for m in mats]).reshape(out.shape)
        assert scaled_err(out, npc, va, va) <= tol
        if not correlation:
            continue
        cor = eng.store_cov(d, pooled=pooled, correlation=True).cpu().numpy()
        want = ref / np.sqrt(va[..., :, None] * va[..., None, :])
        npr = np.stack([np.corrcoef(m.T).reshape(size, size) for m in mats]).reshape(out.shape)
        err = max(np.abs(cor - want).max(), np.abs(cor - npr).max())
        print(f"    correlation: absolute error {err:.3g}")
        assert err <= tol
        assert np.all(np.diagonal(cor, axis1=-2, axis2=-1) == 1.0) and np.abs(cor).max() <= 1.0
        assert np.array_equal(cor, np.swapaxes(cor, -1, -2))


# ---------------------------------------------------------------------------------------------------------- shapes
SHAPES = ([(64, 3, s) for s in (1, 3, 15, 16, 17, 127, 128, 129, 300)] + [(n, 3, 17) for n in (1, 2, 3, 5, 257)]
          + [(5, 1, 129), (5, 64, 129), (257, 64, 129), (1, 1, 16), (2, 64, 300), (257, 1, 3)])


@pytest.mark.parametrize("n_iter,C,size", SHAPES)
def test_shapes_pooled_and_per_chain(n_iter, C, size):
    eng = engine(C)
    both_forms(eng, make_store(size + 7 * n_iter + C, n_iter, C, size))
    eng.close()


def test_long_pooled_contraction_is_split_and_repeatable():
    """R = 204 800 at size 96: one tile, the contraction cut into slices; two calls bit-equal"""
    n_iter, C, size = 3200, 64, 96
    x = make_store(11, n_iter, C, size)
    eng = engine(C)
    d = eng.to_device(x)
    out = eng.store_cov(d).cpu().numpy()
    ref, va, _ = restate_store(x)
    err = scaled_err(out, ref, va, va)
    print(f"long pooled: scaled error {err:.3g}")
    assert err <= TOL
    again = eng.store_cov(d).cpu().numpy()
    assert np.array_equal(out, again)
    cor = eng.store_cov(d, correlation=True).cpu().numpy()
    assert np.array_equal(cor, eng.store_cov(d, correlation=True).cpu().numpy())
    assert np.abs(cor - ref / np.sqrt(np.outer(va, va))).max() <= TOL
    # consistency with what exists: the diagonal is omc_store_moments' variance
    _, var = eng.store_moments(d, pooled=True)
    assert np.max(np.abs(np.diag(out) - var.cpu().numpy()) / va) <= TOL
    eng.close()


def test_long_per_chain_contraction_is_split():
    """C = 2, n_iter = 100 000, size 40: two (chain, tile) pairs, so the per-chain form cuts the contraction too"""
    x = make_store(12, 100_000, 2, 40)
    eng = engine(2)
    d = eng.to_device(x)
    out = eng.store_cov(d, pooled=False).cpu().numpy()
    ref, va, _ = restate_store(x, pooled=False)
    err = scaled_err(out, ref, va, va)
    print(f"long per chain: scaled error {err:.3g}")
    assert err <= TOL
    assert np.array_equal(out, eng.store_cov(d, pooled=False).cpu().numpy())
    _, var = eng.store_moments(d, pooled=False)
    assert np.max(np.abs(np.diagonal(out, axis1=1, axis2=2) - var.cpu().numpy()) / va) <= TOL
    eng.close()


# ---------------------------------------------------------------------------------------------------------- two tensors
@pytest.mark.parametrize("size_a,size_b", [(1, 300), (40, 129), (300, 1), (129, 40)])
def test_cross_covariance_of_two_stores(size_a, size_b):
    n_iter, C = 64, 3
    x = make_store(21 + size_a, n_iter, C, size_a + size_b)
    a, b = np.ascontiguousarray(x[:, :, :size_a]), np.ascontiguousarray(x[:, :, size_a:])
    eng = engine(C)
    da, db = eng.to_device(a), eng.to_device(b)
    for pooled in (True, False):
        ref, va, vb = restate_store(a, b, pooled=pooled)
        out = eng.store_cov(da, db, pooled=pooled).cpu().numpy()
        assert out.shape == ((size_a, size_b) if pooled else (C, size_a, size_b))
        err = scaled_err(out, ref, va, vb)
        print(f"cross {size_a} x {size_b} pooled={pooled}: scaled error {err:.3g}")
        assert err <= TOL
        mats = [x.reshape(-1, size_a + size_b)] if pooled else [x[:, c, :] for c in range(C)]
        block = np.stack([np.cov(m.T)[:size_a, size_a:] for m in mats]).reshape(out.shape)  # np.cov of the stacked variables
        assert scaled_err(out, block, va, vb) <= TOL
        back = eng.store_cov(db, da, pooled=pooled).cpu().numpy()
        assert scaled_err(np.swapaxes(back, -1, -2), ref, va, vb) <= TOL
        cor = eng.store_cov(da, db, pooled=pooled, correlation=True).cpu().numpy()
        rblock = np.stack([np.corrcoef(m.T)[:size_a, size_a:] for m in mats]).reshape(out.shape)
        assert np.abs(cor - rblock).max() <= TOL and np.abs(cor).max() <= 1.0
    with pytest.raises(ValueError):
        eng.store_cov(da, db[:-1].contiguous())
    eng.close()


# ---------------------------------------------------------------------------------------------------------- index
INDEXES = {"permutation": np.random.default_rng(3).permutation(300), "strided": np.arange(2, 300, 7),
           "run": np.arange(50, 200), "repeats": np.array([5, 5, 17, 5, 299, 0, 17]), "one": [128]}


@pytest.mark.parametrize("pooled", [True, False])
def test_index_selects_rows_and_columns_of_the_full_result(pooled):
    import torch

    n_iter, C, size = 64, 3, 300
    x = make_store(31, n_iter, C, size)
    eng = engine(C)
    d = eng.to_device(x)
    full, va, _ = restate_store(x, pooled=pooled)
    got_full = eng.store_cov(d, pooled=pooled).cpu().numpy()
    for name, idx in INDEXES.items():
        ii = np.asarray(idx)
        for as_type in (list, np.asarray, lambda v: torch.as_tensor(np.asarray(v))):
            out = eng.store_cov(d, index_a=as_type(idx), pooled=pooled).cpu().numpy()
            assert out.shape[-2:] == (ii.size, ii.size)
            want = full[..., ii[:, None], ii[None, :]]
            err = scaled_err(out, want, va[..., ii], va[..., ii])
            assert err <= TOL, (name, err)
            assert scaled_err(out, got_full[..., ii[:, None], ii[None, :]], va[..., ii], va[..., ii]) <= TOL
            assert np.array_equal(out, np.swapaxes(out, -1, -2))
        cor = eng.store_cov(d, index_a=idx, pooled=pooled, correlation=True).cpu().numpy()
        want = (full / np.sqrt(va[..., :, None] * va[..., None, :]))[..., ii[:, None], ii[None, :]]
        assert np.abs(cor - want).max() <= TOL
        assert np.all(np.diagonal(cor, axis1=-2, axis2=-1) == 1.0)
        if name == "repeats":  # a repeated index gives bit-equal rows
            for m in (out, cor):
                assert np.array_equal(m[..., 0, :], m[..., 1, :]) and np.array_equal(m[..., 0, :], m[..., 3, :])
                assert np.array_equal(m[..., 2, :], m[..., 6, :])
            assert np.all(cor[..., 0, 1] == 1.0) and np.all(cor[..., 3, 0] == 1.0)
    # the cross form under two indices
    y = make_store(32, n_iter, C, 129)
    dy = eng.to_device(y)
    ia, ib = np.arange(299, 0, -3), np.array([128, 0, 64, 64])
    out = eng.store_cov(d, dy, index_a=ia, index_b=ib, pooled=pooled).cpu().numpy()
    ref, wa, wb = restate_store(x, y, ia, ib, pooled=pooled)
    assert out.shape[-2:] == (ia.size, ib.size) and scaled_err(out, ref, wa, wb) <= TOL
    assert np.array_equal(out[..., 2], out[..., 3])
    eng.close()


def test_index_out_of_range_is_an_invalid_argument_and_leaves_out_alone():
    import torch

    from openmcmc_amd import _abi

    n_iter, C, size = 16, 3, 40
    eng = engine(C)
    d = eng.to_device(make_store(41, n_iter, C, size))
    e = eng.to_device(make_store(42, n_iter, C, 7))
    for bad in ([0, 40], [-1, 3], [2 ** 40]):
        with pytest.raises(ValueError, match="invalid argument"):
            eng.store_cov(d, index_a=bad)
        with pytest.raises(ValueError, match="invalid argument"):
            eng.store_cov(e, d, index_b=bad, pooled=False)
    for bad in ([], [[1, 2]], [0.5]):
        with pytest.raises(ValueError):
            eng.store_cov(d, index_a=bad)
    with pytest.raises(ValueError):
        eng.store_cov(d, index_b=[1])  # no second store
    with pytest.raises(ValueError):
        eng.store_cov(d[:, :2].contiguous())
    # through the C ABI with an output of our own: untouched
    out = eng.full((2, 2), -7.0)
    idx = torch.as_tensor(np.array([3, 40], dtype=np.int64), device=d.device)
    st = _abi.lib.omc_store_cov(eng._ctx, n_iter, size, d.data_ptr(), idx.data_ptr(), 2, 0, None, None, 0, 1, 0, out.data_ptr())
    assert st == _abi.INVALID_ARG
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0)
    # n must equal size without an index
    st = _abi.lib.omc_store_cov(eng._ctx, n_iter, size, d.data_ptr(), None, 2, 0, None, None, 0, 1, 0, out.data_ptr())
    assert st == _abi.INVALID_ARG
    eng.close()


# ---------------------------------------------------------------------------------------------------------- centring
def test_means_far_from_zero_are_centred_before_the_products():
    """|mean| up to 1e8 sd, R = 20 000, size 16.  A two-pass scheme in fp64 is bounded by the rounding of the mean and of
    x - m: about eps |mean| / sd = 1.1e-8 relative to sd_i sd_j; the one-pass formula (X'X - R m m') / (R - 1) is at 1e+2."""
    n_iter, C, size = 5000, 4, 16
    rng = np.random.default_rng(51)
    z = rng.standard_normal((n_iter, C, size))
    x = z + 0.6 * np.roll(z, 1, axis=-1)
    x = x + 10.0 ** np.linspace(0, 8, size) * np.where(np.arange(size) % 2, -1.0, 1.0)
    eng = engine(C)
    d = eng.to_device(x)
    for pooled in (True, False):
        ref, va, _ = restate_store(x, pooled=pooled)
        out = eng.store_cov(d, pooled=pooled).cpu().numpy()
        err = scaled_err(out, ref, va, va)
        print(f"centring pooled={pooled}: scaled error {err:.3g}")
        assert err <= 1e-8
    eng.close()


# ---------------------------------------------------------------------------------------------------------- contract edges
def test_constant_element_nan_draw_and_single_draw():
    n_iter, C, size = 20, 3, 40
    x = make_store(61, n_iter, C, size, mean_over_sd=10.0)
    x[:, :, 3] = 2.5
    eng = engine(C)
    d = eng.to_device(x)
    for pooled in (True, False):
        cov = eng.store_cov(d, pooled=pooled).cpu().numpy()
        cor = eng.store_cov(d, pooled=pooled, correlation=True).cpu().numpy()
        assert not cov[..., 3, :].any() and not cov[..., :, 3].any()  # exactly zero
        assert np.isnan(cor[..., 3, :]).all() and np.isnan(cor[..., :, 3]).all()
        rest = np.delete(np.delete(cor, 3, axis=-1), 3, axis=-2)
        assert np.isfinite(rest).all() and np.all(np.diagonal(rest, axis1=-2, axis2=-1) == 1.0)
        ref, va, _ = restate_store(x, pooled=pooled)
        assert scaled_err(cov, ref, va, va) <= TOL
    # a NaN draw: exactly that element's row and column -- pooled: whichever chain holds it; per chain: that chain only
    x[7, 1, 5] = np.nan
    d = eng.to_device(x)
    mask = np.zeros((size, size), dtype=bool)
    mask[5, :] = mask[:, 5] = True
    for correlation in (False, True):
        out = eng.store_cov(d, pooled=True, correlation=correlation).cpu().numpy()
        const = np.zeros_like(mask)
        const[3, :] = const[:, 3] = correlation
        assert np.array_equal(np.isnan(out), mask | const)
        out = eng.store_cov(d, pooled=False, correlation=correlation).cpu().numpy()
        assert np.array_equal(np.isnan(out[1]), mask | const)
        assert np.array_equal(np.isnan(out[0]), const) and np.array_equal(np.isnan(out[2]), const)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(np.isnan(np.cov(x.reshape(-1, size).T)), mask)  # np.cov's own rule
    # the cross form: a's NaN element is a row, b's a column
    other = make_store(62, n_iter, C, 6, mean_over_sd=10.0)
    other[0, 2, 4] = np.nan
    out = eng.store_cov(d, eng.to_device(other), pooled=True).cpu().numpy()
    want = np.zeros((size, 6), dtype=bool)
    want[5, :] = want[:, 4] = True
    assert np.array_equal(np.isnan(out), want)
    eng.close()
    # a single draw gives 0, as omc_store_moments defines its variance
    eng = engine(1)
    one = eng.to_device(make_store(63, 1, 1, 20))
    assert not eng.store_cov(one).cpu().numpy().any() and not eng.store_cov(one, pooled=False).cpu().numpy().any()
    eng.close()
    eng = engine(5)
    one = eng.to_device(make_store(64, 1, 5, 20))
    per_chain = eng.store_cov(one, pooled=False).cpu().numpy()
    assert per_chain.shape == (5, 20, 20) and not per_chain.any()
    eng.close()


# ---------------------------------------------------------------------------------------------------------- public API
def test_covariance_and_correlation_through_mcmc(golden):
    """A short run of the linear-regression model (coefficients + NormalGamma precisions): MCMC.covariance /
    MCMC.correlation against np.cov / np.corrcoef of the collected store."""
    from test_mcmc_api_gpu import build_linreg

    G = golden("linreg_chain")
    C = 3
    M = build_linreg(G, "ex3_", C)
    M.run_mcmc()
    host = M.collect()  # {key: (C, size, n_iter)}, log_post (C, n_iter, 1)
    beta, tau = host["beta"], host["tau"]
    logp = np.transpose(host["log_post"], (0, 2, 1))
    p = beta.shape[1]

    def pooled_rows(arr):  # (C, size, n_iter) -> (size, n_iter * C) in the store's order (iteration-major)
        return np.transpose(arr, (1, 2, 0)).reshape(arr.shape[1], -1)

    def close(out, want, va, vb):
        return np.all(np.abs(out - want) <= TOL * np.sqrt(va[..., :, None] * vb[..., None, :]))

    vb_pool, vb_per = pooled_rows(beta).var(axis=1, ddof=1), beta.var(axis=2, ddof=1)
    cov = M.covariance("beta")
    assert cov.shape == (p, p) and close(cov, np.cov(pooled_rows(beta)), vb_pool, vb_pool)
    per = M.covariance("beta", pooled=False)
    assert per.shape == (C, p, p) and all(close(per[c], np.cov(beta[c]), vb_per[c], vb_per[c]) for c in range(C))
    for other, arr in (("tau", tau), ("log_post", logp)):
        cross = M.covariance("beta", other=other)
        stacked = np.cov(np.vstack([pooled_rows(beta), pooled_rows(arr)]))
        assert cross.shape == (p, 1) and close(cross, stacked[:p, p:], vb_pool, np.diag(stacked)[p:])
        cor = M.correlation("beta", other=other)
        assert np.abs(cor - np.corrcoef(np.vstack([pooled_rows(beta), pooled_rows(arr)]))[:p, p:]).max() <= TOL
        per = M.covariance("beta", other=other, pooled=False)
        assert per.shape == (C, p, 1)
        for c in range(C):
            stacked = np.cov(np.vstack([beta[c], arr[c]]))
            assert close(per[c], stacked[:p, p:], vb_per[c], np.diag(stacked)[p:])
    lp = M.covariance("log_post")
    assert lp.shape == (1, 1) and abs(lp[0, 0] - pooled_rows(logp).var(ddof=1)) <= TOL * lp[0, 0]
    cor = M.correlation("beta")
    assert np.abs(cor - np.corrcoef(pooled_rows(beta))).max() <= TOL and np.all(np.diag(cor) == 1.0)
    per = M.correlation("beta", pooled=False)
    assert all(np.abs(per[c] - np.corrcoef(beta[c])).max() <= TOL for c in range(C))
    sub = M.covariance("beta", index=[p - 1, 0], other="tau", other_index=[0, 0])
    want = np.cov(np.vstack([pooled_rows(beta), pooled_rows(tau)]))
    assert sub.shape == (2, 2) and close(sub, want[[p - 1, 0], p:][:, [0, 0]], vb_pool[[p - 1, 0]], want[p, p] * np.ones(2))
    assert np.array_equal(sub[:, 0], sub[:, 1])
    M.engine.close()
    # a ring store holds the last iterations only: nothing to reduce on the device
    M = build_linreg(G, "ex3_", C, store_ring=6)
    M.run_mcmc()
    for call in (M.covariance, M.correlation):
        with pytest.raises(ValueError, match="store_ring"):
            call("beta")
    M.engine.close()
