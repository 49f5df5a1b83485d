"""Autocovariance, autocorrelation and integrated autocorrelation time of the device store (omc_store_autocorr,
Engine.store_autocorr, MCMC.autocorrelation) against the numpy + math.fsum restatement of include/omcmc_hip.h written here.

The restatement centres every column on the mean the call itself returned (mean_out), so the only error left is the summation:
every autocovariance is held to
    |got - fsum(d_i d_{i+t}) / den| <= (terms + 2) 2^-53 sum|d_i d_{i+t}| / den,   den = N (per chain) or N C (pooled),
terms = N - t or C (N - t): the worst case of any order of additions of rounded or fused products ((terms + 1) 2^-53 sum|.|, as
tests/test_store_derive_gpu.py derives it for sums), one more 2^-53 for the restatement's own rounded products and the final
division -- derived, not measured.  A plain sequential float sum, or one cut into 64-row slices, stays inside it on these inputs
(below a tenth of it from 32 terms on) and a missing term misses it a million times over, so the bound finds a wrong or missing
term, not noise.  Normalised lags, tau and window are compared with array_equal:
they are fixed sequences of IEEE operations on the device's own autocovariances.

The grid of test 1 holds 9100 columns of 257 draws at its largest.  math.fsum costs 0.1 us per product, so the store of that
test is built from a block of five base elements: element k is base element k % 5 times 2^(k // 5).  A power of two scales
the mean, the deviations, the products and every sum exactly, so the exact lag sums of element k are those of its base element
times 4^(k // 5) and are computed once per (N, C); neighbouring columns still differ, so a term taken from the wrong column or
row is seen.  Where a column's returned mean is not that power of two times its base column's (nothing promises it), the
column is restated on its own."""

import itertools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BASE = 5
PHIS = (0.0, 0.9, -0.7)


# ---------------------------------------------------------------------------------------------------------- restatement
def ar1(rng, N, shape, phi, stationary=False):
    """(N,) + shape: AR(1) columns along axis 0, phi a scalar or an array that broadcasts to shape"""
    e = rng.standard_normal((N,) + tuple(shape))
    x = np.empty_like(e)
    x[0] = e[0] / np.sqrt(1.0 - np.asarray(phi) ** 2) if stationary else e[0]
    for i in range(1, N):
        x[i] = phi * x[i - 1] + e[i]
    return x


def restate(x, mean, L=None):
    """x (N, C, n) finite draws, mean (C, n) the call's own means: exact lag sums by math.fsum and sum|terms| by numpy, lags 0 .. L:
    per chain (C, n, L + 1) twice, pooled (n, L + 1) twice"""
    N, C, n = x.shape
    L = N - 1 if L is None else L
    d = x - mean[None]
    pc, pc_mag = np.empty((C, n, L + 1)), np.empty((C, n, L + 1))
    po, po_mag = np.empty((n, L + 1)), np.empty((n, L + 1))
    for t in range(L + 1):
        p = d[: N - t] * d[t:]  # (N - t, C, n)
        cols = np.ascontiguousarray(np.transpose(p, (1, 2, 0))).reshape(C * n, N - t).tolist()
        pc[:, :, t] = np.array(list(map(math.fsum, cols))).reshape(C, n)
        pc_mag[:, :, t] = np.abs(p).sum(axis=0)
        for k in range(n):
            po[k, t] = math.fsum(itertools.chain.from_iterable(cols[c * n + k] for c in range(C)))
        po_mag[:, t] = np.abs(p).sum(axis=(0, 1))
    return pc, pc_mag, po, po_mag


def geyer(rho):
    """(tau, window) of the rows of rho (..., L + 1): the loop of include/omcmc_hip.h"""
    L = rho.shape[-1] - 1
    flat = rho.reshape(-1, L + 1)
    tau, window = np.empty(len(flat)), np.zeros(len(flat), dtype=np.int32)
    for r, row in enumerate(flat.tolist()):
        if row[0] != row[0]:
            tau[r], window[r] = np.nan, 0
            continue
        acc, k = -1.0, 0
        while 2 * k + 1 <= L:
            pair = row[2 * k] + row[2 * k + 1]
            if not pair > 0.0:
                break
            acc += 2.0 * pair
            k += 1
        tau[r], window[r] = acc, 2 * k
    return tau.reshape(rho.shape[:-1]), window.reshape(rho.shape[:-1])


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def assert_bound(got, exact, mag, N, C_pool, what):
    """got (..., L + 1) autocovariances against exact lag sums and sum|terms| of the same shape; C_pool: chains added (1 per chain)"""
    L = got.shape[-1] - 1
    terms = C_pool * (N - np.arange(L + 1))
    den = float(N) * float(C_pool)
    err, bound = np.abs(got - exact / den), (terms + 2) * U * mag / den
    worst = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
    print(what, "largest error / bound", worst)
    assert got.shape == exact.shape and np.all(err <= bound), (what, worst)


def engine(C, **options):
    from openmcmc_amd.engine import Engine

    eng = Engine(C, seed=1)
    for name, value in options.items():
        eng.set_option(name, value)
    return eng


def device(eng, x):
    return eng.to_device(np.ascontiguousarray(x))


def run(eng, d, L, **kw):
    return tuple(t.cpu().numpy() for t in eng.store_autocorr(d, L, **kw))


def check_call(eng, d, x, L, index=None, what=None):
    """both poolings of one selection at lag L against the restatement: bound, normalisation, tau and window, the mean twice"""
    N, C, _ = x.shape
    sel = x if index is None else x[:, :, np.asarray(index)]
    ref = None
    for pooled in (False, True):
        acv, _, _, mean = run(eng, d, L, index=index, pooled=pooled, normalize=False)
        acf, tau, window, mean2 = run(eng, d, L, index=index, pooled=pooled, normalize=True)
        assert same(mean, mean2) and mean.shape == (C, sel.shape[2])
        if ref is None:
            ref = restate(sel, mean, L)
        exact, mag = (ref[2], ref[3]) if pooled else (ref[0], ref[1])
        assert_bound(acv, exact, mag, N, C if pooled else 1, (what, L, pooled))
        with np.errstate(all="ignore"):
            assert same(acf, acv / acv[..., :1]), (what, L, pooled)
        want_tau, want_window = geyer(acf)
        assert same(tau, want_tau) and same(window, want_window) and window.dtype == np.int32, (what, L, pooled)
    return ref


# ---------------------------------------------------------------------------------------------------------- 1. the bound on the grid
def lags_of(N):
    return sorted({min(L, N - 1) for L in (0, 1, 31, 32, 33, 64, N - 1)})


_grid_cache = {}


def grid_base(N, C):
    """(N, C, BASE) AR(1) columns offset by 5, phi by (chain + element) % 3"""
    rng = np.random.default_rng(100 * N + C)
    phi = np.array(PHIS)[(np.arange(C)[:, None] + np.arange(BASE)[None, :]) % 3]
    return ar1(rng, N, (C, BASE), phi) + 5.0


def grid_reference(N, C, base, mean, size):
    """exact lag sums of the store whose element k is base element k % BASE times 2^(k // BASE), from the base block's: per chain
    (C, size, N) twice, pooled (size, N) twice; mean (C, size) the call's own"""
    nb = min(size, BASE)
    key = (N, C, nb, mean[:, :nb].tobytes())
    if key not in _grid_cache:
        _grid_cache[key] = restate(base[:, :, :nb], mean[:, :nb])
    k = np.arange(size)
    four = 4.0 ** (k // BASE)
    out = [r[..., k % BASE, :] * four[:, None] for r in _grid_cache[key]]
    odd = np.flatnonzero(np.any(mean != mean[:, k % BASE] * 2.0 ** (k // BASE), axis=0))
    for kk in odd:  # a mean that did not scale with its column: that element on its own
        col = base[:, :, kk % BASE: kk % BASE + 1] * 2.0 ** (kk // BASE)
        for o, r in zip(out, restate(col, mean[:, kk: kk + 1])):
            o[..., kk, :] = r[..., 0, :]
    return out


@pytest.mark.parametrize("N", [2, 3, 31, 32, 33, 64, 65, 257])
def test_autocovariance_within_the_bound_on_the_grid(N):
    for C in (1, 3, 70):
        base = grid_base(N, C)
        eng = engine(C)
        for size in (1, 5, 64, 65, 130):
            k = np.arange(size)
            x = base[:, :, k % BASE] * 2.0 ** (k // BASE)
            d = device(eng, x)
            for L in lags_of(N):
                for pooled in (False, True):
                    acv, _, _, mean = run(eng, d, L, pooled=pooled, normalize=False)
                    pc, pc_mag, po, po_mag = grid_reference(N, C, base, mean, size)
                    exact, mag = (po, po_mag) if pooled else (pc, pc_mag)
                    assert_bound(acv, exact[..., : L + 1], mag[..., : L + 1], N, C if pooled else 1, (N, C, size, L, pooled))
        eng.close()
    _grid_cache.clear()


def test_the_bound_separates_rounding_from_a_wrong_term():
    """CPU only.  Sequential and 64-row-sliced float sums of the grid's inputs stay inside the bound (below a tenth of it from 32
    terms on; a sum of two or three terms can use a third of it), and a sum that lacks its largest term misses it a million
    times over: the term is at least sum|terms| / terms, the bound at most (terms + 2) 2^-53 sum|terms|."""
    N, C = 257, 3
    x = grid_base(N, C)
    mean = x.mean(axis=0)
    pc, pc_mag, _, _ = restate(x, mean)
    d = x - mean[None]
    worst, worst_long = 0.0, 0.0
    for t in range(N):
        p = d[: N - t] * d[t:]
        seq = np.zeros((C, BASE))
        for row in p:
            seq = seq + row
        sliced = sum((p[r: r + 64].sum(axis=0) for r in range(0, N - t, 64)), np.zeros((C, BASE)))
        bound = (N - t + 2) * U * pc_mag[:, :, t]
        ratio = max(float(np.max(np.abs(seq - pc[:, :, t]) / bound)), float(np.max(np.abs(sliced - pc[:, :, t]) / bound)))
        worst, worst_long = max(worst, ratio), max(worst_long, ratio if N - t >= 32 else 0.0)
        assert np.all(np.abs(p).max(axis=0) > 1e6 * bound), t
    print("largest error / bound of a plain sum", worst, "from 32 terms on", worst_long)
    assert worst < 1.0 and worst_long < 0.1


# ---------------------------------------------------------------------------------------------------------- 2., 3. normalisation, tau
def test_normalisation_tau_and_window():
    N, C = 400, 3
    rng = np.random.default_rng(3)
    x = np.stack([rng.standard_normal((N, C)), ar1(rng, N, (C,), 0.9, True) + 5.0, ar1(rng, N, (C,), -0.7, True) - 2.0], axis=2)
    eng = engine(C)
    d = device(eng, x)
    windows = {}
    for L in (0, 1, 2, 7, 8, 150, N - 1):
        check_call(eng, d, x, L, what="tau")
        for pooled in (False, True):
            _, tau, window, _ = run(eng, d, L, pooled=pooled)
            windows[L, pooled] = window
            assert tau.shape == window.shape == ((3,) if pooled else (C, 3))
    # phi = 0.9: at 150 lags the sequence ends inside them; at 7 or 8 it runs into max_lag (window >= L, L odd; >= L - 1, L even)
    assert 8 < windows[150, True][1] < 149 and np.all(windows[150, False][:, 1] < 149)
    assert windows[7, True][1] == 8 and windows[8, True][1] == 8 and windows[1, True][1] == 2 and windows[0, True][1] == 0
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 4. seams
@pytest.fixture(scope="module")
def seam_case():
    N, C, size = 257, 3, 65
    rng = np.random.default_rng(4)
    phi = np.array(PHIS)[(np.arange(C)[:, None] + np.arange(size)[None, :]) % 3]
    return ar1(rng, N, (C, size), phi) + 5.0, {}


@pytest.mark.parametrize("rows", [0, 1, 7, 64, 300])
def test_time_slices_hold_the_bound_at_their_seams(seam_case, rows):
    x, refs = seam_case
    N, C, _ = x.shape
    eng = engine(C, autocorr_slice=rows)
    d = device(eng, x)
    for L in (33, 64, 256):
        for pooled in (False, True):
            acv, _, _, mean = run(eng, d, L, pooled=pooled, normalize=False)
            key = mean.tobytes()
            if key not in refs:
                refs[key] = restate(x, mean)
            pc, pc_mag, po, po_mag = refs[key]
            exact, mag = (po, po_mag) if pooled else (pc, pc_mag)
            assert_bound(acv, exact[..., : L + 1], mag[..., : L + 1], N, C if pooled else 1, (rows, L, pooled))
    with pytest.raises(ValueError):
        eng.set_option("autocorr_slice", -1)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 5. index
def test_index_selections():
    import torch

    from openmcmc_amd import _abi

    N, C, size = 65, 3, 20
    rng = np.random.default_rng(5)
    x = ar1(rng, N, (C, size), 0.9) + 5.0
    eng = engine(C)
    d = device(eng, x)
    sub = rng.permutation(size)[:9]
    for L in (0, 33, N - 1):
        for index in (np.concatenate([sub, sub[:3], sub[:1]]), [size // 2], rng.integers(0, size, size + 7), [size - 1]):
            check_call(eng, d, x, L, index=index, what="index")
    index = np.concatenate([sub, sub[:3], sub[:1]])
    for pooled in (False, True):
        acf, tau, window, mean = run(eng, d, 40, index=index, pooled=pooled)  # positions 9 .. 11 repeat 0 .. 2
        assert same(acf[..., 9:12, :], acf[..., :3, :]) and all(same(v[..., 9:12], v[..., :3]) for v in (tau, window, mean))
    # the chunks of option "rank_chunk": same bits
    whole, every = run(eng, d, 40, index=index, pooled=False), run(eng, d, 40)
    eng.set_option("rank_chunk", 4)
    assert all(same(a, b) for a, b in zip(whole, run(eng, d, 40, index=index, pooled=False)))
    assert all(same(a, b) for a, b in zip(every, run(eng, d, 40)))
    eng.set_option("rank_chunk", 0)
    # an index outside the store: refused before anything is written
    L = 10
    for bad in ([0, 1, size], [-1, 2, 3]):
        idx = torch.as_tensor(bad, dtype=torch.int64, device=d.device)
        for per_chain in (0, 1):
            lead = (C,) if per_chain else ()
            acf, tau, mean = eng.full(lead + (3, L + 1), -7.0), eng.full(lead + (3,), -7.0), eng.full((C, 3), -7.0)
            window = torch.full(lead + (3,), -7, dtype=torch.int32, device=d.device)
            st = _abi.lib.omc_store_autocorr(eng._ctx, N, size, d.data_ptr(), idx.data_ptr(), 3, L, per_chain, 1, acf.data_ptr(),
                                             tau.data_ptr(), window.data_ptr(), mean.data_ptr())
            eng.synchronize()
            assert st == _abi.INVALID_ARG and "index outside" in _abi.lib.omc_last_error().decode()
            assert all(np.all(t.cpu().numpy() == -7) for t in (acf, tau, mean, window))
        with pytest.raises(ValueError, match="index outside"):
            eng.store_autocorr(d, L, index=bad)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 6. edge rules
def test_nan_inf_and_constant_columns():
    N, C, size, L = 70, 3, 6, 69
    rng = np.random.default_rng(6)
    clean = ar1(rng, N, (C, size), 0.9) + 5.0
    eng = engine(C)
    want = {p: run(eng, device(eng, clean), L, pooled=p) for p in (False, True)}
    for value, row in ((np.nan, 35), (np.inf, 35), (-np.inf, 0), (np.inf, N - 1)):
        x = clean.copy()
        x[row, 1, 2] = value
        for normalize in (False, True):
            acf, tau, window, _ = run(eng, device(eng, x), L, pooled=False, normalize=normalize)
            assert np.isnan(acf[1, 2]).all() and np.isnan(tau[1, 2]) and window[1, 2] == 0  # every lag, also those whose terms miss the draw
            hit = np.zeros((C, size), dtype=bool)
            hit[1, 2] = True
            assert not np.isnan(acf[~hit]).any() and not np.isnan(tau[~hit]).any()
            if normalize:
                assert same(acf[~hit], want[False][0][~hit]) and same(tau[~hit], want[False][1][~hit])
            acf, tau, window, _ = run(eng, device(eng, x), L, pooled=True, normalize=normalize)
            assert np.isnan(acf[2]).all() and np.isnan(tau[2]) and window[2] == 0
            rest = np.arange(size) != 2
            assert not np.isnan(acf[rest]).any() and (not normalize or (same(acf[rest], want[True][0][rest]) and same(tau[rest], want[True][1][rest])))
    # a column of 0.1 repeated: the rounded mean must not leak in
    x = clean.copy()
    x[:, :, 3] = 0.1
    x[:, 0, 4] = 0.1  # one constant chain of an element whose other chains move
    d = device(eng, x)
    acv, tau, window, mean = run(eng, d, L, pooled=False, normalize=False)
    assert np.all(acv[:, 3] == 0.0) and np.isnan(tau[:, 3]).all() and np.all(window[:, 3] == 0) and np.all(mean[:, 3] == 0.1)
    assert np.all(acv[0, 4] == 0.0) and np.isnan(tau[0, 4]) and window[0, 4] == 0
    acf, tau, window, _ = run(eng, d, L, pooled=False, normalize=True)
    assert np.isnan(acf[:, 3]).all() and np.isnan(acf[0, 4]).all()
    moving = np.ones((C, size), dtype=bool)
    moving[:, 3] = False
    moving[0, 4] = False
    assert same(acf[moving], want[False][0][moving]) and same(tau[moving], want[False][1][moving]) and same(window[moving], want[False][2][moving])
    acv, tau, window, mean = run(eng, d, L, pooled=True, normalize=False)
    assert np.all(acv[3] == 0.0) and np.isnan(tau[3]) and window[3] == 0
    acf = run(eng, d, L, pooled=True, normalize=True)[0]
    assert np.isnan(acf[3]).all()
    rest = np.array([0, 1, 2, 5])
    assert same(acf[rest], want[True][0][rest])
    # the pooled element with one constant chain: that chain adds exactly 0
    y = np.ascontiguousarray(x[:, :, 4:5])
    pc, _, po, po_mag = restate(y, mean[:, 4:5], L)
    assert np.all(pc[0] == 0.0)
    assert_bound(acv[4:5], po, po_mag, N, C, "one constant chain")
    check_call(eng, d, x, L, what="constant columns")
    eng.close()


def test_two_draws_and_invalid_arguments():
    import torch

    from openmcmc_amd import _abi

    C, size = 3, 5
    x = np.random.default_rng(7).standard_normal((2, C, size)) + 5.0
    eng = engine(C)
    d = device(eng, x)
    for L in (0, 1):
        check_call(eng, d, x, L, what="N = 2")
    x4 = np.random.default_rng(8).standard_normal((4, C, size))
    d4 = device(eng, x4)
    idx = torch.as_tensor([0, 1], dtype=torch.int64, device=d4.device)

    def abi(n_iter=4, sz=size, index=None, n_idx=None, L=1):
        acf, tau, mean = eng.full((C, size, 4), -7.0), eng.full((C, size), -7.0), eng.full((C, size), -7.0)
        window = torch.full((C, size), -7, dtype=torch.int32, device=d4.device)
        st = _abi.lib.omc_store_autocorr(eng._ctx, n_iter, sz, d4.data_ptr(), None if index is None else index.data_ptr(),
                                         (size if index is None else index.numel()) if n_idx is None else n_idx, L, 1, 1, acf.data_ptr(),
                                         tau.data_ptr(), window.data_ptr(), mean.data_ptr())
        eng.synchronize()
        return st, _abi.lib.omc_last_error().decode(), all(np.all(t.cpu().numpy() == -7) for t in (acf, tau, mean, window))

    for kw, text_has in (({"n_iter": 1, "L": 0}, "n_iter"), ({"sz": 0}, "size"), ({"L": -1}, "max_lag"), ({"L": 4}, "max_lag"),
                         ({"index": idx, "n_idx": 0}, "n_idx"), ({"n_idx": size - 1}, "n_idx")):
        st, text, untouched = abi(**kw)
        assert st == _abi.INVALID_ARG and text_has in text and untouched, (kw, text)
    assert abi(L=3)[0] == _abi.OK
    # tau, window and mean may be NULL
    acf = eng.full((size, 4), -7.0)
    assert _abi.lib.omc_store_autocorr(eng._ctx, 4, size, d4.data_ptr(), None, size, 3, 0, 0, acf.data_ptr(), None, None, None) == _abi.OK
    assert same(acf.cpu().numpy(), run(eng, d4, 3, normalize=False)[0])
    for bad in (-1, 4):
        with pytest.raises(ValueError, match="max_lag"):
            eng.store_autocorr(d4, bad)
    with pytest.raises(ValueError, match="at least 2"):
        eng.store_autocorr(d4[:1].contiguous(), 0)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 7. determinism
def test_repeated_calls_are_bit_equal():
    N, C, size = 300, 5, 33
    x = ar1(np.random.default_rng(9), N, (C, size), 0.9) + 5.0
    eng = engine(C, autocorr_slice=64)
    d = device(eng, x)
    for index in (None, [3, 32, 3, 0]):
        for pooled in (False, True):
            a, b = (run(eng, d, 100, index=index, pooled=pooled) for _ in range(2))
            assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b)), (index, pooled)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 8. statistical sense
def test_tau_of_known_processes():
    N, C, L, phi = 4000, 8, 200, 0.9
    rng = np.random.default_rng(0)
    x = np.concatenate([ar1(rng, N, (C, 2), phi, stationary=True), rng.standard_normal((N, C, 2))], axis=2)
    eng = engine(C)
    _, tau, window, _ = run(eng, device(eng, x), L, pooled=True)
    print("tau", tau, "window", window)
    assert np.all(np.abs(tau[:2] - (1 + phi) / (1 - phi)) <= 0.25 * 19.0) and np.all(window[:2] < L - 1)
    assert np.all(np.abs(tau[2:] - 1.0) <= 0.05)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 9. through MCMC
def store_of(out, key):
    """(n_iter, C, size) host array of a collect() entry"""
    arr = out[key] if key != "log_post" else np.transpose(out[key], (0, 2, 1))  # (C, size, n_iter)
    return np.ascontiguousarray(np.transpose(arr, (2, 0, 1)))


def test_mcmc_autocorrelation(golden):
    from test_mcmc_api_gpu import build, build_linreg

    M, _ = build(golden("gmrf_chain"), "sparse_", True, 4, fuse=True, n_burn=5, n_iter=120, seed=5)
    M.run_mcmc()
    M.derive("b", "max", name="b_max")
    out = M.collect()
    for key, index in (("b", [0, 3, 0]), ("b", None), ("log_post", None), ("b_max", None)):
        x = store_of(out, key)
        N, C, n = x.shape
        sel = x if index is None else x[:, :, index]
        t = M._store_3d(key)
        for pooled in (True, False):
            mean = M.engine.store_autocorr(t, 30, index=index, pooled=pooled)[3].cpu().numpy()  # the restatement's input
            got = M.autocorrelation(key, max_lag=30, index=index, pooled=pooled, normalize=False)
            assert set(got) == {"acf", "tau", "window"}
            pc, pc_mag, po, po_mag = restate(sel, mean, 30)
            exact, mag = (po, po_mag) if pooled else (pc, pc_mag)
            assert_bound(got["acf"], exact, mag, N, C if pooled else 1, (key, pooled))
            norm = M.autocorrelation(key, max_lag=30, index=index, pooled=pooled)
            with np.errstate(all="ignore"):
                assert same(norm["acf"], got["acf"] / got["acf"][..., :1])
            want_tau, want_window = geyer(norm["acf"])
            assert same(norm["tau"], want_tau) and same(norm["window"], want_window) and same(got["tau"], want_tau)
    assert M.autocorrelation("b")["acf"].shape == (M._store_3d("b").shape[2], 101)  # max_lag = min(100, n_iter - 1)
    M.engine.close()
    M, _ = build(golden("gmrf_chain"), "sparse_", True, 4, fuse=True, n_burn=2, n_iter=12, seed=5)
    M.run_mcmc()
    assert M.autocorrelation("b", pooled=False)["acf"].shape[::2] == (4, 12)  # n_iter - 1 = 11 lags
    M.engine.close()
    M = build_linreg(golden("linreg_chain"), "ex3_", 3, store_ring=6)
    M.run_mcmc()
    with pytest.raises(ValueError, match="store_ring"):
        M.autocorrelation("beta")
    M.engine.close()
