"""Ranks of the device store and the rank-normalised diagnostics built on them (omc_store_ranks, omc_store_rank_diagnostics,
Engine.store_ranks / store_rank_diagnostics, MCMC.ranks / rank_diagnostics): ranks bit for bit against
scipy.stats.rankdata, the diagnostics against a numpy restatement of the definitions in include/omcmc_hip.h (Vehtari et al.
2021) written here, known answers, the edges of the contract, and the public API."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-9  # the project's tolerance for the autocovariance sums of omc_store_rhat_ess (tests/test_store_diagnostics_gpu.py)


# ---------------------------------------------------------------------------------------------------------- restatement
def restate(x):
    """(rhat, ess, lags) of a host store x (N, C, size): the definitions of omc_store_rhat_ess, element by element (a copy of
    the restatement in tests/test_store_diagnostics_gpu.py)."""
    N, C, size = x.shape
    M, J = N // 2, 2 * C
    rhat, ess, lags = np.empty(size), np.empty(size), np.zeros(size, dtype=np.int32)
    for k in range(size):
        if np.isnan(x[:, :, k]).any():
            rhat[k] = ess[k] = np.nan
            continue
        xs = np.concatenate([x[:M, :, k].T, x[N - M:, :, k].T])  # (J, M)
        if np.all(xs == xs[0, 0]):
            rhat[k], ess[k] = np.nan, J * M
            continue
        m = xs[:, :1] + (xs - xs[:, :1]).mean(axis=1, keepdims=True)
        y = xs - m
        cache = {}

        def gbar(t):  # mean_j g_j(t)
            if t not in cache:
                cache[t] = np.sum(y[:, :M - t] * y[:, t:]) / (J * M)
            return cache[t]

        W = gbar(0) * M / (M - 1)
        d = m[:, 0] - m[0, 0]
        B_M = np.sum((d - d.mean()) ** 2) / (J - 1)
        var_plus = W * (M - 1) / M + B_M
        with np.errstate(divide="ignore"):
            rhat[k] = np.sqrt(var_plus / W)

        def rho(t):
            return 1.0 - (W - gbar(t)) / var_plus

        r = np.zeros(M)
        r[0] = 1.0
        even, odd = 1.0, rho(1)
        r[1] = odd
        t = 1
        while t < M - 3 and even + odd > 0:
            even, odd = rho(t + 1), rho(t + 2)
            if even + odd >= 0:
                r[t + 1], r[t + 2] = even, odd
            t += 2
        max_t = t - 2
        if even > 0:
            r[max_t + 1] = even
        t = 1
        while t <= max_t - 2:
            if r[t + 1] + r[t + 2] > r[t - 1] + r[t]:
                r[t + 1] = r[t + 2] = (r[t - 1] + r[t]) / 2
            t += 2
        tau = -1 + 2 * np.sum(r[:max_t + 1]) + r[max_t + 1]
        tau = max(tau, 1 / np.log10(J * M))
        ess[k] = J * M / tau
        lags[k] = max_t + 1
    return rhat, ess, lags


def split_draws(col):
    """(2 M, C) split draws of an (N, C) element: the first and the last M = N // 2 iterations"""
    N = col.shape[0]
    M = N // 2
    return np.concatenate([col[:M], col[N - M:]])


def unsplit(v, N, fill):
    """(N, C) series of (2 M, C) values, the dropped middle row of an odd N filled"""
    M = N // 2
    out = np.full((N, v.shape[1]), fill, dtype=float)
    out[:M], out[N - M:] = v[:M], v[M:]
    return out


def ranks_want(x, split):
    """scipy's average ranks of every element of a host store (N, C, size), in the store's layout"""
    from scipy.stats import rankdata

    N, C, size = x.shape
    out = np.empty((N, C, size))
    for k in range(size):
        col = x[:, :, k]
        if np.isnan(col).any():
            out[:, :, k] = np.nan
        elif split:
            xs = split_draws(col)
            out[:, :, k] = unsplit(rankdata(xs.ravel(), method="average").reshape(xs.shape), N, np.nan)
        else:
            out[:, :, k] = rankdata(col.ravel(), method="average").reshape(N, C)
    return out


def rank_restate(x):
    """(rhat, ess_bulk, ess_tail) of a host store x (N, C, size): include/omcmc_hip.h, omc_store_rank_diagnostics, in numpy"""
    from scipy.special import ndtri
    from scipy.stats import rankdata

    N, C, size = x.shape
    S = 2 * C * (N // 2)
    rhat, bulk, tail = np.empty(size), np.empty(size), np.empty(size)

    def znorm(v):
        r = rankdata(v.ravel(), method="average").reshape(v.shape)
        return ndtri((r - 0.375) / (S + 0.25))

    for k in range(size):
        col = x[:, :, k]
        if not np.isfinite(col).all():
            rhat[k] = bulk[k] = tail[k] = np.nan
            continue
        xs = split_draws(col)
        q05, q95 = np.quantile(xs, 0.05), np.quantile(xs, 0.95)
        four = [znorm(xs), znorm(np.abs(xs - np.median(xs))), (xs <= q05).astype(float), (xs <= q95).astype(float)]
        r4, e4, _ = restate(np.stack([unsplit(v, N, 0.0) for v in four], axis=-1))
        rhat[k] = np.nan if np.isnan(r4[0]) or np.isnan(r4[1]) else max(r4[0], r4[1])
        bulk[k] = e4[0]
        tail[k] = min(e4[2], e4[3])
    return rhat, bulk, tail


def ar1(N, C, phis, seed, mu=None):
    """seeded stationary AR(1) store (N, C, len(phis)), one coefficient per element (the generator of
    tests/test_store_diagnostics_gpu.py)"""
    rng = np.random.default_rng(seed)
    phis = np.asarray(phis, dtype=float)
    x = np.empty((N, C, phis.size))
    x[0] = rng.standard_normal((C, phis.size))
    s = np.sqrt(1 - phis ** 2)
    for n in range(1, N):
        x[n] = phis * x[n - 1] + s * rng.standard_normal((C, phis.size))
    return x if mu is None else x + mu


def phis_for(size, lo=-0.7, hi=0.95):
    return np.linspace(lo, hi, size)


def engine(C, **options):
    from openmcmc_amd.engine import Engine

    eng = Engine(C, seed=1)
    for name, value in options.items():
        eng.set_option(name, value)
    return eng


def device(eng, x):
    return eng.to_device(np.ascontiguousarray(x))


def run_ranks(eng, x, index=None, split=False):
    return eng.store_ranks(device(eng, x), index=index, split=split).cpu().numpy()


def run_diag(eng, x, index=None):
    return tuple(t.cpu().numpy() for t in eng.store_rank_diagnostics(device(eng, x), index=index))


def assert_diag(got, want, rtol=RTOL):
    for name, g, w in zip(("rhat", "ess_bulk", "ess_tail"), got, want):
        print(name, "device", g, "restatement", w)
        np.testing.assert_allclose(g, w, rtol=rtol, atol=0, equal_nan=True, err_msg=name)


# ---------------------------------------------------------------------------------------------------------- 1. ranks
RANK_SHAPES = [(4, 1, 1), (5, 3, 7), (9, 4, 5), (64, 8, 33), (257, 16, 130)]
_stores = {}


def rank_store(shape):
    """the AR(1) store of a shape with the contract's special columns put in, and the two expected rank arrays (made once)"""
    if shape not in _stores:
        N, C, size = shape
        x = ar1(N, C, phis_for(size), seed=N * 7 + size)
        rng = np.random.default_rng(N)
        if size >= 5:
            x[:, :, 1] = np.round(2 * x[:, :, 1]) / 2                       # heavy ties
            x[:, :, 2] = -1.75                                              # every draw equal
            x[:, :, 3] = rng.choice([-0.0, 0.0, 1.0, -1.0], size=(N, C))    # the two zeros are one value
            x[:, :, 4] = rng.choice([-np.inf, np.inf, 0.5, -0.5, 2.0], size=(N, C))
            if size >= 7:
                x[:, :, 6] = np.round(2 * x[:, :, 6]) / 2
                x[N // 2, C - 1, 6] = np.inf                                # one infinite draw, in the middle row of an odd N
        _stores[shape] = (x, ranks_want(x, False), ranks_want(x, True))
    return _stores[shape]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("shape", RANK_SHAPES)
def test_ranks_equal_scipy(shape, split):
    x, want_all, want_split = rank_store(shape)
    eng = engine(shape[1])
    got = run_ranks(eng, x, split=split)
    assert np.array_equal(got, want_split if split else want_all, equal_nan=True)
    eng.close()


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("kind", ["halves", "equal", "zeros", "inf"])
def test_ranks_of_a_single_element_store(kind, split):
    """the smallest store, (4, 1, 1), with each of the special columns"""
    col = {"halves": [0.5, -1.0, 0.5, 0.5], "equal": [3.0] * 4, "zeros": [0.0, -0.0, -1.0, -0.0],
           "inf": [np.inf, -np.inf, 0.0, np.inf]}[kind]
    x = np.array(col, dtype=float).reshape(4, 1, 1)
    eng = engine(1)
    assert np.array_equal(run_ranks(eng, x, split=split), ranks_want(x, split))
    eng.close()


@pytest.mark.parametrize("split", [False, True])
def test_ranks_under_an_index(split):
    shape = (9, 4, 5)
    x, want_all, want_split = rank_store(shape)
    idx = [4, 0, 0, 3, 1, 4]
    eng = engine(shape[1])
    got = run_ranks(eng, x, index=idx, split=split)
    assert got.shape == (9, 4, len(idx))
    assert np.array_equal(got, (want_split if split else want_all)[:, :, idx], equal_nan=True)
    eng.close()


# S = 63, 64, 65, 128, 130, 2050 draws per column against tiles of 64 keys: one tile, padding, two tiles, 33 tiles of draws
@pytest.mark.parametrize("N,C,split", [(9, 7, False), (8, 8, False), (16, 4, True), (13, 5, False), (16, 8, False), (27, 5, True),
                                       (13, 10, False), (205, 10, False), (83, 25, True)])
def test_ranks_at_tile_edges(N, C, split):
    S = 2 * C * (N // 2) if split else N * C
    assert S in (63, 64, 65, 128, 130, 2050)
    size = 3
    x = ar1(N, C, phis_for(size), seed=S)
    x[:, :, 1] = np.round(2 * x[:, :, 1]) / 2
    want = ranks_want(x, split)
    for tile in (64, 0):
        eng = engine(C, rank_tile=tile)
        assert np.array_equal(run_ranks(eng, x, split=split), want, equal_nan=True), tile
        eng.close()


@pytest.mark.parametrize("split", [False, True])
def test_a_nan_draw_poisons_its_column_only(split):
    N, C, size = 9, 4, 5
    x = ar1(N, C, phis_for(size), seed=3)
    x[2, 1, 3] = np.nan
    x[N // 2, 0, 0] = np.nan  # the middle row: dropped from the split draws, still a draw of the element
    eng = engine(C)
    got = run_ranks(eng, x, split=split)
    assert np.all(np.isnan(got[:, :, [0, 3]]))
    assert np.array_equal(got, ranks_want(x, split), equal_nan=True)
    keep = np.arange(N) != N // 2 if split else np.ones(N, dtype=bool)
    assert np.all(np.isfinite(got[keep][:, :, [1, 2, 4]]))
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 2. restatement
DIAG_SHAPES = [(4, 1, 3), (5, 3, 7), (9, 4, 5), (64, 8, 9), (257, 4, 6), (1000, 16, 12)]
_diag = {}


def diag_store(shape):
    if shape not in _diag:
        N, C, size = shape
        # coefficients from -0.3: an antithetic AR(1) series has an ESS of S (1 - phi) / (1 + phi), and below phi = -0.5 that is
        # past the cap S log10(S) of these shapes (log10(S) = 3.0 .. 4.2) -- the ESS would then test the cap, not the sums
        x = ar1(N, C, phis_for(size, lo=-0.3), seed=N * 7 + size)
        _diag[shape] = (x, rank_restate(x))
    return _diag[shape]


@pytest.mark.parametrize("shape", DIAG_SHAPES)
def test_diagnostics_match_restatement(shape):
    N, C, size = shape
    x, want = diag_store(shape)
    assert all(np.all(np.isfinite(w)) for w in want), want
    S = 2 * C * (N // 2)
    cap = S * np.log10(S)
    if N >= 64:  # the shapes that test the ESS: below its cap
        assert np.all(want[1] < cap) and np.all(want[2] < cap), (want, cap)
    eng = engine(C)
    assert_diag(run_diag(eng, x), want)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 3. chunks, repeats, tiles
def test_chunks_agree_and_repeats_are_bit_equal():
    shape = (64, 8, 9)
    x, want = diag_store(shape)
    outs = {}
    for chunk in (1, 3, 0):
        eng = engine(shape[1], rank_chunk=chunk)
        d = device(eng, x)
        a, b = ([t.cpu().numpy() for t in eng.store_rank_diagnostics(d)] for _ in range(2))
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes(), chunk
        assert d.cpu().numpy().tobytes() == x.tobytes()  # the store is untouched
        outs[chunk] = a
        eng.close()
    for chunk in (1, 3):
        assert_diag(outs[chunk], outs[0])
    assert_diag(outs[0], want)


def test_chunked_ranks_are_bit_equal():
    shape = (9, 4, 5)
    x, want_all, _ = rank_store(shape)
    for chunk in (1, 2):
        eng = engine(shape[1], rank_chunk=chunk)
        assert np.array_equal(run_ranks(eng, x, index=[4, 0, 0, 3, 1]), want_all[:, :, [4, 0, 0, 3, 1]])
        eng.close()


def test_small_tiles_give_the_same_bits():
    shape = (257, 4, 6)  # S = 2048: one tile by default, 32 tiles of 64, 8 tiles of 256
    x, want = diag_store(shape)
    outs = []
    for tile in (0, 64, 256):
        eng = engine(shape[1], rank_tile=tile)
        outs.append(run_diag(eng, x))
        eng.close()
    for other in outs[1:]:
        for u, v in zip(outs[0], other):
            assert np.array_equal(u, v)
    assert_diag(outs[0], want)


def test_options_are_validated():
    eng = engine(2)
    for name, value in (("rank_tile", 32), ("rank_tile", 96), ("rank_tile", 16384), ("rank_chunk", -1)):
        with pytest.raises(ValueError):
            eng.set_option(name, value)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 4. known answers
@pytest.mark.parametrize("shape", DIAG_SHAPES)
def test_ess_is_invariant_under_a_monotone_map(shape):
    x, _ = diag_store(shape)
    eng = engine(shape[1])
    a, b = run_diag(eng, x), run_diag(eng, np.exp(3 * x))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    eng.close()


def test_a_chain_of_another_scale_is_seen():
    """four chains of 400 N(0, 1) draws, one of them scaled by 5: the chain means agree, so the classic split R-hat is 1;
    the folded rank-normalised one is not"""
    x = np.random.default_rng(11).standard_normal((400, 4, 1))
    x[:, 2] *= 5.0
    eng = engine(4)
    got, want = run_diag(eng, x), rank_restate(x)
    assert_diag(got, want)
    classic = eng.store_rhat_ess(device(eng, x))[0].cpu().numpy()
    print("classic", classic, "rank-normalised", got[0])
    assert np.all(got[0] - classic > 0.1), (got[0], classic)
    eng.close()


def test_cauchy_draws():
    x = np.random.default_rng(12).standard_cauchy((400, 4, 4))
    eng = engine(4)
    got = run_diag(eng, x)
    assert all(np.all(np.isfinite(g)) for g in got)
    assert_diag(got, rank_restate(x))
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 5. edges
def test_three_iterations_are_refused():
    from openmcmc_amd import _abi

    eng = engine(2)
    d = device(eng, np.zeros((3, 2, 4)))
    with pytest.raises(ValueError):
        eng.store_rank_diagnostics(d)
    with pytest.raises(ValueError):
        eng.store_ranks(d, split=True)
    out = eng.empty(4)
    assert _abi.lib.omc_store_rank_diagnostics(eng._ctx, 3, 4, d.data_ptr(), None, 4, out.data_ptr(), None, None) == _abi.INVALID_ARG
    ranks = eng.empty(3, 2, 4)
    assert _abi.lib.omc_store_ranks(eng._ctx, 3, 4, d.data_ptr(), None, 4, 1, ranks.data_ptr()) == _abi.INVALID_ARG
    assert np.array_equal(run_ranks(eng, np.zeros((3, 2, 4))), np.full((3, 2, 4), 3.5))  # without the split, N = 3 is fine
    eng.close()


def test_an_index_out_of_range_is_refused_before_anything_is_written():
    import torch

    from openmcmc_amd import _abi

    N, C, size = 9, 2, 5
    eng = engine(C)
    d = device(eng, ar1(N, C, phis_for(size), seed=1))
    for bad in ([0, size], [-1, 2], [1, 2, 3, 2 ** 40]):
        idx = torch.as_tensor(bad, dtype=torch.int64, device=d.device)
        outs = [eng.full((len(bad),), -7.0) for _ in range(3)]
        st = _abi.lib.omc_store_rank_diagnostics(eng._ctx, N, size, d.data_ptr(), idx.data_ptr(), len(bad), *(o.data_ptr() for o in outs))
        assert st == _abi.INVALID_ARG
        ranks = eng.full((N, C, len(bad)), -7.0)
        assert _abi.lib.omc_store_ranks(eng._ctx, N, size, d.data_ptr(), idx.data_ptr(), len(bad), 0, ranks.data_ptr()) == _abi.INVALID_ARG
        eng.synchronize()
        assert all(np.all(o.cpu().numpy() == -7.0) for o in outs) and np.all(ranks.cpu().numpy() == -7.0)
        with pytest.raises(ValueError):
            eng.store_rank_diagnostics(d, index=bad)
    eng.close()


@pytest.mark.parametrize("N", [9, 130])
def test_constant_infinite_and_nan_elements(N):
    C, size = 3, 6
    x = ar1(N, C, phis_for(size), seed=N)
    x[:, :, 1] = 2.5
    x[N // 3, 1, 3] = np.inf
    x[N // 2, 2, 4] = -np.inf  # the middle row of an odd N
    x[1, 0, 5] = np.nan
    eng = engine(C)
    rhat, bulk, tail = got = run_diag(eng, x)
    S = 2 * C * (N // 2)
    assert np.isnan(rhat[1]) and bulk[1] == S and tail[1] == S
    for k in (3, 4, 5):
        assert np.isnan(rhat[k]) and np.isnan(bulk[k]) and np.isnan(tail[k])
    for k in (0, 2):
        assert np.isfinite(rhat[k]) and np.isfinite(bulk[k]) and np.isfinite(tail[k])
    assert_diag(got, rank_restate(x))
    eng.close()


def test_null_outputs_are_accepted():
    from openmcmc_amd import _abi

    N, C, size = 64, 8, 9
    x, want = diag_store((N, C, size))
    eng = engine(C)
    d = device(eng, x)
    for keep in range(3):
        out = eng.full((size,), -7.0)
        ptrs = [out.data_ptr() if i == keep else None for i in range(3)]
        assert _abi.lib.omc_store_rank_diagnostics(eng._ctx, N, size, d.data_ptr(), None, size, *ptrs) == _abi.OK
        np.testing.assert_allclose(out.cpu().numpy(), want[keep], rtol=RTOL, atol=0)
    assert _abi.lib.omc_store_rank_diagnostics(eng._ctx, N, size, d.data_ptr(), None, size, None, None, None) == _abi.OK
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 6. public API
def store_of(out, key):
    """(n_iter, C, size) host array of a collect() entry"""
    arr = out[key] if key != "log_post" else np.transpose(out[key], (0, 2, 1))  # (C, size, n_iter)
    return np.ascontiguousarray(np.transpose(arr, (2, 0, 1)))


def test_mcmc_rank_diagnostics_and_ranks_gmrf(golden):
    from test_mcmc_api_gpu import build

    G = golden("gmrf_chain")
    M, _ = build(G, "sparse_", True, 6, fuse=True, n_burn=5, n_iter=300, seed=5)
    M.run_mcmc()
    out = M.collect()
    n = store_of(out, "b").shape[2]
    for key, index in (("b", [n - 1, 0, 3, 0]), ("lambda", None), ("log_post", None)):
        x = store_of(out, key)
        sel = x if index is None else x[:, :, index]
        got = M.rank_diagnostics(key, index=index)
        assert sorted(got) == ["ess_bulk", "ess_tail", "rhat"]
        assert_diag((got["rhat"], got["ess_bulk"], got["ess_tail"]), rank_restate(sel))
        assert got["rhat"].shape == (sel.shape[2],)
        for split in (False, True):
            ranks = M.ranks(key, index=index, split=split)
            assert ranks.shape == sel.shape and np.array_equal(ranks, ranks_want(sel, split), equal_nan=True)
    assert M.ranks("log_post").shape == (300, 6, 1)  # a 2-D entry counts as one element
    M.engine.close()


def test_a_ring_store_is_refused(golden):
    from test_mcmc_api_gpu import build_linreg

    M = build_linreg(golden("linreg_chain"), "ex3_", 3, store_ring=6)
    M.run_mcmc()
    for call in (lambda: M.rank_diagnostics("beta"), lambda: M.ranks("beta")):
        with pytest.raises(ValueError, match="store_ring"):
            call()
    M.engine.close()
