"""Highest-density intervals of the device store (omc_store_hdi, Engine.store_hdi, MCMC.hdi) against the numpy restatement of
the definition in include/omcmc_hip.h (ArviZ's unimodal hdi) written here.  Both limits are stored draws, so every comparison is
np.array_equal(..., equal_nan=True): there is no tolerance in this file."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- restatement
def hdi_ref(col, prob, omit_nan=True):
    """(lower, upper) of one column of draws"""
    col = np.asarray(col, dtype=np.float64).ravel()
    nan = np.isnan(col)
    if np.isinf(col).any() or (nan.any() and not omit_nan):
        return np.nan, np.nan
    x = np.sort(col[~nan])
    n = x.size
    if n == 0:
        return np.nan, np.nan
    m = min(int(np.floor(np.float64(prob) * n)), n - 1)
    w = x[m:] - x[:n - m]
    i = int(np.argmin(w))
    return x[i], x[i + m]


def hdi_want(x, probs, pooled=True, omit_nan=True):
    """(n_prob, size, 2) or (n_prob, C, size, 2) of a host store x (N, C, size)"""
    N, C, size = x.shape
    probs = np.atleast_1d(probs)
    out = np.empty((len(probs), size, 2) if pooled else (len(probs), C, size, 2))
    for p, prob in enumerate(probs):
        for k in range(size):
            if pooled:
                out[p, k] = hdi_ref(x[:, :, k], prob, omit_nan)
            else:
                for c in range(C):
                    out[p, c, k] = hdi_ref(x[:, c, k], prob, omit_nan)
    return out


def count_want(x, pooled=True):
    ok = ~np.isnan(x)
    return ok.sum(axis=(0, 1)) if pooled else ok.sum(axis=0)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def engine(C, **options):
    from openmcmc_amd.engine import Engine

    eng = Engine(C, seed=1)
    for name, value in options.items():
        eng.set_option(name, value)
    return eng


def device(eng, x):
    return eng.to_device(np.ascontiguousarray(x))


def run(eng, x, prob, **kw):
    """(hdi, n_valid) of Engine.store_hdi as host arrays"""
    out, cnt = eng.store_hdi(x if hasattr(x, "is_cuda") else device(eng, x), prob, **kw)
    return out.cpu().numpy(), cnt.cpu().numpy()


def abi(eng, d, probs, idx=None, per_chain=False, omit_nan=True, out=None, cnt=None):
    """status of omc_store_hdi called through the bare C ABI on a device store d (N, C, size)"""
    from openmcmc_amd import _abi

    N, _, size = d.shape
    host = (ctypes.c_double * len(probs))(*probs)
    return _abi.lib.omc_store_hdi(eng._ctx, N, size, d.data_ptr(), None if idx is None else idx.data_ptr(),
                                  size if idx is None else idx.numel(), host, len(probs), int(per_chain), int(omit_nan),
                                  None if out is None else out.data_ptr(), None if cnt is None else cnt.data_ptr())


def draws(N, C, size, seed):
    """normal draws with a column of heavy ties (when there are three columns)"""
    x = np.random.default_rng(seed).standard_normal((N, C, size))
    if size >= 3:
        x[:, :, 1] = np.round(2 * x[:, :, 1]) / 2
    return x


PROBS3 = [0.5, 0.94, 0.2]


# ---------------------------------------------------------------------------------------------------------- 1. column lengths
# pooled S = 1, 2, 5, 63, 64, 65, 200, 257 draws per column; with tiles of 64 keys S = 200 and 257 run the global passes
@pytest.mark.parametrize("tile", [64, 0])
@pytest.mark.parametrize("N,C", [(1, 1), (1, 2), (5, 1), (9, 7), (8, 8), (13, 5), (25, 8), (257, 1)])
def test_pooled_lengths_around_the_sorts_edges(N, C, tile):
    import torch

    assert N * C in (1, 2, 5, 63, 64, 65, 200, 257)
    x = draws(N, C, 3, seed=N * C)
    eng = engine(C, rank_tile=tile)
    d = device(eng, x)
    want = hdi_want(x, PROBS3)
    got, cnt = run(eng, d, PROBS3)
    assert same(got, want)
    assert np.array_equal(cnt, np.full(3, N * C))
    # the same through the bare C ABI
    out = eng.full((3, 3, 2), -7.0)
    n_valid = torch.full((3,), -7, dtype=torch.int64, device=d.device)
    assert abi(eng, d, PROBS3, out=out, cnt=n_valid) == 0
    assert same(out.cpu().numpy(), want) and np.array_equal(n_valid.cpu().numpy(), cnt)
    assert abi(eng, d, PROBS3, out=out) == 0  # n_valid_out may be NULL
    eng.close()


def test_pooled_above_the_default_tile():
    """3000 x 4 = 12 000 draws, P = 16 384: two tiles of the shipped 8192 keys, a global pass, one slice of a 256-thread workgroup"""
    x = draws(3000, 4, 3, seed=12)
    x[:, :, 2] = np.random.default_rng(1).gamma(2.0, size=(3000, 4))
    eng = engine(4)
    assert len(eng.rank_schedule(12000)) > 1
    got, _ = run(eng, x, PROBS3)
    assert same(got, hdi_want(x, PROBS3))
    eng.close()


@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 4, 65, 200])
def test_per_chain_lengths(N, C):
    x = draws(N, C, 3, seed=100 * N + C)
    outs = []
    for tile in (64, 0):
        eng = engine(C, rank_tile=tile)
        got, cnt = run(eng, x, PROBS3, pooled=False)
        assert same(got, hdi_want(x, PROBS3, pooled=False)), tile
        assert np.array_equal(cnt, np.full((C, 3), N))
        outs.append(got)
        eng.close()
    assert outs[0].tobytes() == outs[1].tobytes()


def test_per_chain_over_many_elements():
    """more elements than a gather tile holds (16), and an odd count"""
    x = draws(37, 5, 35, seed=9)
    eng = engine(5)
    got, _ = run(eng, x, [0.8], pooled=False)
    assert same(got, hdi_want(x, [0.8], pooled=False))
    got, _ = run(eng, x, [0.8])
    assert same(got, hdi_want(x, [0.8]))
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("pooled", [True, False])
def test_integer_draws_and_a_constant_column(pooled):
    N, C = 50, 4
    rng = np.random.default_rng(2)
    x = np.empty((N, C, 3))
    x[:, :, 0] = rng.integers(0, 4, size=(N, C))
    x[:, :, 1] = -1.75
    x[:, :, 2] = rng.integers(0, 4, size=(N, C)) * 0.5
    eng = engine(C)
    got, _ = run(eng, x, PROBS3, pooled=pooled)
    assert same(got, hdi_want(x, PROBS3, pooled=pooled))
    assert np.all(got[:, ..., 1, :] == -1.75)
    eng.close()


def test_equal_windows_go_to_the_first():
    """a shuffled arange(S): every window is exactly m wide, so the answer is (0, m).  S = 40 000 is three slices of the window
    kernel (16 384 windows each) at the smallest probability, and 4 x 256 threads' strides within a slice"""
    N, C = 5000, 8
    S = N * C
    x = np.random.default_rng(3).permutation(S).astype(np.float64).reshape(N, C, 1)
    probs = [0.1, 0.5, 0.94]
    eng = engine(C)
    got, _ = run(eng, x, probs)
    for p, prob in enumerate(probs):
        m = int(np.floor(prob * S))
        assert S - m > 2 * 16384 or p > 0
        assert got[p, 0, 0] == 0.0 and got[p, 0, 1] == float(m), (prob, got[p])
    assert same(got, hdi_want(x, probs))
    # per chain the same holds chain by chain for a shuffled arange(N) in every chain: N = 5000 is the 256-thread form, one slice
    rng = np.random.default_rng(4)
    y = np.stack([rng.permutation(N) for _ in range(C)], axis=1).astype(np.float64).reshape(N, C, 1)
    got, _ = run(eng, y, [0.3], pooled=False)
    assert np.all(got[0, :, 0, 0] == 0.0) and np.all(got[0, :, 0, 1] == float(int(np.floor(0.3 * N))))
    eng.close()


@pytest.mark.parametrize("n,shape", [(200, (25, 8)), (40000, (5000, 8))])
def test_the_minimum_at_three_and_again_near_the_end(n, shape):
    """gaps of 2 between neighbouring order statistics, of 1 inside the window at i = 3 and inside the last but one window:
    both are exactly m wide, every other window is wider"""
    prob = 0.3
    m = int(np.floor(prob * n))
    L = n - m
    gaps = np.full(n - 1, 2.0)
    gaps[3:3 + m] = 1.0
    gaps[L - 2:L - 2 + m] = 1.0
    xs = np.concatenate([[0.0], np.cumsum(gaps)]) - 17.0
    w = xs[m:] - xs[:L]
    assert w.min() == m and list(np.flatnonzero(w == w.min())) == [3, L - 2]
    x = np.random.default_rng(5).permutation(xs).reshape(*shape, 1)
    eng = engine(shape[1])
    got, _ = run(eng, x, [prob])
    assert got[0, 0, 0] == xs[3] and got[0, 0, 1] == xs[3 + m]
    assert same(got, hdi_want(x, [prob]))
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 3. probabilities
def test_m_zero_and_m_n_minus_one():
    N, C = 25, 2  # n = 50
    x = draws(N, C, 3, seed=6)
    eng = engine(C)
    got, _ = run(eng, x, [0.01, 0.999])
    lo, hi = x.min(axis=(0, 1)), x.max(axis=(0, 1))
    assert np.array_equal(got[0, :, 0], lo) and np.array_equal(got[0, :, 1], lo)  # prob n < 1: (x[0], x[0])
    assert np.array_equal(got[1, :, 0], lo) and np.array_equal(got[1, :, 1], hi)  # floor(0.999 50) = 49 = n - 1
    assert same(got, hdi_want(x, [0.01, 0.999]))
    got, _ = run(eng, x, [0.01, 0.999], pooled=False)
    assert same(got, hdi_want(x, [0.01, 0.999], pooled=False))
    eng.close()


@pytest.mark.parametrize("pooled", [True, False])
def test_three_probabilities_equal_three_calls(pooled):
    x = draws(200, 3, 4, seed=7)
    eng = engine(3)
    d = device(eng, x)
    got, _ = run(eng, d, PROBS3, pooled=pooled)
    for p, prob in enumerate(PROBS3):
        one, _ = run(eng, d, prob, pooled=pooled)  # a scalar is one probability
        assert one.shape[0] == 1 and one[0].tobytes() == got[p].tobytes()
    full, _ = run(eng, d, np.linspace(0.1, 0.9, 8), pooled=pooled)
    assert same(full, hdi_want(x, np.linspace(0.1, 0.9, 8), pooled=pooled))
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 4. NaN
def ragged(N, C, size, seed):
    """a store padded with NaN: another number of valid draws in every (chain, element), among them none, one and all"""
    rng = np.random.default_rng(seed)
    x = rng.gamma(2.0, size=(N, C, size))
    keep = rng.integers(0, N + 1, size=(C, size))
    keep[0, 0], keep[-1, 0] = 0, 1
    keep[:, 1] = N  # an element without a NaN
    keep[:, 2] = 0  # an element without a valid draw in any chain
    for c in range(C):
        for k in range(size):
            x[rng.permutation(N)[keep[c, k]:], c, k] = np.nan
    return x, keep


@pytest.mark.parametrize("pooled", [True, False])
def test_nan_padding_is_left_out(pooled):
    N, C, size = 70, 3, 6
    x, keep = ragged(N, C, size, seed=8)
    assert np.array_equal(count_want(x, pooled=False), keep)
    eng = engine(C)
    d = device(eng, x)
    got, cnt = run(eng, d, PROBS3, pooled=pooled)
    assert same(got, hdi_want(x, PROBS3, pooled=pooled))
    assert np.array_equal(cnt, count_want(x, pooled=pooled))
    assert np.all(np.isnan(got[:, ..., 2, :]))  # no valid draw
    if not pooled:
        assert np.all(np.isnan(got[:, 0, 0, :]))
        one = x[:, C - 1, 0][~np.isnan(x[:, C - 1, 0])]
        assert one.size == 1 and np.all(got[:, C - 1, 0, :] == one[0])  # one valid draw: (x, x)
    # omit_nan=False: NaN wherever the column holds one, the count is still that of the valid draws
    got, cnt = run(eng, d, PROBS3, pooled=pooled, omit_nan=False)
    want = hdi_want(x, PROBS3, pooled=pooled, omit_nan=False)
    assert same(got, want)
    assert np.array_equal(cnt, count_want(x, pooled=pooled))
    whole = count_want(x, pooled=pooled) == (N * C if pooled else N)
    assert np.array_equal(np.isnan(got[0, ..., 0]), ~whole) and whole.any()
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 5. other inputs
@pytest.mark.parametrize("pooled", [True, False])
def test_an_infinite_draw_poisons_its_column_only(pooled):
    N, C, size = 40, 3, 5
    x = draws(N, C, size, seed=10)
    x[7, 1, 0] = np.inf
    x[0, 2, 3] = -np.inf
    x[1, 0, 3] = np.nan
    eng = engine(C)
    got, _ = run(eng, x, [0.9], pooled=pooled)
    assert same(got, hdi_want(x, [0.9], pooled=pooled))
    if pooled:
        assert np.array_equal(np.isnan(got[0, :, 0]), [True, False, False, True, False])
    else:
        assert np.isnan(got[0, 1, 0, 0]) and np.isnan(got[0, 2, 3, 0]) and np.isnan(got).sum() == 4
    eng.close()


def test_the_two_zeros_are_one_value():
    N, C = 30, 2
    rng = np.random.default_rng(11)
    x = np.empty((N, C, 2))
    x[:, :, 0] = rng.choice([-0.0, 0.0], size=(N, C))
    x[:, :, 1] = rng.choice([-0.0, 0.0, 1.0, -1.0], size=(N, C), p=[0.4, 0.4, 0.1, 0.1])
    eng = engine(C)
    for pooled in (True, False):
        got, _ = run(eng, x, [0.5, 0.9], pooled=pooled)
        assert same(got, hdi_want(x, [0.5, 0.9], pooled=pooled))
        assert np.all(got[:, ..., 0, :] == 0.0)
    eng.close()


def test_an_index_with_repeats_in_any_order():
    x = draws(33, 4, 20, seed=13)
    idx = [19, 0, 0, 7, 3, 19, 18, 1, 0, 2, 4, 5, 6, 8, 9, 10, 11, 17]  # 18: more than one gather tile
    eng = engine(4)
    for pooled in (True, False):
        got, cnt = run(eng, x, PROBS3, index=idx, pooled=pooled)
        assert same(got, hdi_want(x[:, :, idx], PROBS3, pooled=pooled))
        assert cnt.shape == ((len(idx),) if pooled else (4, len(idx)))
    eng.close()


def test_bad_arguments_are_refused_before_anything_is_written():
    import torch

    from openmcmc_amd import _abi

    N, C, size = 9, 2, 5
    eng = engine(C)
    d = device(eng, draws(N, C, size, seed=14))
    for per_chain in (False, True):
        shape = (1, C, 3, 2) if per_chain else (1, 3, 2)
        for bad in ([0, 1, size], [-1, 2, 3], [1, 2, 2 ** 40]):
            idx = torch.as_tensor(bad, dtype=torch.int64, device=d.device)
            out = eng.full(shape, -7.0)
            cnt = torch.full(shape[1:-1], -7, dtype=torch.int64, device=d.device)
            assert abi(eng, d, [0.9], idx=idx, per_chain=per_chain, out=out, cnt=cnt) == _abi.INVALID_ARG
            eng.synchronize()
            assert np.all(out.cpu().numpy() == -7.0) and np.all(cnt.cpu().numpy() == -7)
            with pytest.raises(ValueError):
                eng.store_hdi(d, 0.9, index=bad, pooled=not per_chain)
        for probs in ([0.0], [1.0], [0.5, -0.1], [0.5, float("nan")], [1.5], [0.5] * 9, []):
            out = eng.full((max(len(probs), 1),) + shape[1:], -7.0)
            assert abi(eng, d, probs, per_chain=per_chain, out=out) == _abi.INVALID_ARG
            eng.synchronize()
            assert np.all(out.cpu().numpy() == -7.0)
            with pytest.raises(ValueError):
                eng.store_hdi(d, probs, pooled=not per_chain)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 6. repeats and options
@pytest.mark.parametrize("pooled", [True, False])
def test_chunks_and_repeats_are_bit_equal(pooled):
    N, C, size = 70, 3, 7
    x, _ = ragged(N, C, size, seed=15)
    outs = {}
    for chunk in (1, 3, 0):
        eng = engine(C, rank_chunk=chunk)
        d = device(eng, x)
        (a, ca), (b, cb) = (run(eng, d, PROBS3, pooled=pooled) for _ in range(2))
        assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes(), chunk
        assert d.cpu().numpy().tobytes() == x.tobytes()  # the store is untouched
        outs[chunk] = (a, ca)
        eng.close()
    for chunk in (1, 3):
        assert outs[chunk][0].tobytes() == outs[0][0].tobytes() and outs[chunk][1].tobytes() == outs[0][1].tobytes(), chunk
    assert same(outs[0][0], hdi_want(x, PROBS3, pooled=pooled))


# ---------------------------------------------------------------------------------------------------------- 7. a skewed law
def test_gamma_draws_give_an_interval_no_wider_than_the_equal_tailed_one():
    N, C = 2000, 4
    x = np.random.default_rng(16).gamma(2.0, size=(N, C, 1))
    prob = 0.94
    eng = engine(C)
    got, _ = run(eng, x, prob)
    lo, hi = got[0, 0]
    col = x.ravel()
    n = col.size
    m = min(int(np.floor(prob * n)), n - 1)
    q03, q97 = np.quantile(col, [0.03, 0.97])
    print("hdi", lo, hi, "equal-tailed", q03, q97)
    assert hi - lo <= q97 - q03
    assert np.count_nonzero((col >= lo) & (col <= hi)) >= m + 1
    assert lo < q03  # the mode of Gamma(2) is left of its median: the interval shifts to the left
    assert same(got, hdi_want(x, [prob]))
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 8. the sort's other user
def test_ranks_still_equal_scipy():
    from scipy.stats import rankdata

    N, C, size = 65, 5, 3  # S = 325: tiles of 64 run the global passes
    x = draws(N, C, size, seed=17)
    for tile in (64, 0):
        eng = engine(C, rank_tile=tile)
        got = eng.store_ranks(device(eng, x)).cpu().numpy()
        for k in range(size):
            assert np.array_equal(got[:, :, k], rankdata(x[:, :, k].ravel(), method="average").reshape(N, C))
        eng.close()


# ---------------------------------------------------------------------------------------------------------- 9. public API
def store_of(out, key):
    """(n_iter, C, size) host array of a collect() entry"""
    arr = out[key] if key != "log_post" else np.transpose(out[key], (0, 2, 1))  # (C, size, n_iter)
    return np.ascontiguousarray(np.transpose(arr, (2, 0, 1)))


def test_mcmc_hdi_gmrf(golden):
    from test_mcmc_api_gpu import build

    G = golden("gmrf_chain")
    M, _ = build(G, "sparse_", True, 6, fuse=True, n_burn=5, n_iter=300, seed=5)
    M.run_mcmc()
    out = M.collect()
    n = store_of(out, "b").shape[2]
    nine = np.linspace(0.1, 0.9, 9)
    for key, index in (("b", [n - 1, 0, 3, 0]), ("lambda", None), ("log_post", None)):
        x = store_of(out, key)
        sel = x if index is None else x[:, :, index]
        for pooled in (True, False):
            got = M.hdi(key, index=index, pooled=pooled)  # prob = 0.94, the leading axis dropped
            assert same(got, hdi_want(sel, [0.94], pooled=pooled)[0])
            got = M.hdi(key, prob=nine, index=index, pooled=pooled)  # nine probabilities: two calls of omc_store_hdi
            assert same(got, hdi_want(sel, nine, pooled=pooled))
            assert same(M.hdi(key, prob=[0.5], index=index, pooled=pooled), hdi_want(sel, [0.5], pooled=pooled))
    assert M.hdi("log_post").shape == (1, 2) and M.hdi("log_post", pooled=False).shape == (6, 1, 2)  # a 2-D entry is one element
    with pytest.raises(ValueError):
        M.hdi("b", prob=1.0)
    with pytest.raises(ValueError):
        M.hdi("b", prob=[])
    M.engine.close()


def test_a_ring_store_is_refused(golden):
    from test_mcmc_api_gpu import build_linreg

    M = build_linreg(golden("linreg_chain"), "ex3_", 3, store_ring=6)
    M.run_mcmc()
    with pytest.raises(ValueError, match="store_ring"):
        M.hdi("beta")
    M.engine.close()
