"""Linear maps and posterior-predictive draws of the device store (omc_store_project, Engine.store_project) against numpy.

Exact data.  Store entries, weights, offsets and bases are integers in [-2^10, 2^10] times a power of two: every product and every
partial sum of at most 65 of them is an integer below 2^27 times that power, so every order of additions gives the same bits and
the result must be np.array_equal to the integer matmul.  Rounded data is held to the bound of the header,
(n_idx + 2) 2^-53 (|base| + |offset| + sum|terms|) around math.fsum of the terms: n_idx - 1 additions of rounded or fused products
plus the two additions of offset and base -- derived, not measured.  The in-kernel noise is held to tests/philox_model.py within
1e-12 / sqrt(prec) (the bound tests/test_rng_gpu.py holds omc_fill_normal to, divided as the noise is) plus 4 ulp of the result
(the rounded square root, division and addition).

The kernel has one form (no "project_algo" option): a tile of T_R rows x T_M outputs, slabs of T_K selection positions; with
m <= T_M / 2 the tile is 2 T_R rows x T_M / 2 outputs, so both sides of that edge are in the grid of m."""

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_R, T_M, T_K = 64, 128, 32  # PJ_TR, PJ_TM, PJ_TK of omc_project.hip
SHAPES = [(1, 1), (3, 5), (17, 7), (33, 8)]  # (n_iter, C); 33 * 8 = 264 rows: more than 2 * (2 T_R), no multiple of T_R
N_IDX = [1, 2, 3, 4, 5, T_K - 1, T_K, T_K + 1, 2 * T_K + 1]
M_OUT = [1, 2, 3, 4, 5, T_M // 2 - 1, T_M // 2, T_M // 2 + 1, T_M - 1, T_M, T_M + 1, 2 * T_M + 1]
GUARD = -12345.0


@pytest.fixture(scope="module")
def engines():
    from openmcmc_amd.engine import Engine

    made = {}

    def get(C, **kw):
        key = (C,) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = Engine(C, **kw)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def dyadic(rng, shape, power):
    return rng.integers(-1024, 1025, size=shape).astype(np.int64), 2.0 ** power


def make_index(rng, size, n):
    """unsorted, with repeats, holding a contiguous run where there is room; n may exceed size"""
    idx = rng.integers(0, size, size=n)
    run = min(n // 2, size)
    if run >= 2:
        at = int(rng.integers(0, n - run + 1))
        idx[at: at + run] = np.arange(run) + int(rng.integers(0, size - run + 1))
    return idx.astype(np.int64)


def guarded(eng, n_iter, C, m, fill=GUARD):
    """(out, whole): out (n_iter, C, m) with a band of one more iteration slab behind it"""
    whole = eng.full((n_iter + 1, C, m), fill)
    return whole[:n_iter], whole


def run_exact(eng, rng, n_iter, C, size, n, m, with_index, wide_w):
    R = n_iter * C
    xi, sx = dyadic(rng, (R, size), -3)
    wi, sw = dyadic(rng, (m, n), 5)
    oi, bi = dyadic(rng, (m,), 2)[0], dyadic(rng, (R, m), 2)[0]
    idx = make_index(rng, size, n) if with_index else None
    sel = xi if idx is None else xi[:, idx]
    want = (sel @ wi.T).astype(np.float64) * (sx * sw) + oi[None, :] * 4.0 + bi * 4.0
    store = eng.to_device((xi * sx).reshape(n_iter, C, size))
    W = wi * sw
    if wide_w and m > 1:  # rows of a wider device matrix: ld_w = n + 3
        big = eng.to_device(np.concatenate([W, np.full((m, 3), np.nan)], axis=1))
        W = big[:, :n]
        assert W.stride(0) == n + 3
    out, whole = guarded(eng, n_iter, C, m)
    got = eng.store_project(store, W, index=idx, offset=oi * 4.0, base=eng.to_device((bi * 4.0).reshape(n_iter, C, m)), out=out)
    assert got.data_ptr() == out.data_ptr()
    h = whole.cpu().numpy()
    assert np.array_equal(h[:n_iter].reshape(R, m), want), (n_iter, C, size, n, m, with_index)
    assert np.all(h[n_iter] == GUARD)


@pytest.mark.parametrize("n_iter,C", SHAPES)
def test_exact_dyadic_grid(engines, n_iter, C):
    """every (n_idx, m) of the tile edges, without an index (size = n_idx, odd and even: the rows change their 16-byte
    alignment, the even ones take the 16-byte loads) and with one over an odd and an even size"""
    eng = engines(C)
    rng = np.random.default_rng(100 * n_iter + C)
    for j, (n, m) in enumerate((n, m) for n in N_IDX for m in M_OUT):
        run_exact(eng, rng, n_iter, C, n, n, m, False, wide_w=j % 2 == 0)
        run_exact(eng, rng, n_iter, C, 7 if j % 2 else 10, n, m, True, wide_w=j % 3 == 0)


def test_exact_without_base_and_offset(engines):
    eng = engines(5)
    rng = np.random.default_rng(5)
    xi, sx = dyadic(rng, (15, 33), 0)
    wi, sw = dyadic(rng, (3, 33), 0)
    store = eng.to_device(xi.astype(np.float64).reshape(3, 5, 33))
    got = eng.store_project(store, wi.astype(np.float64)).cpu().numpy()
    assert got.shape == (3, 5, 3) and np.array_equal(got.reshape(15, 3), (xi @ wi.T).astype(np.float64))
    one = eng.store_project(store, wi[1].astype(np.float64)).cpu().numpy()  # a 1-D W: one output
    assert one.shape == (3, 5, 1) and np.array_equal(one[..., 0], got[..., 1])


# ---------------------------------------------------------------------------------------------------------------- NaN rules
def nan_case(rng, n_iter, C, size, n, m, with_index):
    R = n_iter * C
    xi, sx = dyadic(rng, (R, size), -2)
    x = xi * sx
    idx = make_index(rng, size, n) if with_index else None
    last = size - 1 if idx is None else int(idx[-1])
    x[rng.random((R, size)) < 0.1] = np.nan
    x[1 % R, :] = np.nan        # an all-NaN row
    x[R - 1, last] = np.nan     # a NaN at the last selected position of the last row
    x[R // 2, last] = np.nan
    wi, sw = dyadic(rng, (m, n), 1)
    return x, wi * sw, idx


@pytest.mark.parametrize("n_iter,C,size,n,m,with_index", [
    (3, 5, 33, 33, 5, False), (17, 7, 34, 34, T_M + 1, False), (3, 5, 9, T_K + 1, 3, True), (33, 8, 65, 65, 17, False),
    (17, 7, 12, 2 * T_K + 1, T_M - 1, True)])
def test_nan_rules(engines, n_iter, C, size, n, m, with_index):
    eng = engines(C)
    rng = np.random.default_rng(n_iter * 1000 + n)
    R = n_iter * C
    x, W, idx = nan_case(rng, n_iter, C, size, n, m, with_index)
    sel = x if idx is None else x[:, idx]
    store = eng.to_device(x.reshape(n_iter, C, size))
    out, whole = guarded(eng, n_iter, C, m)
    eng.store_project(store, W, index=idx, omit_nan=True, out=out)
    h = whole.cpu().numpy()
    want = np.nan_to_num(sel, nan=0.0) @ W.T
    assert np.array_equal(h[:n_iter].reshape(R, m), want)  # (no NaN anywhere: nothing of a padded edge leaked)
    assert np.all(h[n_iter] == GUARD)
    assert np.all(h[1 % R // C, 1 % R % C] == 0.0)  # the all-NaN row: nothing left, no base, no offset
    out, whole = guarded(eng, n_iter, C, m)
    eng.store_project(store, W, index=idx, omit_nan=False, out=out)
    h = whole.cpu().numpy()
    with np.errstate(invalid="ignore"):
        plain = sel @ W.T
    got = h[:n_iter].reshape(R, m)
    assert np.array_equal(np.isnan(got), np.isnan(plain))
    assert np.array_equal(np.isnan(got), np.repeat(np.isnan(sel).any(axis=1)[:, None], m, axis=1))  # whole rows, nothing else
    assert np.array_equal(got[~np.isnan(plain)], plain[~np.isnan(plain)])
    assert np.all(h[n_iter] == GUARD)


def test_inf_against_zero_weight_is_nan(engines):
    eng = engines(5)
    rng = np.random.default_rng(11)
    xi, _ = dyadic(rng, (15, 6), 0)
    wi, _ = dyadic(rng, (4, 6), 0)
    x, W = xi.astype(np.float64), wi.astype(np.float64)
    x[7, 2] = np.inf
    W[:, 2] = [0.0, 1.0, -1.0, 0.0]
    for omit in (True, False):
        got = eng.store_project(eng.to_device(x.reshape(3, 5, 6)), W, omit_nan=omit).cpu().numpy().reshape(15, 4)
        with np.errstate(invalid="ignore"):
            want = x @ W.T
        assert np.array_equal(got, want, equal_nan=True)
        assert np.isnan(got[7, 0]) and np.isnan(got[7, 3]) and got[7, 1] == np.inf and got[7, 2] == -np.inf


# ------------------------------------------------------------------------------------------------------------- rounded data
def test_rounded_data_within_the_bound(engines):
    """Gaussian entries spread over 2^+-20 with heavy cancellation (every row of W is repeated with the opposite sign on a
    slightly perturbed copy of the elements), three slabs of the contraction, with an index."""
    n_iter, C, size, m = 5, 7, 40, 19
    eng = engines(C)
    rng = np.random.default_rng(3)
    R = n_iter * C
    half = rng.standard_normal((R, size // 2)) * 2.0 ** rng.integers(-20, 21, size=(R, size // 2))
    x = np.concatenate([half, half * (1 + 1e-9 * rng.standard_normal(half.shape))], axis=1)
    idx = np.concatenate([rng.permutation(size), rng.integers(0, size, 27)]).astype(np.int64)  # 67 positions
    n = idx.size
    wh = rng.standard_normal((m, size)) * 2.0 ** rng.integers(-20, 21, size=(m, size))
    wh[:, size // 2:] = -wh[:, : size // 2]
    W = wh[:, idx]
    offset = rng.standard_normal(m) * 2.0 ** rng.integers(-20, 21, size=m)
    base = rng.standard_normal((R, m)) * 2.0 ** rng.integers(-20, 21, size=(R, m))
    got = eng.store_project(eng.to_device(x.reshape(n_iter, C, size)), W, index=idx, offset=offset,
                            base=eng.to_device(base.reshape(n_iter, C, m))).cpu().numpy().reshape(R, m)
    sel = x[:, idx]
    worst = 0.0
    for r in range(R):
        for j in range(m):
            t = W[j] * sel[r]
            exact = math.fsum(list(t) + [offset[j], base[r, j]])
            bound = (n + 2) * 2.0 ** -53 * (abs(base[r, j]) + abs(offset[j]) + math.fsum(np.abs(t)))
            worst = max(worst, abs(got[r, j] - exact) / bound)
    print("largest error / bound:", worst)
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- regrouping
@pytest.mark.parametrize("size,m", [(33, 5), (34, T_M + 1), (66, 17)])
def test_rows_keep_their_bits_in_a_smaller_store(engines, size, m):
    """rows [a:b] alone against the same rows of the whole store (odd sizes: another alignment of every row; even sizes: the
    16-byte loads on one side of an 8-byte shift of the buffer and the 8-byte loads on the other); two calls are bit-equal"""
    import torch

    n_iter, C = 21, 7
    eng = engines(C)
    rng = np.random.default_rng(size)
    x = rng.standard_normal((n_iter, C, size)) * 2.0 ** rng.integers(-8, 9, size=(n_iter, C, size))
    W = rng.standard_normal((m, size))
    store = eng.to_device(x)
    whole = eng.store_project(store, W).cpu().numpy()
    assert np.array_equal(whole, eng.store_project(store, W).cpu().numpy())
    for a, b in [(0, 1), (3, 4), (5, 20), (1, 21)]:
        part = eng.store_project(store[a:b], W).cpu().numpy()
        assert np.array_equal(part, whole[a:b]), (a, b)
    flat = torch.empty(x.size + 1, dtype=torch.float64, device=eng.device)
    shifted = flat[1:].view(n_iter, C, size)
    shifted.copy_(store)
    assert shifted.data_ptr() % 16 == 8 and store.data_ptr() % 16 == 0
    assert np.array_equal(eng.store_project(shifted, W).cpu().numpy(), whole)
    idx = np.arange(size, dtype=np.int64)  # the identity as an index: the gathered loads
    assert np.array_equal(eng.store_project(store, W, index=idx).cpu().numpy(), whole)


def test_chains_sharded_over_engines(engines):
    """Engine(8) against two Engine(4) at chain offsets 0 and 4: the linear part and the in-kernel noise"""
    n_iter, size, m, seed = 6, 35, 9, 77
    rng = np.random.default_rng(8)
    x = rng.standard_normal((n_iter, 8, size))
    W = rng.standard_normal((m, size))
    prec = rng.random((n_iter, 8, 1)) + 0.5
    full = engines(8, seed=seed)
    lin = full.store_project(full.to_device(x), W).cpu().numpy()
    noisy = full.store_project(full.to_device(x), W, prec=full.to_device(prec), replicate=3).cpu().numpy()
    assert not np.array_equal(lin, noisy)
    for lo in (0, 4):
        e = engines(4, seed=seed, chain_id_offset=lo)
        xs, ps = e.to_device(x[:, lo: lo + 4].copy()), e.to_device(prec[:, lo: lo + 4].copy())
        assert np.array_equal(e.store_project(xs, W).cpu().numpy(), lin[:, lo: lo + 4])
        assert np.array_equal(e.store_project(xs, W, prec=ps, replicate=3).cpu().numpy(), noisy[:, lo: lo + 4])


def test_in_place_accumulation(engines):
    n_iter, C, size, m = 9, 5, 21, T_M + 3
    eng = engines(C)
    rng = np.random.default_rng(4)
    x = eng.to_device(rng.standard_normal((n_iter, C, size)))
    W = rng.standard_normal((m, size))
    base = eng.to_device(rng.standard_normal((n_iter, C, m)))
    prec = eng.to_device(rng.random((n_iter, C, m)) + 0.5)
    for kw in ({}, {"prec": prec, "replicate": 2}):
        apart = eng.store_project(x, W, base=base, **kw).cpu().numpy()
        acc = base.clone()
        got = eng.store_project(x, W, base=acc, out=acc, **kw)
        assert got.data_ptr() == acc.data_ptr()
        assert np.array_equal(acc.cpu().numpy(), apart)


# --------------------------------------------------------------------------------------------------------------------- noise
@pytest.mark.parametrize("prec_size", ["one", "m"])
def test_injected_noise_is_exact(engines, prec_size):
    n_iter, C, size, m = 17, 7, 33, T_M + 1
    eng = engines(C)
    rng = np.random.default_rng(21)
    R = n_iter * C
    xi, _ = dyadic(rng, (R, size), 0)
    wi, _ = dyadic(rng, (m, size), 0)
    zi, _ = dyadic(rng, (R, m), 0)
    k = rng.integers(0, 6, size=(R, 1 if prec_size == "one" else m))
    lin = (xi @ wi.T).astype(np.float64)
    want = lin + zi * 2.0 ** -k  # z / sqrt(4^k), exact
    got = eng.store_project(eng.to_device(xi.astype(np.float64).reshape(n_iter, C, size)), wi.astype(np.float64),
                            prec=eng.to_device((4.0 ** k).reshape(n_iter, C, -1)),
                            z=eng.to_device(zi.astype(np.float64).reshape(n_iter, C, m))).cpu().numpy().reshape(R, m)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("offset_chain", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("m", [5, T_M + 2])
def test_stream_noise_matches_the_model(engines, offset_chain, m):
    import philox_model as pm

    n_iter, C, size, seed = 4, 3, 6, 0x1234567887654321
    eng = engines(C, seed=seed, chain_id_offset=offset_chain)
    rng = np.random.default_rng(m)
    x = eng.to_device(rng.standard_normal((n_iter, C, size)))
    W = rng.standard_normal((m, size))
    lin = eng.store_project(x, W).cpu().numpy()
    seen = {}
    for prec_size in (1, m):
        prec = 10.0 ** rng.uniform(-3, 3, size=(n_iter, C, prec_size))
        for rep in (0, 1, 15):
            got = eng.store_project(x, W, prec=eng.to_device(prec), replicate=rep).cpu().numpy()
            for it in range(n_iter):
                for c in range(C):
                    z = pm.normals(seed, (1 << 41) + it + (rep << 44), offset_chain + c, m)
                    want = lin[it, c] + z / np.sqrt(prec[it, c])
                    tol = 1e-12 / np.sqrt(prec[it, c]) + 4 * np.spacing(np.abs(got[it, c]))
                    assert np.all(np.abs(got[it, c] - want) <= tol), (prec_size, rep, it, c)
            seen[(prec_size, rep)] = got
    assert not np.array_equal(seen[(1, 0)], seen[(1, 1)]) and not np.array_equal(seen[(1, 1)], seen[(1, 15)])


# -------------------------------------------------------------------------------------------------------------------- errors
def test_invalid_arguments_through_the_abi(engines):
    import torch

    from openmcmc_amd import _abi

    eng = engines(5)
    lib = _abi.lib
    n_iter, size, m = 3, 6, 4
    store, W, out = eng.zeros(n_iter, 5, size), eng.zeros(m, size), eng.full((n_iter, 5, m), GUARD)
    prec, z = eng.full((n_iter, 5, m), 1.0), eng.zeros(n_iter, 5, m)
    idx = torch.zeros(3, dtype=torch.int64, device=eng.device)
    good = dict(ctx=eng._ctx, n_iter=n_iter, size=size, store=store.data_ptr(), idx=None, n_idx=size, m=m, W=W.data_ptr(), ld_w=size,
                offset=None, base=None, omit_nan=1, prec=None, prec_size=0, z=None, replicate=0, out=out.data_ptr())
    assert lib.omc_store_project(*good.values()) == _abi.OK
    eng.check_status()
    out.fill_(GUARD)
    bad = [("context", dict(ctx=None)), ("n_iter", dict(n_iter=0)), ("size", dict(size=0)), ("m < 1", dict(m=0)), ("NULL", dict(store=None)),
           ("NULL", dict(W=None)), ("NULL", dict(out=None)), ("n_idx", dict(n_idx=0)), ("n_idx", dict(n_idx=size - 1)),
           ("ld_w", dict(ld_w=size - 1)), ("ld_w", dict(idx=idx.data_ptr(), n_idx=3, ld_w=2)), ("prec_size", dict(prec=prec.data_ptr(), prec_size=2)),
           ("together", dict(prec=prec.data_ptr(), prec_size=0)), ("together", dict(prec=None, prec_size=1)),
           ("z_inject", dict(z=z.data_ptr())), ("replicate", dict(prec=prec.data_ptr(), prec_size=m, replicate=16))]
    for text, change in bad:
        args = dict(good, **change)
        assert lib.omc_store_project(*args.values()) == _abi.INVALID_ARG, change
        assert text.encode() in lib.omc_last_error(), (text, lib.omc_last_error())
    assert np.all(out.cpu().numpy() == GUARD)


def test_invalid_arguments_raise_value_error(engines):
    eng = engines(5)
    store, W = eng.zeros(3, 5, 6), np.zeros((4, 6))
    prec, z = eng.full((3, 5, 4), 1.0), eng.zeros(3, 5, 4)
    with pytest.raises(ValueError, match="n_iter < 1"):
        eng.store_project(eng.zeros(0, 5, 6), W)
    for kw in (dict(W=np.zeros((4, 5))), dict(W=np.zeros((0, 6))), dict(offset=np.zeros(3)), dict(base=eng.zeros(2, 5, 4)),
               dict(base=eng.zeros(3, 5, 3)), dict(prec=eng.zeros(3, 5, 2)), dict(z=z), dict(prec=prec, replicate=16),
               dict(prec=prec, replicate=-1), dict(out=eng.zeros(3, 5, 5)), dict(W=np.zeros((6, 6)), out=store), dict(index=[0.5]), dict(index=[])):
        with pytest.raises(ValueError):
            eng.store_project(store, **dict(dict(W=W), **kw))
    for bad_idx in ([0, 6], [-1, 2, 3]):
        out = eng.full((3, 5, 4), GUARD)
        with pytest.raises(ValueError, match="outside"):
            eng.store_project(store, np.zeros((4, len(bad_idx))), index=bad_idx, out=out)
        assert np.all(out.cpu().numpy() == GUARD)
    eng.check_status()
