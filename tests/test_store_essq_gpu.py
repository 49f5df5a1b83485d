"""omc_store_ess_indicator and omc_store_order_stats (Engine.store_ess_indicator, Engine.store_order_stats) on the device, held to
the exact model of tests/essq_model.py on the inputs of tests/essq_cases.py: the integer counts, the lags and the thresholds
array_equal, the ESS within the project's fp64 tolerance 1e-10 (its only roundings are one conversion of Z(t) and Geyer's
arithmetic; tests/test_essq_model_host.py checks that no decision on these inputs is closer to zero than 1e-9).  Then bit-equality
over repeats, sort tiles, chunk sizes and the two forms of the lag kernel, the refusals, and consistency with the tail ESS of
omc_store_rank_diagnostics."""

import ctypes as C

import numpy as np
import pytest
from essq_cases import case, cases, model

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in cases()]


def engine(n_chains, **options):
    from openmcmc_amd.engine import Engine

    eng = Engine(n_chains, seed=1)
    for name, value in options.items():
        eng.set_option(name, value)
    return eng


def run(c, algo=0, **options):
    eng = engine(c["x"].shape[1], **options)
    try:
        store = eng.to_device(c["x"])
        out = eng.store_ess_indicator(store, c["lo"], c["hi"], index=c["idx"], counts=c["n_cnt"], algo=algo)
        got = dict(zip(("ess", "lags", "q", "counts"), (t.cpu().numpy() for t in out)))
        assert np.array_equal(store.cpu().numpy(), c["x"], equal_nan=True)  # the store is read only
        return got
    finally:
        eng.close()


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.int64) if b[k].dtype == np.float64 else b[k]) for k in a) and set(a) == set(b)


@pytest.mark.parametrize("name", NAMES)
def test_held_to_the_exact_model(name):
    c, m = case(name), model(name)
    got = run(c)
    live = ~m["dead"]
    if c["n_cnt"]:
        assert np.array_equal(got["counts"], m["counts"])
    assert np.array_equal(got["lags"], m["lags"])
    assert np.array_equal(got["q"][:, live], m["q"][:, live], equal_nan=True)
    assert np.all(np.isnan(got["ess"][:, m["dead"]]))
    err = np.abs(got["ess"][:, live] - m["ess"][:, live]) / m["ess"][:, live]
    print(name, "largest relative error of the ESS:", err.max(), "longest sequence:", got["lags"].max())
    assert err.max() <= 1e-10


def test_the_known_answers():
    ends, lev = run(case("ends")), run(case("levels"))
    JM = 2 * 2 * 45
    assert np.all(ends["ess"][[1, 2]] == JM) and np.all(ends["lags"][[1, 2]] == 0)  # prob 1 and (0, 1): the all-ones indicator
    assert np.all(ends["counts"][[1, 2], :, 0] == JM)
    assert np.all(lev["lags"][0] == 16) and np.all(np.isfinite(lev["ess"]))  # W == 0 < B_M: rho = 1 up to the M - 3 limit


@pytest.mark.parametrize("name", ["edge-N129", "edge-N257", "slow", "32-intervals", "selection", "non-finite"])
def test_same_bits_whatever_the_tiling_chunking_and_form(name):
    c = case(name)
    base = run(c)
    for kw in ({}, {"rank_tile": 64}, {"rank_chunk": 1}, {"rank_chunk": 3}, {"algo": 1}, {"algo": 2}):
        assert same_bits(base, run(c, **kw)), kw


def test_the_large_store_in_both_forms():
    c = case("large")
    assert same_bits(run(c, algo=1), run(c, algo=2))


def raw_call(eng, store, n_iter, size, idx, n_idx, lo, hi, outs, n_cnt=0, algo=0):
    from openmcmc_amd._abi import lib

    dp = C.POINTER(C.c_double)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return lib.omc_store_ess_indicator(eng._ctx, n_iter, size, store.data_ptr(), None if idx is None else idx.data_ptr(), n_idx,
                                       lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), lo.size, algo, *(t.data_ptr() for t in outs), n_cnt)


def test_refusals_leave_the_outputs_untouched():
    import torch

    from openmcmc_amd import _abi

    eng = engine(2)
    try:
        x = case("ends")["x"]
        store = eng.to_device(x)
        N, size = x.shape[0], x.shape[2]

        def outputs(n_p, n):
            return [torch.full((n_p, n), -7.0, dtype=torch.float64, device=store.device),
                    torch.full((n_p, n), -7, dtype=torch.int32, device=store.device),
                    torch.full((n_p, n, 2), -7.0, dtype=torch.float64, device=store.device),
                    torch.full((n_p, n, 2), -7, dtype=torch.int64, device=store.device)]

        far = torch.tensor([0, size], dtype=torch.int64, device=store.device)
        neg = torch.tensor([-1, 0], dtype=torch.int64, device=store.device)
        refused = [
            ("n_iter 3", dict(store=eng.to_device(x[:3]), n_iter=3, lo=[-1.0], hi=[0.5])),
            ("n_p 0", dict(lo=[], hi=[])),
            ("n_p 33", dict(lo=[-1.0] * 33, hi=[0.5] * 33)),
            ("lo > hi", dict(lo=[-1.0, 0.6], hi=[0.5, 0.4])),
            ("prob > 1", dict(lo=[-1.0], hi=[1.5])),
            ("lo > 1", dict(lo=[1.5], hi=[1.0])),
            ("NaN prob", dict(lo=[-1.0], hi=[np.nan])),
            ("index == size", dict(idx=far, n_idx=2, lo=[-1.0], hi=[0.5])),
            ("index < 0", dict(idx=neg, n_idx=2, lo=[-1.0], hi=[0.5])),
            ("n_cnt > M", dict(lo=[-1.0], hi=[0.5], n_cnt=N // 2 + 1)),
            ("algo 3", dict(lo=[-1.0], hi=[0.5], algo=3)),
        ]
        for what, kw in refused:
            n_idx = kw.get("n_idx", size)
            outs = outputs(max(len(kw["lo"]), 1), n_idx)
            st = raw_call(eng, kw.get("store", store), kw.get("n_iter", N), size, kw.get("idx"), n_idx, kw["lo"], kw["hi"], outs,
                          n_cnt=kw.get("n_cnt", 0), algo=kw.get("algo", 0))
            assert st == _abi.INVALID_ARG, what
            torch.cuda.synchronize()
            assert all(bool((t == -7).all()) for t in outs), what
        with pytest.raises(ValueError):
            eng.store_ess_indicator(store, [0.6], [0.4])
        # the call still works afterwards, and NULL outputs are allowed
        outs = outputs(1, size)
        from openmcmc_amd._abi import lib

        one = (C.c_double * 1)(-1.0), (C.c_double * 1)(0.5)
        assert lib.omc_store_ess_indicator(eng._ctx, N, size, store.data_ptr(), None, size, one[0], one[1], 1, 0, outs[0].data_ptr(), None,
                                           None, None, 0) == _abi.OK
        assert np.array_equal(outs[0].cpu().numpy(), eng.store_ess_indicator(store, None, [0.5])[0].cpu().numpy())
    finally:
        eng.close()


def test_a_store_too_long_for_exact_integers_is_unsupported():
    import torch

    eng = engine(1)
    try:
        N = 2 * 1_330_000  # J M^3 = 2 M^3 >= 2^62
        assert 2 * (N // 2) ** 3 >= 2 ** 62
        store = torch.zeros((N, 1, 1), dtype=torch.float64, device=eng.device)
        with pytest.raises(NotImplementedError):
            eng.store_ess_indicator(store, None, [0.5])
    finally:
        eng.close()


def test_the_tails_agree_with_rank_diagnostics():
    c = case("large")
    eng = engine(c["x"].shape[1])
    try:
        store = eng.to_device(c["x"])
        ess = eng.store_ess_indicator(store, None, [0.05, 0.95])[0].cpu().numpy()
        tail = eng.store_rank_diagnostics(store)[2].cpu().numpy()
        np.testing.assert_allclose(ess.min(axis=0), tail, rtol=1e-8, atol=0)
    finally:
        eng.close()


@pytest.mark.parametrize("split", [True, False])
def test_order_stats(split):
    x = case("non-finite")["x"].copy()  # N = 131: the split drops the middle row, which holds the NaN of element 1
    x[3, 0, 0], x[4, 1, 0] = -0.0, 0.0
    N, Cn, size = x.shape
    M = N // 2
    idx = np.array([4, 0, 3, 0, 2, 1])
    rng = np.random.default_rng(1)
    eng = engine(Cn)
    try:
        store = eng.to_device(x)
        for chunk in (0, 1, 4):
            eng.set_option("rank_chunk", chunk)
            for index in (None, idx):
                cols = np.arange(size) if index is None else index
                S = 2 * Cn * M if split else N * Cn
                pos = np.concatenate([np.zeros((cols.size, 1), dtype=np.int64), np.full((cols.size, 1), S - 1),
                                      rng.integers(0, S, size=(cols.size, 5))], axis=1)
                got = eng.store_order_stats(store, pos, index=index, split=split).cpu().numpy()
                for k, col in enumerate(cols):
                    draws = (np.concatenate([x[:M, :, col], x[N - M:, :, col]]) if split else x[:, :, col]).reshape(-1)
                    if np.isnan(x[:, :, col]).any():
                        assert np.all(np.isnan(got[k]))
                    else:
                        assert np.array_equal(got[k], np.sort(draws)[pos[k]])
                        assert not np.any(np.signbit(got[k][got[k] == 0]))  # a zero comes back as +0.0
        eng.set_option("rank_chunk", 0)
        before = eng.store_order_stats(store, np.zeros((size, 1), dtype=np.int64), split=split)
        S = 2 * Cn * M if split else N * Cn
        for bad in (S, -1):
            pos = np.zeros((size, 2), dtype=np.int64)
            pos[2, 1] = bad
            with pytest.raises(ValueError):
                eng.store_order_stats(store, pos, split=split)
        with pytest.raises(ValueError):
            eng.store_order_stats(store, np.zeros((2, 1), dtype=np.int64), index=[0, size], split=split)
        assert np.array_equal(before.cpu().numpy(), eng.store_order_stats(store, np.zeros((size, 1), dtype=np.int64), split=split).cpu().numpy(),
                              equal_nan=True)
    finally:
        eng.close()
