"""Pareto-smoothed importance sampling of the device store (omc_store_psis, Engine.store_psis) against the numpy restatement
tests/psis_model.py at np.longdouble, on the columns tests/test_psis_model_host.py checks on the CPU: nine columns per call that mix
the regimes (k on both sides of 0.7, tails of 4 draws or fewer, ties at the cut).  The restatement runs on the pointwise
log-likelihoods the device itself made (omc_store_loglik's ll_out), so both sort the same numbers: the tail lengths must be
np.array_equal, elpd and k within 1e-10 of max(1, |value|) -- the project's fp64 parity tolerance; the CPU check leaves four orders
of room below it."""

import numpy as np
import pytest
from psis_model import PSIS_SHAPES, psis, psis_inputs, tail_max_of

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def cases(engines):
    """per shape: the device inputs, the device's own ll and the restatement's answer on it, computed once"""
    made = {}

    def get(n_iter, C):
        if (n_iter, C) not in made:
            eng = engines(C)
            S = n_iter * C
            mu, y, tau = psis_inputs(S)
            d = dict(eng=eng, S=S, M=tail_max_of(S), mean=eng.to_device(mu.reshape(n_iter, C, 9)), y=eng.to_device(y),
                     prec=eng.to_device(tau.reshape(n_iter, C, 9)))
            d["ll"] = eng.store_loglik(d["mean"], d["y"], d["prec"], lse=False, mean=False, var=False, ll=True)[3]
            d["want"] = psis(d["ll"].cpu().numpy().reshape(S, 9), d["M"], np.longdouble)
            made[(n_iter, C)] = d
        return made[(n_iter, C)]

    return get


def close(got, want):
    return np.abs(got - want) <= 1e-10 * np.maximum(1.0, np.abs(want))


@pytest.mark.parametrize("n_iter,C", PSIS_SHAPES)
def test_against_the_restatement(cases, n_iter, C):
    d = cases(n_iter, C)
    eng, S = d["eng"], d["S"]
    elpd, k, tail = (t.cpu().numpy() for t in eng.store_psis(d["ll"], d["M"]))
    e_w, k_w, t_w, _ = d["want"]
    print((n_iter, C), "tail", tail, "k", k, "elpd error", np.max(np.abs(elpd - e_w)))
    assert np.array_equal(tail, t_w)
    assert np.array_equal(np.isinf(k), tail <= 4) and np.array_equal(np.isinf(k), np.isinf(k_w)) and np.all(k[np.isinf(k)] > 0)
    fin = np.isfinite(k_w)
    assert np.all(close(k[fin], k_w[fin])) and np.all(close(elpd, e_w))
    if S >= 25:
        assert tail[8] < d["M"]  # the ties at the cut are not tail
    # the mean entry with y and the precision: ll computed on load, the same bits as over ll_out
    for a, b in zip(eng.store_psis(d["mean"], d["M"], y=d["y"], prec=d["prec"]), (elpd, k, tail)):
        assert np.array_equal(a.cpu().numpy(), b)
    # a selection (unsorted, with a repeat), per-column tail lengths, a scalar precision, and the same call twice
    idx = np.array([8, 1, 1, 3, 0])
    tm = np.array([d["M"], max(1, d["M"] - 1), d["M"], 1, S - 1])
    e_s, k_s, t_s, _ = psis(d["ll"].cpu().numpy().reshape(S, 9)[:, idx], tm, np.longdouble)
    first = [t.cpu().numpy() for t in eng.store_psis(d["ll"], tm, index=idx)]
    assert np.array_equal(first[2], t_s) and np.all(close(first[0], e_s))
    f = np.isfinite(k_s)
    assert np.all(close(first[1][f], k_s[f])) and np.array_equal(np.isinf(first[1]), np.isinf(k_s))
    for a, b in zip(first, eng.store_psis(d["ll"], tm, index=idx)):
        assert np.array_equal(a, b.cpu().numpy())
    one = d["prec"][:, :, :1].contiguous()  # tau = 1: columns 0 .. 3 and 8 are as before
    sub = np.array([0, 2, 8, 3])
    for a, b in zip(eng.store_psis(d["mean"], d["M"], index=sub, y=d["y"][sub], prec=one), (elpd, k, tail)):
        assert np.array_equal(a.cpu().numpy(), b[sub])


@pytest.mark.parametrize("n_iter,C", [(125, 8), (4099, 1)])
def test_sort_options_give_the_same_bits(cases, n_iter, C):
    from openmcmc_amd.engine import Engine

    d = cases(n_iter, C)
    base = [t.cpu().numpy() for t in d["eng"].store_psis(d["ll"], d["M"])]
    eng = Engine(C)
    try:
        eng.set_option("rank_tile", 64)
        eng.set_option("rank_chunk", 1)
        for a, b in zip(base, eng.store_psis(d["ll"], d["M"])):
            assert np.array_equal(a, b.cpu().numpy())
    finally:
        eng.close()


def test_non_finite_columns(cases):
    d = cases(16, 4)
    eng = d["eng"]
    clean = [t.cpu().numpy() for t in eng.store_psis(d["ll"], d["M"])]
    for col, value in ((0, np.nan), (3, np.inf), (8, -np.inf)):
        ll = d["ll"].clone()
        ll[5, 2, col] = value
        elpd, k, tail = (t.cpu().numpy() for t in eng.store_psis(ll, d["M"]))
        keep = [j for j in range(9) if j != col]
        assert np.isnan(elpd[col]) and np.isnan(k[col]) and tail[col] == -1
        for a, b in zip((elpd, k, tail), clean):
            assert np.array_equal(a[keep], b[keep])
    prec = d["prec"].clone()  # a precision that is not positive, through the mean route
    prec[0, 0, 4] = 0.0
    elpd, k, tail = (t.cpu().numpy() for t in eng.store_psis(d["mean"], d["M"], y=d["y"], prec=prec))
    assert np.isnan(elpd[4]) and np.isnan(k[4]) and tail[4] == -1 and np.array_equal(tail[:4], clean[2][:4])


def test_invalid_arguments(cases):
    import torch

    from openmcmc_amd._abi import INVALID_ARG, lib

    d = cases(16, 4)
    eng, S = d["eng"], d["S"]
    for bad in (0, S, -1):
        tm = np.full(9, d["M"])
        tm[4] = bad
        with pytest.raises(ValueError, match="tail_max"):
            eng.store_psis(d["ll"], tm)
    with pytest.raises(ValueError, match="index outside"):
        eng.store_psis(d["ll"], d["M"], index=[0, 9])
    with pytest.raises(ValueError, match="together"):
        eng.store_psis(d["mean"], d["M"], y=d["y"])
    # the library itself: outputs untouched
    out = eng.full((2, 9), -7.0)
    tm = torch.zeros(9, dtype=torch.int64, device=eng.device)
    st = lib.omc_store_psis(eng._ctx, 16, 9, d["ll"].data_ptr(), None, 9, None, None, 0, tm.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), None)
    torch.cuda.synchronize()
    assert st == INVALID_ARG and b"tail_max" in lib.omc_last_error() and bool((out == -7.0).all())
    for kw in (dict(ctx=None), dict(store=None), dict(tm=None), dict(n_idx=0), dict(n_idx=8), dict(size=0), dict(prec_size=2)):
        good = torch.full((9,), 3, dtype=torch.int64, device=eng.device)
        y = d["y"].data_ptr() if "prec_size" in kw else None
        pr = d["prec"].data_ptr() if "prec_size" in kw else None
        st = lib.omc_store_psis(kw.get("ctx", eng._ctx), 16, kw.get("size", 9), kw.get("store", d["ll"].data_ptr()), None, kw.get("n_idx", 9), y, pr,
                                kw.get("prec_size", 0), kw.get("tm", good.data_ptr()), out[0].data_ptr(), out[1].data_ptr(), None)
        torch.cuda.synchronize()
        assert st == INVALID_ARG and lib.omc_last_error() and bool((out == -7.0).all()), kw
