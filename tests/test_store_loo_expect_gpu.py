"""PSIS-LOO expectations of the device store (omc_store_loo_expect, Engine.store_loo_expect) against the numpy restatement
tests/loo_expect_model.py at np.longdouble, on the shapes of test_store_psis_gpu.py: nine columns per call that mix the regimes (k on
both sides of 0.7, tails of 4 draws or fewer, ties at the cut and inside the tail), one and several row slices, an odd row count.
The restatement runs on the pointwise log-likelihoods the device itself made (omc_store_loglik's ll_out), so both sort the same
numbers: tail and k must be np.array_equal to omc_store_psis, every fp64 result within 1e-10 of max(1, |value|) -- the project's fp64
parity tolerance; the CPU check (test_loo_expect_model_host.py) leaves more than three orders of room below it."""

import numpy as np
import pytest
from loo_expect_model import loo_expect, loo_inputs, normal_cdf
from psis_model import PSIS_SHAPES, logsumexp, tail_max_of

pytestmark = pytest.mark.gpu

FP = ("mean", "var", "below", "ess", "invprec")
ALL = FP + ("k", "tail")


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
    """per shape: the device inputs, the device's own ll and the restatement's answers on it, computed once"""
    made = {}

    def get(n_iter, C):
        if (n_iter, C) not in made:
            eng = engines(C)
            S = n_iter * C
            mu, y, tau, y_rep = loo_inputs(S)
            d = dict(eng=eng, S=S, n_iter=n_iter, C=C, M=tail_max_of(S), mu=mu, y_h=y, tau=tau, y_rep=y_rep,
                     thr_mu=np.median(mu, axis=0), mean=eng.to_device(mu.reshape(n_iter, C, 9)), y=eng.to_device(y),
                     prec=eng.to_device(tau.reshape(n_iter, C, 9)), rep=eng.to_device(y_rep.reshape(n_iter, C, 9)))
            d["ll"] = eng.store_loglik(d["mean"], d["y"], d["prec"], lse=False, mean=False, var=False, ll=True)[3]
            d["ll_h"] = d["ll"].cpu().numpy().reshape(S, 9)
            d["want_entry"] = loo_expect(d["ll_h"], d["M"], y_rep, y, tau, np.longdouble)
            d["want_mean"] = loo_expect(d["ll_h"], d["M"], mu, d["thr_mu"], tau, np.longdouble)
            d["want_cdf"] = loo_expect(d["ll_h"], d["M"], normal_cdf(mu, y, tau), None, tau, np.longdouble)
            made[(n_iter, C)] = d
        return made[(n_iter, C)]

    return get


def close(got, want):
    return np.abs(got - want) <= 1e-10 * np.maximum(1.0, np.abs(want))


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def entry(d, eng=None, ll=None, rep=None, **kw):
    """the ll-entry route with f the replicates: everything but invprec"""
    kw.setdefault("threshold", d["y_h"])
    kw.setdefault("want", ("mean", "var", "below", "ess", "k", "tail"))
    return host((eng or d["eng"]).store_loo_expect(d["ll"] if ll is None else ll, kw.pop("tail_max", d["M"]), f="entry",
                                                   values=d["rep"] if rep is None else rep, lw=True, **kw))


def same(a, b, names=None):
    return all(np.array_equal(a[n], b[n], equal_nan=True) for n in (names or a))


@pytest.mark.parametrize("n_iter,C", PSIS_SHAPES)
def test_against_the_restatement(cases, n_iter, C):
    d = cases(n_iter, C)
    eng, S = d["eng"], d["S"]
    _, k_p, t_p = (t.cpu().numpy() for t in eng.store_psis(d["ll"], d["M"]))
    got = entry(d)
    want = d["want_entry"]
    assert np.array_equal(got["tail"], t_p) and np.array_equal(got["k"], k_p) and np.array_equal(got["tail"], want["tail"])
    for name in ("mean", "var", "below", "ess"):
        print((n_iter, C), name, "worst error", np.max(np.abs(got[name] - want[name]) / np.maximum(1.0, np.abs(want[name]))))
        assert np.all(close(got[name], want[name])), name
    lw = got["lw"].reshape(S, 9)
    print((n_iter, C), "lw worst error", np.max(np.abs(lw - want["lw"])))
    assert np.all(close(lw, want["lw"]))
    assert np.all(np.abs(logsumexp(lw.astype(np.longdouble), axis=0)) <= 1e-10)
    top = np.nonzero(d["ll_h"][:, 8] == d["ll_h"][:, 8].min())[0]  # ties inside the tail: one weight
    assert top.size >= 3 and np.all(lw[top, 8] == lw[top[0], 8])
    # the mean entry with y and the precision (ll made on load): the same bits; f = the entry itself and the Normal cdf
    via_mean = host(eng.store_loo_expect(d["mean"], d["M"], y=d["y"], prec=d["prec"], f="entry", values=d["rep"], threshold=d["y_h"],
                                         want=("mean", "var", "below", "ess", "invprec", "k", "tail"), lw=True))
    assert same(got, via_mean)
    assert np.all(close(via_mean["invprec"], want["invprec"]))
    m = host(eng.store_loo_expect(d["mean"], d["M"], y=d["y"], prec=d["prec"], f="mean", threshold=d["thr_mu"], want=ALL))
    for name in FP:
        assert np.all(close(m[name], d["want_mean"][name])), name
    assert np.array_equal(m["k"], k_p) and np.array_equal(m["tail"], t_p) and np.array_equal(m["ess"], got["ess"])
    c = host(eng.store_loo_expect(d["mean"], d["M"], y=d["y"], prec=d["prec"], f="cdf", want=("mean", "var", "ess")))
    assert np.all(close(c["mean"], d["want_cdf"]["mean"])) and np.all(close(c["var"], d["want_cdf"]["var"]))
    assert np.all((c["mean"] >= 0) & (c["mean"] <= 1)) and np.array_equal(c["ess"], got["ess"])
    # a scalar precision (tau = 1: columns 0 .. 3 and 8 are as before), through an index
    one = d["prec"][:, :, :1].contiguous()
    sub = np.array([0, 2, 8, 3])
    s = host(eng.store_loo_expect(d["mean"], d["M"], index=sub, y=d["y"][sub], prec=one, f="entry", values=d["rep"], values_index=sub,
                                  threshold=d["y_h"][sub], want=("mean", "var", "below", "ess", "invprec", "k", "tail"), lw=True))
    for name in s:
        assert np.array_equal(s[name], via_mean[name][..., sub]), name
    # a subset of the outputs holds the bits of the whole set, and the same call twice
    part = host(eng.store_loo_expect(d["ll"], d["M"], f="entry", values=d["rep"], want=("ess",)))
    assert np.array_equal(part["ess"], got["ess"])
    only = host(eng.store_loo_expect(d["ll"], d["M"], f="entry", values=d["rep"], want=(), lw=True))
    assert np.array_equal(only["lw"], got["lw"])
    assert same(got, entry(d))


@pytest.mark.parametrize("n_iter,C", PSIS_SHAPES)
def test_selections_and_load_forms(cases, n_iter, C):
    d = cases(n_iter, C)
    eng, S = d["eng"], d["S"]
    base = entry(d)
    # unsorted with a repeat, per-column tail lengths
    idx = np.array([8, 1, 1, 3, 0])
    tm = np.array([d["M"], max(1, d["M"] - 1), d["M"], 1, S - 1])
    want = loo_expect(d["ll_h"][:, idx], tm, d["y_rep"][:, idx], d["y_h"][idx], None, np.longdouble)
    got = entry(d, index=idx, values_index=idx, threshold=d["y_h"][idx], tail_max=tm)
    _, k_p, t_p = (t.cpu().numpy() for t in eng.store_psis(d["ll"], tm, index=idx))
    assert np.array_equal(got["tail"], want["tail"]) and np.array_equal(got["tail"], t_p) and np.array_equal(got["k"], k_p)
    for name in ("mean", "var", "below", "ess"):
        assert np.all(close(got[name], want[name])), name
    assert np.all(close(got["lw"].reshape(S, 5), want["lw"]))
    # 33 columns and 1 column: the workgroup's column edge; a column's bits do not depend on its place in the selection
    for idx in (np.arange(33) % 9, np.array([4])):
        got = entry(d, index=idx, values_index=idx, threshold=d["y_h"][idx])
        for name in got:
            assert np.array_equal(got[name], base[name][..., idx]), (name, len(idx))
    # an even size without an index takes 16-byte loads, the 9-wide store through an index 8-byte loads: the same bits
    even = np.arange(8)
    ll8, rep8 = d["ll"][:, :, :8].contiguous(), d["rep"][:, :, :8].contiguous()
    assert ll8.data_ptr() % 16 == 0 and rep8.data_ptr() % 16 == 0
    wide = entry(d, ll=ll8, rep=rep8, threshold=d["y_h"][:8])
    narrow = entry(d, index=even, values_index=even, threshold=d["y_h"][:8])
    for name in wide:
        assert np.array_equal(wide[name], narrow[name]) and np.array_equal(wide[name], base[name][..., :8]), name
    mean8, prec8 = d["mean"][:, :, :8].contiguous(), d["prec"][:, :, :8].contiguous()
    kw = dict(y=d["y"][:8], prec=prec8, f="mean", threshold=d["thr_mu"][:8], want=ALL, lw=True)
    wide, narrow = host(eng.store_loo_expect(mean8, d["M"], **kw)), host(eng.store_loo_expect(mean8, d["M"], index=even, **kw))
    assert same(wide, narrow)
    for name in FP:
        assert np.all(close(wide[name], d["want_mean"][name][:8])), name


@pytest.mark.parametrize("n_iter,C", [(125, 8), (4099, 1)])
def test_sort_options_give_the_same_bits(cases, n_iter, C):
    from openmcmc_amd.engine import Engine

    d = cases(n_iter, C)
    base = entry(d)
    eng = Engine(C)
    try:
        eng.set_option("rank_tile", 64)
        eng.set_option("rank_chunk", 1)
        assert same(base, entry(d, eng=eng))
    finally:
        eng.close()


@pytest.mark.parametrize("n_iter,C", PSIS_SHAPES)
def test_permuted_rows(cases, n_iter, C):
    """the draws regrouped over iterations and chains: the weight of a draw depends on its value alone"""
    import torch

    d = cases(n_iter, C)
    S = d["S"]
    perm = np.random.default_rng(S).permutation(S)
    pt = torch.as_tensor(perm, device=d["ll"].device)
    ll = d["ll"].reshape(S, 9)[pt].reshape(n_iter, C, 9).contiguous()
    rep = d["rep"].reshape(S, 9)[pt].reshape(n_iter, C, 9).contiguous()
    base, got = entry(d), entry(d, ll=ll, rep=rep)
    assert np.array_equal(got["tail"], base["tail"]) and np.array_equal(got["k"], base["k"])
    for name in ("mean", "var", "below", "ess"):
        assert np.all(close(got[name], base[name])), name
    a, b = base["lw"].reshape(S, 9), got["lw"].reshape(S, 9)
    assert np.all(close(b, a[perm]))
    top = np.nonzero(d["ll_h"][:, 8] == d["ll_h"][:, 8].min())[0]
    moved = np.nonzero(np.isin(perm, top))[0]
    assert moved.size == top.size and np.all(b[moved, 8] == a[top[0], 8])


def test_non_finite_columns(cases):
    d = cases(16, 4)
    clean = entry(d)
    for col, value in ((0, np.nan), (3, np.inf), (8, -np.inf)):
        ll = d["ll"].clone()
        ll[5, 2, col] = value
        got = entry(d, ll=ll)
        keep = [j for j in range(9) if j != col]
        assert all(np.isnan(got[n][col]) for n in ("mean", "var", "below", "ess", "k")) and got["tail"][col] == -1
        assert np.all(np.isnan(got["lw"][:, :, col]))
        for name in got:
            assert np.array_equal(got[name][..., keep], clean[name][..., keep]), name
    prec = d["prec"].clone()  # a precision that is not positive, through the mean route
    prec[0, 0, 4] = 0.0
    got = host(d["eng"].store_loo_expect(d["mean"], d["M"], y=d["y"], prec=prec, f="mean", want=("mean", "invprec", "tail")))
    assert np.isnan(got["mean"][4]) and np.isnan(got["invprec"][4]) and got["tail"][4] == -1
    assert np.array_equal(got["tail"][:4], clean["tail"][:4])
    rep = d["rep"].clone()  # an f that is not finite: the mean, and nothing of the weights
    rep[3, 1, 2] = np.nan
    got = entry(d, rep=rep)
    assert np.isnan(got["mean"][2]) and np.isnan(got["var"][2])
    keep = [j for j in range(9) if j != 2]
    for name in got:
        cols = keep if name in ("mean", "var", "below") else slice(None)  # (a NaN f counts as not below)
        assert np.array_equal(got[name][..., cols], clean[name][..., cols]), name


def test_invalid_arguments(cases):
    import torch

    from openmcmc_amd._abi import INVALID_ARG, lib

    d = cases(16, 4)
    eng, S = d["eng"], d["S"]
    for bad in (0, S, -1):
        tm = np.full(9, d["M"])
        tm[4] = bad
        with pytest.raises(ValueError, match="tail_max"):
            eng.store_loo_expect(d["ll"], tm, f="entry", values=d["rep"])
    with pytest.raises(ValueError, match="index outside"):
        eng.store_loo_expect(d["ll"], d["M"], index=[0, 9], f="entry", values=d["rep"], values_index=[0, 1])
    with pytest.raises(ValueError, match="vidx outside"):
        eng.store_loo_expect(d["ll"], d["M"], index=[0, 1], f="entry", values=d["rep"], values_index=[0, 9])
    with pytest.raises(ValueError, match="together"):
        eng.store_loo_expect(d["mean"], d["M"], y=d["y"], f="mean")
    with pytest.raises(ValueError, match="need y"):
        eng.store_loo_expect(d["ll"], d["M"], f="cdf")
    # the library itself: every output untouched
    out = eng.full((6, 9), -7.0)
    tail = torch.full((9,), -7, dtype=torch.int64, device=eng.device)
    lw = eng.full((16, 4, 9), -7.0)
    good = torch.full((9,), 3, dtype=torch.int64, device=eng.device)
    zero = torch.zeros(9, dtype=torch.int64, device=eng.device)
    far = torch.full((9,), 9, dtype=torch.int64, device=eng.device)
    near = torch.arange(9, dtype=torch.int64, device=eng.device)
    ll, mean, y, prec, rep, thr = (t.data_ptr() for t in (d["ll"], d["mean"], d["y"], d["prec"], d["rep"], d["y"]))
    ok = dict(ctx=eng._ctx, n_iter=16, size=9, store=ll, idx=None, n_idx=9, y=None, prec=None, prec_size=0, tm=good.data_ptr(), f=0,
              values=rep, vsize=9, vidx=None, thr=thr, outs=True)
    cases_bad = [dict(ctx=None), dict(store=None), dict(tm=None), dict(n_idx=0), dict(n_idx=8), dict(size=0), dict(n_iter=0),
                 dict(store=mean, y=y), dict(store=mean, prec=prec), dict(store=mean, y=y, prec=prec, prec_size=2),
                 dict(tm=zero.data_ptr()), dict(idx=far.data_ptr()), dict(f=3), dict(f=-1), dict(values=None), dict(vsize=0),
                 dict(vsize=8), dict(f=1), dict(f=2), dict(invprec=True), dict(thr=None), dict(below=False),
                 dict(idx=near.data_ptr(), vidx=far.data_ptr()), dict(outs=False)]
    for kw in cases_bad:
        a = dict(ok, **kw)
        o = [out[i].data_ptr() for i in range(6)] + [tail.data_ptr(), lw.data_ptr()]
        o[4] = o[4] if a.get("invprec") else None
        o[2] = o[2] if a.get("below", True) else None
        if not a["outs"]:
            o, a["thr"] = [None] * 8, None
        st = lib.omc_store_loo_expect(a["ctx"], a["n_iter"], a["size"], a["store"], a["idx"], a["n_idx"], a["y"], a["prec"], a["prec_size"],
                                      a["tm"], a["f"], a["values"], a["vsize"], a["vidx"], a["thr"], *o)
        torch.cuda.synchronize()
        assert st == INVALID_ARG and lib.omc_last_error(), kw
        assert bool((out == -7.0).all()) and bool((tail == -7).all()) and bool((lw == -7.0).all()), kw
    # and the same arguments without a fault are taken
    o = [out[i].data_ptr() for i in range(6)] + [tail.data_ptr(), lw.data_ptr()]
    o[4] = None
    a = ok
    st = lib.omc_store_loo_expect(a["ctx"], a["n_iter"], a["size"], a["store"], a["idx"], a["n_idx"], a["y"], a["prec"], a["prec_size"],
                                  a["tm"], a["f"], a["values"], a["vsize"], a["vidx"], a["thr"], *o)
    torch.cuda.synchronize()
    assert st == 0 and bool((out[:4] != -7.0).all()) and bool((out[4] == -7.0).all()) and bool((tail != -7).all())
