"""The numpy restatement of omc_store_loo_expect (tests/loo_expect_model.py) against itself and against what is already trusted
(tests/psis_model.py), on the CPU.  Its fp64 run must stay within the cap of its own np.longdouble run: 1e-10 * max(1, |value|), the
project's parity tolerance of test_store_psis_gpu.py -- a condition on the inputs, which leave more than three orders of room (the
worst gap over mean, var, below and ess for S = 5 .. 20000 is 3.8e-14).  Three identities tie it to the PSIS restatement."""

import numpy as np
import pytest
from loo_expect_model import draw_weights, loo_expect, loo_inputs, smoothed_column
from psis_model import PSIS_S_HOST, loglik, logsumexp, psis, psis_column, tail_max_of

F_KINDS = ["mean", "replicates", "likelihood"]


def close(got, want):
    return np.abs(got - want) <= 1e-10 * np.maximum(1.0, np.abs(want))


@pytest.fixture(scope="module")
def columns():
    made = {}

    def get(S):
        if S not in made:
            mu, y, tau, y_rep = loo_inputs(S)
            ll = loglik(mu, y, tau)
            made[S] = dict(mu=mu, y=y, tau=tau, y_rep=y_rep, ll=ll, M=tail_max_of(S),
                           f={"mean": mu, "replicates": y_rep, "likelihood": np.exp(ll)})
        return made[S]

    return get


@pytest.mark.parametrize("S", PSIS_S_HOST)
def test_the_fit_is_psis_models(columns, S):
    d = columns(S)
    _, k_w, t_w, _ = psis(d["ll"], d["M"])
    for j in range(9):
        _, _, k, T, smooth = smoothed_column(d["ll"][:, j], d["M"])
        assert T == t_w[j] and (k == k_w[j] or (np.isinf(k) and np.isinf(k_w[j]))) and smooth == bool(np.isfinite(k_w[j]))


@pytest.mark.parametrize("kind", F_KINDS)
@pytest.mark.parametrize("S", PSIS_S_HOST)
def test_fp64_within_the_cap_of_longdouble(columns, S, kind):
    d = columns(S)
    f = d["f"][kind]
    thr = d["y"] if kind == "replicates" else np.median(f, axis=0)
    got = loo_expect(d["ll"], d["M"], f, thr, d["tau"])
    want = loo_expect(d["ll"], d["M"], f, thr, d["tau"], np.longdouble)
    assert np.array_equal(got["tail"], want["tail"])
    for name in ("mean", "var", "below", "ess", "invprec"):
        gap = np.abs(got[name] - want[name]) / np.maximum(1.0, np.abs(want[name]))
        print(S, kind, name, "worst gap", gap.max())
        assert np.all(close(got[name], want[name])), name
    assert np.all(close(got["lw"], want["lw"]))
    assert np.all(np.abs(logsumexp(want["lw"].astype(np.longdouble), axis=0)) <= 1e-10)
    if kind == "likelihood":  # E_loo[p(y_i | draw)] is the elpd PSIS-LOO reports
        for j in range(9):
            elpd = float(psis_column(d["ll"][:, j], d["M"], np.longdouble)[0])
            assert close(np.log(want["mean"][j]), elpd), (j, np.log(want["mean"][j]), elpd)


@pytest.mark.parametrize("S", PSIS_S_HOST)
def test_constant_f_and_ties(columns, S):
    d = columns(S)
    for dtype in (np.float64, np.longdouble):
        got = loo_expect(d["ll"], d["M"], np.full(d["ll"].shape, 2.5), np.array([2.5] * 5 + [2.0] * 4), None, dtype)
        assert np.all(np.abs(got["mean"] - 2.5) <= 1e-15) and np.all(np.abs(got["var"]) <= 1e-28)
        assert np.all(np.abs(got["below"][:5] - 1.0) <= 1e-15) and np.all(got["below"][5:] == 0.0)
    # the three largest -ll of column 8 are tied: one weight, the mean of their positions' weights
    w, lw, _, T = draw_weights(d["ll"][:, 8], d["M"], np.longdouble)
    top = np.nonzero(d["ll"][:, 8] == d["ll"][:, 8].min())[0]
    assert top.size >= 3 and np.all(w[top] == w[top[0]]) and np.all(lw[top] == lw[top[0]])
    if T > 4:
        _, xs, _, _, _ = smoothed_column(d["ll"][:, 8], d["M"], np.longdouble)
        assert abs(w[top[0]] - np.exp(xs[S - top.size:]).mean()) <= 1e-17


@pytest.mark.parametrize("S", PSIS_S_HOST)
def test_short_tails_are_plain_importance_sampling(columns, S):
    d = columns(S)
    tm = min(4, S - 1)  # T <= 4: nothing is smoothed
    got = loo_expect(d["ll"], tm, d["y_rep"], d["y"], d["tau"], np.longdouble)
    assert np.all(got["tail"] <= 4) and np.all(np.isinf(got["k"]))
    ll = d["ll"].astype(np.longdouble)
    w = np.exp(-ll - np.max(-ll, axis=0))
    w = w / w.sum(axis=0)
    f = d["y_rep"].astype(np.longdouble)
    mean = (w * f).sum(axis=0)
    assert np.all(close(got["mean"], mean.astype(np.float64)))
    assert np.all(close(got["var"], (w * (f - mean) ** 2).sum(axis=0).astype(np.float64)))
    assert np.all(close(got["below"], np.where(f <= d["y"], w, 0).sum(axis=0).astype(np.float64)))
    assert np.all(close(got["ess"], (1 / (w * w).sum(axis=0)).astype(np.float64)))
    assert np.all(close(got["lw"], np.log(w).astype(np.float64)))
