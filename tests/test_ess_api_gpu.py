"""MCMC.ess, MCMC.mcse and MCMC.summarize on a small stored run (a regression: 4 coefficients and a precision, 6 chains, 50 stored
iterations): every method and every MCSE held to the restatement of tests/essq_model.py, fed with the run's own store, within the
project's fp64 parity tolerance 1e-10; summarize's columns array_equal to the separate calls; the ring-store refusal."""

import numpy as np
import pytest
from essq_model import ess_sd_fp64, indicator_exact, mcse_quantile, mcse_sd, rhat_ess_fp64, split_series
from scipy import sparse

pytestmark = pytest.mark.gpu

N, P, C, N_ITER = 30, 4, 6, 50


def build_regression(**mcmc_kw):
    from openmcmc_amd.distribution.distribution import Gamma
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.mcmc import MCMC
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombination, ScaledMatrix
    from openmcmc_amd.sampler.sampler import NormalGamma, NormalNormal

    rng = np.random.default_rng(42)
    X = rng.standard_normal((N, P))
    y = X @ np.arange(1.0, P + 1) + 0.3 * rng.standard_normal(N)
    mdl = Model([Normal("y", mean=LinearCombination(form={"beta": "X"}), precision=ScaledMatrix(matrix="P_tau", scalar="tau")),
                 Normal("beta", mean="mu", precision=ScaledMatrix(matrix="P_lambda", scalar="lambda")),
                 Gamma("tau", shape="a_tau", rate="b_tau")], response={"y": "mean"})
    samplers = [NormalNormal("beta", mdl), NormalGamma("tau", mdl)]
    state = {"y": y, "X": X, "beta": [0.0] * P, "P_tau": sparse.csc_matrix(np.eye(N)), "tau": 1, "P_lambda": sparse.csc_matrix(np.eye(P)),
             "mu": [0.0] * P, "lambda": 0.01, "a_tau": 1e-3, "b_tau": 1e-3}
    return MCMC(state, samplers, model=mdl, n_burn=3, n_iter=N_ITER, n_chains=C, seed=5, **mcmc_kw)


@pytest.fixture(scope="module")
def run():
    M = build_regression()
    M.run_mcmc()
    yield M, M._store_3d("beta").cpu().numpy(), M._store_3d("tau").cpu().numpy()
    M.engine.close()


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= 1e-10 * np.maximum(1.0, np.abs(want))))


def exact(x, cols, lo, hi):
    """ess (n_cols,) of the indicator by the exact model; every decision of these inputs must be clear of zero"""
    r = [indicator_exact(split_series(x[:, :, k]), lo, hi) for k in cols]
    assert min(v["margin"] for v in r) > 1e-9
    return np.array([v["ess"] for v in r])


def test_ess_methods(run):
    M, beta, tau = run
    cols = np.arange(P)
    rank = M.rank_diagnostics("beta")
    assert np.array_equal(M.ess("beta"), rank["ess_bulk"]) and np.array_equal(M.ess("beta", method="tail"), rank["ess_tail"])
    assert close(M.ess("beta", method="mean"), [rhat_ess_fp64(split_series(beta[:, :, k]))[0] for k in cols])
    assert np.array_equal(M.ess("beta", method="mean"), M.diagnostics("beta")["ess"])
    assert close(M.ess("beta", method="sd"), [ess_sd_fp64(beta[:, :, k]) for k in cols])
    # quantile: a number, a sequence, the median; an index with a repeat; a 2-D entry counts as one element
    assert close(M.ess("beta", method="quantile", prob=0.1), exact(beta, cols, -1.0, 0.1))
    probs = np.linspace(0.05, 0.95, 20)  # the profile of az.plot_ess(kind="quantile")
    got = M.ess("beta", method="quantile", prob=probs)
    assert got.shape == (20, P) and close(got, [exact(beta, cols, -1.0, p) for p in probs])
    assert close(M.ess("beta", method="median"), exact(beta, cols, -1.0, 0.5))
    back = np.array([3, 0, 3, 1])
    assert close(M.ess("beta", method="quantile", prob=[0.9], index=back), [exact(beta, back, -1.0, 0.9)])
    for method in ("mean", "sd", "tail"):
        assert np.array_equal(M.ess("beta", method=method, index=back), M.ess("beta", method=method)[back])
    assert close(M.ess("tau", method="median"), exact(tau, [0], -1.0, 0.5))
    assert close(M.ess("tau", method="sd"), [ess_sd_fp64(tau[:, :, 0])])
    # local: a pair, a sequence of pairs (the profile of az.plot_ess(kind="local"))
    assert close(M.ess("beta", method="local", prob=(0.2, 0.4)), exact(beta, cols, 0.2, 0.4))
    edges = np.linspace(0, 1, 21)
    pairs = np.stack([edges[:-1], edges[1:]], axis=1)
    got = M.ess("beta", method="local", prob=pairs)
    assert got.shape == (20, P) and close(got, [exact(beta, cols, a, b) for a, b in pairs])
    # more than 32 intervals go in groups
    many = np.linspace(0.02, 0.98, 40)
    assert np.array_equal(M.ess("beta", method="quantile", prob=many)[35], M.ess("beta", method="quantile", prob=many[35]))
    for bad in (dict(method="quantile"), dict(method="quantile", prob=1.5), dict(method="local", prob=0.5),
                dict(method="local", prob=(0.6, 0.4)), dict(method="other"), dict(method="mean", index=[0, P])):
        with pytest.raises(ValueError):
            M.ess("beta", **bad)


def test_mcse_methods(run):
    M, beta, tau = run
    cols = np.arange(P)
    sd = np.array([np.std(beta[:, :, k], ddof=1) for k in cols])
    ess_mean = np.array([rhat_ess_fp64(split_series(beta[:, :, k]))[0] for k in cols])
    assert close(M.mcse("beta"), sd / np.sqrt(ess_mean))
    assert close(M.mcse("beta"), M.diagnostics("beta")["mcse_mean"])
    assert close(M.mcse("beta", method="sd"), mcse_sd(sd, np.array([ess_sd_fp64(beta[:, :, k]) for k in cols])))
    for p in (0.05, 0.5, 0.9):
        want = [mcse_quantile(split_series(beta[:, :, k]), exact(beta, [k], -1.0, p)[0], p) for k in cols]
        assert close(M.mcse("beta", method="quantile", prob=p), want)
    got = M.mcse("beta", method="quantile", prob=[0.05, 0.9], index=[2, 2, 0])
    assert got.shape == (2, 3) and np.array_equal(got[0], M.mcse("beta", method="quantile", prob=0.05)[[2, 2, 0]])
    assert np.array_equal(M.mcse("beta", method="median"), M.mcse("beta", method="quantile", prob=0.5))
    assert close(M.mcse("tau", method="median"), [mcse_quantile(split_series(tau[:, :, 0]), exact(tau, [0], -1.0, 0.5)[0], 0.5)])
    with pytest.raises(ValueError):
        M.mcse("beta", method="local", prob=(0.1, 0.2))


def test_summarize_is_the_separate_calls(run):
    M, beta, _ = run
    for index in (None, [2, 0, 2]):
        s = M.summarize("beta", index=index)
        assert list(s) == ["mean", "sd", "hdi_lo", "hdi_hi", "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat"]
        n = P if index is None else 3
        assert all(v.shape == (n,) for v in s.values())
        cols = np.arange(P) if index is None else np.array(index)
        assert close(s["mean"], beta[:, :, cols].mean(axis=(0, 1))) and close(s["sd"], beta[:, :, cols].std(axis=(0, 1), ddof=1))
        hdi, rank = M.hdi("beta", prob=0.94, index=index), M.rank_diagnostics("beta", index=index)
        assert np.array_equal(s["hdi_lo"], hdi[:, 0]) and np.array_equal(s["hdi_hi"], hdi[:, 1])
        assert np.array_equal(s["mcse_mean"], M.mcse("beta", index=index)) and np.array_equal(s["mcse_sd"], M.mcse("beta", method="sd", index=index))
        assert np.array_equal(s["ess_bulk"], M.ess("beta", index=index)) and np.array_equal(s["ess_tail"], M.ess("beta", method="tail", index=index))
        assert np.array_equal(s["r_hat"], rank["rhat"])
    assert np.array_equal(M.summarize("beta", hdi_prob=0.5)["hdi_lo"], M.hdi("beta", prob=0.5)[:, 0])


def test_store_ring_guard():
    M = build_regression(store_ring=4)
    try:
        M.run_mcmc()
        for call in (M.ess, M.mcse, M.summarize):
            with pytest.raises(ValueError, match="store_ring"):
                call("beta")
    finally:
        M.engine.close()
