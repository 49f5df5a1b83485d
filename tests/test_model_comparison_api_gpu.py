"""MCMC.log_likelihood, MCMC.waic and MCMC.loo on two small runs: a random-walk smoother whose mean is the stored parameter itself
(40 nodes, 4 chains, 12 stored iterations) and the regression of tests/test_project_api_gpu.py whose mean is a LinearCombination
and whose precision is stored (12 observations, 6 chains, 9 stored iterations).  The device results are held to the numpy
restatement (tests/psis_model.py, np.longdouble) applied to the pointwise log-likelihood computed on the host from collect(),
within the project's fp64 parity tolerance 1e-10 of max(1, |value|)."""

import numpy as np
import pytest
from psis_model import HALF_LOG_2PI, column_summaries, loglik, psis, tail_max_of
from scipy import sparse
from test_project_api_gpu import C, N, N_ITER, P, build

pytestmark = pytest.mark.gpu

NS, CS, ITS = 40, 4, 12  # the smoother: nodes, chains, stored iterations
U = 2.0 ** -53


def build_smoother():
    from openmcmc_amd.distribution.distribution import Gamma
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.mcmc import MCMC
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import ScaledMatrix
    from openmcmc_amd.sampler.sampler import NormalGamma, NormalNormal

    rng = np.random.default_rng(9)
    t = np.linspace(0, 1, NS)
    y = np.sin(2 * np.pi * t) + 0.2 * rng.standard_normal(NS)
    y[7] += 2.0  # an outlier: a heavy importance tail
    D = sparse.diags([-np.ones(NS - 1), np.ones(NS - 1)], offsets=[0, 1], shape=(NS - 1, NS))
    Pm = (D.T @ D + 1e-3 * sparse.identity(NS)).tocsc()
    mdl = Model([Normal("y", mean="b", precision=ScaledMatrix(matrix="P_tau", scalar="tau")),
                 Normal("b", mean="mu", precision=ScaledMatrix(matrix="P_lambda", scalar="lambda")),
                 Gamma("lambda", shape="a_lam", rate="b_lam"), Gamma("tau", shape="a_tau", rate="b_tau")])
    state = {"y": y, "b": y, "mu": np.zeros(NS), "lambda": 10, "P_lambda": Pm, "a_lam": 1, "b_lam": 0.1, "tau": 1,
             "P_tau": sparse.csc_matrix(np.eye(NS)), "a_tau": 1, "b_tau": 1}
    samplers = [NormalNormal("b", mdl), NormalGamma("lambda", mdl), NormalGamma("tau", mdl)]
    return MCMC(state, samplers, model=mdl, n_burn=5, n_iter=ITS, n_chains=CS, seed=3), y


@pytest.fixture(scope="module")
def smoother():
    M, y = build_smoother()
    M.run_mcmc()
    yield M, y
    M.engine.close()


@pytest.fixture(scope="module")
def regression():
    M, X = build()
    M.run_mcmc()
    yield M, X
    M.engine.close()


def host_ll(M, mean_of, y):
    """(S, m) from collect(): entries (C, size, n_iter) -> rows (n_iter, C)"""
    host = M.collect()
    rows = lambda key: np.moveaxis(host[key], -1, 0).reshape(-1, host[key].shape[1])
    return loglik(mean_of(rows), np.asarray(y, dtype=np.float64).reshape(-1), rows("tau"), np.longdouble)


def close(got, want):
    return np.all(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) <= 1e-10 * np.maximum(1.0, np.abs(np.asarray(want, dtype=np.float64))))


def check_against_host(M, ll, m):
    S = ll.shape[0]
    got_ll = M.log_likelihood("y")
    assert got_ll.shape == (S // M.n_chains, M.n_chains, m) and close(got_ll.reshape(S, m), ll)
    lse, _, var = column_summaries(ll)
    lppd_i = lse - np.log(np.longdouble(S))
    elpd_i = lppd_i - var
    w = M.waic("y", pointwise=True)
    assert close(w["elpd_i"], elpd_i) and close(w["p_i"], var) and close(w["lppd_i"], lppd_i)
    assert close(w["elpd_waic"], elpd_i.sum()) and close(w["p_waic"], var.sum()) and close(w["lppd"], lppd_i.sum())
    assert close(w["se"], np.sqrt(m * np.var(elpd_i.astype(np.float64)))) and w["n_high_var"] == int(np.sum(var > 0.4))
    assert set(M.waic("y")) == {"elpd_waic", "se", "p_waic", "lppd", "n_high_var"}
    for reff in (1.0, np.linspace(0.3, 1.0, m)):
        tm = np.array([tail_max_of(S, r) for r in np.broadcast_to(reff, (m,))])
        e_w, k_w, t_w, margin = psis(ll, tm, np.longdouble)
        assert margin.min() >= 1e-6
        lo = M.loo("y", pointwise=True, reff=reff)
        print("pareto_k", lo["pareto_k"], "tail", lo["tail"])
        assert np.array_equal(lo["tail"], t_w) and close(lo["elpd_i"], e_w) and close(lo["pareto_k"], k_w)
        assert close(lo["elpd_loo"], e_w.sum()) and close(lo["p_loo"], float(lppd_i.sum()) - e_w.sum())
        assert close(lo["se"], np.sqrt(m * np.var(e_w))) and lo["n_bad_k"] == int(np.sum(k_w > 0.7))
        assert lo["pareto_k"].shape == (m,)
    assert set(M.loo("y")) == {"elpd_loo", "se", "p_loo", "pareto_k", "n_bad_k", "tail"}
    return got_ll


def test_smoother_with_an_identity_mean(smoother):
    M, y = smoother
    ll = host_ll(M, lambda rows: rows("b"), y)
    before = set(M.store)
    check_against_host(M, ll, NS)
    assert set(M.store) == before  # an Identity mean reads the store directly: no work entry


def test_regression_with_a_linear_combination_mean(regression):
    M, X = regression
    ll = host_ll(M, lambda rows: rows("beta") @ X.T, M.state["y"])
    check_against_host(M, ll, N)


def test_named_log_likelihood_is_a_key_of_the_summaries(regression):
    M, X = regression
    assert M.log_likelihood("y", name="ll") is None
    t = M.store["ll"]
    assert tuple(t.shape) == (N_ITER, C, N) and "ll" in M._derived
    assert np.array_equal(t.cpu().numpy(), M.log_likelihood("y"))
    mean, var = M.summary("ll")
    assert np.allclose(mean, t.cpu().numpy().reshape(-1, N).mean(axis=0), rtol=1e-12)
    assert M.quantiles("ll", [0.1, 0.9]).shape == (2, N)
    # PSIS over the stored entry: the same bits as loo over the mean
    e, k, tail = M.engine.store_psis(t, tail_max_of(N_ITER * C))
    lo = M.loo("y", pointwise=True)
    assert np.array_equal(e.cpu().numpy(), lo["elpd_i"]) and np.array_equal(k.cpu().numpy(), lo["pareto_k"])
    assert M.collect()["ll"].shape == (C, N, N_ITER)
    with pytest.raises(ValueError, match="store entry of the run"):
        M.log_likelihood("y", name="beta")


def test_two_observation_chunkings_agree_within_the_bound_of_project(regression):
    M, X = regression
    whole = M.log_likelihood("y")
    w1, l1 = M.waic("y", pointwise=True), M.loo("y", pointwise=True)
    M.pointwise_work_bytes = 8 * N_ITER * C * 5  # five observations per chunk: 5 + 5 + 2
    try:
        parts = M.log_likelihood("y")
        w2, l2 = M.waic("y", pointwise=True), M.loo("y", pointwise=True)
    finally:
        del M.pointwise_work_bytes
    host = M.collect()
    beta = np.moveaxis(host["beta"], -1, 0).reshape(-1, P)
    tau = np.moveaxis(host["tau"], -1, 0).reshape(-1, 1)
    db = 2 * (P + 2) * U * (np.abs(beta) @ np.abs(X.T))  # two results within project's bound of the exact mean
    r = np.abs(M.state["y"].reshape(1, -1) - beta @ X.T) + db
    E = np.abs(0.5 * np.log(tau)) + HALF_LOG_2PI + 0.5 * tau * r * r
    assert np.all(np.abs(whole - parts).reshape(-1, N) <= tau * r * db + 8 * U * E)
    assert close(w2["elpd_i"], w1["elpd_i"]) and close(l2["elpd_i"], l1["elpd_i"]) and close(l2["pareto_k"], l1["pareto_k"])
    assert np.array_equal(l2["tail"], l1["tail"])


def test_posterior_predictive_is_unchanged(regression):
    M, X = regression
    assert np.array_equal(M.posterior_predictive("y", noise=False), M.project("beta", X))
    assert np.array_equal(M.posterior_predictive("y", replicate=2), M.project("beta", X, noise_precision="tau", replicate=2))


def test_unsupported_model_parts_are_named():
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.parameter import Identity, LinearCombination, LinearCombinationWithTransform, ScaledMatrix

    M, X = build(extra_state={"P_full": np.eye(N) + 0.1, "gamma": np.zeros(3), "Z": np.zeros((N, 3))})
    try:
        M.run_mcmc()
        eng = M.engine
        y = M.model["y"]
        y_host = M.state["y"]
        for call in (M.log_likelihood, M.waic, M.loo):
            what = call.__name__
            with pytest.raises(NotImplementedError, match=f"{what}: a response of type Gamma"):
                call("tau")
            y.mean = LinearCombinationWithTransform(form={"beta": "X"}, transform={"beta": False})
            with pytest.raises(NotImplementedError, match=f"{what}: a mean of type LinearCombinationWithTransform"):
                call("y")
            y.mean = LinearCombination(form={"beta": "X", "gamma": "Z"})
            with pytest.raises(NotImplementedError, match=f"{what}: the term 'gamma' is not in the store"):
                call("y")
            y.mean = Identity("mu")
            with pytest.raises(NotImplementedError, match=f"{what}: the mean 'mu' is not in the store"):
                call("y")
            y.mean = LinearCombination(form={"beta": "X"})
            M.state["X"] = ChainArray(eng.zeros(C, N, P))
            with pytest.raises(NotImplementedError, match=f"{what}: the design matrix 'X' is per chain"):
                call("y")
            M.state["X"] = X
            y.precision = ScaledMatrix(matrix="P_full", scalar="tau")
            with pytest.raises(NotImplementedError, match=f"{what}: the precision matrix 'P_full' is not diagonal"):
                call("y")
            y.precision = Identity("P_full")
            with pytest.raises(NotImplementedError, match=f"{what}: the precision 'P_full' is a matrix"):
                call("y")
            y.precision = ScaledMatrix(matrix="P_tau", scalar="tau")
            M.state["y"] = ChainArray(eng.zeros(C, N))
            with pytest.raises(NotImplementedError, match=f"{what}: the response 'y' is per chain"):
                call("y")
            M.state["y"] = np.zeros((N, 2))
            with pytest.raises(NotImplementedError, match=f"{what}: the response 'y' is replicated"):
                call("y")
            M.state["y"] = y_host
        assert M.log_likelihood("y").shape == (N_ITER, C, N)  # the supported form still runs after the round trip
    finally:
        M.engine.close()


def test_store_ring_guard():
    M, X = build(store_ring=4)
    try:
        M.run_mcmc()
        for call in (M.log_likelihood, M.waic, M.loo):
            with pytest.raises(ValueError, match="store_ring"):
                call("y")
    finally:
        M.engine.close()
