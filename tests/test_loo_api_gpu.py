"""MCMC.loo_predictive, MCMC.loo_pit, MCMC.loo_expectation and MCMC.loo_weights on two small runs: a random-walk smoother whose mean
is the stored parameter itself (40 nodes, 4 chains, 60 stored iterations) and a regression whose mean is a LinearCombination and
whose precision is stored (30 observations, 6 chains, 50 stored iterations).  The device results are held to the numpy restatement
(tests/loo_expect_model.py, np.longdouble) fed with log_likelihood() and posterior_predictive() of the same run, within the
project's fp64 parity tolerance 1e-10 of max(1, |value|)."""

import numpy as np
import pytest
from loo_expect_model import loo_expect, normal_cdf
from psis_model import logsumexp, tail_max_of
from scipy import sparse

pytestmark = pytest.mark.gpu

NS, CS, ITS = 40, 4, 60   # the smoother: nodes, chains, stored iterations
N, P, C, N_ITER = 30, 4, 6, 50  # the regression: observations, coefficients, chains, stored iterations


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
    return MCMC(state, samplers, model=mdl, n_burn=5, n_iter=ITS, n_chains=CS, seed=3)


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
    y[3] += 1.5  # an outlier
    mdl = Model([Normal("y", mean=LinearCombination(form={"beta": "X"}), precision=ScaledMatrix(matrix="P_tau", scalar="tau")),
                 Normal("beta", mean="mu", precision=ScaledMatrix(matrix="P_lambda", scalar="lambda")),
                 Gamma("tau", shape="a_tau", rate="b_tau")], response={"y": "mean"})
    samplers = [NormalNormal("beta", mdl), NormalGamma("tau", mdl)]
    state = {"y": y, "X": X, "beta": [0.0] * P, "P_tau": sparse.csc_matrix(np.eye(N)), "tau": 1, "P_lambda": sparse.csc_matrix(np.eye(P)),
             "mu": [0.0] * P, "lambda": 0.01, "a_tau": 1e-3, "b_tau": 1e-3}
    return MCMC(state, samplers, model=mdl, n_burn=3, n_iter=N_ITER, n_chains=C, seed=5, **mcmc_kw)


def prepared(M):
    """the run with its replicates left in the store, and the restatement's inputs from the run's own host results"""
    M.run_mcmc()
    assert M.posterior_predictive("y", name="y_rep") is None
    S = M.n_iter * M.n_chains
    m = M.state["y"].size
    d = dict(M=M, S=S, m=m, y=np.asarray(M.state["y"], dtype=np.float64).reshape(-1), ll=M.log_likelihood("y").reshape(S, m),
             mu=M.posterior_predictive("y", noise=False).reshape(S, m), y_rep=M.store["y_rep"].cpu().numpy().reshape(S, m),
             tau=np.moveaxis(M.collect()["tau"], -1, 0).reshape(S, 1))
    return d


@pytest.fixture(scope="module")
def smoother():
    d = prepared(build_smoother())
    yield d
    d["M"].engine.close()


@pytest.fixture(scope="module")
def regression():
    d = prepared(build_regression())
    yield d
    d["M"].engine.close()


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all(np.abs(got - want) <= 1e-10 * np.maximum(1.0, np.abs(want))))


def check_against_the_restatement(d):
    M, S, m, y = d["M"], d["S"], d["m"], d["y"]
    for reff in (1.0, np.linspace(0.3, 1.0, m)):
        tm = np.array([tail_max_of(S, r) for r in np.broadcast_to(reff, (m,))])
        # loo_predictive
        want = loo_expect(d["ll"], tm, d["mu"], None, d["tau"], np.longdouble)
        got = M.loo_predictive("y", reff=reff)
        assert set(got) == {"mean", "sd", "residual", "z", "r2", "pareto_k"}
        sd = np.sqrt(want["invprec"] + want["var"])
        res = y - want["mean"]
        print("pareto_k", got["pareto_k"], "r2", got["r2"])
        assert close(got["mean"], want["mean"]) and close(got["sd"], sd) and close(got["residual"], res) and close(got["z"], res / sd)
        assert close(got["r2"], 1 - np.var(res) / np.var(y)) and close(got["pareto_k"], want["k"])
        assert np.array_equal(got["pareto_k"], M.loo("y", reff=reff)["pareto_k"])
        # loo_pit: the analytic form and the replicates' (az.loo_pit's definition)
        pit = M.loo_pit("y", reff=reff)
        assert pit.shape == (m,) and close(pit, loo_expect(d["ll"], tm, normal_cdf(d["mu"], y, d["tau"]), None, None, np.longdouble)["mean"])
        want = loo_expect(d["ll"], tm, d["y_rep"], y, None, np.longdouble)
        pit_rep = M.loo_pit("y", y_rep="y_rep", reff=reff)
        assert pit_rep.shape == (m,) and close(pit_rep, want["below"]) and np.all((pit_rep >= 0) & (pit_rep <= 1))
        assert np.all((pit >= 0) & (pit <= 1))
        # loo_expectation of the replicates, whole and through an index
        got = M.loo_expectation("y", "y_rep", threshold=y, reff=reff)
        assert set(got) == {"mean", "sd", "ess", "pareto_k", "below"}
        assert close(got["mean"], want["mean"]) and close(got["sd"], np.sqrt(want["var"])) and close(got["ess"], want["ess"])
        assert close(got["below"], want["below"]) and np.array_equal(got["below"], pit_rep)
        back = np.arange(m)[::-1].copy()
        want = loo_expect(d["ll"], tm, d["y_rep"][:, back], np.full(m, 0.25), None, np.longdouble)
        got = M.loo_expectation("y", "y_rep", index=back, threshold=0.25, reff=reff)
        assert close(got["mean"], want["mean"]) and close(got["sd"], np.sqrt(want["var"])) and close(got["below"], want["below"])
        assert set(M.loo_expectation("y", "y_rep")) == {"mean", "sd", "ess", "pareto_k"}
        # loo_weights
        lw = M.loo_weights("y", reff=reff)
        assert lw.shape == (S // M.n_chains, M.n_chains, m) and close(lw.reshape(S, m), want["lw"])
        assert np.all(np.abs(logsumexp(lw.reshape(S, m).astype(np.longdouble), axis=0)) <= 1e-10)


def test_smoother_with_an_identity_mean(smoother):
    check_against_the_restatement(smoother)


def test_regression_with_a_linear_combination_mean(regression):
    check_against_the_restatement(regression)


def test_named_weights_are_a_key_of_the_summaries(regression):
    M = regression["M"]
    assert M.loo_weights("y", name="lw") is None
    t = M.store["lw"]
    assert tuple(t.shape) == (N_ITER, C, N) and "lw" in M._derived
    assert np.array_equal(t.cpu().numpy(), M.loo_weights("y"))
    assert M.quantiles("lw", [0.1, 0.9]).shape == (2, N)
    assert M.collect()["lw"].shape == (C, N, N_ITER)
    # the weights average any other stored quantity leave-one-out: here the replicates, as loo_expectation does
    w = np.exp(t.cpu().numpy().reshape(-1, N))
    assert close((w * regression["y_rep"]).sum(axis=0), M.loo_expectation("y", "y_rep")["mean"])
    with pytest.raises(ValueError, match="store entry of the run"):
        M.loo_weights("y", name="beta")
    with pytest.raises(ValueError, match="observations"):
        M.loo_expectation("y", "beta")


def test_three_observation_chunks_give_the_same_bits(regression):
    M, y = regression["M"], regression["y"]
    calls = [lambda: M.loo_predictive("y"), lambda: {"pit": M.loo_pit("y")}, lambda: {"pit": M.loo_pit("y", y_rep="y_rep")},
             lambda: M.loo_expectation("y", "y_rep", threshold=y), lambda: {"lw": M.loo_weights("y")}]
    whole = [c() for c in calls]
    M.pointwise_work_bytes = 8 * N_ITER * C * 10  # ten observations per chunk: three chunks
    try:
        parts = [c() for c in calls]
    finally:
        del M.pointwise_work_bytes
    for a, b in zip(whole, parts):
        for name in a:
            assert np.array_equal(a[name], b[name]), name


def test_unsupported_model_parts_are_named():
    from openmcmc_amd.parameter import LinearCombination, LinearCombinationWithTransform

    M = build_regression()
    try:
        M.run_mcmc()
        y = M.model["y"]
        M.posterior_predictive("y", name="y_rep")
        calls = {"loo_expectation": lambda r: M.loo_expectation(r, "y_rep"), "loo_predictive": M.loo_predictive, "loo_pit": M.loo_pit,
                 "loo_weights": M.loo_weights}
        for what, call in calls.items():
            with pytest.raises(NotImplementedError, match=f"{what}: a response of type Gamma"):
                call("tau")
            y.mean = LinearCombinationWithTransform(form={"beta": "X"}, transform={"beta": False})
            with pytest.raises(NotImplementedError, match=f"{what}: a mean of type LinearCombinationWithTransform"):
                call("y")
            y.mean = LinearCombination(form={"beta": "X"})
            M.state["y"] = np.zeros((N, 2))
            with pytest.raises(NotImplementedError, match=f"{what}: the response 'y' is replicated"):
                call("y")
            M.state["y"] = M.state["y"][:, 0] + 1.0
        assert M.loo_pit("y").shape == (N,)  # the supported form still runs after the round trip
    finally:
        M.engine.close()


def test_store_ring_guard():
    M = build_regression(store_ring=4)
    try:
        M.run_mcmc()
        for call in (M.loo_predictive, M.loo_pit, M.loo_weights):
            with pytest.raises(ValueError, match="store_ring"):
                call("y")
    finally:
        M.engine.close()
