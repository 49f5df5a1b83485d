"""MCMC.project and MCMC.posterior_predictive on a small regression run (12 observations, 5 coefficients, 6 chains, 9 stored
iterations; NormalNormal + NormalGamma): the linear maps against the host loop over collect(), the named entries as keys of the
other store summaries, in-place accumulation, and the model parts posterior_predictive reports as unsupported.  The error bound is
the header's: (n_idx + 2) 2^-53 (|base| + |offset| + sum|terms|) around math.fsum of the terms."""

import math

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

N, P, C, N_ITER = 12, 5, 6, 9


def build(mean=None, precision=None, extra_state=None, response=True, **mcmc_kw):
    from openmcmc_amd.distribution.distribution import Gamma
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.mcmc import MCMC
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombination, ScaledMatrix
    from openmcmc_amd.sampler.sampler import NormalGamma, NormalNormal

    rng = np.random.default_rng(42)
    X = rng.standard_normal((N, P))
    y = X @ np.arange(1.0, P + 1) + 0.3 * rng.standard_normal(N)
    mdl = Model([Normal("y", mean=mean or LinearCombination(form={"beta": "X"}),
                        precision=precision or ScaledMatrix(matrix="P_tau", scalar="tau")),
                 Normal("beta", mean="mu", precision=ScaledMatrix(matrix="P_lambda", scalar="lambda")),
                 Gamma("tau", shape="a_tau", rate="b_tau")], response={"y": "mean"} if response else None)
    samplers = [NormalNormal("beta", mdl), NormalGamma("tau", mdl)]
    state = {"y": y, "X": X, "beta": [0.0] * P, "P_tau": sparse.csc_matrix(np.eye(N)), "tau": 1, "P_lambda": sparse.csc_matrix(np.eye(P)),
             "mu": [0.0] * P, "lambda": 0.01, "a_tau": 1e-3, "b_tau": 1e-3}
    state.update(extra_state or {})
    return MCMC(state, samplers, model=mdl, n_burn=3, n_iter=N_ITER, n_chains=C, seed=5, **mcmc_kw), X


@pytest.fixture(scope="module")
def run():
    M, X = build()
    M.run_mcmc()
    yield M, X
    M.engine.close()


def within_bound(got, rows, W, offset=None, base=None):
    """got (R, m) against math.fsum of the terms of rows (R, n) under W (m, n)"""
    R, n = rows.shape
    for r in range(R):
        for j in range(W.shape[0]):
            t = W[j] * rows[r]
            o = 0.0 if offset is None else offset[j]
            b = 0.0 if base is None else base[r, j]
            exact = math.fsum(list(t) + [o, b])
            assert abs(got[r, j] - exact) <= (n + 2) * 2.0 ** -53 * (abs(o) + abs(b) + math.fsum(np.abs(t))), (r, j)


def test_project_against_the_host_loop(run):
    M, X = run
    host = M.collect()
    beta = np.moveaxis(host["beta"], -1, 0)  # (C, p, n_iter) -> (n_iter, C, p)
    rng = np.random.default_rng(0)
    A = rng.standard_normal((17, P))
    got = M.project("beta", A)
    assert got.shape == (N_ITER, C, 17)
    within_bound(got.reshape(-1, 17), beta.reshape(-1, P), A)
    off = rng.standard_normal(4)
    idx = [4, 0, 0, 2]
    got = M.project("beta", A[:4, :4], index=idx, offset=off)
    within_bound(got.reshape(-1, 4), beta.reshape(-1, P)[:, idx], A[:4, :4], offset=off)
    lp = M.project("log_post", [2.0])  # a 2-D entry counts as one element
    assert lp.shape == (N_ITER, C, 1) and np.array_equal(lp[..., 0], 2.0 * host["log_post"][:, :, 0].T)
    # the run's own fitted values (response={"y": "mean"}) are the same linear map
    fitted = np.moveaxis(host["y"], -1, 0)
    assert np.allclose(M.project("beta", X), fitted, rtol=1e-12, atol=1e-12)


def test_named_entry_is_a_key_of_the_other_summaries(run):
    M, X = run
    assert M.project("beta", X, name="curve") is None
    t = M.store["curve"]
    assert tuple(t.shape) == (N_ITER, C, N) and "curve" in M._derived
    assert np.array_equal(t.cpu().numpy(), M.project("beta", X))
    q = M.quantiles("curve", [0.1, 0.9])
    assert q.shape == (2, N) and np.all(q[0] <= q[1])
    assert M.hdi("curve", 0.8).shape == (N, 2)
    d = M.diagnostics("curve")
    assert d["rhat"].shape == (N,) and d["ess"].shape == (N,)
    band = M.simultaneous_band("curve", 0.9)
    assert band["lower"].shape == (N,) and np.all(band["lower"] <= band["upper"]) and band["critical"] > 0
    mean, _ = M.summary("curve")
    assert np.allclose(mean, t.cpu().numpy().reshape(-1, N).mean(axis=0), rtol=1e-12)
    host = M.collect()
    assert host["curve"].shape == (C, N, N_ITER)
    assert np.array_equal(np.moveaxis(host["curve"], -1, 0), t.cpu().numpy())
    assert M.project("beta", 2.0 * X, name="curve") is None  # a derived name may be made again
    assert np.array_equal(M.store["curve"].cpu().numpy(), M.project("beta", 2.0 * X))
    for own in ("beta", "tau", "y", "log_post"):
        with pytest.raises(ValueError, match="store entry of the run"):
            M.project("beta", X, name=own)


def test_two_terms_accumulate_through_base(run):
    M, X = run
    rng = np.random.default_rng(1)
    B = rng.standard_normal((N, 1))
    M.project("beta", X, name="f")
    first = M.store["f"]
    ptr, before = first.data_ptr(), first.cpu().numpy()
    assert M.project("tau", B, base="f", name="f") is None
    assert M.store["f"].data_ptr() == ptr  # in place
    M.project("beta", X, name="g")
    want = M.project("tau", B, base="g")  # out of place: the same bits
    assert np.array_equal(M.store["f"].cpu().numpy(), want)
    tau = M.store["tau"].cpu().numpy().reshape(-1, 1)
    within_bound(want.reshape(-1, N), tau, B, base=before.reshape(-1, N))
    with pytest.raises(ValueError, match="cannot be accumulated"):
        M.project("f", np.eye(N), base="f", name="f")


def test_posterior_predictive_is_the_composition(run):
    M, X = run
    fitted = M.posterior_predictive("y", noise=False)
    assert np.array_equal(fitted, M.project("beta", X))
    for rep in (0, 3):
        got = M.posterior_predictive("y", replicate=rep)
        assert got.shape == (N_ITER, C, N)
        assert np.array_equal(got, M.project("beta", X, noise_precision="tau", replicate=rep))
    assert not np.array_equal(M.posterior_predictive("y"), M.posterior_predictive("y", replicate=1))
    assert "_predictive_of_y" not in M.store
    assert M.posterior_predictive("y", name="y_rep") is None
    assert np.array_equal(M.store["y_rep"].cpu().numpy(), M.posterior_predictive("y"))
    # the noise has the scale the stored precision gives it
    tau = M.store["tau"].cpu().numpy().reshape(N_ITER, C, 1)
    zs = (M.posterior_predictive("y") - fitted) * np.sqrt(tau)
    assert abs(zs.mean()) < 5 / np.sqrt(zs.size) and abs(zs.std() - 1) < 0.15
    with pytest.raises(ValueError, match="store entry of the run"):
        M.posterior_predictive("y", name="y")


def test_store_ring_guard():
    M, X = build(store_ring=4)
    try:
        M.run_mcmc()
        with pytest.raises(ValueError, match="store_ring"):
            M.project("beta", X)
        with pytest.raises(ValueError, match="store_ring"):
            M.posterior_predictive("y")
    finally:
        M.engine.close()


def test_constant_and_diagonal_precisions():
    """a constant of the state as the precision (Identity), and a scalar times a diagonal matrix that is not the identity"""
    from openmcmc_amd.parameter import Identity, ScaledMatrix

    d = np.linspace(0.5, 2.0, N)
    M, X = build(extra_state={"P_w": sparse.diags(d).tocsc(), "kappa": 4.0})
    try:
        M.run_mcmc()
        fitted = M.project("beta", X)
        M.model["y"].precision = ScaledMatrix(matrix="P_w", scalar="tau")
        tau = M.store["tau"].cpu().numpy().reshape(N_ITER, C, 1)
        M.store["tau_d"] = M.engine.to_device(tau * d)
        M._derived.add("tau_d")
        assert np.array_equal(M.posterior_predictive("y"), M.project("beta", X, noise_precision="tau_d"))
        M.model["y"].precision = Identity("kappa")
        got = M.posterior_predictive("y")
        assert tuple(M.store["_precision_kappa"].shape) == (N_ITER, C, 1)
        M.store["four"] = M.engine.full((N_ITER, C, 1), 4.0)
        M._derived.add("four")
        assert np.array_equal(got, M.project("beta", X, noise_precision="four"))
        assert not np.array_equal(got, fitted)
        M.model["y"].mean = Identity("beta")  # a stored parameter as the mean: the entry itself
        assert np.array_equal(M.posterior_predictive("y", noise=False), M.store["beta"].cpu().numpy())
    finally:
        M.engine.close()


def test_unsupported_model_parts_are_named():
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.distribution import Gamma
    from openmcmc_amd.parameter import Identity, LinearCombination, LinearCombinationWithTransform, ScaledMatrix

    M, X = build(extra_state={"P_full": np.eye(N) + 0.1, "gamma": np.zeros(3), "Z": np.zeros((N, 3))})
    try:
        M.run_mcmc()
        eng = M.engine
        y = M.model["y"]
        with pytest.raises(NotImplementedError, match="Gamma"):
            M.posterior_predictive("tau")
        assert isinstance(M.model["tau"], Gamma)
        y.mean = LinearCombinationWithTransform(form={"beta": "X"}, transform={"beta": False})
        with pytest.raises(NotImplementedError, match="LinearCombinationWithTransform"):
            M.posterior_predictive("y")
        y.mean = LinearCombination(form={"beta": "X", "gamma": "Z"})
        with pytest.raises(NotImplementedError, match="'gamma' is not in the store"):
            M.posterior_predictive("y")
        y.mean = Identity("mu")
        with pytest.raises(NotImplementedError, match="'mu' is not in the store"):
            M.posterior_predictive("y")
        y.mean = LinearCombination(form={"beta": "X"})
        M.state["X"] = ChainArray(eng.zeros(C, N, P))
        with pytest.raises(NotImplementedError, match="'X' is per chain"):
            M.posterior_predictive("y")
        M.state["X"] = X
        y.precision = ScaledMatrix(matrix="P_full", scalar="tau")
        with pytest.raises(NotImplementedError, match="'P_full' is not diagonal"):
            M.posterior_predictive("y")
        y.precision = Identity("P_full")
        with pytest.raises(NotImplementedError, match="'P_full' is a matrix"):
            M.posterior_predictive("y")
        y.precision = ScaledMatrix(matrix="P_tau", scalar="tau")
        assert M.posterior_predictive("y", noise=False).shape == (N_ITER, C, N)
    finally:
        M.engine.close()
