"""The models of NormalNormal's routes at the smallest sizes that cross a block: USER model code on chain-batched state, shared by
tests/test_normal_normal_routes_gpu.py and benchmarks/normal_normal_same_bits.py.  Every builder takes (..., C, rng, eng) and
returns (model, state, samplers, the parameters whose NormalNormal block takes injected UNIFORMS: a truncated prior).  The
package is imported inside the builders, so a caller that compares two source trees decides which one they build on."""

import numpy as np


def rw1(n):
    from scipy import sparse

    d = np.full(n, 2.0)
    d[0] = d[-1] = 1.0
    d[0] += 1e-3
    return sparse.diags((-np.ones(n - 1), d, -np.ones(n - 1)), offsets=[-1, 0, 1], format="csc")


def rw2(n):
    from scipy import sparse

    D = sparse.diags((np.ones(n - 2), -2.0 * np.ones(n - 2), np.ones(n - 2)), offsets=[0, 1, 2], shape=(n - 2, n))
    return (D.T @ D + 1e-2 * sparse.identity(n)).tocsc()


def full_spd(n):
    A = np.random.default_rng(5).standard_normal((n + 5, n))
    return A.T @ A / n + 0.5 * np.eye(n)


def smoother(P, variant, n, C, rng, eng):
    """y ~ N(b [+ X beta], (tau I)^-1), b ~ N(mu, (lambda P)^-1) and what `variant` adds: the route follows P."""
    from scipy import sparse

    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.distribution import Gamma
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombination, ScaledMatrix
    from openmcmc_amd.sampler.sampler import NormalGamma, NormalNormal

    eye = sparse.identity(n, format="csc")
    t = np.arange(n) * 60.0 / n
    y = np.sin(t / 20) + 2 * np.cos(t / 12) + 2 + 0.3 * rng.standard_normal(n)
    st = {"y": y, "b": y.copy(), "mu": np.zeros(n), "lambda": 50, "P_lambda": P, "a_lam": 10, "b_lam": 1, "tau": 1, "P_tau": eye,
          "a_tau": 1, "b_tau": 1}
    parts = set(variant.split("+"))
    y_mean, b_mean, b_kw, more, normals, uniform = "b", "mu", {}, [], ["b"], set()
    if "offset" in parts:
        y_mean = LinearCombination(form={"b": "A", "beta": "X"})
        st.update(A=eye, X=rng.standard_normal((n, 4)), beta=np.zeros(4), mu_beta=np.zeros(4), P_beta=sparse.csc_matrix(0.5 * np.eye(4)))
        more.append(Normal("beta", mean="mu_beta", precision="P_beta"))
        normals.append("beta")
    if parts & {"mean", "mean_first", "two_vectors"}:
        b_mean = "m"
        st.update(m=np.full(n, 1.0), m0=np.zeros(n), P_m=sparse.csc_matrix(0.5 * np.eye(n)))
        more.append(Normal("m", mean="m0", precision="P_m"))
        normals = ["m"] + normals if "mean_first" in parts else normals + ["m"]
    if "mean_lincomb" in parts:  # (g is per chain and not sampled; the residual of b needs an identity design on a per-chain term)
        b_mean = LinearCombination(form={"g": "A_g"})
        st.update(A_g=eye, g=ChainArray(eng.to_device(1.0 + 0.1 * rng.standard_normal((C, n, 1)))))
    if "two_vectors" in parts:
        st.update(w=y.copy(), v=y + 0.1 * rng.standard_normal(n), P_w=sparse.csc_matrix(2.0 * np.eye(n)), P_v=sparse.csc_matrix(3.0 * np.eye(n)))
        more += [Normal("w", mean="b", precision="P_w"), Normal("v", mean="w", precision="P_v")]
        normals.append("w")
    if "replicated" in parts:
        st["y"] = y[:, None] + 0.2 * rng.standard_normal((n, 3))
    if parts & {"trunc1", "trunc2"}:
        b_kw = {"domain_response_lower": np.array(0.5)}
        if "trunc2" in parts:
            b_kw["domain_response_upper"] = np.array(4.5)
        st["b"] = np.clip(y, 0.7, 4.3)
        uniform.add("b")
    gammas = ["lambda"]
    if "const" in parts:  # an unscaled constant-diagonal term next to the prior
        st["P_y"] = sparse.csc_matrix(4.0 * np.eye(n))
        dists = [Normal("y", mean=y_mean, precision="P_y")]
    else:
        dists = [Normal("y", mean=y_mean, precision=ScaledMatrix(matrix="P_tau", scalar="tau")), Gamma("tau", shape="a_tau", rate="b_tau")]
        gammas.append("tau")
    dists += [Normal("b", mean=b_mean, precision=ScaledMatrix(matrix="P_lambda", scalar="lambda"), **b_kw),
              Gamma("lambda", shape="a_lam", rate="b_lam")] + more
    mdl = Model(dists)
    return mdl, st, [NormalNormal(k, mdl) for k in normals] + [NormalGamma(k, mdl) for k in gammas], uniform


def regression(variant, p, C, rng, eng):
    """y ~ N(X beta [+ Z gamma], (tau W)^-1), beta ~ N(mu, (lambda I)^-1): the dense route through the Gram matrix."""
    from scipy import sparse

    from openmcmc_amd.distribution.distribution import Gamma
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombination, ScaledMatrix
    from openmcmc_amd.sampler.sampler import NormalGamma, NormalNormal

    parts = set(variant.split("+"))
    n_obs, q = 90, 5
    X, Z = rng.standard_normal((n_obs, p)), rng.standard_normal((n_obs, q))
    y = X @ (rng.standard_normal(p) + 1.0) + 0.5 * rng.standard_normal(n_obs)
    W = (rw1(n_obs) + sparse.identity(n_obs)).tocsc() if "corr" in parts else sparse.csc_matrix(np.diag(0.5 + rng.random(n_obs)))
    st = {"y": y, "X": X, "Z": Z, "beta": np.full(p, 0.5), "gamma": np.zeros(q), "mu_b": np.zeros(p), "mu_g": np.zeros(q), "P_tau": W,
          "tau": 1, "P_lambda": sparse.csc_matrix(np.eye(p)), "lambda": 0.1, "P_g": sparse.csc_matrix(np.eye(q) + 0.3), "a_tau": 1e-2,
          "b_tau": 1e-2, "a_lambda": 1e-2, "b_lambda": 1e-2}
    form, more, normals, b_kw, uniform = {"beta": "X"}, [], ["beta"], {}, set()
    if "offset" in parts:
        form["gamma"] = "Z"
        more.append(Normal("gamma", mean="mu_g", precision="P_g"))
        normals.append("gamma")
    if "trunc" in parts:
        b_kw, uniform = {"domain_response_lower": np.array(0.0)}, {"beta"}
    mdl = Model([Normal("y", mean=LinearCombination(form=form), precision=ScaledMatrix(matrix="P_tau", scalar="tau")),
                 Normal("beta", mean="mu_b", precision=ScaledMatrix(matrix="P_lambda", scalar="lambda"), **b_kw),
                 Gamma("tau", shape="a_tau", rate="b_tau"), Gamma("lambda", shape="a_lambda", rate="b_lambda")] + more, response={"y": "mean"})
    samplers = [NormalNormal(k, mdl) for k in normals] + [NormalGamma("tau", mdl), NormalGamma("lambda", mdl)]
    if "factorise" in parts:
        samplers[0].spectral = False
    return mdl, st, samplers, uniform


def mixture(variant, p, C, rng, eng):
    """The mixture-prior regression of benchmarks/mixture_regression.py at a small size, with a lower limit for `trunc`."""
    from openmcmc_amd.distribution.distribution import Categorical, Gamma
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import Identity, LinearCombination, MixtureParameterMatrix, MixtureParameterVector
    from openmcmc_amd.sampler.sampler import MixtureAllocation, NormalGamma, NormalNormal

    n_obs, K = 90, 3
    X = rng.standard_normal((n_obs, p))
    means = np.array([0.5, 1.0, 2.0])
    beta = means[rng.integers(0, K, size=p)] + 0.1 * rng.standard_normal(p)
    y = X @ beta + 0.5 * rng.standard_normal(n_obs)
    st = {"response": y.reshape(n_obs, 1), "prefactor_matrix": X, "parameter": np.full((p, 1), 0.5), "prior_mean": means.reshape(K, 1),
          "precision_matrix": np.diag(np.full(n_obs, 4.0)), "prior_precision_vector": np.ones(K), "gamma_shape": 2.0 * np.ones((K,)),
          "gamma_rate": 1.0 * np.ones((K,)), "allocation": rng.integers(0, K, size=(p, 1)), "prior_allocation_prob": np.array([[0.3, 0.4, 0.3]])}
    kw = {"domain_response_lower": np.array([[0.0]])} if variant == "trunc" else {}
    mdl = Model([
        Normal("response", mean=LinearCombination({"parameter": "prefactor_matrix"}), precision=Identity("precision_matrix")),
        Normal("parameter", mean=MixtureParameterVector("prior_mean", "allocation"),
               precision=MixtureParameterMatrix("prior_precision_vector", "allocation"), **kw),
        Gamma("prior_precision_vector", shape=Identity("gamma_shape"), rate=Identity("gamma_rate")),
        Categorical("allocation", prob="prior_allocation_prob")])
    samplers = [NormalNormal("parameter", mdl), NormalGamma("prior_precision_vector", mdl),
                MixtureAllocation("allocation", mdl, response_param="parameter")]
    return mdl, st, samplers, ({"parameter"} if kw else set())


def ragged(variant, n, C, rng, eng):
    """The reversible-jump regression of tests/rj_problem.py: a variable-size NormalNormal block with a per-chain design."""
    from rj_problem import build

    n_max = 5
    X = np.linspace(-8.0, 8.0, n)
    y = np.sin(X / 2.0) + 0.2 * rng.standard_normal(n)
    k0 = np.array([1 + c % 3 for c in range(C)])
    theta = [rng.uniform(-8, 8, size=int(k)) for k in k0]
    beta = [0.5 + rng.random(int(k)) for k in k0]
    mdl, st, samplers = build(y, X, rw1(n).toarray(), n_max, eng, theta, beta, k0)
    if variant == "limits":
        mdl["beta"].domain_response_lower = np.array([[0.0]])
    return mdl, st, samplers, ({"beta"} if variant == "limits" else set())
