"""Truncated mixture priors on the GPU: omc_small_gibbs_truncated (ragged route) and omc_dense_gibbs_truncated with a
per-chain diagonal against a numpy restatement of gmrf.gibbs_canonical_truncated_normal (gmrf.py:239-264), their
in-kernel uniforms, the domain rule of a mixture Normal's log_p over the live entries (location_scale.py:162-188), and
two models replayed against the reference through MCMC.run_mcmc: the mixture regression with coefficients >= 0 (dense
route, tests/golden/truncated_mixture.npz) and the cfg5 reversible-jump model with beta >= 0 (ragged route,
tests/golden/rj_truncated_chain.npz), both made by tests/golden/make_golden_r5.py."""

import numpy as np
import pytest
from scipy import stats

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def tn_ref(mean, sd, lo, hi, u):
    """gmrf.truncated_normal_rv with the uniform behind truncnorm.rvs given."""
    return stats.truncnorm.ppf(u, (lo - mean) / sd, (hi - mean) / sd) * sd + mean


def scan_ref(Q, b, x, lo, hi, u):
    """gmrf.gibbs_canonical_truncated_normal (gmrf.py:239-264) with recorded uniforms, in float64 numpy."""
    x = np.array(x, dtype=np.float64)
    p = x.size
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (p,))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), (p,))
    if p == 0:
        return x
    if p == 1:  # gmrf.py:244-247
        return np.array([tn_ref(b[0] / Q[0, 0], 1 / np.sqrt(Q[0, 0]), lo[0], hi[0], u[0])])
    for i in range(p):
        v = 1 / Q[i, i]
        x[i] = tn_ref(v * (b[i] - Q[i, :] @ x + Q[i, i] * x[i]), np.sqrt(v), lo[i], hi[i], u[i])
    return x


def relerr(got, ref):
    return np.max(np.abs(got - ref) / np.maximum(1e-3, np.abs(ref)), initial=0.0)


def small_problem(rng, C, kmax, counts, lo, hi, where):
    """Per-chain Gram matrices, prior precisions / means, likelihood scales; the unconstrained conditional mean of every
    site put `where` = "bind" (5 sd beyond the limit) or "far" (50 sd inside)."""
    gram = np.zeros((C, kmax, kmax))
    rhs = np.zeros((C, kmax))
    prec = np.ones((C, kmax))
    pmean = np.zeros((C, kmax))
    tau = 0.5 + rng.random(C)
    x0 = np.zeros((C, kmax))
    Qs, bs = [], []
    for c, k in enumerate(counts):
        A = rng.standard_normal((k + 3, k))
        G = A.T @ A
        gram[c, :k, :k] = G
        prec[c, :k] = 0.5 + 2 * rng.random(k)
        Q = np.diag(prec[c, :k]) + tau[c] * G
        sd = 1 / np.sqrt(np.diag(Q)) if k else np.zeros(0)
        if where == "bind":
            m = (lo - 5 * sd) if np.isfinite(lo) else (hi + 5 * sd)
        else:
            m = (lo + 50 * sd) if np.isfinite(lo) else (hi - 50 * sd) if np.isfinite(hi) else rng.standard_normal(k)
        pmean[c, :k] = rng.standard_normal(k)
        b = Q @ m
        rhs[c, :k] = (b - prec[c, :k] * pmean[c, :k]) / tau[c]
        bs.append(prec[c, :k] * pmean[c, :k] + tau[c] * rhs[c, :k])
        Qs.append(Q)
        lo_f = lo if np.isfinite(lo) else (hi - 1.0)
        hi_f = hi if np.isfinite(hi) else (lo + 1.0)
        x0[c, :k] = rng.uniform(lo_f, hi_f, size=k)
    return gram, rhs, prec, pmean, tau, x0, Qs, bs


LIMITS = [(0.0, np.inf), (-np.inf, 0.5), (-0.3, 0.4)]


@pytest.mark.parametrize("kmax", [1, 7, 20, 36, 64])
def test_small_gibbs_truncated_matches_restatement(kmax):
    from openmcmc_amd.engine import Engine

    rng = np.random.default_rng(kmax)
    counts = sorted({0, 1, kmax, max(kmax // 2, 0), max(kmax - 1, 0), int(rng.integers(0, kmax + 1))})
    C = len(counts)
    eng = Engine(C, seed=3)
    worst = 0.0
    for lo, hi in LIMITS:
        for where in ("bind", "far"):
            if where == "far" and np.isfinite(lo) and np.isfinite(hi):
                lo_, hi_ = -1e3, 1e3  # both limits, far from every conditional mean
            else:
                lo_, hi_ = lo, hi
            gram, rhs, prec, pmean, tau, x0, Qs, bs = small_problem(rng, C, kmax, counts, lo_, hi_, where)
            u = rng.random((C, kmax))
            t = eng.to_device
            x = t(np.where(np.arange(kmax)[None, :] < np.array(counts)[:, None], x0, 7.0))  # garbage in the padding
            eng.small_gibbs_truncated(t(gram), t(rhs), t(prec), x, lower=lo_, upper=hi_, lik_scale=t(tau), prior_mean=t(pmean),
                                      count=t(np.array(counts, dtype=np.float64)), u=t(u))
            eng.check_status()
            got = x.cpu().numpy()
            for c, k in enumerate(counts):
                ref = scan_ref(Qs[c], bs[c], x0[c, :k], lo_, hi_, u[c, :k])
                err = relerr(got[c, :k], ref)
                worst = max(worst, err)
                assert err < RTOL, (kmax, k, lo_, hi_, where, err)
                assert np.all(got[c, :k] >= lo_) and np.all(got[c, :k] <= hi_)
                assert np.all(got[c, k:] == 0.0)  # padding exactly 0
    print("worst relative difference", worst)
    eng.close()


@pytest.mark.parametrize("p", [1, 7, 64, 300])
def test_dense_gibbs_truncated_diag_chain_matches_restatement(p):
    from openmcmc_amd.engine import Engine

    rng = np.random.default_rng(100 + p)
    C = 3
    eng = Engine(C, seed=4)
    A = rng.standard_normal((p + 5, p))
    M = A.T @ A / p
    r = rng.standard_normal(p)
    s = 0.5 + rng.random(C)
    d = 0.5 + 3 * rng.random((C, p))
    rc = rng.standard_normal((C, p)) * 3
    lower = np.where(rng.random(p) < 0.5, 0.0, -np.inf)
    x0 = np.abs(rng.standard_normal((C, p)))
    u = rng.random((C, p))
    t = eng.to_device
    x = t(x0)
    terms = [{"mat": t(M), "rhs": t(r), "scale": t(s)}]
    eng.dense_gibbs_truncated(p, terms, x, lower=t(lower), u=t(u), rhs_chain=t(rc), diag_chain=t(d))
    eng.check_status()
    got = x.cpu().numpy()
    for c in range(C):
        Q = s[c] * M + np.diag(d[c])
        b = s[c] * r + rc[c]
        ref = scan_ref(Q, b, x0[c], lower, np.inf, u[c])
        assert relerr(got[c], ref) < RTOL, (p, c, relerr(got[c], ref))
        assert np.all(got[c] >= lower)
    eng.close()


@pytest.mark.parametrize("p", [1, 7, 65])
def test_dense_gibbs_truncated_zero_diag_chain_is_the_plain_scan(p):
    """The two instantiations of k_dense_gibbs_truncated are one source: a per-chain diagonal of zeros adds 0 to positive
    diagonal entries (no signed zero arises) and the scan is the one without diag_chain, bit for bit.  The inputs of
    test_dense_gibbs_truncated_diag_chain_matches_restatement; p = 65 makes the lanes stride."""
    from openmcmc_amd.engine import Engine

    rng = np.random.default_rng(100 + p)
    C = 3
    eng = Engine(C, seed=4)
    A = rng.standard_normal((p + 5, p))
    M = A.T @ A / p
    r = rng.standard_normal(p)
    s = 0.5 + rng.random(C)
    rng.random((C, p))  # (the diagonal d of that test: its draws keep the streams of the inputs below in step)
    rc = rng.standard_normal((C, p)) * 3
    lower = np.where(rng.random(p) < 0.5, 0.0, -np.inf)
    x0 = np.abs(rng.standard_normal((C, p)))
    u = rng.random((C, p))
    t = eng.to_device
    terms = [{"mat": t(M), "rhs": t(r), "scale": t(s)}]
    x_plain, x_zero = t(x0), t(x0)
    eng.dense_gibbs_truncated(p, terms, x_plain, lower=t(lower), u=t(u), rhs_chain=t(rc))
    eng.dense_gibbs_truncated(p, terms, x_zero, lower=t(lower), u=t(u), rhs_chain=t(rc), diag_chain=t(np.zeros((C, p))))
    eng.check_status()
    plain, zero = x_plain.cpu().numpy(), x_zero.cpu().numpy()
    assert np.all(np.isfinite(plain)) and not np.array_equal(plain, x0)
    assert np.array_equal(plain, zero), (p, np.max(np.abs(plain - zero)))
    eng.close()


def test_small_gibbs_truncated_in_kernel_uniforms():
    """Same draw_index: bit-equal; identical chains differ; count == 1 draws follow scipy's truncnorm (KS)."""
    from openmcmc_amd.engine import Engine

    rng = np.random.default_rng(9)
    C, kmax = 16, 20
    eng = Engine(C, seed=11)
    t = eng.to_device
    counts = np.full(C, 12.0)
    gram, rhs, prec, pmean, tau, x0, _, _ = small_problem(rng, 1, kmax, [12], 0.0, np.inf, "bind")
    rep = lambda a: t(np.repeat(a, C, axis=0))  # noqa: E731  every chain the same problem
    outs = []
    for _ in range(2):
        x = rep(x0)
        eng.small_gibbs_truncated(rep(gram), rep(rhs), rep(prec), x, lower=0.0, lik_scale=t(np.repeat(tau, C)),
                                  prior_mean=rep(pmean), count=t(counts), draw_index=5)
        outs.append(x.cpu().numpy())
    eng.check_status()
    assert np.array_equal(outs[0], outs[1])
    assert len({outs[0][c].tobytes() for c in range(C)}) == C
    assert np.all(outs[0][:, :12] >= 0.0) and np.all(outs[0][:, 12:] == 0.0)
    eng.close()

    C = 4096
    eng = Engine(C, seed=12)
    t = eng.to_device
    # Q = prec + tau * g = 4, b = Q * mean: mean -1 (the limit 0 binds at 2 sd) or 0.3 with the limit 10 sd below
    for mean, lo in ((-1.0, 0.0), (0.3, -5.0)):
        x = t(np.full((C, 1), max(lo, 0.0) + 0.1))
        eng.small_gibbs_truncated(t(np.full((C, 1, 1), 2.0)), t(np.full((C, 1), 4.0 * mean)), t(np.full((C, 1), 2.0)), x,
                                  lower=lo, lik_scale=t(np.ones(C)), count=t(np.ones(C)), draw_index=1)
        eng.check_status()
        draws = x.cpu().numpy().ravel()
        sd = 0.5
        ks = stats.kstest(draws, stats.truncnorm((lo - mean) / sd, np.inf, loc=mean, scale=sd).cdf)
        assert ks.pvalue > 1e-3, (mean, lo, ks)
        assert np.all(draws >= lo)
    eng.close()


def test_truncated_mixture_model_replays_reference(golden):
    """The mixture regression with coefficients >= 0 (dense route, diag_chain) through MCMC.run_mcmc with the reference's
    draws: allocations identical, coefficients, component precisions and log_post to 1e-10."""
    import torch

    from openmcmc_amd.distribution.distribution import Categorical, Gamma
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.mcmc import MCMC
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import Identity, LinearCombination, MixtureParameterMatrix, MixtureParameterVector
    from openmcmc_amd.sampler.sampler import MixtureAllocation, NormalGamma, NormalNormal

    G = golden("truncated_mixture")
    n, p, K, n_iter = int(G["n"]), int(G["p"]), int(G["K"]), int(G["n_iter"])
    st = {"response": G["y"].reshape(n, 1), "prefactor_matrix": G["X"], "parameter": G["parameter0"].reshape(p, 1),
          "prior_mean": G["prior_mean"].reshape(K, 1), "precision_matrix": np.diag(G["w"]), "prior_precision_vector": G["prec0"],
          "gamma_shape": 2.0 * np.ones((K,)), "gamma_rate": 1.0 * np.ones((K,)), "allocation": G["alloc0"].reshape(p, 1),
          "prior_allocation_prob": G["prob"]}
    mdl = Model([
        Normal("response", mean=LinearCombination({"parameter": "prefactor_matrix"}), precision=Identity("precision_matrix")),
        Normal("parameter", mean=MixtureParameterVector("prior_mean", "allocation"),
               precision=MixtureParameterMatrix("prior_precision_vector", "allocation"),
               domain_response_lower=np.array([[float(G["lower"])]])),
        Gamma("prior_precision_vector", shape=Identity("gamma_shape"), rate=Identity("gamma_rate")),
        Categorical("allocation", prob="prior_allocation_prob")])
    samplers = [NormalNormal("parameter", mdl), NormalGamma("prior_precision_vector", mdl),
                MixtureAllocation("allocation", mdl, response_param="parameter")]
    C = 2
    dev = torch.device("cuda", 0)
    tile = lambda a: torch.as_tensor(np.tile(a, (C, 1)), device=dev)  # noqa: E731
    samplers[0].inject = lambda s, it: tile(G["u_trunc"][it])
    samplers[1].inject = lambda s, it: tile(G["g"][it])
    samplers[2].inject = lambda s, it: tile(G["u"][it])
    M = MCMC(st, samplers, model=mdl, n_burn=0, n_iter=n_iter, n_chains=C)
    M.run_mcmc()
    got = M.collect()
    for c in range(C):
        assert np.array_equal(got["allocation"][c], G["store_allocation"])
        assert np.all(got["parameter"][c] >= 0.0)
        for key in ("parameter", "prior_precision_vector", "log_post"):
            ref = G["store_" + key]
            err = np.max(np.abs(got[key][c] - ref) / np.maximum(1.0, np.abs(ref)))
            assert err < 1e-10, (key, err)


def _nan0(a, fill=0.5):
    return np.where(np.isnan(a), fill, a)


def test_rj_truncated_chain_matches_reference(golden):
    """cfg5 shape with beta >= 0: five chains with different starting dimensions together, every draw injected from the
    reference's tape.  The bar of tests/test_rj_chain_gpu.py: dimension trace identical, accept counters identical, the
    rest to 1e-10 (the fitted mean is not stored in this fixture: it follows from b, beta and theta)."""
    import torch

    from openmcmc_amd.engine import Engine
    from openmcmc_amd.mcmc import MCMC
    from rj_problem import build

    G = golden("rj_truncated_chain")
    n_max, n_iter = int(G["n_max"]), int(G["n_iter"])
    P = np.diag(G["P_diag"]) + np.diag(G["P_off"], 1) + np.diag(G["P_off"], -1)
    k0 = G["init_k"]
    C = k0.size
    init_theta = [G["init_theta"][c][: int(k)] for c, k in enumerate(k0)]
    init_beta = [G["init_beta"][c][: int(k)] for c, k in enumerate(k0)]
    tape = {k[5:]: G[k] for k in G.files if k.startswith("tape_")}
    eng = Engine(C)
    dev = eng.device
    mdl, state, samplers = build(G["y"], G["X"], P, n_max, eng, init_theta, init_beta, k0)
    mdl["beta"].domain_response_lower = np.array([[float(G["lower"])]])

    def t(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)

    s_b, s_beta, s_lam, s_tau, s_rw, s_rj = samplers
    s_b.inject = lambda s, it: t(tape["z_b"][:, it])
    s_beta.inject = lambda s, it: t(_nan0(tape["u_beta"][:, it]))  # the truncated scan's uniforms
    s_lam.inject = lambda s, it: t(tape["g"][:, it, 0])
    s_tau.inject = lambda s, it: t(tape["g"][:, it, 1])
    s_rw.inject = lambda s, it, j: t(_nan0(tape["rw_u"][:, it, j]).reshape(C, 1))
    s_rw.inject_uniform = lambda s, it, j: t(_nan0(tape["rw_acc_u"][:, it, j]))
    s_rj.inject_move = lambda s, it: (t(_nan0(tape["rj_move_u"][:, it])),
                                      torch.as_tensor(np.maximum(tape["rj_idx"][:, it], 0).astype(np.int64), device=dev))
    s_rj.inject_associated = lambda s, it: {"theta": t(_nan0(tape["rj_theta_u"][:, it]).reshape(C, 1))}
    s_rj.inject_match = lambda s, it: t(_nan0(tape["rj_beta_u"][:, it]))
    s_rj.inject_uniform = lambda s, it: t(_nan0(tape["rj_acc_u"][:, it]))
    M = MCMC(state, samplers, model=mdl, n_burn=0, n_iter=n_iter, n_chains=C, engine=eng)
    M.run_mcmc()
    got = M.collect()
    assert np.array_equal(got["n_basis"], G["store_n_basis"])
    for key in ("theta", "beta"):
        assert np.array_equal(np.isnan(got[key]), np.isnan(G["store_" + key])), key
    assert np.nanmin(got["beta"]) >= 0.0
    for key in ("theta", "beta", "b", "lambda", "tau", "log_post"):
        ref = G["store_" + key]
        err = np.nanmax(np.abs(got[key] - ref) / np.maximum(1.0, np.abs(ref)))
        assert err < 1e-10, (key, err)
    assert np.array_equal(s_rw.accept_rate.accept.cpu().numpy(), G["accept_rw"][:, 0].astype(np.int64))
    assert np.array_equal(s_rj.accept_rate.accept.cpu().numpy(), G["accept_rj"][:, 0].astype(np.int64))
    assert np.array_equal(s_rj.accept_rate.proposal.cpu().numpy(), G["accept_rj"][:, 1].astype(np.int64))


def test_mixture_log_p_domain_rule_over_live_entries():
    """A chain with one live element outside gets -inf; padding outside the limits does not; the other chains equal the
    untruncated log-density bit for bit.  Ragged (count) and fixed-size forms."""
    from openmcmc_amd.chains import ragged_from_lists
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.engine import Engine
    from openmcmc_amd.parameter import MixtureParameterMatrix, MixtureParameterVector

    C, n_max = 4, 6
    eng = Engine(C)
    dev = eng.device
    lists = [np.array([1.5, 2.0, 1.1]), np.array([1.5, 0.9, 3.0, 1.2]), np.array([1.0]), np.array([2.0, 1.3, 1.7, 4.0, 1.01, 1.2])]
    ks = [v.size for v in lists]
    import torch

    from openmcmc_amd.chains import ChainArray

    state = {"beta": ragged_from_lists(lists, n_max, 0, "k", dev),
             "alloc": ragged_from_lists([np.arange(k) % 2 for k in ks], n_max, 0, "k", dev),
             "k": ChainArray(torch.as_tensor(np.array(ks, dtype=np.float64), device=dev).reshape(-1, 1, 1)),
             "mu": np.array([[0.5], [-1.0]]), "prec": np.array([[2.0], [0.25]])}
    kw = dict(mean=MixtureParameterVector("mu", "alloc"), precision=MixtureParameterMatrix("prec", "alloc"))
    plain = Normal("beta", **kw).log_p(state, engine=eng).cpu().numpy()
    limited = Normal("beta", domain_response_lower=np.array([[1.0]]), **kw).log_p(state, engine=eng).cpu().numpy()
    assert np.isneginf(limited[1])  # live 0.9 < 1
    for c in (0, 2, 3):  # zero padding below the limit ignored
        assert np.isfinite(limited[c]) and limited[c] == plain[c], c
    upper = Normal("beta", domain_response_upper=np.array([[3.5]]), **kw).log_p(state, engine=eng).cpu().numpy()
    assert np.isneginf(upper[3]) and all(upper[c] == plain[c] for c in (0, 1, 2))

    # fixed size, one limit per element (count None)
    fixed = {"beta": ChainArray(torch.as_tensor(np.array([[1.0, 2.0, 3.0]] * C), device=dev).reshape(C, 3, 1)),
             "alloc": ChainArray(torch.as_tensor(np.array([[0.0, 1.0, 0.0]] * C), device=dev).reshape(C, 3, 1)),
             "mu": state["mu"], "prec": state["prec"]}
    fixed["beta"].data[2, 1, 0] = -1.0
    lo = np.array([[0.0], [-2.0], [0.5]])
    base = Normal("beta", **kw).log_p(fixed, engine=eng).cpu().numpy()
    lim = Normal("beta", domain_response_lower=lo, **kw).log_p(fixed, engine=eng).cpu().numpy()
    assert np.array_equal(lim, base)
    fixed["beta"].data[1, 2, 0] = 0.2  # below its own limit 0.5
    base = Normal("beta", **kw).log_p(fixed, engine=eng).cpu().numpy()
    lim = Normal("beta", domain_response_lower=lo, **kw).log_p(fixed, engine=eng).cpu().numpy()
    assert np.isneginf(lim[1]) and all(lim[c] == base[c] for c in (0, 2, 3))
    eng.close()


def test_cfg5_size_with_positivity():
    """512 chains, n = 5000, n_max = 20, beta >= 0, in-kernel streams, 50 sweeps: every stored live beta >= 0, no NaN
    log_post, and the dimension moves."""
    import torch

    from openmcmc_amd import gmrf
    from openmcmc_amd.engine import Engine
    from openmcmc_amd.mcmc import MCMC
    from rj_problem import build, make_basis_host

    n, n_max, C, S = 5000, 20, 512, 50
    rng = np.random.default_rng(0)
    X = np.linspace(-10, 10, n)
    y = (make_basis_host(X.reshape(n, 1), np.array([[-6.0, -1.0, 4.5]])) @ np.array([[3.0], [2.0], [4.0]])).ravel()
    y = y + 0.05 * np.cumsum(rng.standard_normal(n)) * np.sqrt(48.0 / n) + 0.1 * rng.standard_normal(n)
    P = gmrf.precision_irregular(np.arange(float(n))).tolil()
    P[0, 0] += 1e-3
    k0 = np.clip(rng.poisson(5, size=C), 1, n_max)
    init_theta = [rng.uniform(-10, 10, size=k) for k in k0]
    init_beta = [np.abs(rng.standard_normal(k)) for k in k0]
    eng = Engine(C, seed=2)
    mdl, state, samplers = build(y, X, P.tocsc(), n_max, eng, init_theta, init_beta, k0.astype(float))
    mdl["beta"].domain_response_lower = np.array([[0.0]])
    M = MCMC(state, samplers, model=mdl, n_burn=0, n_iter=S, n_chains=C, seed=2, engine=eng)
    M.run_mcmc()
    torch.cuda.synchronize()
    got = M.collect()
    beta = got["beta"]
    assert np.nanmin(beta) >= 0.0
    assert not np.any(np.isnan(got["log_post"]))
    nb = got["n_basis"].reshape(C, -1)
    assert np.any(nb != nb[:, :1])
    assert samplers[5].accept_rate.accept.cpu().numpy().sum() > 0


def test_per_element_limits_on_a_ragged_parameter_raise():
    """One limit per element has no meaning for a variable-size parameter: NormalNormal.sample and log_p name it."""
    import torch

    from openmcmc_amd.chains import ChainArray, ragged_from_lists
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.engine import Engine
    from openmcmc_amd.parameter import MixtureParameterMatrix, MixtureParameterVector
    from rj_problem import build

    C, n_max = 2, 6
    eng = Engine(C)
    dev = eng.device
    lists = [np.array([1.5, 2.0]), np.array([0.5, 0.9, 3.0])]
    state = {"beta": ragged_from_lists(lists, n_max, 0, "k", dev),
             "alloc": ragged_from_lists([np.zeros(v.size) for v in lists], n_max, 0, "k", dev),
             "k": ChainArray(torch.as_tensor(np.array([2.0, 3.0]), device=dev).reshape(-1, 1, 1)),
             "mu": np.zeros((1, 1)), "prec": np.ones((1, 1))}
    d = Normal("beta", mean=MixtureParameterVector("mu", "alloc"), precision=MixtureParameterMatrix("prec", "alloc"),
               domain_response_lower=np.array([[0.0], [1.0]]))
    with pytest.raises(ValueError, match="beta: a variable-size parameter takes scalar domain limits only"):
        d.log_p(state, engine=eng)

    n = 48
    X = np.linspace(-10, 10, n)
    P = np.diag(np.full(n, 2.0)) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)
    P[0, 0] = P[-1, -1] = 1.001
    y = np.sin(X)
    mdl, st, samplers = build(y, X, P, n_max, eng, [np.array([1.0, 4.0]), np.array([-3.0])], [np.array([0.5, 1.0]), np.array([0.2])],
                              np.array([2.0, 1.0]))
    mdl["beta"].domain_response_lower = np.array([[0.0], [0.0]])
    s_beta = samplers[1]
    s_beta.bind(eng)
    with pytest.raises(ValueError, match="beta: a variable-size parameter takes scalar domain limits only"):
        s_beta.sample(st)
    eng.close()
