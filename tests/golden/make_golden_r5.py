"""Golden vectors for truncated mixture priors (a mixture prior on coefficients with a domain limit: the spike-and-slab
prior on non-negative coefficients), made by RUNNING the reference (openMCMC v1.0.7) in the build container:

    PYTHONPATH=/root/reference/src python3 tests/golden/make_golden_r5.py

Writes truncated_mixture.npz and rj_truncated_chain.npz (pass names to regenerate a subset).  Fixtures hold data only:
inputs, the draws the reference consumed and what it produced.  truncnorm.rvs(a, b, loc, scale) is recorded as the uniform
u behind it (value = truncnorm.ppf(u, a, b) * scale + loc), as in make_golden_r2.gen_band_truncated.
"""

import os
import sys

import numpy as np
from scipy import stats

REF_SRC = "/root/reference/src"
if REF_SRC not in sys.path:
    sys.path.insert(0, REF_SRC)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden_rj import Tape, chain_init, rj_gmrf_problem, run_reference_chain  # noqa: E402
from openmcmc import parameter  # noqa: E402
from openmcmc.distribution.distribution import Categorical, Gamma  # noqa: E402
from openmcmc.distribution.location_scale import Normal  # noqa: E402
from openmcmc.mcmc import MCMC  # noqa: E402
from openmcmc.model import Model  # noqa: E402
from openmcmc.sampler.sampler import MixtureAllocation, NormalGamma, NormalNormal  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def gen_truncated_mixture():
    """The mixture-prior regression of make_golden_rj.gen_mixture_chain (K = 3 components, NormalGamma on the component
    precisions, MixtureAllocation, 40 sweeps) with domain_response_lower = 0 on the coefficients: NormalNormal takes
    gmrf.gibbs_canonical_truncated_normal.  Component means -2, 0, 1.5: under the first two the limit binds."""
    rng = np.random.default_rng(5)
    n, p_, K, n_iter = 40, 7, 3, 40
    X = rng.standard_normal((n, p_))
    st = {"response": rng.standard_normal((n, 1)), "prefactor_matrix": X, "parameter": np.abs(rng.standard_normal((p_, 1))),
          "prior_mean": np.array([[-2.0], [0.0], [1.5]]), "precision_matrix": np.diag(rng.random(n) + 0.5),
          "prior_precision_vector": 0.5 + rng.random(K), "gamma_shape": 2.0 * np.ones((K,)), "gamma_rate": 1.0 * np.ones((K,)),
          "allocation": rng.integers(0, K, size=(p_, 1)), "prior_allocation_prob": np.array([[0.3, 0.4, 0.3]])}
    out = {"n": n, "p": p_, "K": K, "n_iter": n_iter, "X": X, "y": st["response"].ravel(), "w": np.diag(st["precision_matrix"]).copy(),
           "parameter0": st["parameter"].ravel().copy(), "prior_mean": st["prior_mean"].ravel(), "prec0": np.asarray(st["prior_precision_vector"]).ravel(),
           "alloc0": st["allocation"].ravel().astype(float), "prob": st["prior_allocation_prob"], "lower": 0.0}
    mdl = Model([
        Normal("response", mean=parameter.LinearCombination({"parameter": "prefactor_matrix"}), precision=parameter.Identity("precision_matrix")),
        Normal("parameter", mean=parameter.MixtureParameterVector("prior_mean", "allocation"),
               precision=parameter.MixtureParameterMatrix("prior_precision_vector", "allocation"),
               domain_response_lower=np.array([[0.0]])),
        Gamma("prior_precision_vector", shape=parameter.Identity("gamma_shape"), rate=parameter.Identity("gamma_rate")),
        Categorical("allocation", prob="prior_allocation_prob")])
    samplers = [NormalNormal("parameter", mdl), NormalGamma("prior_precision_vector", mdl),
                MixtureAllocation("allocation", mdl, response_param="parameter")]
    # (parameter0 is a copy: the truncated scan updates the state's array in place, gmrf.py:264)
    rd = np.random.default_rng(62)
    ts, gs, us, binds = [], [], [], []

    def _trunc(a, b, loc=0, scale=1, size=None, **_):
        u = rd.random(size)
        ts.append(float(np.asarray(u).reshape(-1)[0]))
        binds.append(float(np.asarray(a).reshape(-1)[0]) > -2.0)  # the limit is within two sd of the conditional mean
        return stats.truncnorm.ppf(u, a, b) * scale + loc

    def _gamma(a, loc=0, scale=1, size=None, **_):
        g = rd.standard_gamma(np.asarray(a, dtype=np.float64), size=size)
        gs.append(np.asarray(g, dtype=float).reshape(-1))
        return loc + g * scale

    def _uniform(loc=0, scale=1, size=None, **_):
        u = rd.random(size)
        us.append(np.asarray(u, dtype=float).reshape(-1))
        return loc + u * scale

    def _norm(*a, **k):
        raise RuntimeError("no normal draw expected")

    saved = (stats.norm.rvs, stats.gamma.rvs, stats.uniform.rvs, stats.truncnorm.rvs)
    stats.norm.rvs, stats.gamma.rvs, stats.uniform.rvs, stats.truncnorm.rvs = _norm, _gamma, _uniform, _trunc
    try:
        M = MCMC(st, samplers, model=mdl, n_burn=0, n_iter=n_iter)
        M.run_mcmc()
    finally:
        stats.norm.rvs, stats.gamma.rvs, stats.uniform.rvs, stats.truncnorm.rvs = saved
    out["u_trunc"] = np.array(ts).reshape(n_iter, p_)
    out["g"], out["u"] = np.array(gs), np.array(us)
    for key in ("parameter", "prior_precision_vector", "allocation", "log_post"):
        out["store_" + key] = np.asarray(M.store[key], dtype=float)
    print("allocation counts", np.bincount(M.store["allocation"].astype(int).ravel(), minlength=K),
          "share of sites with the limit within 2 sd", np.mean(binds), "min draw", np.min(M.store["parameter"]))
    np.savez_compressed(os.path.join(OUT, "truncated_mixture.npz"), **out)


class TruncTape(Tape):
    """make_golden_rj.Tape with the uniforms of the coefficients' truncated scan recorded per site (u_beta)."""

    def new_sweep(self):
        super().new_sweep()
        self.cur["u_beta"] = np.full(self.n_max, np.nan)
        self._site = 0

    def truncnorm(self, a, b, loc=0, scale=1, size=None, **_):
        if self.where != "beta":
            return super().truncnorm(a, b, loc=loc, scale=scale, size=size)
        u = self.rng.random(size)
        self.cur["u_beta"][self._site] = float(np.asarray(u).reshape(-1)[0])
        self._site += 1
        return stats.truncnorm.ppf(u, a, b) * scale + loc


def gen_rj_truncated_chain():
    """make_golden_rj.gen_rj_gmrf_chain (cfg5 shape: n = 48, n_max = 6, five chains with different k0, 150 sweeps) with
    beta >= 0 (domain_response_lower = 0 on its mixture prior): the tape, the MH internals per sweep, the store."""
    n, n_max, n_iter = 48, 6, 150
    mdl, shared, make_samplers = rj_gmrf_problem(n, n_max, seed=2)
    mdl["beta"].domain_response_lower = np.array([[0.0]])
    out = {"n": n, "n_max": n_max, "n_iter": n_iter, "y": shared["y"].ravel(), "X": shared["X"].ravel(), "lower": 0.0}
    P = shared["P_lambda"].toarray()
    out["P_diag"], out["P_off"] = np.diag(P).copy(), np.diag(P, -1).copy()
    inits = (1, 3, 5, 6, 2)
    per_chain = []
    for c, k0 in enumerate(inits):
        rng = np.random.default_rng(900 + c)
        st = chain_init(shared, k0, rng)
        st["beta"] = np.abs(st["beta"])
        init = {"theta": np.full(n_max, np.nan), "beta": np.full(n_max, np.nan)}
        init["theta"][:k0], init["beta"][:k0] = st["theta"].ravel(), st["beta"].ravel()
        tape = TruncTape(4000 + c, n, n_max)
        samplers = make_samplers()
        M = run_reference_chain(mdl, st, samplers, tape, n_iter)
        rec = {"init_theta": init["theta"], "init_beta": init["beta"], "init_k": float(k0)}
        for key in tape.rows[0]:
            rec["tape_" + key] = np.array([row[key] for row in tape.rows])
        # (the fitted mean M.store["y"] = B beta + b is left out: it follows from the stored b, beta and theta, and with it
        #  the file would exceed 1 MiB)
        for key in ("b", "beta", "lambda", "tau", "theta", "n_basis", "log_post"):
            rec["store_" + key] = np.asarray(M.store[key])
        rec["accept_rw"] = np.array([samplers[4].accept_rate.count["accept"], samplers[4].accept_rate.count["proposal"]], dtype=float)
        rec["accept_rj"] = np.array([samplers[5].accept_rate.count["accept"], samplers[5].accept_rate.count["proposal"]], dtype=float)
        per_chain.append(rec)
        print("chain", c, "k0", k0, "n_basis visits", np.unique(M.store["n_basis"]), samplers[4].accept_rate.get_acceptance_rate(),
              samplers[5].accept_rate.get_acceptance_rate(), "min beta", np.nanmin(M.store["beta"]),
              "rejected jumps with -inf", int(np.sum(np.isneginf(rec["tape_rj_log_accept"]))))
    for key in per_chain[0]:
        out[key] = np.stack([rec[key] for rec in per_chain])
    np.savez_compressed(os.path.join(OUT, "rj_truncated_chain.npz"), **out)


GENERATORS = {"truncated_mixture": gen_truncated_mixture, "rj_truncated_chain": gen_rj_truncated_chain}

if __name__ == "__main__":
    which = sys.argv[1:] or list(GENERATORS)
    for name in which:
        GENERATORS[name]()
        print(name + ".npz", os.path.getsize(os.path.join(OUT, name + ".npz")))
