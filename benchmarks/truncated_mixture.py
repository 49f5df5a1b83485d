"""Cost of truncated mixture priors (omc_truncmix.hip, omc_trunc_dense.h).  Prints one JSON line with
  * cfg5 (reversible jump over Gaussian-kernel knots next to a GMRF, n = 5000, n_max = 20, 512 chains) in ms per sweep,
    with and without beta >= 0 on the coefficients' mixture prior;
  * omc_small_gibbs_truncated next to omc_small_sample_canonical at C = 512, kmax = 20 (in-kernel streams, live counts
    ~ Poisson(5) clipped to [1, 20] as in cfg5, and all 20), per launch;
  * omc_dense_gibbs_truncated with a per-chain diagonal at the mixture_chain shape scaled to p = 500, 256 chains.
Kernel times are device-event times over back-to-back launches; rocprofv3 --kernel-trace --stats gives the per-kernel
split (profiles/README.md).

python benchmarks/truncated_mixture.py [--steps 20 --warmup 3 --reps 200] [--kernels-only]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import argparse  # noqa: E402
import json  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--kernels-only", action="store_true")
a = ap.parse_args()

from openmcmc_amd.engine import Engine  # noqa: E402


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def cfg5_ms_per_sweep(positive):
    from openmcmc_amd import gmrf
    from openmcmc_amd.mcmc import MCMC
    from rj_problem import build, make_basis_host

    n, n_max, C = 5000, 20, 512
    rng = np.random.default_rng(0)
    X = np.linspace(-10, 10, n)
    y = (make_basis_host(X.reshape(n, 1), np.array([[-6.0, -1.0, 4.5]])) @ np.array([[3.0], [-2.0], [4.0]])).ravel()
    y = y + 0.05 * np.cumsum(rng.standard_normal(n)) * np.sqrt(48.0 / n) + 0.1 * rng.standard_normal(n)
    P = gmrf.precision_irregular(np.arange(float(n))).tolil()
    P[0, 0] += 1e-3
    k0 = np.clip(rng.poisson(5, size=C), 1, n_max)
    init_theta = [rng.uniform(-10, 10, size=k) for k in k0]
    init_beta = [np.abs(rng.standard_normal(k)) for k in k0]
    eng = Engine(C, seed=1)
    mdl, state, samplers = build(y, X, P.tocsc(), n_max, eng, init_theta, init_beta, k0.astype(float))
    if positive:
        mdl["beta"].domain_response_lower = np.array([[0.0]])
    M = MCMC(state, samplers, model=mdl, n_burn=a.warmup, n_iter=a.steps, n_chains=C, seed=1, engine=eng)
    n_iter = M.n_iter
    M.n_iter = 0
    M.run_mcmc()
    torch.cuda.synchronize()
    M.n_burn, M.n_iter = 0, n_iter
    t0 = time.perf_counter()
    M.run_mcmc()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    out = {"ms_per_sweep": 1e3 * dt, "accept_n_basis": samplers[5].accept_rate.acceptance_rate,
           "n_basis_mean": float(M.store["n_basis"][:, :, 0].mean().item())}
    eng.close()
    return out


def small_kernels():
    C, kmax = 512, 20
    rng = np.random.default_rng(3)
    eng = Engine(C, seed=2)
    t = eng.to_device
    res = {}
    for label, counts in (("cfg5_counts", np.clip(rng.poisson(5, size=C), 1, kmax)), ("full", np.full(C, kmax))):
        gram = np.zeros((C, kmax, kmax))
        for c, k in enumerate(counts):
            A = rng.standard_normal((k + 5, k))
            gram[c, :k, :k] = A.T @ A
        g, rhs = t(gram), t(rng.standard_normal((C, kmax)))
        prec, pmean = t(np.where(rng.random((C, kmax)) < 0.5, 100.0, 0.25)), t(np.zeros((C, kmax)))  # spike and slab
        tau, cnt = t(np.full(C, 10.0)), t(counts.astype(np.float64))
        x = t(np.abs(rng.standard_normal((C, kmax))))
        ms_can = event_ms(lambda: eng.small_sample_canonical(g, rhs, prec, lik_scale=tau, prior_mean=pmean, count=cnt), a.reps)
        ms_tr = event_ms(lambda: eng.small_gibbs_truncated(g, rhs, prec, x, lower=0.0, lik_scale=tau, prior_mean=pmean,
                                                           count=cnt), a.reps)
        eng.check_status()
        res[label] = {"small_sample_canonical_us": 1e3 * ms_can, "small_gibbs_truncated_us": 1e3 * ms_tr,
                      "ratio": ms_tr / ms_can, "share_at_limit": float((x.cpu().numpy() < 1e-3).mean())}
    eng.close()
    return res


def dense_diag_kernel():
    C, p = 256, 500
    rng = np.random.default_rng(4)
    eng = Engine(C, seed=3)
    t = eng.to_device
    Xd = rng.standard_normal((800, p))
    terms = [{"mat": t(Xd.T @ Xd), "rhs": t(Xd.T @ rng.standard_normal(800))}]
    d = t(np.array([0.5, 2.0, 1.0])[rng.integers(0, 3, size=(C, p))])
    rc = t(rng.standard_normal((C, p)))
    lower = t(np.zeros(p))
    x = t(np.abs(rng.standard_normal((C, p))))
    T = eng.dense_terms(terms, p)
    ms = event_ms(lambda: eng.dense_gibbs_truncated(p, T, x, lower=lower, rhs_chain=rc, diag_chain=d), max(a.reps // 20, 5))
    eng.check_status()
    eng.close()
    return {"dense_gibbs_truncated_diag_ms": ms, "chains": C, "p": p}


out = {"workload": "truncated mixture priors", "small": small_kernels(), "dense": dense_diag_kernel()}
if not a.kernels_only:
    plain, pos = cfg5_ms_per_sweep(False), cfg5_ms_per_sweep(True)
    out["cfg5"] = {"plain": plain, "beta_nonneg": pos, "ratio": pos["ms_per_sweep"] / plain["ms_per_sweep"]}
print(json.dumps(out))
