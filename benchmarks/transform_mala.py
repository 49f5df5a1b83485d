"""Time per ManifoldMALA step on an exp-transformed parameter (LinearCombinationWithTransform), C = 1024 chains, n = 2000 rows:

  fused     ManifoldMALA(fused=True): one omc_mala_transform_step per step
  general   ManifoldMALA(fused=False): analytic per-chain Hessians (omc_transform_grad_hess), then launch by launch
  baseline  the calls the launch-by-launch route issued for a per-chain Hessian before this feature, on a fixed Lambda and
            gradient: omc_small_spd_ops x 4, omc_small_sample_canonical x 2 and the tensor glue between them.  It leaves out the
            gradient / Hessian evaluations and the accept step, so it is a lower bound of what a step cost.

Events around STEPS steps after a warm-up, REPEATS repeats with the three arms interleaved in one process; medians and the
spread (max - min) of the repeats.  Prints one JSON line per p.

    python benchmarks/transform_mala.py [--steps 200] [--repeats 5] [--p 16 32 64]
"""

import argparse
import json
import os
import sys

import numpy as np
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def setup(p, C, n, fused, seed=7):
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.engine import Engine
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombinationWithTransform, ScaledMatrix
    from openmcmc_amd.sampler.metropolis_hastings import ManifoldMALA

    rng = np.random.default_rng(p)
    A = (rng.random((n, p)) + 0.1) * (rng.random((n, p)) < max(0.15, 2.0 / p))
    A[np.arange(n), np.arange(n) % p] += 0.5
    truth = 0.3 * rng.standard_normal(p)
    w = 40.0 * (rng.random(n) + 0.5)
    y = A @ np.exp(truth) + rng.standard_normal(n) / np.sqrt(w)
    R = rng.standard_normal((p, 2 * p))
    P0 = R @ R.T / (2 * p) + 0.5 * np.eye(p)
    eng = Engine(C, seed=seed)
    lik = Normal("y", mean=LinearCombinationWithTransform(form={"s": "A"}, transform={"s": True}), precision=ScaledMatrix("W", "tau"))
    mdl = Model([lik, Normal("s", mean="m0", precision="P0")])
    x0 = truth[None, :] + 0.01 * rng.standard_normal((C, p))
    state = {"A": A, "y": y.reshape(n, 1), "s": ChainArray(eng.to_device(x0)), "W": sparse.diags(w, format="csc"),
             "tau": ChainArray(eng.full((C, 1, 1), 1.0)), "m0": np.full((p, 1), 0.1), "P0": 0.5 * (P0 + P0.T)}
    smp = ManifoldMALA("s", mdl, step=np.array(0.5), fused=fused).bind(eng)
    return eng, smp, state


def baseline_step(eng, Lam, xv, grad, zero):
    """The launch sequence of the per-chain-Hessian route (metropolis_hastings.py:325-373) without its model evaluations."""
    from openmcmc_amd.sampler.metropolis_hastings import _lin

    Cn, d = xv.shape
    Lx, _, logdet_f = eng.small_spd_ops(Lam, xv, want_Av=True, want_logdet=True)
    mu_f = eng.empty(Cn, d)
    xp = eng.small_sample_canonical(Lam, _lin(eng, 1.0, Lx, 0.5, grad), zero, mean_out=mu_f)
    _, quad_f, _ = eng.small_spd_ops(Lam, _lin(eng, 1.0, xp, -1.0, mu_f), want_quad=True)
    lq_f = _lin(eng, 0.5, logdet_f, -0.5, quad_f)
    Lxp, _, logdet_r = eng.small_spd_ops(Lam, xp, want_Av=True, want_logdet=True)
    mu_r = eng.empty(Cn, d)
    eng.small_sample_canonical(Lam, _lin(eng, 1.0, Lxp, 0.5, grad), zero, z=zero, mean_out=mu_r)
    _, quad_r, _ = eng.small_spd_ops(Lam, _lin(eng, 1.0, xv, -1.0, mu_r), want_quad=True)
    return lq_f, _lin(eng, 0.5, logdet_r, -0.5, quad_r)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--p", type=int, nargs="+", default=[16, 32, 64])
    args = ap.parse_args()
    for p in args.p:
        arms = {}
        for name, fused in (("fused", True), ("general", False)):
            eng, smp, state = setup(p, args.chains, args.rows, fused)
            arms[name] = (eng, smp, state)
        eng_b, smp_b, state_b = setup(p, args.chains, args.rows, False)
        grad, H = smp_b._grad_hess_per_chain(state_b)
        Lam, xv, zero = (H / 0.25).contiguous(), state_b["s"].vector().contiguous(), eng_b.zeros(args.chains, p)

        def run(name, k):
            if name == "baseline":
                for _ in range(k):
                    baseline_step(eng_b, Lam, xv, grad, zero)
                return
            eng, smp, state = arms[name]
            for _ in range(k):
                state = smp.sample(state)
            arms[name] = (eng, smp, state)

        times = {name: [] for name in ("fused", "general", "baseline")}
        for name in times:
            run(name, args.warmup)
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for name in times:  # interleaved
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run(name, args.steps)
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / args.steps)
        for eng, _, _ in list(arms.values()) + [(eng_b, None, None)]:
            eng.check_status()
        rec = {"p": p, "chains": args.chains, "rows": args.rows, "steps": args.steps, "repeats": args.repeats,
               "accept_rate_fused": arms["fused"][1].accept_rate.acceptance_rate}
        for name, ts in times.items():
            rec[name + "_us_per_step_median"] = float(np.median(ts))
            rec[name + "_us_per_step_spread"] = float(max(ts) - min(ts))
        rec["fused_wins"] = bool(max(times["fused"]) < min(times["baseline"]))
        print(json.dumps(rec), flush=True)
        for eng, _, _ in list(arms.values()) + [(eng_b, None, None)]:
            eng.close()


if __name__ == "__main__":
    main()
