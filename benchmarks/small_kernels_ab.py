#!/usr/bin/env python3
"""A/B timing of two builds of libomcmc_hip.so on the small per-chain kernels whose machine code is not byte-identical between
them (profiles/small_kernels_refactor_same_code.txt lists which and why).

    bash benchmarks/build_rev.sh HEAD~1 before
    python3 benchmarks/small_kernels_ab.py [--before build/ab/libomcmc_hip_before.so] [--rounds 5] [--out FILE]

The two builds run alternately -- before, after, before, after, ... -- one fresh process per run, the other build through
OMC_HIP_LIB.  A run is this script's own child (device-event time per launch over back-to-back launches of each entry point, at the
shapes the models use them at) and benchmarks/truncated_mixture.py --kernels-only (the dense truncated scan with a per-chain
diagonal, the ragged scan and the ragged draw).  Per case: the median of either side and the spread (max - min over the rounds) of
the BEFORE side, which is the only measurement of that spread there is; the case passes when the median after is not above the
median before by more than that spread.  Exit status 1 if a case does not pass.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(reps):
    import torch

    from openmcmc_amd.engine import Engine

    def event_us(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / reps

    C, kmax, n = 512, 20, 5000  # cfg5: reversible jump over <= 20 knots, 5000 nodes
    rng = np.random.default_rng(1)
    eng = Engine(C, seed=1)
    t = eng.to_device
    res = {}
    counts = np.clip(rng.poisson(5, size=C), 1, kmax)
    live = np.arange(kmax)[None, :] < counts[:, None]
    gram = np.zeros((C, kmax, kmax))
    for c, k in enumerate(counts):
        A = rng.standard_normal((k + 5, k))
        gram[c, :k, :k] = A.T @ A
    g, rhs, prec, cnt = t(gram), t(rng.standard_normal((C, kmax))), t(0.5 + rng.random((C, kmax))), t(counts.astype(np.float64))
    x = t(rng.standard_normal((C, kmax)) * live)
    res["small_sample_canonical_us"] = event_us(lambda: eng.small_sample_canonical(g, rhs, prec, count=cnt))
    full = t(np.stack([a.T @ a + np.eye(kmax) for a in rng.standard_normal((C, kmax + 5, kmax))]))
    res["small_spd_ops_us"] = event_us(lambda: eng.small_spd_ops(full, x, want_Av=True, want_quad=True, want_logdet=True))
    B, coef = t(rng.standard_normal((C, kmax, n)) * live[:, :, None]), t(rng.standard_normal((C, kmax)) * live)
    B_odd = t(rng.standard_normal((C, kmax, n - 1)) * live[:, :, None])
    add, out = t(rng.standard_normal(n)), eng.empty(C, n)
    res["design_predict_batched_2wide_us"] = event_us(lambda: eng.design_predict_batched(B, coef, add_shared=add, out=out))
    out_odd = eng.empty(C, n - 1)
    res["design_predict_batched_1wide_us"] = event_us(lambda: eng.design_predict_batched(B_odd, coef, add_shared=add[: n - 1].contiguous(), out=out_odd))
    lp = eng.empty(C)
    res["diag_gauss_logpdf_us"] = event_us(lambda: eng.diag_gauss_logpdf(x, prec, lp, count=cnt))
    res["diag_gauss_logpdf_limits_us"] = event_us(lambda: eng.diag_gauss_logpdf_limits(x, prec, lp, lower=-10.0, count=cnt))
    eng.check_status()
    eng.close()
    C, p = 256, 500  # the mixture regression: 500 coefficients
    eng = Engine(C, seed=2)
    t = eng.to_device
    y = t(rng.standard_normal((C, p)))
    prior, mean, pr = t(np.array([[0.3, 0.7]])), t(np.zeros(2)), t(np.array([100.0, 0.25]))
    res["mixture_allocation_us"] = event_us(lambda: eng.mixture_allocation(y, prior, mean, pr, draw_index=1))
    prec_p, lp = t(0.5 + rng.random((C, p))), eng.empty(C)
    res["diag_gauss_logpdf_p500_us"] = event_us(lambda: eng.diag_gauss_logpdf(y, prec_p, lp))
    res["diag_gauss_logpdf_limits_p500_us"] = event_us(lambda: eng.diag_gauss_logpdf_limits(y, prec_p, lp, lower=-10.0))
    res["log_transform_us"] = event_us(lambda: eng.log_transform(prec_p))
    M = t(np.eye(p))
    yM, q = eng.design_predict(M, y), eng.empty(C)
    from openmcmc_amd._abi import check, lib
    res["centered_rowdot_us"] = event_us(lambda: check(lib.omc_centered_rowdot(eng._ctx, p, eng._p(y, C, p), y.stride(0), None, eng._p(yM, C, p),
                                                                              yM.stride(0), None, eng._p(q))))
    Xd = rng.standard_normal((800, p))
    T = eng.dense_terms([{"mat": t(Xd.T @ Xd), "rhs": t(Xd.T @ rng.standard_normal(800))}], p)
    xs, lower = t(np.abs(rng.standard_normal((C, p)))), t(np.zeros(p))
    reps = max(reps // 20, 5)
    res["dense_gibbs_truncated_plain_us"] = event_us(lambda: eng.dense_gibbs_truncated(p, T, xs, lower=lower))
    eng.check_status()
    eng.close()
    print(json.dumps(res))


def flat(node, path=""):
    """{case: value} of the timings (keys ending in _us or _ms) of a JSON line"""
    found = {}
    for k, v in node.items():
        if isinstance(v, dict):
            found.update(flat(v, f"{path}{k}/"))
        elif isinstance(v, (int, float)) and (k.endswith("_us") or k.endswith("_ms")):
            found[f"{path}{k}"] = float(v)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", default="build/ab/libomcmc_hip_before.so")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps)
    sink = open(args.out, "a") if args.out else None

    def say(text):
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    runs = [("small_kernels_ab.py", [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]),
            ("truncated_mixture.py --kernels-only", [sys.executable, os.path.join(ROOT, "benchmarks", "truncated_mixture.py"), "--kernels-only", "--reps", str(args.reps)])]
    val = {"before": {}, "after": {}}
    for r in range(args.rounds):
        for side in ("before", "after"):
            env = dict(os.environ)
            env.pop("OMC_HIP_LIB", None)
            if side == "before":
                env["OMC_HIP_LIB"] = os.path.join(ROOT, args.before)
            for label, cmd in runs:
                run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
                if run.returncode != 0 or not lines:
                    say(f"{label} round {r} {side}: status {run.returncode}\n{run.stderr[-1500:]}")
                    return 2
                for k, v in flat(json.loads(lines[-1])).items():
                    val[side].setdefault(k, []).append(v)
    failed = 0
    say(f"before = {args.before}, after = the in-tree build; {args.rounds} rounds, before and after alternately, a fresh process per run")
    say(f"  {'case (time per launch)':<56s} {'before':>10s} {'spread':>10s} {'after':>10s} {'spread':>10s}  verdict")
    for k, b in val["before"].items():
        a = val["after"][k]
        mb, ma, spread = statistics.median(b), statistics.median(a), max(b) - min(b)
        ok = ma <= mb + spread
        failed += not ok
        say(f"  {k:<56s} {mb:10.3f} {spread:10.3f} {ma:10.3f} {max(a) - min(a):10.3f}  {'pass' if ok else 'FAIL'}")
    say(f"{failed} cases fail")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
