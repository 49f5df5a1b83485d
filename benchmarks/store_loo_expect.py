#!/usr/bin/env python3
"""PSIS-LOO expectations of the device store (omc_store_loo_expect) beside omc_store_psis on the same columns (the yardstick: the
same gather, sort and fit, and no pass over the draws), omc_store_loglik over the same bytes (the yardstick of the expectation
pass alone: the same loads and one exp per element) and the torch expression of the same sums from a gathered ll and f.

    python3 benchmarks/store_loo_expect.py [--reps 7] [--iters 128] [--chains 1024] [--nodes 10000] [--index 512]

Prints a table and one JSON line.  One process on one card; every device time is the median of --reps calls timed one by one with
device events after a warm-up call, with the smallest and largest beside it.  --index indexed nodes of the --iters x --chains x
--nodes store, one stored precision per draw, tails of ceil(min(S / 5, 3 sqrt(S))) draws.
  The expectation pass alone is the new call with tails of ONE draw (nothing to fit, nothing smoothed, no draw bisects) less
  omc_store_psis with tails of one draw (gather, sort and the fit kernel's final sums); what the tail draws add -- the bisection of
  the sorted column and the smoothed value made again per draw -- is the rest of the difference to the full call.
  The torch route computes, from the gathered mean entry, ll, the self-normalised weights exp(-ll - max(-ll)) and the weighted
  mean, variance, effective sample size and mean of 1 / tau: what the new call with tails of one draw computes (it is checked against
  it), not the Pareto smoothing, for which torch has no expression.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=128)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--index", type=int, default=512)
    args = ap.parse_args()
    import torch

    from openmcmc_amd.engine import Engine

    def timed(fn):
        """(median, min, max) ms of --reps calls, each between its own pair of device events, after one warm-up call"""
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    n_iter, C, size, n = args.iters, args.chains, args.nodes, args.index
    S = n_iter * C
    eng = Engine(C, seed=3)
    g = torch.Generator(device=eng.device)
    g.manual_seed(6)
    shift = torch.linspace(-1, 1, size, dtype=torch.float64, device=eng.device)
    x = torch.empty((n_iter, C, size), dtype=torch.float64, device=eng.device)
    for i in range(n_iter):  # (slab by slab: no second store-sized temporary)
        x[i] = torch.randn((C, size), generator=g, dtype=torch.float64, device=eng.device) + shift
    y = torch.randn(size, generator=g, dtype=torch.float64, device=eng.device)
    prec = torch.rand((n_iter, C, 1), generator=g, dtype=torch.float64, device=eng.device) + 0.5
    idx = torch.arange(size // 4, size // 4 + n, device=eng.device)
    yi = y[idx].contiguous()
    rep = x[:, :, size // 4: size // 4 + n] + torch.randn((n_iter, C, n), generator=g, dtype=torch.float64, device=eng.device) / prec.sqrt()
    rec = {"store": f"{n_iter} iterations x {C} chains x {size}", "store_GB": 8.0 * S * size / 1e9, "index": n, "reps": args.reps, "rows": []}
    print(f"{rec['store']} ({rec['store_GB']:.2f} GB), {n} indexed nodes", flush=True)

    def row(label, t, base=None, what="omc_store_psis"):
        ms, lo, hi = t
        r = {"case": label, "ms": ms, "ms_min": lo, "ms_max": hi}
        text = f"  {label:<92s} {ms:10.3f} ms [{lo:9.3f} .. {hi:9.3f}]"
        if base is not None:
            r["ratio"] = ms / base
            text += f"   x{ms / base:5.2f} of {what}"
        rec["rows"].append(r)
        print(text, flush=True)
        return ms

    tail = int(min(S - 1, np.ceil(min(S / 5.0, 3.0 * np.sqrt(S)))))
    moments = ("mean", "var", "ess", "invprec", "k", "tail")
    kw = dict(index=idx, y=yi, prec=prec)
    t_psis = row(f"omc_store_psis from the mean entry, tails of {tail} (yardstick)", timed(lambda: eng.store_psis(x, tail, **kw)))
    t_psis1 = row("omc_store_psis the same with tails of 1 draw (no fit)", timed(lambda: eng.store_psis(x, 1, **kw)))
    t_ll = row("omc_store_loglik lse + mean + var over the same columns (yardstick of the pass)", timed(lambda: eng.store_loglik(x, yi, prec, index=idx)))
    t_full = row(f"omc_store_loo_expect f = mean: mean, var, ess, invprec, k, tail; tails of {tail}",
                 timed(lambda: eng.store_loo_expect(x, tail, f="mean", want=moments, **kw)), t_psis)
    t_one = row("omc_store_loo_expect the same with tails of 1 draw (no fit, no draw bisects)",
                timed(lambda: eng.store_loo_expect(x, 1, f="mean", want=moments, **kw)), t_psis1, "omc_store_psis with tails of 1")
    t_lw = row(f"omc_store_loo_expect the same with lw_out written ({8.0 * S * n / 1e9:.2f} GB), tails of {tail}",
               timed(lambda: eng.store_loo_expect(x, tail, f="mean", want=moments, lw=True, **kw)), t_psis)
    row(f"omc_store_loo_expect f = cdf: mean (the analytic LOO-PIT), tails of {tail}",
        timed(lambda: eng.store_loo_expect(x, tail, f="cdf", want=("mean",), **kw)), t_psis)
    row(f"omc_store_loo_expect f = entry of replicates: below (az.loo_pit), tails of {tail}",
        timed(lambda: eng.store_loo_expect(x, tail, f="entry", values=rep, threshold=yi, want=("below",), **kw)), t_psis)
    row(f"omc_store_loo_expect lw_out alone (az.psislw), tails of {tail}",
        timed(lambda: eng.store_loo_expect(x, tail, f="mean", want=(), lw=True, **kw)), t_psis)

    def by_torch():
        sel = x.view(S, size).index_select(1, idx)
        tau = prec.view(S, 1)
        v = -(0.5 * torch.log(tau) - 0.9189385332046727 - 0.5 * tau * (yi - sel) ** 2)
        w = torch.exp(v - v.max(dim=0).values)
        W = w.sum(dim=0)
        mean = (w * sel).sum(dim=0) / W
        return mean, (w * (sel - mean) ** 2).sum(dim=0) / W, W * W / (w * w).sum(dim=0), (w / tau).sum(dim=0) / W

    t_torch = row("torch: the same sums with self-normalised weights from the gathered mean entry", timed(by_torch), t_one,
                  "omc_store_loo_expect with tails of 1")
    got = eng.store_loo_expect(x, 1, f="mean", want=moments, **kw)
    for a, name in zip(by_torch(), ("mean", "var", "ess", "invprec")):
        assert float((got[name] - a).abs().max()) <= 1e-9 * max(1.0, float(a.abs().max())), name
    rec.update({"ratio_to_psis": t_full / t_psis, "pass_alone_ms": t_one - t_psis1, "pass_alone_to_loglik": (t_one - t_psis1) / t_ll,
                "tail_draws_ms": (t_full - t_one) - (t_psis - t_psis1), "lw_out_ms": t_lw - t_full, "torch_to_call_with_tails_of_1": t_torch / t_one,
                "torch_to_pass_alone": t_torch / (t_one - t_psis1)})
    print(f"  omc_store_loo_expect / omc_store_psis = {rec['ratio_to_psis']:.2f}; the expectation pass alone {rec['pass_alone_ms']:.3f} ms = "
          f"{rec['pass_alone_to_loglik']:.2f} of omc_store_loglik over the same bytes; the tail draws add {rec['tail_draws_ms']:.3f} ms; "
          f"lw_out costs {rec['lw_out_ms']:.3f} ms", flush=True)
    print(f"  torch route / new call with tails of 1 = {rec['torch_to_call_with_tails_of_1']:.2f} (gather and sort included in the call); "
          f"torch route / expectation pass alone = {rec['torch_to_pass_alone']:.2f}", flush=True)
    eng.check_status()
    eng.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
