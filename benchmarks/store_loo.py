#!/usr/bin/env python3
"""Pointwise log-likelihood summaries and PSIS-LOO of the device store (omc_store_loglik, omc_store_psis) beside the project's own
one-read pass over the same bytes (omc_store_moments), the torch expression a user would write on the device (torch.logsumexp
plus var, store-sized temporaries included) and transfer plus numpy on the host.

    python3 benchmarks/store_loo.py [--reps 7] [--iters 128] [--chains 1024] [--nodes 10000] [--index 512] [--host-nodes 64]

Prints a table and one JSON line.  One process on one card; every device time is the median of --reps calls timed one by one with
device events after a warm-up call, with the smallest and largest beside it.  Bytes and exp counts come from the shapes: one read of
the selected elements (8 S n_idx bytes) and one exp per element (S n_idx).  Whether the pass is bound by HBM or by the vector ALU is
read off two numbers: its time against omc_store_moments over the same bytes (the same loads, no exp), and against itself with the
pointwise entry written as well (twice the bytes, the same exp).
  loglik  all --nodes elements and --index indexed nodes of the --iters x --chains x --nodes store, one stored precision per draw;
          the host route (transfer + numpy) on --host-nodes indexed nodes, scaled by the element count in the table.
  psis    --index indexed nodes beside omc_store_ranks on the same columns (the same gather and sort); the fit kernel's share is
          the difference to a call whose tails are one draw long (nothing to fit: gather, sort and the final sums only).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=128)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--index", type=int, default=512)
    ap.add_argument("--host-nodes", type=int, default=64)
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

    n_iter, C, size = args.iters, args.chains, args.nodes
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
    idx = torch.arange(size // 4, size // 4 + args.index, device=eng.device)
    rec = {"store": f"{n_iter} iterations x {C} chains x {size}", "store_GB": 8.0 * S * size / 1e9, "reps": args.reps, "rows": []}
    print(f"{rec['store']} ({rec['store_GB']:.2f} GB)", flush=True)

    def row(label, t, n_elem=None, base=None, exps=True):
        ms, lo, hi = t
        r = {"case": label, "ms": ms, "ms_min": lo, "ms_max": hi}
        text = f"  {label:<78s} {ms:10.3f} ms [{lo:9.3f} .. {hi:9.3f}]"
        if n_elem:
            r["TB_per_s"] = 8.0 * n_elem / (ms * 1e-3) / 1e12
            text += f" {r['TB_per_s']:6.2f} TB/s read"
            if exps:
                r["Gexp_per_s"] = n_elem / (ms * 1e-3) / 1e9
                text += f" {r['Gexp_per_s']:7.1f} Gexp/s"
        if base is not None:
            r["ratio_to_moments"] = ms / base
            text += f"   x{ms / base:5.2f} of moments"
        rec["rows"].append(r)
        print(text, flush=True)
        return ms

    def by_torch(index):
        sel = x.view(S, size) if index is None else x.view(S, size).index_select(1, index)
        yy = y if index is None else y[index]
        tau = prec.view(S, 1)
        ll = 0.5 * torch.log(tau) - 0.9189385332046727 - 0.5 * tau * (yy - sel) ** 2
        return torch.logsumexp(ll, dim=0), ll.var(dim=0)

    # ---- omc_store_loglik
    for label, index, n in ((f"all {size} elements", None, size), (f"{args.index} indexed nodes", idx, args.index)):
        yy = y if index is None else y[index]
        sub = x if index is None else x[:, :, size // 4: size // 4 + args.index].contiguous()
        t_mom = row(f"omc_store_moments pooled, {label} (yardstick: one read, no exp)", timed(lambda: eng.store_moments(sub, pooled=True)),
                    S * n, exps=False)
        row(f"omc_store_loglik lse + mean + var, {label}", timed(lambda: eng.store_loglik(x, yy, prec, index=index)), S * n, t_mom)
        if index is not None or 8.0 * S * n <= 16e9:
            row(f"omc_store_loglik the same with ll_out written, {label}",
                timed(lambda: eng.store_loglik(x, yy, prec, index=index, ll=True)), S * n, t_mom)
        try:
            row(f"torch logsumexp + var, {label}", timed(lambda: by_torch(index)), S * n, t_mom)
            a, b = by_torch(index)
            lse, _, var, _ = eng.store_loglik(x, yy, prec, index=index)
            assert float((lse - a).abs().max()) <= 1e-9 * float(a.abs().max()) and float((var - b).abs().max()) <= 1e-9 * float(b.abs().max())
            del a, b
        except torch.OutOfMemoryError:
            print(f"  torch logsumexp + var, {label}: out of memory (store-sized temporaries)", flush=True)
        torch.cuda.empty_cache()
    # transfer + numpy on the host, on a few nodes
    hn = min(args.host_nodes, args.index)
    t0 = time.perf_counter()
    hx = x[:, :, size // 4: size // 4 + hn].contiguous().cpu().numpy().reshape(S, hn)
    ht = prec.cpu().numpy().reshape(S, 1)
    hy = y[size // 4: size // 4 + hn].cpu().numpy()
    ll = 0.5 * np.log(ht) - 0.9189385332046727 - 0.5 * ht * (hy - hx) ** 2
    mx = ll.max(axis=0)
    _ = np.log(np.exp(ll - mx).sum(axis=0)) + mx, ll.var(axis=0, ddof=1)
    host_ms = (time.perf_counter() - t0) * 1e3
    rec["rows"].append({"case": f"host: transfer + numpy, {hn} nodes", "ms": host_ms, "ms_per_node": host_ms / hn})
    print(f"  host: transfer + numpy, {hn} nodes: {host_ms:.1f} ms = {host_ms / hn:.2f} ms per node "
          f"({host_ms / hn * size / 1e3:.1f} s for all {size})", flush=True)

    # ---- omc_store_psis
    tail = int(min(S - 1, np.ceil(min(S / 5.0, 3.0 * np.sqrt(S)))))
    t_rank = row(f"omc_store_ranks, {args.index} indexed nodes (the same gather and sort)", timed(lambda: eng.store_ranks(x, index=idx)))
    t_psis = row(f"omc_store_psis from the mean entry, {args.index} indexed nodes, tails of {tail}",
                 timed(lambda: eng.store_psis(x, tail, index=idx, y=y[idx], prec=prec)))
    t_nofit = row(f"omc_store_psis the same with tails of 1 draw (no fit)", timed(lambda: eng.store_psis(x, 1, index=idx, y=y[idx], prec=prec)))
    rec["psis_fit_share"] = (t_psis - t_nofit) / t_psis
    rec["psis_ratio_to_ranks"] = t_psis / t_rank
    print(f"  the fit's share of omc_store_psis: {100 * rec['psis_fit_share']:.0f} %; omc_store_psis / omc_store_ranks = {t_psis / t_rank:.2f}", flush=True)
    eng.check_status()
    eng.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
