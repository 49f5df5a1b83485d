#!/usr/bin/env python3
"""Rank-normalised diagnostics of the device store (omc_store_rank_diagnostics) beside the classic ones and beside a library sort.

    python3 benchmarks/store_rank_diagnostics.py [--iters 128] [--chains 1024] [--nodes 10000] [--index 512] [--reps 5]

Prints a table and one JSON line.  The store is the cfg3 store (store["b"] of GmrfSweep.run_fused: iters x chains x nodes); the
selection is --index contiguous nodes from a quarter of the way in.  Three timings, medians of --reps calls timed one by one
with device events after a warm-up call, in one process on one card:
  omc_store_rank_diagnostics on the selection (two sorts of every column, four series, one omc_store_rhat_ess over them);
  what MCMC.diagnostics costs on the same selection: omc_store_rhat_ess and the pooled omc_store_moments of the gathered columns
    (the gather itself, store[:, :, idx].contiguous(), is timed apart: the classic call has no index argument);
  torch.sort of the same gathered columns, (index, iters x chains) fp64 along the draws: a yardstick for ONE of the two sorts.
omc_store_ranks (one sort and the bisections) is timed as well.  No threshold is attached to any of these.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=128)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--index", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch

    from bench import GmrfSweep
    from openmcmc_amd.engine import Engine

    def timed(fn):
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
        return float(np.median(ms))

    n, C, K = args.nodes, args.chains, args.iters
    sw = GmrfSweep(n, C, seed=7, chain_offset=0, device=0, n_store=K)
    sw.run_fused(K + 8)
    torch.cuda.synchronize()
    store, eng = sw.store_b, sw.eng
    idx = torch.arange(n // 4, n // 4 + args.index, device=store.device)
    S = 2 * C * (K // 2)
    P = 1 << (S - 1).bit_length()
    sched = Engine.rank_schedule(S)
    rows = []

    def row(label, ms):
        rows.append({"case": label, "ms": ms})
        print(f"  {label:<86s} {ms:10.3f} ms", flush=True)

    print(f"cfg3 store: {K} iterations x {C} chains x {n} nodes ({8e-9 * K * C * n:.2f} GB), {args.index} indexed nodes; "
          f"columns of S = {S} split draws, P = {P} keys, {sum(1 for l in sched if l[0] != 1)} tile launches and "
          f"{sum(1 for l in sched if l[0] == 1)} global passes per sort", flush=True)
    row("omc_store_rank_diagnostics (rhat, ess_bulk, ess_tail)", timed(lambda: eng.store_rank_diagnostics(store, index=idx)))
    row("omc_store_ranks, split (one sort, the bisections, ranks written)", timed(lambda: eng.store_ranks(store, index=idx, split=True)))
    row("gather of the selection, store[:, :, idx].contiguous()", timed(lambda: store[:, :, idx].contiguous()))
    sel = store[:, :, idx].contiguous()

    def classic():
        eng.store_rhat_ess(sel)
        eng.store_moments(sel, pooled=True)

    row("classic diagnostics of the gathered selection (omc_store_rhat_ess + omc_store_moments)", timed(classic))
    cols = sel.reshape(K * C, args.index).t().contiguous()
    row("torch.sort of the gathered columns along the draws (yardstick for one sort)", timed(lambda: torch.sort(cols, dim=1)))
    rhat, bulk, tail = (t.cpu().numpy() for t in eng.store_rank_diagnostics(store, index=idx))
    classic_rhat = eng.store_rhat_ess(sel)[0].cpu().numpy()
    eng.check_status()
    print(json.dumps({"store": f"{K} x {C} x {n}", "index": args.index, "S": S, "P": P, "reps": args.reps, "rows": rows,
                      "rhat_rank_median": float(np.nanmedian(rhat)), "rhat_classic_median": float(np.nanmedian(classic_rhat)),
                      "ess_bulk_median": float(np.nanmedian(bulk)), "ess_tail_median": float(np.nanmedian(tail))}))


if __name__ == "__main__":
    main()
