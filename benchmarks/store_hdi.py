#!/usr/bin/env python3
"""Highest-density intervals of the device store (omc_store_hdi) beside the ranks of the same columns and beside the host route.

    python3 benchmarks/store_hdi.py [--iters 128] [--chains 1024] [--nodes 10000] [--index 512] [--reps 5]

Prints a table and one JSON line.  The store is the cfg3 store (store["b"] of GmrfSweep.run_fused: iters x chains x nodes); the
selection is --index contiguous nodes from a quarter of the way in.  Timings are medians of --reps calls timed one by one with
device events after a warm-up call, in one process on one card:
  omc_store_hdi on the selection, pooled and per chain, at prob = 0.94 and at three probabilities;
  omc_store_ranks (no split) on the same columns: the same gather and the same sort as the pooled intervals, then the bisections
    and the ranks written instead of the count and the window pass;
  the host route, timed by the wall clock, once: the selection gathered on the device and copied to the host, then the numpy
    definition (sort, the window widths, argmin) column by column.
The device results are compared with the host route's before anything is printed.  No threshold is attached to these numbers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def hdi_numpy(cols, probs):
    """(n_prob, n_col, 2) of host columns (n_col, n): the definition of include/omcmc_hip.h, omc_store_hdi, without NaN or inf"""
    x = np.sort(cols, axis=1)
    n = x.shape[1]
    out = np.empty((len(probs), x.shape[0], 2))
    rows = np.arange(x.shape[0])
    for p, prob in enumerate(probs):
        m = min(int(np.floor(prob * n)), n - 1)
        i = np.argmin(x[:, m:] - x[:, :n - m], axis=1)
        out[p, :, 0], out[p, :, 1] = x[rows, i], x[rows, i + m]
    return out


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
    S = K * C
    sched = Engine.rank_schedule(S)
    three = [0.5, 0.8, 0.94]
    rows = []

    def row(label, ms):
        rows.append({"case": label, "ms": ms})
        print(f"  {label:<92s} {ms:10.3f} ms", flush=True)

    # the host route first: it is also the check of what is timed afterwards
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = store[:, :, idx].contiguous().cpu().numpy()
    t1 = time.perf_counter()
    want_pooled = hdi_numpy(host.reshape(K * C, args.index).T, three)
    t2 = time.perf_counter()
    want_chain = hdi_numpy(host.transpose(1, 2, 0).reshape(C * args.index, K), three).reshape(3, C, args.index, 2)
    t3 = time.perf_counter()
    got_pooled = eng.store_hdi(store, three, index=idx)[0].cpu().numpy()
    got_chain = eng.store_hdi(store, three, index=idx, pooled=False)[0].cpu().numpy()
    eng.check_status()
    assert np.array_equal(got_pooled, want_pooled) and np.array_equal(got_chain, want_chain), "device and host intervals differ"

    print(f"cfg3 store: {K} iterations x {C} chains x {n} nodes ({8e-9 * K * C * n:.2f} GB), {args.index} indexed nodes; pooled: "
          f"{args.index} columns of S = {S} draws, {sum(1 for l in sched if l[0] != 1)} tile launches and "
          f"{sum(1 for l in sched if l[0] == 1)} global passes per sort; per chain: {C * args.index} columns of {K} draws; "
          f"the intervals equal the host route's bit for bit", flush=True)
    row("omc_store_hdi pooled, prob = 0.94", timed(lambda: eng.store_hdi(store, 0.94, index=idx)))
    row("omc_store_hdi pooled, three probabilities", timed(lambda: eng.store_hdi(store, three, index=idx)))
    row("omc_store_hdi per chain, prob = 0.94", timed(lambda: eng.store_hdi(store, 0.94, index=idx, pooled=False)))
    row("omc_store_hdi per chain, three probabilities", timed(lambda: eng.store_hdi(store, three, index=idx, pooled=False)))
    row("omc_store_ranks, no split, same columns (same gather and sort; bisections, ranks written)",
        timed(lambda: eng.store_ranks(store, index=idx)))
    row("host route: gather of the selection and transfer (wall clock, once)", 1e3 * (t1 - t0))
    row("host route: numpy definition, pooled, three probabilities (wall clock, once)", 1e3 * (t2 - t1))
    row("host route: numpy definition, per chain, three probabilities (wall clock, once)", 1e3 * (t3 - t2))
    width = got_pooled[2, :, 1] - got_pooled[2, :, 0]
    print(json.dumps({"store": f"{K} x {C} x {n}", "index": args.index, "S": S, "reps": args.reps, "rows": rows,
                      "hdi94_width_median": float(np.median(width))}))


if __name__ == "__main__":
    main()
