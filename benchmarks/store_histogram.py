#!/usr/bin/env python3
"""Marginal histograms and ranges of the device store (omc_store_histogram, omc_store_minmax) against the project's own
one-read kernel over the same bytes, omc_store_moments.

    python3 benchmarks/store_histogram.py [--reps 12] [--cfg2-iters 500] [--cfg2-chains 256] [--cfg2-size 1000]
                                          [--cfg3-iters 64] [--cfg3-chains 1024] [--cfg3-size 10000] [--cfg3-index 512]

Prints a table and one JSON line.  Two stores filled on the device with normal draws around per-element means:
  small  500 iterations x 256 chains x 1000 elements (1 GB);
  cfg3   64 iterations x 1024 chains x 10 000 nodes (5.2 GB).
Per store, pooled over chains and iterations, in one process on one card (median of --reps calls timed one by one with device
events, after a warm-up call): omc_store_moments (the yardstick), omc_store_minmax, and omc_store_histogram with 32 and 256 bins,
with shared evenly spaced edges and with per-element edges (evenly spaced over the element's own range, and the same edges
through the bisection, option hist_algo = 1); every time also as store bytes per second and as a ratio to the moments pass.
Then the same four histogram cases on a store whose columns are constant (every lane of a column adds to one counter), and
MCMC.histogram end to end (ranges, host-built edges, upload, counts, download) for --cfg3-index nodes of the cfg3 store.
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
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--cfg2-iters", type=int, default=500)
    ap.add_argument("--cfg2-chains", type=int, default=256)
    ap.add_argument("--cfg2-size", type=int, default=1000)
    ap.add_argument("--cfg3-iters", type=int, default=64)
    ap.add_argument("--cfg3-chains", type=int, default=1024)
    ap.add_argument("--cfg3-size", type=int, default=10000)
    ap.add_argument("--cfg3-index", type=int, default=512)
    args = ap.parse_args()
    import torch

    from openmcmc_amd.engine import Engine
    from openmcmc_amd.mcmc import MCMC

    def timed(fn):
        """median ms of --reps calls, each between its own pair of device events, after one warm-up call"""
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

    def measure(name, n_iter, C, size, n_index, seed):
        eng = Engine(C, seed=3)
        g = torch.Generator(device=eng.device)
        g.manual_seed(seed)
        shift = torch.linspace(-1, 1, size, dtype=torch.float64, device=eng.device)
        x = torch.empty((n_iter, C, size), dtype=torch.float64, device=eng.device)
        for i in range(n_iter):  # (slab by slab: no second store-sized temporary)
            x[i] = torch.randn((C, size), generator=g, dtype=torch.float64, device=eng.device) + shift
        nbytes = 8.0 * n_iter * C * size
        rec = {"store": f"{n_iter} iterations x {C} chains x {size}", "store_GB": nbytes / 1e9, "rows": []}

        def row(label, ms, base=None):
            r = {"case": label, "ms": ms, "TB_per_s": nbytes / (ms * 1e-3) / 1e12}
            if base is not None:
                r["ratio_to_moments"] = ms / base
            rec["rows"].append(r)
            print(f"  {label:<58s} {ms:9.3f} ms {r['TB_per_s']:6.2f} TB/s" + (f"   x{ms / base:5.2f} of moments" if base else ""), flush=True)

        print(f"{name}: {rec['store']} ({rec['store_GB']:.2f} GB), pooled", flush=True)
        t_mom = timed(lambda: eng.store_moments(x, pooled=True))
        row("omc_store_moments (yardstick)", t_mom)
        row("omc_store_minmax", timed(lambda: eng.store_minmax(x)), t_mom)
        mn, mx, _ = eng.store_minmax(x)
        mn, mx = mn.cpu().numpy(), mx.cpu().numpy()
        for data, what in ((x, "normal draws"), (None, "constant columns")):
            if data is None:
                x[:] = shift  # every column constant: the contention case
                mn = mx = shift.cpu().numpy()
            for nb in (32, 256):
                lo, hi = (mn, mx) if what == "normal draws" else (mn - 0.5, mx + 0.5)
                shared = eng.to_device(np.linspace(lo.min(), hi.max(), nb + 1))
                per = eng.to_device(np.stack([np.linspace(a, b, nb + 1) for a, b in zip(lo, hi)]))
                row(f"histogram {nb:3d} bins, shared even edges, {what}", timed(lambda: eng.store_histogram(x, shared)), t_mom)
                row(f"histogram {nb:3d} bins, per-element even edges, {what}", timed(lambda: eng.store_histogram(x, per)), t_mom)
                eng.set_option("hist_algo", 1)
                row(f"histogram {nb:3d} bins, shared edges by bisection, {what}", timed(lambda: eng.store_histogram(x, shared)), t_mom)
                row(f"histogram {nb:3d} bins, per-element edges by bisection, {what}", timed(lambda: eng.store_histogram(x, per)), t_mom)
                eng.set_option("hist_algo", 0)
        if n_index is not None:  # MCMC.histogram end to end on the object's store, wall clock
            for i in range(n_iter):
                x[i] = torch.randn((C, size), generator=g, dtype=torch.float64, device=eng.device) + shift
            M = MCMC.__new__(MCMC)
            M.engine, M.store, M.store_ring, M.n_iter, M._n_dev = eng, {"x": x}, None, n_iter, n_iter
            idx = np.arange(size // 4, size // 4 + n_index)
            M.histogram("x", bins=32, index=idx)
            torch.cuda.synchronize()
            wall = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                M.histogram("x", bins=32, index=idx)
                wall.append((time.perf_counter() - t0) * 1e3)
            rec["mcmc_histogram_ms"] = float(np.median(wall))
            rec["mcmc_histogram_case"] = f"MCMC.histogram(bins=32, index of {n_index} contiguous nodes), end to end, wall clock"
            print(f"  {rec['mcmc_histogram_case']:<58s} {rec['mcmc_histogram_ms']:9.3f} ms", flush=True)
        eng.check_status()
        eng.close()
        del x
        torch.cuda.empty_cache()
        return rec

    out = {"reps": args.reps,
           "small": measure("small", args.cfg2_iters, args.cfg2_chains, args.cfg2_size, None, 5),
           "cfg3": measure("cfg3", args.cfg3_iters, args.cfg3_chains, args.cfg3_size, args.cfg3_index, 6)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
