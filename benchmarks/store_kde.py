#!/usr/bin/env python3
"""Kernel density estimates of the device store (MCMC.kde: omc_store_minmax, omc_store_histogram, omc_kde_binned) on the
cfg3-shaped store, beside the host route and a torch expression of the same convolution.

    python3 benchmarks/store_kde.py [--reps 7] [--iters 64] [--chains 1024] [--size 10000] [--index 512] [--host-cols 4]

Prints a table and one JSON line.  One store of --iters x --chains x --size normal draws around per-element means (5.2 GB by
default), --index contiguous nodes selected, in one process on one card:
  MCMC.kde end to end (wall clock around a call that ends with the results on the host), pooled (--index columns) and per chain
    (--chains x --index columns), split into its three device parts, each timed alone by device events: the ranges
    (omc_store_minmax), the counts (omc_store_histogram over per-element edges) and omc_kde_binned;
  omc_kde_binned alone for every rule (ISJ by count: up to 107 evaluations of Phi, six sums of G - 1 terms with an exp each -- about
    330 000 exp per column at G = 512) and for G = 128 / 512 / 1024;
  the host route for --host-cols columns: the column to the host, scipy.stats.gaussian_kde (its own normal-reference bandwidth)
    evaluated on the same 512 grid points;
  the same binned convolution as a torch expression on the device (a (columns, G, G) Gaussian matrix and a batched product),
    pooled columns only, with the kernel's bandwidths.
Medians of --reps calls after a warm-up call (3 calls where a single one takes more than a second)."""
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
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--index", type=int, default=512)
    ap.add_argument("--host-cols", type=int, default=4)
    args = ap.parse_args()
    import torch

    from openmcmc_amd.engine import Engine
    from openmcmc_amd.mcmc import MCMC

    def timed(fn, wall=False):
        """median ms of the calls after one warm-up call: device events, or the host clock around a call that ends synchronised"""
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps = 3 if time.perf_counter() - t0 > 1.0 else args.reps
        ms = []
        for _ in range(reps):
            if wall:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    n_iter, C, size = args.iters, args.chains, args.size
    eng = Engine(C, seed=3)
    g = torch.Generator(device=eng.device)
    g.manual_seed(6)
    shift = torch.linspace(-1, 1, size, dtype=torch.float64, device=eng.device)
    x = torch.empty((n_iter, C, size), dtype=torch.float64, device=eng.device)
    for i in range(n_iter):  # (slab by slab: no second store-sized temporary)
        x[i] = torch.randn((C, size), generator=g, dtype=torch.float64, device=eng.device) + shift
    M = MCMC.__new__(MCMC)
    M.engine, M.store, M.store_ring, M.n_iter, M._n_dev = eng, {"x": x}, None, n_iter, n_iter
    idx = np.arange(size // 4, size // 4 + args.index)
    rows = []

    def row(label, ms, cols=None):
        r = {"case": label, "ms": ms}
        if cols:
            r["us_per_column"] = ms * 1e3 / cols
        rows.append(r)
        print(f"  {label:<86s} {ms:11.3f} ms" + (f" {r['us_per_column']:9.3f} us/column" if cols else ""), flush=True)

    print(f"store: {n_iter} iterations x {C} chains x {size} ({8.0 * n_iter * C * size / 1e9:.2f} GB), {args.index} nodes selected", flush=True)
    mn, mx, _ = (v.cpu().numpy() for v in eng.store_minmax(x, index=idx))
    a, b = mn - 0.1 * (mx - mn), mx + 0.1 * (mx - mn)
    for pooled in (True, False):
        cols = args.index * (1 if pooled else C)
        what = f"pooled ({cols} columns of {n_iter * C} draws)" if pooled else f"per chain ({cols} columns of {n_iter} draws)"
        print(what, flush=True)
        row("MCMC.kde(grid_len=512, bw='experimental'), end to end, wall clock", timed(lambda: M.kde("x", index=idx, pooled=pooled), wall=True), cols)
        row("  part: omc_store_minmax (the ranges, always pooled)", timed(lambda: eng.store_minmax(x, index=idx)))
        lead = (args.index,) if pooled else (C, args.index)
        for G in (512, 128, 1024):
            edges = eng.to_device(np.stack([np.linspace(p, q, G + 1) for p, q in zip(a, b)]))
            row(f"  part: omc_store_histogram, {G} bins, per-element edges", timed(lambda: eng.store_histogram(x, edges, index=idx, pooled=pooled)))
            counts, _ = eng.store_histogram(x, edges, index=idx, pooled=pooled)
            lo, hi = eng.to_device(np.array(np.broadcast_to(a, lead))), eng.to_device(np.array(np.broadcast_to(b, lead)))
            given = eng.to_device(np.array(np.broadcast_to(0.05 * (b - a), lead)))
            for rule in (("given", "scott", "silverman", "isj", "experimental") if G == 512 else ("given", "experimental")):
                bw = given if rule == "given" else None
                row(f"  part: omc_kde_binned, G = {G}, rule {rule}", timed(lambda: eng.kde_binned(counts, lo, hi, rule=rule, bw=bw)), cols)
            if G == 512:
                flags = eng.kde_binned(counts, lo, hi, rule="isj")[3]
                print(f"      (ISJ flags: {int((flags == 0).sum())} ok, {int((flags == 1).sum())} fell back, {int((flags == 2).sum())} degenerate)", flush=True)
            if G == 512 and pooled:
                dens, h, _, _ = eng.kde_binned(counts, lo, hi, rule="experimental")

                def torch_route():
                    d = torch.arange(G, dtype=torch.float64, device=eng.device)
                    step = ((hi - lo) / G / h)[:, None, None]
                    W = torch.exp(-0.5 * ((d[None, :, None] - d[None, None, :]) * step) ** 2)
                    N = counts.sum(dim=-1, keepdim=True).to(torch.float64)
                    return torch.bmm(W, counts.to(torch.float64)[:, :, None])[:, :, 0] / (N * h[:, None] * (2 * np.pi) ** 0.5)

                err = float(((torch_route() - dens).abs() / dens.abs().clamp_min(1e-300)).max())
                row(f"  torch expression of the convolution, G = 512, given the bandwidths (max rel. difference {err:.1e})", timed(torch_route), cols)
            del counts
            torch.cuda.empty_cache()
    print("host route", flush=True)
    from scipy.stats import gaussian_kde

    k = args.host_cols
    grid = np.stack([np.linspace(p, q, 513) for p, q in zip(a[:k], b[:k])])
    grid = 0.5 * (grid[:, :-1] + grid[:, 1:])

    def host_route():
        cols = x[:, :, idx[0]:idx[0] + k].reshape(-1, k).cpu().numpy()
        return [gaussian_kde(cols[:, j])(grid[j]) for j in range(k)]

    t0 = time.perf_counter()
    host_route()
    t_host = (time.perf_counter() - t0) * 1e3
    row(f"transfer + scipy.stats.gaussian_kde on 512 grid points, {k} pooled columns, wall clock, one call", t_host, k)
    eng.check_status()
    eng.close()
    print(json.dumps({"reps": args.reps, "store": f"{n_iter} x {C} x {size}", "index": args.index, "rows": rows}))


if __name__ == "__main__":
    main()
