#!/usr/bin/env python3
"""Joint 2-D histograms and occupancy maps of the device store (omc_store_histogram2d) against the marginal pass over the same
columns (omc_store_histogram, the yardstick) and against the route a user has without it: transfer of the selected columns and
np.histogram2d on the host.

    python3 benchmarks/store_histogram2d.py [--reps 12] [--host-reps 3] [--cfg3-iters 64] [--cfg3-chains 1024] [--cfg3-size 10000]
                                            [--cfg3-index 512] [--rj-iters 2000] [--rj-chains 512] [--rj-nmax 20]

Prints a table and one JSON line.  In one process on one card, pooled over chains and iterations, median of --reps calls timed one
by one with device events after a warm-up call (the host route: wall clock, median of --host-reps):
  cfg3    64 iterations x 1024 chains x 10 000 nodes (5.2 GB): --cfg3-index contiguous nodes against the next as many, a 32 x 32
          grid per pair, shared and per-pair evenly spaced edges; beside it omc_store_histogram at 32 bins over the same two sets
          of columns (one call with both index sets), and the host route;
  ragged  two NaN-padded stores of --rj-iters x --rj-chains x --rj-nmax (location, coefficient; live length uniform on
          0 .. n_max), all pairs pooled into one map with occupancy, 64 x 64 (counters in LDS) and 512 x 512 (the direct form),
          also 64 x 64 forced into the direct form; beside each omc_store_histogram over both stores at the same bins per axis,
          and the host route (np.histogram2d of the flattened stores: the counts only -- the occupancy loop over the stored
          states, one np.histogram2d each, is timed on a 1/64 sample of the rows and scaled).
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
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--cfg3-iters", type=int, default=64)
    ap.add_argument("--cfg3-chains", type=int, default=1024)
    ap.add_argument("--cfg3-size", type=int, default=10000)
    ap.add_argument("--cfg3-index", type=int, default=512)
    ap.add_argument("--rj-iters", type=int, default=2000)
    ap.add_argument("--rj-chains", type=int, default=512)
    ap.add_argument("--rj-nmax", type=int, default=20)
    args = ap.parse_args()
    import torch

    from openmcmc_amd.engine import Engine

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

    def wall(fn, reps):
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms))

    def row(rec, label, ms, base=None):
        r = {"case": label, "ms": ms}
        if base is not None:
            r["ratio_to_marginals"] = ms / base
        rec["rows"].append(r)
        print(f"  {label:<74s} {ms:10.3f} ms" + (f"   x{ms / base:6.2f} of the marginal pass" if base else ""), flush=True)

    def cfg3():
        n_iter, C, size, n = args.cfg3_iters, args.cfg3_chains, args.cfg3_size, args.cfg3_index
        eng = Engine(C, seed=3)
        g = torch.Generator(device=eng.device)
        g.manual_seed(6)
        shift = torch.linspace(-1, 1, size, dtype=torch.float64, device=eng.device)
        x = torch.empty((n_iter, C, size), dtype=torch.float64, device=eng.device)
        for i in range(n_iter):  # (slab by slab: no second store-sized temporary)
            x[i] = torch.randn((C, size), generator=g, dtype=torch.float64, device=eng.device) + shift
        ix, iy = np.arange(size // 4, size // 4 + n), np.arange(size // 4 + n, size // 4 + 2 * n)
        both = np.concatenate([ix, iy])
        rec = {"store": f"{n_iter} iterations x {C} chains x {size}", "pairs": n, "columns_GB": 8.0 * n_iter * C * 2 * n / 1e9, "rows": []}
        print(f"cfg3: {rec['store']}, {n} nodes against the next {n} ({rec['columns_GB']:.2f} GB of columns), 32 x 32 per pair", flush=True)
        mn, mx, _ = eng.store_minmax(x, index=both)
        mn, mx = mn.cpu().numpy(), mx.cpu().numpy()
        shared = eng.to_device(np.linspace(mn.min(), mx.max(), 33))
        per = eng.to_device(np.stack([np.linspace(a, b, 33) for a, b in zip(mn, mx)]))
        t1 = timed(lambda: eng.store_histogram(x, shared, index=both))
        row(rec, "omc_store_histogram, 32 bins, both sets of columns, shared edges (yardstick)", t1)
        t1p = timed(lambda: eng.store_histogram(x, per, index=both))
        row(rec, "omc_store_histogram, 32 bins, both sets of columns, per-element edges", t1p)
        row(rec, "omc_store_histogram2d, 32 x 32 per pair, shared edges", timed(lambda: eng.store_histogram2d(x, x, shared, shared, ix, iy)), t1)
        row(rec, "omc_store_histogram2d, 32 x 32 per pair, per-pair edges",
            timed(lambda: eng.store_histogram2d(x, x, per[:n], per[n:], ix, iy)), t1p)
        eng.set_option("hist2d_algo", 1)
        row(rec, "omc_store_histogram2d, 32 x 32 per pair, shared edges, direct form", timed(lambda: eng.store_histogram2d(x, x, shared, shared, ix, iy)), t1)
        eng.set_option("hist2d_algo", 0)
        e = shared.cpu().numpy()

        def host():
            cols = x[:, :, size // 4: size // 4 + 2 * n].cpu().numpy().reshape(-1, 2 * n)
            return [np.histogram2d(cols[:, k], cols[:, n + k], bins=[e, e])[0] for k in range(n)]

        row(rec, "host: transfer of the columns + np.histogram2d per pair", wall(host, args.host_reps), t1)
        eng.check_status()
        eng.close()
        return rec

    def ragged():
        n_iter, C, n_max = args.rj_iters, args.rj_chains, args.rj_nmax
        eng = Engine(C, seed=3)
        g = torch.Generator(device=eng.device)
        g.manual_seed(7)
        dev = eng.device
        k = torch.randint(0, n_max + 1, (n_iter, C, 1), generator=g, device=dev)
        live = torch.arange(n_max, device=dev) < k
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        loc = torch.where(live, torch.rand((n_iter, C, n_max), generator=g, dtype=torch.float64, device=dev) * 10.0, nan).contiguous()
        coef = torch.where(live, torch.randn((n_iter, C, n_max), generator=g, dtype=torch.float64, device=dev), nan).contiguous()
        rec = {"stores": f"2 x ({n_iter} iterations x {C} chains x {n_max})", "stores_GB": 16.0 * n_iter * C * n_max / 1e9, "rows": []}
        print(f"ragged: {rec['stores']} ({rec['stores_GB']:.2f} GB), all pairs pooled, with occupancy", flush=True)
        for nb, algo, what in ((64, 0, "counters in LDS"), (64, 1, "direct form (forced)"), (512, 0, "direct form")):
            ex, ey = eng.to_device(np.linspace(0.0, 10.0, nb + 1)), eng.to_device(np.linspace(-4.0, 4.0, nb + 1))
            t1 = timed(lambda: (eng.store_histogram(loc, ex), eng.store_histogram(coef, ey)))
            row(rec, f"omc_store_histogram, {nb} bins, the two stores one after the other (yardstick)", t1)
            eng.set_option("hist2d_algo", algo)
            row(rec, f"omc_store_histogram2d, {nb} x {nb}, pooled pairs, {what}",
                timed(lambda: eng.store_histogram2d(loc, coef, ex, ey, pool_pairs=True)), t1)
            row(rec, f"omc_store_histogram2d, {nb} x {nb}, pooled pairs with occupancy, {what}",
                timed(lambda: eng.store_histogram2d(loc, coef, ex, ey, pool_pairs=True, occupancy=True)), t1)
            eng.set_option("hist2d_algo", 0)
            hx, hy = ex.cpu().numpy(), ey.cpu().numpy()

            def host_counts():
                a, b = loc.cpu().numpy().ravel(), coef.cpu().numpy().ravel()
                ok = ~np.isnan(a)
                return np.histogram2d(a[ok], b[ok], bins=[hx, hy])[0]

            row(rec, f"host: transfer of the stores + np.histogram2d, {nb} x {nb} (counts only)", wall(host_counts, args.host_reps), t1)
            if nb == 64:
                a, b = loc.cpu().numpy().reshape(-1, n_max)[::64], coef.cpu().numpy().reshape(-1, n_max)[::64]

                def host_occupancy():
                    occ = np.zeros((nb, nb))
                    for r in range(a.shape[0]):
                        ok = ~np.isnan(a[r])
                        occ += np.histogram2d(a[r][ok], b[r][ok], bins=[hx, hy])[0] > 0
                    return occ

                row(rec, f"host: occupancy loop over the stored states, {nb} x {nb} (1/64 of the rows, x 64)", 64.0 * wall(host_occupancy, 1), t1)
        eng.check_status()
        eng.close()
        return rec

    out = {"reps": args.reps, "cfg3": cfg3(), "ragged": ragged()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
