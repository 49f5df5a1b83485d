#!/usr/bin/env python3
"""Linear maps of the device store (omc_store_project) beside the torch expression a user would write outside the library
(index_select / nan_to_num / matmul on the same device, temporaries included) and beside the project's own one-read kernel over
the same bytes, omc_store_moments.

    python3 benchmarks/store_project.py [--reps 7] [--iters 128] [--chains 1024] [--nodes 10000] [--index 512]
                                        [--rj-iters 2000] [--rj-chains 512] [--rj-slots 20]

Prints a table and one JSON line.  One process on one card; every time is the median of --reps calls timed one by one with device
events after a warm-up call, with the smallest and largest of them beside it.  Store bytes per second count ONE read of the store
(m <= 128 reads it once, m = 256 twice: the figure is then what a user gets, not what the memory moves); flop are 2 R n_idx m,
the padded columns not counted.
  cfg3   --iters x --chains x --nodes normal draws (128 x 1024 x 10 000: 10.5 GB): omc_store_moments pooled (the yardstick); all
         elements under m = 1, 16, 64, 256; --index indexed nodes under m = 32; m = 16 with noise (one stored precision per draw).
  rj     --rj-iters x --rj-chains x --rj-slots, NaN beyond a random live length (2000 x 512 x 20), omit_nan, m = 100.
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
    ap.add_argument("--rj-iters", type=int, default=2000)
    ap.add_argument("--rj-chains", type=int, default=512)
    ap.add_argument("--rj-slots", type=int, default=20)
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

    def table(rec, nbytes):
        def row(label, t, base=None, flop=None, bytes_read=nbytes):
            ms, lo, hi = t
            r = {"case": label, "ms": ms, "ms_min": lo, "ms_max": hi}
            text = f"  {label:<72s} {ms:9.3f} ms [{lo:8.3f} .. {hi:8.3f}]"
            if bytes_read:
                r["TB_per_s"] = bytes_read / (ms * 1e-3) / 1e12
                text += f" {r['TB_per_s']:6.2f} TB/s"
            if flop:
                r["TFLOP_per_s"] = flop / (ms * 1e-3) / 1e12
                text += f" {r['TFLOP_per_s']:6.2f} TFLOP/s"
            if base is not None:
                r["ratio_to_moments"] = ms / base
                text += f"   x{ms / base:5.2f} of moments"
            rec["rows"].append(r)
            print(text, flush=True)
        return row

    def pair(eng, x, row, t_mom, label, m, index=None, omit_nan=False, prec=None):
        """the library call and the torch expression for one shape, and that they agree"""
        n_iter, C, size = x.shape
        R = n_iter * C
        n = size if index is None else index.numel()
        g = torch.Generator(device=eng.device)
        g.manual_seed(m)
        W = torch.randn((m, n), generator=g, dtype=torch.float64, device=eng.device)
        flop = 2.0 * R * n * m
        out = eng.empty(n_iter, C, m)
        row(f"omc_store_project {label}", timed(lambda: eng.store_project(x, W, index=index, omit_nan=omit_nan, prec=prec, out=out)),
            t_mom, flop, 8.0 * R * n)

        def by_torch():
            sel = x.view(R, size) if index is None else x.view(R, size).index_select(1, index)
            if omit_nan:
                sel = torch.nan_to_num(sel, nan=0.0)
            y = (sel @ W.T).view(n_iter, C, m)
            if prec is not None:
                y = y + torch.randn(y.shape, dtype=torch.float64, device=y.device) / prec.sqrt()
            return y

        row(f"torch {label}", timed(by_torch), t_mom, flop, 8.0 * R * n)
        if prec is None:
            ref = by_torch()
            got = eng.store_project(x, W, index=index, omit_nan=omit_nan)
            scale = float(ref.abs().max())
            assert float((got - ref).abs().max()) <= 1e-9 * scale, (label, float((got - ref).abs().max()), scale)
            assert torch.equal(got, eng.store_project(x, W, index=index, omit_nan=omit_nan))
            del ref, got
        torch.cuda.empty_cache()

    def cfg3():
        n_iter, C, size = args.iters, args.chains, args.nodes
        eng = Engine(C, seed=3)
        g = torch.Generator(device=eng.device)
        g.manual_seed(6)
        shift = torch.linspace(-1, 1, size, dtype=torch.float64, device=eng.device)
        x = torch.empty((n_iter, C, size), dtype=torch.float64, device=eng.device)
        for i in range(n_iter):  # (slab by slab: no second store-sized temporary)
            x[i] = torch.randn((C, size), generator=g, dtype=torch.float64, device=eng.device) + shift
        nbytes = 8.0 * n_iter * C * size
        rec = {"store": f"{n_iter} iterations x {C} chains x {size}", "store_GB": nbytes / 1e9, "rows": []}
        row = table(rec, nbytes)
        print(f"cfg3: {rec['store']} ({rec['store_GB']:.2f} GB)", flush=True)
        t_mom = timed(lambda: eng.store_moments(x, pooled=True))
        row("omc_store_moments pooled (yardstick)", t_mom)
        for m in (1, 16, 64, 256):
            pair(eng, x, row, t_mom[0], f"all elements, m = {m}", m)
        idx = torch.arange(size // 4, size // 4 + args.index, device=eng.device)
        pair(eng, x, row, t_mom[0], f"{args.index} indexed nodes, m = 32", 32, index=idx)
        prec = torch.rand((n_iter, C, 1), generator=g, dtype=torch.float64, device=eng.device) + 0.5
        pair(eng, x, row, t_mom[0], "all elements, m = 16, with noise", 16, prec=prec)
        eng.check_status()
        eng.close()
        del x
        torch.cuda.empty_cache()
        return rec

    def rj():
        n_iter, C, size = args.rj_iters, args.rj_chains, args.rj_slots
        eng = Engine(C, seed=3)
        g = torch.Generator(device=eng.device)
        g.manual_seed(7)
        x = torch.randn((n_iter, C, size), generator=g, dtype=torch.float64, device=eng.device)
        live = torch.randint(0, size + 1, (n_iter, C, 1), generator=g, device=eng.device)
        x[torch.arange(size, device=eng.device).expand(n_iter, C, size) >= live] = float("nan")
        nbytes = 8.0 * n_iter * C * size
        rec = {"store": f"{n_iter} iterations x {C} chains x {size}, NaN beyond the live length", "store_GB": nbytes / 1e9, "rows": []}
        row = table(rec, nbytes)
        print(f"rj: {rec['store']} ({rec['store_GB']:.3f} GB)", flush=True)
        t_mom = timed(lambda: eng.store_moments(x, pooled=True))
        row("omc_store_moments pooled (yardstick)", t_mom)
        pair(eng, x, row, t_mom[0], "omit_nan, m = 100", 100, omit_nan=True)
        eng.check_status()
        eng.close()
        return rec

    out = {"reps": args.reps, "cfg3": cfg3(), "rj": rj()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
