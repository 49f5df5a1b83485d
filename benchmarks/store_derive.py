#!/usr/bin/env python3
"""Per-draw reductions of the device store (omc_store_reduce) beside the project's own one-read kernel over the same bytes,
omc_store_moments, and beside the torch expressions a user would write outside the library.

    python3 benchmarks/store_derive.py [--reps 9] [--iters 128] [--chains 1024] [--nodes 10000] [--index 512]
                                       [--rj-iters 2000] [--rj-chains 512] [--rj-slots 20] [--sweep-GB 1.0]

Prints a table and one JSON line.  One process on one card; every time is the median of --reps calls timed one by one with device
events after a warm-up call, with the smallest and largest of them beside it, as store bytes per second and as a ratio to the
moments pass of the same store.
  cfg3   --iters x --chains x --nodes normal draws (128 x 1024 x 10 000: 10.5 GB): omc_store_moments pooled (the yardstick); max, sum,
         supnorm and count_above over all nodes and over --index indexed nodes; torch.amax, torch.nansum and the standardised
         maximum ((x - mean).abs() / sd).amax(-1) with its store-sized temporaries; MCMC.simultaneous_band end to end (wall clock)
         on the indexed nodes and on all nodes, and MCMC.hdi on the same indexed nodes.
  rj     --rj-iters x --rj-chains x --rj-slots, NaN beyond a random live length (2000 x 512 x 20): count, sum and max under the
         short form, the long form and the automatic choice, beside (~isnan).sum(-1), nansum and the NaN-masked amax of torch.
  sweep  stores of --sweep-GB with rows of 20 .. 4096 elements: sum and max under both forms -- where the automatic choice switches.
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=128)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--index", type=int, default=512)
    ap.add_argument("--rj-iters", type=int, default=2000)
    ap.add_argument("--rj-chains", type=int, default=512)
    ap.add_argument("--rj-slots", type=int, default=20)
    ap.add_argument("--sweep-GB", type=float, default=1.0)
    args = ap.parse_args()
    import torch

    from openmcmc_amd.engine import Engine
    from openmcmc_amd.mcmc import MCMC

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

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    def table(rec, nbytes):
        def row(label, t, base=None, bytes_read=nbytes):
            ms, lo, hi = t
            r = {"case": label, "ms": ms, "ms_min": lo, "ms_max": hi}
            text = f"  {label:<64s} {ms:9.3f} ms [{lo:8.3f} .. {hi:8.3f}]"
            if bytes_read:
                r["TB_per_s"] = bytes_read / (ms * 1e-3) / 1e12
                text += f" {r['TB_per_s']:6.2f} TB/s"
            if base is not None:
                r["ratio_to_moments"] = ms / base
                text += f"   x{ms / base:5.2f} of moments"
            rec["rows"].append(r)
            print(text, flush=True)
        return row

    def mcmc_over(eng, x, n_iter):
        M = MCMC.__new__(MCMC)  # the summaries need the engine, the store and the ring fields only
        M.engine, M.store, M._derived, M.store_ring, M.n_iter, M._n_dev = eng, {"x": x}, set(), None, n_iter, n_iter
        return M

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
        mean, var = eng.store_moments(x, pooled=True)
        sd = var.sqrt()
        idx = torch.arange(size // 4, size // 4 + args.index, device=eng.device)
        for what, index, a_of in (("all nodes", None, lambda v: v), (f"{args.index} indexed nodes", idx, lambda v: v[idx])):
            for op, a, b in (("max", None, None), ("sum", None, None), ("supnorm", a_of(mean), a_of(sd)), ("count_above", a_of(mean) + 1.0, None)):
                a, b = (None if v is None else v.contiguous() for v in (a, b))
                # (an indexed call does not read the store: no bytes per second for it)
                row(f"omc_store_reduce {op}, {what}", timed(lambda: eng.store_reduce(x, op, index=index, a=a, b=b)), t_mom[0],
                    nbytes if index is None else None)
        # what the results must be (same inputs, the sizes timed)
        assert torch.equal(eng.store_reduce(x, "max")[0], torch.amax(x, dim=-1))
        s = eng.store_reduce(x, "sum")[0]
        assert torch.allclose(s, torch.nansum(x, dim=-1), rtol=0, atol=1e-9)
        assert s.cpu().numpy().tobytes() == eng.store_reduce(x, "sum")[0].cpu().numpy().tobytes()
        row("torch.amax(x, dim=-1)", timed(lambda: torch.amax(x, dim=-1)), t_mom[0])
        row("torch.nansum(x, dim=-1)", timed(lambda: torch.nansum(x, dim=-1)), t_mom[0])
        row("torch ((x - mean).abs() / sd).amax(-1), store-sized temporaries", timed(lambda: ((x - mean).abs() / sd).amax(-1)), t_mom[0])
        torch.cuda.empty_cache()
        M = mcmc_over(eng, x, n_iter)
        host_idx = idx.cpu().numpy()
        row(f"MCMC.simultaneous_band, {args.index} indexed nodes, end to end, wall clock", wall(lambda: M.simultaneous_band("x", index=host_idx)), None, None)
        row("MCMC.simultaneous_band, all nodes, end to end, wall clock", wall(lambda: M.simultaneous_band("x")), None, None)
        row(f"MCMC.hdi(prob=0.94), the same {args.index} nodes, end to end, wall clock", wall(lambda: M.hdi("x", index=host_idx)), None, None)
        band = M.simultaneous_band("x")
        rec["critical_all_nodes_0.95"] = band["critical"]
        print(f"  critical value of the 0.95 band over all {size} nodes: {band['critical']:.4f} (pointwise normal quantile: 1.96)", flush=True)
        eng.check_status()
        eng.close()
        del x, M
        torch.cuda.empty_cache()
        return rec

    def forms(eng, x, cases, row, base=None):
        """every case under reduce_algo 1, 2 and 0; returns {case: (short ms, long ms, auto ms)}"""
        got = {}
        for label, fn in cases:
            t = []
            for algo, name in ((1, "short"), (2, "long"), (0, "auto")):
                eng.set_option("reduce_algo", algo)
                t.append(timed(fn))
                row(f"omc_store_reduce {label}, {name} form", t[-1], base)
            got[label] = [v[0] for v in t]
        eng.set_option("reduce_algo", 0)
        return got

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
        assert torch.equal(eng.store_reduce(x, "sum")[1], live[:, :, 0])
        # ("count" is the count output of any op: the cheapest is taken)
        rec["forms_ms"] = forms(eng, x, [("count (count output of min)", lambda: eng.store_reduce(x, "min")),
                                         ("sum", lambda: eng.store_reduce(x, "sum")), ("max", lambda: eng.store_reduce(x, "max"))], row, t_mom[0])
        row("torch (~isnan(x)).sum(-1)", timed(lambda: (~torch.isnan(x)).sum(-1)), t_mom[0])
        row("torch.nansum(x, dim=-1)", timed(lambda: torch.nansum(x, dim=-1)), t_mom[0])
        row("torch.nan_to_num(x, nan=-inf).amax(-1)", timed(lambda: torch.nan_to_num(x, nan=float("-inf")).amax(-1)), t_mom[0])
        eng.close()
        return rec

    def sweep():
        rec = {"rows": [], "forms_ms": {}}
        C = 256
        print(f"sweep: stores of {args.sweep_GB} GB, {C} chains, normal draws", flush=True)
        for size in (20, 32, 64, 128, 256, 512, 1024, 2048, 4096):
            n_iter = max(1, int(args.sweep_GB * 1e9 / (8 * C * size)))
            eng = Engine(C, seed=3)
            x = torch.randn((n_iter, C, size), dtype=torch.float64, device=eng.device)
            row = table(rec, 8.0 * n_iter * C * size)
            rec["forms_ms"][size] = forms(eng, x, [(f"sum, size {size}", lambda: eng.store_reduce(x, "sum")),
                                                   (f"max, size {size}", lambda: eng.store_reduce(x, "max"))], row)
            eng.close()
            del x
        return rec

    out = {"reps": args.reps, "cfg3": cfg3(), "rj": rj(), "sweep": sweep()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
