#!/usr/bin/env python3
"""First failures of the device store (omc_store_first_failure, the pass behind MCMC.excursion and MCMC.contour_map) beside the
nearest existing pass over the same bytes, omc_store_reduce COUNT_ABOVE, and beside the torch expression of the same counts that a
user would write outside the library: compare, permuted where, amin, bincount.

    python3 benchmarks/store_excursion.py [--reps 9] [--iters 128] [--chains 1024] [--nodes 10000] [--index 512]
                                          [--rj-iters 2000] [--rj-chains 512] [--rj-slots 20] [--sweep-GB 0.5]

Prints a table and one JSON line.  One process on one card; every time is the median of --reps calls timed one by one with device
events after a warm-up call, with the smallest and largest of them beside it, as store bytes per second and as a ratio to
COUNT_ABOVE of the same selection.  The times of omc_store_first_failure include its validation (one read-back of two words).
  cfg3   --iters x --chains x --nodes draws of a planted smooth field plus noise (128 x 1024 x 10 000: 10.5 GB): all nodes with 1, 2
         and 8 slots, --index indexed nodes with 1 and 8 slots; the torch expression for one slot (it makes two store-sized
         temporaries per slot); MCMC.excursion at one and at eight levels and MCMC.contour_map end to end (wall clock).
  short  --rj-iters x --rj-chains x --rj-slots (2000 x 512 x 20): 1 and 8 slots under the short form, the long form and the automatic
         choice.
  sweep  stores of --sweep-GB with rows of 20 .. 1024 elements, one slot under both forms -- where the automatic choice switches.
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
    ap.add_argument("--sweep-GB", type=float, default=0.5)
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
            text = f"  {label:<72s} {ms:9.3f} ms [{lo:8.3f} .. {hi:8.3f}]"
            if bytes_read:
                r["TB_per_s"] = bytes_read / (ms * 1e-3) / 1e12
                text += f" {r['TB_per_s']:6.2f} TB/s"
            if base is not None:
                r["ratio_to_count_above"] = ms / base
                text += f"   x{ms / base:5.2f} of count_above"
            rec["rows"].append(r)
            print(text, flush=True)
        return row

    def slots(x, L, index, level):
        """(lo, hi, pos) (L, n) device tables: slot l is the positive excursion at level + 0.1 l, ordered by the marginal counts"""
        sel_mean = x.mean(dim=(0, 1)) if index is None else x[:, :, index].mean(dim=(0, 1))
        n = sel_mean.numel()
        lo = torch.stack([torch.full((n,), level + 0.1 * l, dtype=torch.float64, device=x.device) for l in range(L)])
        hi = torch.full((L, n), float("inf"), dtype=torch.float64, device=x.device)
        order = torch.argsort(-sel_mean, stable=True)  # (a stand-in for the order by counts: the field's mean ranks the nodes alike)
        pos1 = torch.empty(n, dtype=torch.int64, device=x.device)
        pos1[order] = torch.arange(n, device=x.device)
        return lo, hi, pos1.repeat(L, 1).contiguous()

    def torch_counts(x, index, lo, hi, pos):
        """h (n + 1,) of one slot in torch: compare, permuted where, amin, bincount"""
        sel = x.reshape(-1, x.shape[2]) if index is None else x.reshape(-1, x.shape[2])[:, index]
        n = sel.shape[1]
        agree = (sel > lo) & (sel < hi)  # (finite lo, hi = +inf; a NaN compares false)
        r = torch.where(agree, n, pos.to(torch.int32)).amin(dim=1)
        return torch.bincount(r, minlength=n + 1)

    def mcmc_over(eng, x, n_iter):
        M = MCMC.__new__(MCMC)  # the summaries need the engine, the store and the ring fields only
        M.engine, M.store, M._derived, M.store_ring, M.n_iter, M._n_dev = eng, {"x": x}, set(), 0, n_iter, n_iter
        return M

    def cfg3():
        n_iter, C, size = args.iters, args.chains, args.nodes
        eng = Engine(C, seed=3)
        g = torch.Generator(device=eng.device)
        g.manual_seed(6)
        field = 2.5 * torch.sin(torch.linspace(0, 3.14159, size, dtype=torch.float64, device=eng.device))  # above 0 inside, near it at the ends
        x = torch.empty((n_iter, C, size), dtype=torch.float64, device=eng.device)
        for i in range(n_iter):  # (slab by slab: no second store-sized temporary)
            x[i] = 0.5 * torch.randn((C, size), generator=g, dtype=torch.float64, device=eng.device) + field
        nbytes = 8.0 * n_iter * C * size
        rec = {"store": f"{n_iter} iterations x {C} chains x {size}", "store_GB": nbytes / 1e9, "rows": []}
        row = table(rec, nbytes)
        print(f"cfg3: {rec['store']} ({rec['store_GB']:.2f} GB)", flush=True)
        idx = torch.arange(size // 4, size // 4 + args.index, device=eng.device)
        for what, index in (("all nodes", None), (f"{args.index} indexed nodes", idx)):
            n = size if index is None else args.index
            thr = torch.zeros(n, dtype=torch.float64, device=eng.device)
            t_cnt = timed(lambda: eng.store_reduce(x, "count_above", index=index, a=thr))
            # (an indexed call does not read the whole store: no bytes per second for it)
            row(f"omc_store_reduce count_above, {what} (yardstick)", t_cnt, None, nbytes if index is None else None)
            for L in ((1, 2, 8) if index is None else (1, 8)):
                lo, hi, pos = slots(x, L, index, 0.0)
                row(f"omc_store_first_failure, {L} slot(s), {what}", timed(lambda: eng.store_first_failure(x, lo, hi, pos, index=index)),
                    t_cnt[0], nbytes if index is None else None)
                if L == 1:
                    row(f"the same with the rows written (want_rows), {what}",
                        timed(lambda: eng.store_first_failure(x, lo, hi, pos, index=index, want_rows=True)), t_cnt[0],
                        nbytes if index is None else None)
            lo, hi, pos = slots(x, 8, index, 0.0)
            h = eng.store_first_failure(x, lo, hi, pos, index=index)[0]
            for l in (0, 7):  # what the results must be (same inputs, the sizes timed)
                assert torch.equal(h[l], torch_counts(x, index, lo[l], hi[l], pos[l]))
            torch.cuda.empty_cache()
            row(f"torch: where(compare, n, pos).amin(1), bincount -- ONE slot, {what}",
                timed(lambda: torch_counts(x, index, lo[0], hi[0], pos[0])), t_cnt[0], nbytes if index is None else None)
            torch.cuda.empty_cache()
            rec[f"rows_agreeing_everywhere, {what}"] = [int(v) for v in h[:, -1].cpu().numpy()]
        M = mcmc_over(eng, x, n_iter)
        row("MCMC.excursion, one level, all nodes, end to end, wall clock", wall(lambda: M.excursion("x", 0.0)), None, None)
        levels = [0.1 * l for l in range(8)]
        row("MCMC.excursion, eight levels, all nodes, end to end, wall clock", wall(lambda: M.excursion("x", levels)), None, None)
        row("MCMC.contour_map, four levels, all nodes, end to end, wall clock", wall(lambda: M.contour_map("x", [0.5, 1.0, 1.5, 2.0])), None, None)
        out = M.excursion("x", 0.0)
        rec["set_sizes"] = {"joint_0.95": int(out["set"].sum()), "pointwise_0.95": int((out["marginal"] >= 0.95).sum())}
        print(f"  nodes in the 0.95 excursion set above 0: {rec['set_sizes']['joint_0.95']}; nodes with P(x > 0) >= 0.95: "
              f"{rec['set_sizes']['pointwise_0.95']}", flush=True)
        eng.check_status()
        eng.close()
        del x, M
        torch.cuda.empty_cache()
        return rec

    def forms(eng, cases, row, base=None):
        """every case under algo 1, 2 and 0; returns {case: (short ms, long ms, auto ms)}"""
        got = {}
        for label, fn in cases:
            t = []
            for algo, name in ((1, "short"), (2, "long"), (0, "auto")):
                t.append(timed(lambda: fn(algo)))
                row(f"omc_store_first_failure {label}, {name} form", t[-1], base)
            got[label] = [v[0] for v in t]
        return got

    def short():
        n_iter, C, size = args.rj_iters, args.rj_chains, args.rj_slots
        eng = Engine(C, seed=3)
        g = torch.Generator(device=eng.device)
        g.manual_seed(7)
        x = torch.randn((n_iter, C, size), generator=g, dtype=torch.float64, device=eng.device) + 1.5
        nbytes = 8.0 * n_iter * C * size
        rec = {"store": f"{n_iter} iterations x {C} chains x {size}", "store_GB": nbytes / 1e9, "rows": []}
        row = table(rec, nbytes)
        print(f"short: {rec['store']} ({rec['store_GB']:.3f} GB)", flush=True)
        thr = torch.zeros(size, dtype=torch.float64, device=eng.device)
        t_cnt = timed(lambda: eng.store_reduce(x, "count_above", a=thr))
        row("omc_store_reduce count_above (yardstick)", t_cnt)
        tabs = {L: slots(x, L, None, 0.0) for L in (1, 8)}
        assert torch.equal(eng.store_first_failure(x, *tabs[8], algo=1)[0], eng.store_first_failure(x, *tabs[8], algo=2)[0])
        rec["forms_ms"] = forms(eng, [(f"{L} slot(s)", lambda algo, L=L: eng.store_first_failure(x, *tabs[L], algo=algo)) for L in (1, 8)],
                                row, t_cnt[0])
        row("torch: where(compare, n, pos).amin(1), bincount -- ONE slot", timed(lambda: torch_counts(x, None, *(v[0] for v in tabs[1]))), t_cnt[0])
        eng.close()
        return rec

    def sweep():
        rec = {"rows": [], "forms_ms": {}}
        C = 256
        print(f"sweep: stores of {args.sweep_GB} GB, {C} chains, normal draws, one slot", flush=True)
        for size in (20, 64, 128, 256, 512, 1024):
            n_iter = max(1, int(args.sweep_GB * 1e9 / (8 * C * size)))
            eng = Engine(C, seed=3)
            x = torch.randn((n_iter, C, size), dtype=torch.float64, device=eng.device) + 1.5
            row = table(rec, 8.0 * n_iter * C * size)
            tab = slots(x, 1, None, 0.0)
            rec["forms_ms"][size] = forms(eng, [(f"size {size}", lambda algo: eng.store_first_failure(x, *tab, algo=algo))], row)
            eng.close()
            del x
        return rec

    out = {"reps": args.reps, "cfg3": cfg3(), "short": short(), "sweep": sweep()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
