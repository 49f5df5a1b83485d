#!/usr/bin/env python3
"""The ESS of quantile indicators on the device store (omc_store_ess_indicator) beside the route the library offered before it.

    python3 benchmarks/store_ess.py [--shapes cfg3,cfg4,thin] [--reps 5] [--out profiles/store_ess.txt]

Prints a table (also written to --out) and one JSON line.  Workloads:
  cfg3   512 indexed nodes of the cfg3 store (128 iterations x 1024 chains x 10 000 nodes, store["b"] of GmrfSweep.run_fused), at 2
         probabilities (the pair behind ess_tail) and at the 20 of az.plot_ess(kind="quantile");
  cfg4   a cfg4-shaped store (2000 x 512 x 500, iid normal), 16 elements, 20 probabilities;
  thin   the long thin store of benchmarks/store_autocorr.py (100 000 x 4 chains x 4 elements, AR(1) with phi = 0.9), 20 probabilities.
Each is timed -- medians of --reps calls timed one by one with device events after a warm-up call, one process, one card -- against
  (a) the fp64 route: the indicator series written as an fp64 store [N][C][n_p n_idx] with torch (thresholds given), then
      Engine.store_rhat_ess over it -- what omc_store_rank_diagnostics does for its two tails;
  (b) omc_store_ranks (split) on the same columns: the sort both routes pay, with the bisections of the ranks.
The split of one call into sort / thresholds / pack / lags comes from torch.profiler's kernel records of one further call, and the
pack pass is set beside omc_store_moments over the same bytes (the gathered selection).  No threshold is attached to any number."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,cfg4,thin")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "store_ess.txt"))
    args = ap.parse_args()
    import torch

    from openmcmc_amd.engine import Engine

    lines, rows = [], []

    def say(text):
        print(text, flush=True)
        lines.append(text)

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

    def row(shape, label, ms, note=""):
        rows.append({"shape": shape, "case": label, "ms": ms})
        say(f"  {shape:<5s} {label:<92s} {ms:10.3f} ms  {note}")

    def kernel_split(fn):
        """device time of one call by stage, from the profiler's kernel records (None where the profiler gives none)"""
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            split = {"sort": 0.0, "thresholds": 0.0, "pack": 0.0, "lags": 0.0}
            for ev in prof.events():
                name = ev.name
                us = float(ev.device_time_total if hasattr(ev, "device_time_total") else ev.cuda_time_total)
                for stage, pieces in (("sort", ("k_rank_gather", "k_rank_sort")), ("thresholds", ("k_essq_thresholds",)),
                                      ("pack", ("k_essq_pack",)), ("lags", ("k_essq_lags",))):
                    if any(p in name for p in pieces):
                        split[stage] += us / 1e3
            return split if sum(split.values()) > 0 else None
        except Exception as exc:  # the numbers above do not depend on it
            say(f"        (no kernel records: {type(exc).__name__}: {exc})")
            return None

    def shape_rows(shape, eng, store, idx, probs):
        N, C, size = store.shape
        n_idx = size if idx is None else idx.numel()
        sel_of = (lambda: store) if idx is None else (lambda: store[:, :, idx].contiguous())
        n_p = len(probs)
        new = lambda: eng.store_ess_indicator(store, None, probs, index=idx)  # noqa: E731
        ms_new = timed(new)
        ess, lags, q = new()
        row(shape, f"omc_store_ess_indicator, {n_p} probabilities x {n_idx} elements, whole call", ms_new,
            f"longest sequence {int(lags.max())} lags")

        def fp64_route():
            sel = sel_of()
            ind = (sel.unsqueeze(2) <= q[:, :, 1].unsqueeze(0).unsqueeze(0)).to(torch.float64).reshape(N, C, n_p * n_idx)
            return eng.store_rhat_ess(ind)[1]

        ms_old = timed(fp64_route)
        dev = float(((fp64_route().reshape(n_p, n_idx) - ess).abs() / ess).max())
        row(shape, f"(a) fp64 route: indicators as an fp64 store of {8e-9 * N * C * n_p * n_idx:.2f} GB with torch + omc_store_rhat_ess", ms_old,
            f"{ms_old / ms_new:.2f} x the new route; largest relative deviation of the ESS {dev:.1e}")
        ms_rank = timed(lambda: eng.store_ranks(store, index=idx, split=True))
        row(shape, "(b) omc_store_ranks, split, same columns (one sort, the bisections, ranks written)", ms_rank, f"{ms_rank / ms_new:.2f} x the new route")
        sel = sel_of()
        ms_mom = timed(lambda: eng.store_moments(sel, pooled=True))
        split = kernel_split(new)
        if split:
            say("        one call by stage: " + ", ".join(f"{k} {v:.3f} ms" for k, v in split.items())
                + f"; pack / omc_store_moments over the same bytes ({ms_mom:.3f} ms) = {split['pack'] / ms_mom:.2f}")
            rows.append({"shape": shape, "case": f"stages at {n_p} probabilities", **split, "moments_ms": ms_mom})
        return ms_new, ms_old

    shapes = args.shapes.split(",")
    p20 = np.linspace(0.05, 0.95, 20)
    if "cfg3" in shapes:
        from bench import GmrfSweep

        n, C, K = 10000, 1024, 128
        sw = GmrfSweep(n, C, seed=7, chain_offset=0, device=0, n_store=K)
        sw.run_fused(K + 8)
        torch.cuda.synchronize()
        idx = torch.arange(n // 4, n // 4 + 512, device=sw.store_b.device)
        say(f"cfg3 store: {K} iterations x {C} chains x {n} nodes, 512 indexed nodes")
        shape_rows("cfg3", sw.eng, sw.store_b, idx, np.array([0.05, 0.95]))
        shape_rows("cfg3", sw.eng, sw.store_b, idx, p20)
        tail = sw.eng.store_rank_diagnostics(sw.store_b, index=idx)[2]
        two = sw.eng.store_ess_indicator(sw.store_b, None, [0.05, 0.95], index=idx)[0].min(dim=0).values
        say(f"        min over p = 0.05, 0.95 against ess_tail of omc_store_rank_diagnostics: largest relative deviation "
            f"{float(((two - tail).abs() / tail).max()):.1e}")
        del sw
        torch.cuda.empty_cache()
    if "cfg4" in shapes:
        eng = Engine(512, seed=1)
        store = torch.randn((2000, 512, 500), dtype=torch.float64, device=eng.device, generator=torch.Generator(device=eng.device).manual_seed(4))
        say("cfg4-shaped store: 2000 iterations x 512 chains x 500 elements (iid), 16 indexed elements")
        shape_rows("cfg4", eng, store, torch.arange(100, 116, device=store.device), p20)
        del store
        eng.close()
        torch.cuda.empty_cache()
    if "thin" in shapes:
        eng = Engine(4, seed=1)
        rng = np.random.default_rng(5)
        e = rng.standard_normal((100000, 4, 4))
        x = np.empty_like(e)
        x[0] = e[0] / np.sqrt(1 - 0.81)
        for i in range(1, len(e)):
            x[i] = 0.9 * x[i - 1] + e[i]
        store = eng.to_device(x)
        say("long thin store: 100 000 iterations x 4 chains x 4 elements (AR(1), phi = 0.9)")
        shape_rows("thin", eng, store, None, p20)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
