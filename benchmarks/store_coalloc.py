#!/usr/bin/env python3
"""Co-allocation matrix and least-squares partition of the device store (omc_store_coalloc, omc_store_partition_score).

    python3 benchmarks/store_coalloc.py [--reps 7] [--out profiles/store_coalloc.txt] [--small]

Prints a table (also written to --out) and one JSON line.  Stores of fp64 labels drawn uniformly on the device:
  mixture  2000 iterations x 256 chains x 500 coefficients (R = 512 000 draws, 2 GB), all elements, K = 3; also K = 2 and K = 64;
  cfg3     64 iterations x 1024 chains x 10 000 nodes (5.2 GB), a contiguous index of 512 nodes, K = 3, pooled and per chain.
Per case, medians of --reps calls timed one by one with device events after a warm-up call:
  omc_store_coalloc, per_label too; omc_store_partition_score;
  the kernels of one call each (pack, tiles, join, score) from torch.profiler's device times, where it reports them;
  omc_store_cov over the same selection: the fp64 Gram of the same output shape from the same bytes;
  torch on the device: sum_k O_k' O_k with O_k = (Z == k) in fp32 (exact while R < 2^24) for the counts, and
  sum_k rowsum((O_k W) * O_k) in fp64 with W = triu(R - 2 counts, 1) for the scores, both from the fp64 store;
  for the first 8 iterations of cfg3: transfer of the selected columns and the broadcast compare in numpy (one wall-clock call).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = (("pack", "k_coalloc_pack"), ("tiles", "k_coalloc_mfma"), ("join", "k_coalloc_join"), ("score", "k_partition_score"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="stores a hundredth the size (a check of the script)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "store_coalloc.txt"))
    args = ap.parse_args()
    import torch

    from openmcmc_amd.engine import Engine

    lines, rows = [], []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), r

    def per_kernel(fn):
        """{pass: ms} of one call from the profiler's device times; {} where it does not report kernels"""
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            out = {}
            for ev in prof.key_averages():
                t = getattr(ev, "device_time_total", None)
                t = getattr(ev, "cuda_time_total", 0.0) if t is None else t
                for name, kernel in KERNELS:
                    if kernel in ev.key:
                        out[name] = out.get(name, 0.0) + t / 1e3
            return out
        except Exception as err:  # noqa: BLE001 (a profiler that is not there is not the benchmark's failure)
            return {"unavailable": str(err)[:80]}

    def labels(eng, n_iter, C, size, K, seed):
        g = torch.Generator(device=eng.device)
        g.manual_seed(seed)
        x = torch.empty((n_iter, C, size), dtype=torch.float64, device=eng.device)
        step = max(1, n_iter // 16)
        for i in range(0, n_iter, step):  # (slab by slab: no second store-sized temporary)
            x[i:i + step] = torch.randint(0, K, x[i:i + step].shape, generator=g, device=eng.device).to(torch.float64)
        return x

    def torch_counts(x, cols, K, pooled):
        z = x if cols is None else x[:, :, cols[0]:cols[1]]
        z = z.reshape(-1, z.shape[2]) if pooled else z.permute(1, 0, 2)
        out = None
        for k in range(K):
            o = (z == k).to(torch.float32)
            t = o.transpose(-1, -2) @ o
            out = t if out is None else out + t
        return out.to(torch.int64)

    def torch_scores(x, cols, K, counts):
        z = x if cols is None else x[:, :, cols[0]:cols[1]]
        z = z.reshape(-1, z.shape[2])
        W = torch.triu(float(z.shape[0]) - 2.0 * counts.to(torch.float64), 1)
        out = torch.zeros(z.shape[0], dtype=torch.float64, device=z.device)
        for k in range(K):
            o = (z == k).to(torch.float64)
            out += ((o @ W) * o).sum(dim=1)
        return out.to(torch.int64)

    def case(name, eng, x, K, cols, pooled, with_torch=True, with_score=True, with_per_label=True):
        n_iter, C, size = x.shape
        idx = None if cols is None else torch.arange(cols[0], cols[1], device=eng.device)
        n = size if cols is None else cols[1] - cols[0]
        R = n_iter * C if pooled else n_iter
        say(f"{name}: {n_iter} iterations x {C} chains x {size}, {n} elements, K = {K}, {'pooled' if pooled else 'per chain'} "
            f"({8e-9 * n_iter * C * n:.2f} GB of columns, R = {R})")
        rec = {"case": name, "K": K, "elements": n, "rows": R, "pooled": pooled}
        t_cov, _ = timed(lambda: eng.store_cov(x, index_a=idx, pooled=pooled))
        t_co, (counts, _) = timed(lambda: eng.store_coalloc(x, K, index=idx, pooled=pooled))
        rec.update({"cov_ms": t_cov, "coalloc_ms": t_co})
        say(f"  omc_store_cov, the fp64 Gram of the same columns (yardstick)          {t_cov:10.3f} ms")
        say(f"  omc_store_coalloc                                                    {t_co:10.3f} ms   x {t_co / t_cov:6.2f} of the covariance")
        passes = per_kernel(lambda: eng.store_coalloc(x, K, index=idx, pooled=pooled))
        rec["coalloc_passes_ms"] = passes
        say("    one call by kernel: " + ", ".join(f"{k} {v:.3f} ms" if isinstance(v, float) else f"{k}: {v}" for k, v in passes.items()))
        if with_per_label:
            t_pl, _ = timed(lambda: eng.store_coalloc(x, K, index=idx, pooled=pooled, per_label=True))
            rec["coalloc_per_label_ms"] = t_pl
            say(f"  omc_store_coalloc, per_label                                         {t_pl:10.3f} ms")
        if with_score:
            t_sc, (score, _) = timed(lambda: eng.store_partition_score(x, K, counts, index=idx, pooled=pooled))
            rec["score_ms"] = t_sc
            say(f"  omc_store_partition_score                                            {t_sc:10.3f} ms")
            passes = per_kernel(lambda: eng.store_partition_score(x, K, counts, index=idx, pooled=pooled))
            rec["score_passes_ms"] = passes
            say("    one call by kernel: " + ", ".join(f"{k} {v:.3f} ms" if isinstance(v, float) else f"{k}: {v}" for k, v in passes.items()))
        if with_torch:
            t_tc, ref = timed(lambda: torch_counts(x, cols, K, pooled))
            rec.update({"torch_counts_ms": t_tc, "torch_counts_equal": bool(torch.equal(ref, counts))})
            say(f"  torch: sum_k O_k' O_k in fp32 from the fp64 store                    {t_tc:10.3f} ms   x {t_tc / t_co:6.2f} of omc_store_coalloc"
                f"   (equal: {rec['torch_counts_equal']})")
            if with_score and pooled:
                t_ts, ref = timed(lambda: torch_scores(x, cols, K, counts))
                rec.update({"torch_scores_ms": t_ts, "torch_scores_equal": bool(torch.equal(ref, score.reshape(-1)))})
                say(f"  torch: sum_k rowsum((O_k W) * O_k) in fp64                           {t_ts:10.3f} ms   x {t_ts / t_sc:6.2f} of omc_store_partition_score"
                    f"   (equal: {rec['torch_scores_equal']})")
        rows.append(rec)
        return counts

    say("python benchmarks/store_coalloc.py   (one MI355X, one process; medians of %d calls by device events after a warm-up call;" % args.reps)
    say("by kernel: device times of one call from torch.profiler; host row: wall clock of one call; last line: the same as JSON)")
    say("No hardware-counter run has been made: where the time goes is read off these timings and the kernels' structure only.")
    say("")
    f = 100 if args.small else 1
    eng = Engine(256, seed=3)
    for K in (3, 2, 64):
        x = labels(eng, 2000 // f, 256, 500, K, 10 + K)
        case("mixture", eng, x, K, None, True, with_per_label=K != 64)
        del x
        torch.cuda.empty_cache()
    eng.close()
    eng = Engine(1024, seed=3)
    x = labels(eng, max(8, 64 // f), 1024, 10000 // f if args.small else 10000, 3, 5)
    cols = (x.shape[2] // 4, x.shape[2] // 4 + min(512, x.shape[2] // 2))
    case("cfg3", eng, x, 3, cols, True)
    case("cfg3", eng, x, 3, cols, False, with_score=True)
    # the host's way for the first 8 iterations: transfer of the selected columns, then the broadcast compare in row chunks
    t0 = time.perf_counter()
    z = x[:8, :, cols[0]:cols[1]].cpu().numpy().reshape(-1, cols[1] - cols[0])
    t1 = time.perf_counter()
    host = np.zeros((z.shape[1], z.shape[1]), dtype=np.int64)
    for a in range(0, z.shape[0], 256):
        host += (z[a:a + 256, :, None] == z[a:a + 256, None, :]).sum(axis=0)
    t2 = time.perf_counter()
    t_dev, (dev, _) = timed(lambda: eng.store_coalloc(x[:8].contiguous(), 3, index=torch.arange(cols[0], cols[1], device=eng.device)))
    say(f"cfg3, the first 8 iterations ({z.shape[0]} rows x {z.shape[1]} elements)")
    say(f"  host: transfer {1e3 * (t1 - t0):.1f} ms + numpy broadcast compare {1e3 * (t2 - t1):.1f} ms = {1e3 * (t2 - t0):10.1f} ms")
    say(f"  omc_store_coalloc on the same rows                                   {t_dev:10.3f} ms   (equal: {bool(np.array_equal(dev.cpu().numpy(), host))})")
    rows.append({"case": "cfg3 first 8 iterations", "host_transfer_ms": 1e3 * (t1 - t0), "host_compare_ms": 1e3 * (t2 - t1), "coalloc_ms": t_dev})
    eng.close()
    line = json.dumps({"reps": args.reps, "rows": rows})
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n" + line + "\n")
    print(line)


if __name__ == "__main__":
    main()
