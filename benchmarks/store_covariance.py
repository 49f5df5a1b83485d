#!/usr/bin/env python3
"""Posterior covariance of the device store (omc_store_cov) against the project's own MFMA contraction without centring.

    python3 benchmarks/store_covariance.py [--reps 12] [--cfg2-iters 500] [--cfg2-chains 256] [--cfg2-size 1000]
                                           [--cfg3-iters 64] [--cfg3-chains 1024] [--cfg3-size 10000] [--cfg3-index 512]

Prints one JSON line.  Two stores filled with normal draws around means of 1e3 sd on the device:
  cfg2-like  500 iterations x 256 chains x 1000 coefficients (R = 128 000 draws, 1 GB): pooled symmetric covariance;
  cfg3       64 iterations x 1024 chains x 10 000 nodes (5.2 GB): pooled covariance of a contiguous index of 512 nodes.
Per store: omc_store_cov (median of --reps calls timed one by one with device events, after a warm-up call), and in the same
process on the same card the yardstick t_gram + t_moments: omc_gram on the same shape (n = R, p = size, no weights; for
cfg3 on a packed copy of the 512 columns) and omc_store_moments of what the covariance's means pass reads (the whole
store; for cfg3 the packed copy); ratio = t_cov / (t_gram + t_moments).  Beside them torch.cov on the same tensor where its
centred copy fits, the per-chain form, the correlation, and the difference between the covariance and torch.cov's.
"""
import argparse
import json
import os
import sys

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

    def timed(fn):
        """median ms of --reps calls, each between its own pair of device events, after one warm-up call"""
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

    def fill(eng, n_iter, C, size, seed):
        g = torch.Generator(device=eng.device)
        g.manual_seed(seed)
        x = torch.empty((n_iter, C, size), dtype=torch.float64, device=eng.device)
        sd = 10.0 ** torch.linspace(-2, 2, size, dtype=torch.float64, device=eng.device)
        for i in range(n_iter):  # (slab by slab: no second store-sized temporary)
            z = torch.randn((C, size), generator=g, dtype=torch.float64, device=eng.device)
            x[i] = (z + 0.6 * torch.roll(z, 1, dims=-1) + 1e3) * sd
        return x

    def measure(n_iter, C, size, n_index, seed):
        eng = Engine(C, seed=3)
        x = fill(eng, n_iter, C, size, seed)
        R = n_iter * C
        idx = None if n_index is None else torch.arange(size // 4, size // 4 + n_index, device=eng.device)
        p = size if idx is None else n_index
        t_cov, cov = timed(lambda: eng.store_cov(x, index_a=idx))
        rec = {"store": f"{n_iter} iterations x {C} chains x {size}", "store_GB": 8 * R * size / 1e9, "draws": R,
               "elements": p, "index": None if idx is None else f"contiguous, {n_index} from {size // 4}", "cov_ms": t_cov,
               "cov_TFLOPs": 2.0 * R * p * p / (t_cov * 1e-3) / 1e12}
        packed = x.reshape(R, size) if idx is None else x.reshape(R, size)[:, size // 4: size // 4 + n_index].contiguous()
        t_gram, _ = timed(lambda: eng.gram(packed))
        eng_m = Engine(1, seed=3)  # (the packed columns as a one-chain store of R iterations)
        t_mom, _ = timed(lambda: eng_m.store_moments(packed.unsqueeze(1), pooled=True))
        rec.update({"gram_ms": t_gram, "moments_ms": t_mom, "ratio_cov_over_gram_plus_moments": t_cov / (t_gram + t_mom)})
        rec["correlation_ms"], _ = timed(lambda: eng.store_cov(x, index_a=idx, correlation=True))
        if idx is not None or C * p * p * 8 <= 4e9:
            rec["per_chain_ms"], _ = timed(lambda: eng.store_cov(x, index_a=idx, pooled=False))
        try:  # torch.cov makes a centred copy of what it is given
            t_torch, tc = timed(lambda: torch.cov(packed.T))
            sd = torch.sqrt(torch.diagonal(tc))
            rec.update({"torch_cov_ms": t_torch, "max_scaled_diff_to_torch_cov": float(((cov - tc).abs() / torch.outer(sd, sd)).max())})
            del tc
        except RuntimeError as e:  # out of memory
            rec["torch_cov_ms"] = None
            rec["torch_cov_error"] = str(e).splitlines()[0][:120]
        eng.check_status()
        eng_m.close()
        eng.close()
        del x, packed
        torch.cuda.empty_cache()
        return rec

    out = {"reps": args.reps,
           "cfg2": measure(args.cfg2_iters, args.cfg2_chains, args.cfg2_size, None, 5),
           "cfg3": measure(args.cfg3_iters, args.cfg3_chains, args.cfg3_size, args.cfg3_index, 6)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
