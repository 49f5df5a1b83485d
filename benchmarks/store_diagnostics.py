#!/usr/bin/env python3
"""Split R-hat and ESS of the device store (omc_store_rhat_ess) at the headline size and on a long store.

    python3 benchmarks/store_diagnostics.py [--iters 128] [--chains 1024] [--nodes 10000]
                                            [--long-iters 4000] [--long-chains 512] [--long-size 500]

Prints one JSON line.  Stores: the cfg3 store (store["b"] of GmrfSweep.run_fused: iters x chains x nodes; M = iters / 2
<= 64 takes the one-read short-series form) and a long AR(1) store (one coefficient per element from -0.5 to 0.95; blocks
of 32 lags).  Per store: wall time (device events, warmed, repeated), lag blocks and max(lags), the reads of the store the
algorithm makes (8 N C size bytes each) and the FMAs of its lag sums, the achieved rates and the share of peak, named for
whichever of HBM (8.0 TB/s spec) and fp64 vector issue (78.6 TFLOP/s spec = 39.3 T FMA/s) bounds it.  Host route: the same
diagnostics from a host copy (the transfer collect() makes plus a vectorised numpy restatement) on a slice that fits.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12       # bytes/s (MI355X spec)
FMA_PEAK = 78.6e12 / 2  # fp64 vector FMA/s (MI355X spec)
L, S_L, SHORT_MAX = 32, 16, 64  # lags per block (long form), lags per wave (short form), longest short half-series


def cost(N, C, size, max_lag):
    """(reads of the store, lag-sum FMAs, lag blocks) of omc_store_rhat_ess, from the shape and max(lags)"""
    M, J = N // 2, 2 * C
    if M <= SHORT_MAX:
        fma = sum(math.ceil(max(M - S_L * b, 0) / S_L) * S_L * S_L for b in range(SHORT_MAX // S_L))
        return 1, J * size * fma, 1
    blocks = min((max_lag + 1) // L + 1, math.ceil(M / L))
    fma = sum(math.ceil((M - L * b) / L) * L * L for b in range(blocks))
    return 1 + 1 + 2 * (blocks - 1), J * size * fma, blocks


def host_route(x):
    """rhat, ess of a host store x (N, C, size): direct lag sums vectorised over elements, Geyer per element"""
    N, C, size = x.shape
    M, J = N // 2, 2 * C
    xs = np.concatenate([x[:M], x[N - M:]], axis=1)  # (M, J, size)
    m = xs[0] + (xs - xs[0]).mean(axis=0)
    y = xs - m
    g = np.stack([np.einsum("ijk,ijk->k", y[: M - t], y[t:]) for t in range(M)]) / (J * M)  # (M, size)
    W = g[0] * M / (M - 1)
    B = m.var(axis=0, ddof=1)
    vp = W * (M - 1) / M + B
    rhat = np.sqrt(vp / W)
    rho = 1 - (W - g) / vp
    ess = np.empty(size)
    for k in range(size):
        r = np.zeros(M)
        r[0], even, odd, t = 1.0, 1.0, rho[1, k], 1
        r[1] = odd
        while t < M - 3 and even + odd > 0:
            even, odd = rho[t + 1, k], rho[t + 2, k]
            if even + odd >= 0:
                r[t + 1], r[t + 2] = even, odd
            t += 2
        max_t = t - 2
        if even > 0:
            r[max_t + 1] = even
        t = 1
        while t <= max_t - 2:
            if r[t + 1] + r[t + 2] > r[t - 1] + r[t]:
                r[t + 1] = r[t + 2] = (r[t - 1] + r[t]) / 2
            t += 2
        tau = max(-1 + 2 * np.sum(r[: max_t + 1]) + r[max_t + 1], 1 / np.log10(J * M))
        ess[k] = J * M / tau
    return rhat, ess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=128)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--long-iters", type=int, default=4000)
    ap.add_argument("--long-chains", type=int, default=512)
    ap.add_argument("--long-size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-size", type=int, default=100)
    args = ap.parse_args()
    import torch

    from bench import GmrfSweep
    from openmcmc_amd.engine import Engine

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, r

    def measure(eng, store, tag):
        N, C, size = store.shape
        ms, (rhat, ess, lags) = timed(lambda: eng.store_rhat_ess(store), args.reps)
        max_lag = int(lags.max().item())
        reads, fmas, blocks = cost(N, C, size, max_lag)
        nbytes = 8 * N * C * size
        t = ms * 1e-3
        hbm_t, fma_t = reads * nbytes / HBM_PEAK, fmas / FMA_PEAK
        r = rhat.cpu().numpy()
        return {"store": f"{N} iterations x {C} chains x {size}", "store_GB": nbytes / 1e9, "ms": ms,
                "form": "short-series (one read)" if N // 2 <= SHORT_MAX else "lag blocks", "lag_blocks": blocks,
                "max_lags": max_lag, "reads": reads, "GB_read": reads * nbytes / 1e9, "TBps": reads * nbytes / t / 1e12,
                "TBps_per_read": nbytes / (t / reads) / 1e12, "GFMA": fmas / 1e9, "TFMAps": fmas / t / 1e12,
                "bound": "HBM" if hbm_t >= fma_t else "fp64 issue", "share_of_peak": max(hbm_t, fma_t) / t,
                "rhat_median": float(np.nanmedian(r)), "ess_median": float(np.nanmedian(ess.cpu().numpy()))}

    out = {}
    # cfg3 store
    n, C, K = args.nodes, args.chains, args.iters
    sw = GmrfSweep(n, C, seed=7, chain_offset=0, device=0, n_store=K)
    sw.run_fused(K + 8)
    torch.cuda.synchronize()
    store = sw.store_b
    eng = sw.eng
    out["cfg3"] = measure(eng, store, "cfg3")
    # host route on a slice of the same store: the transfer plus the numpy restatement, against the device on that slice
    sl = store[:, :, : args.host_size].contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = sl.cpu().numpy()
    t1 = time.perf_counter()
    hr, he = host_route(host)
    t2 = time.perf_counter()
    ms_dev, (dr, de, _) = timed(lambda: eng.store_rhat_ess(sl), args.reps)
    out["host_route"] = {"store": f"{K} iterations x {C} chains x {args.host_size}", "transfer_s": t1 - t0, "numpy_s": t2 - t1,
                         "device_ms": ms_dev, "speedup": (t2 - t0) / (ms_dev * 1e-3),
                         "max_rel_diff_rhat": float(np.max(np.abs(dr.cpu().numpy() / hr - 1))),
                         "max_rel_diff_ess": float(np.max(np.abs(de.cpu().numpy() / he - 1)))}
    eng.check_status()
    del store, sl, sw, eng
    torch.cuda.empty_cache()

    # long store: AR(1) filled on the device, one coefficient per element
    N, C2, size = args.long_iters, args.long_chains, args.long_size
    eng = Engine(C2, seed=3)
    g = torch.Generator(device=eng.device)
    g.manual_seed(11)
    phi = torch.linspace(-0.5, 0.95, size, dtype=torch.float64, device=eng.device)
    s = torch.sqrt(1 - phi * phi)
    x = torch.empty((N, C2, size), dtype=torch.float64, device=eng.device)
    x[0] = torch.randn((C2, size), generator=g, dtype=torch.float64, device=eng.device)
    for i in range(1, N):
        x[i] = phi * x[i - 1] + s * torch.randn((C2, size), generator=g, dtype=torch.float64, device=eng.device)
    torch.cuda.synchronize()
    out["long"] = measure(eng, x, "long")
    eng.check_status()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
