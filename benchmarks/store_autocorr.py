#!/usr/bin/env python3
"""Autocorrelation of the device store (omc_store_autocorr) beside what a user can do without it on the same columns.

    python3 benchmarks/store_autocorr.py [--reps 5] [--skip-host]

Prints a table and one JSON line.  Three shapes:
  cfg3   512 indexed nodes of the cfg3 store (store["b"] of GmrfSweep.run_fused: 128 iterations x 1024 chains x 10 000 nodes),
         max_lag 100, pooled and per chain;
  cfg4   every element of a cfg4-shaped store (2000 x 512 chains x 500, normal draws), max_lag 100;
  thin   100 000 draws x 4 chains x 4 elements (AR(1), phi = 0.9), max_lag 1000: what the time slices exist for.
Timings are medians of --reps calls timed one by one with device events after a warm-up call, in one process on one card:
  omc_store_autocorr, whole call (means, pre-pass, lag kernel, join);
  the torch route: the selected columns gathered and centred, torch.fft.rfft of the zero-padded columns, |.|^2, irfft, fp64 on the device;
  the host route, by the wall clock, once: the gathered selection copied to the host, then the same FFT route in numpy
    (cfg4: on the first 32 elements only, and said so).
The device result is compared with the torch route's before anything is printed.  Beside the times: the call's share of the FMA
floor, cols * N * (max_lag + 1) FMAs at the 78.6 TFLOP/s fp64 vector peak, and the store bytes its kernels read, counted from the
shapes, over one read of the selected columns.  No threshold is attached to these numbers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FMA_PER_S = 78.6e12 / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--shapes", default="cfg3,cfg4,thin")
    args = ap.parse_args()
    import torch

    from bench import GmrfSweep
    from openmcmc_amd.engine import Engine

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

    def fft_route(xp, sel, L, pooled):
        """autocovariance (..., n, L + 1) of gathered columns sel (N, C, n) by the FFT; xp is torch or numpy"""
        N = sel.shape[0]
        P = 1
        while P < N + L:
            P <<= 1
        d = sel - sel.mean(0, keepdims=True) if xp is np else sel - sel.mean(0, keepdim=True)
        F = xp.fft.rfft(d, n=P, axis=0) if xp is np else xp.fft.rfft(d, n=P, dim=0)
        power = F.real ** 2 + F.imag ** 2
        g = (xp.fft.irfft(power, n=P, axis=0) if xp is np else xp.fft.irfft(power, n=P, dim=0))[: L + 1] / N  # (L + 1, C, n)
        return xp.moveaxis(g.mean(1), 0, -1) if pooled else xp.moveaxis(g, 0, -1)

    rows = []

    def row(shape, label, ms, extra=""):
        rows.append({"shape": shape, "case": label, "ms": ms})
        print(f"  {shape:<5s} {label:<72s} {ms:10.3f} ms  {extra}", flush=True)

    def shape_rows(name, eng, store, idx, L, poolings, host_elements=None):
        N, C, size = store.shape
        n = size if idx is None else idx.numel()
        cols = C * n
        n_lb = L // 32 + 1
        floor_ms = 1e3 * cols * N * (L + 1) / FMA_PER_S
        once = 8.0 * N * cols  # bytes of one read of the selected columns
        # the means and the pre-pass read the selected columns once each; the lag kernel reads the store itself only without an index
        reads = 2 if idx is not None else 2 + 2 * n_lb - 1
        own = 0 if idx is None else once * (1 + 2 * n_lb - 1)  # the centred copy: written once, read by the lag kernel
        print(f"{name}: store {N} x {C} x {size} ({8e-9 * N * C * size:.2f} GB), {n} {'indexed ' if idx is not None else ''}elements = {cols} "
              f"columns of {N} draws, max_lag {L}: FMA floor {floor_ms:.3f} ms; one read of the selected columns {once / 1e9:.3f} GB, "
              f"the call reads the store {reads} times over that ({reads * once / 1e9:.2f} GB)"
              + (f" and moves {own / 1e9:.2f} GB of its centred copy" if own else ""), flush=True)
        sel_of = (lambda: store) if idx is None else (lambda: store[:, :, idx])
        for pooled in poolings:
            tag = "pooled" if pooled else "per chain"
            got = eng.store_autocorr(store, L, index=idx, pooled=pooled, normalize=False)[0]
            want = fft_route(torch, sel_of(), L, pooled)
            eng.check_status()
            scale = want[..., :1].abs().clamp_min(1e-300)
            dev = float(((got - want).abs() / scale).max())
            assert dev < 1e-9, (name, tag, dev)
            del got, want, scale
            ms = timed(lambda: eng.store_autocorr(store, L, index=idx, pooled=pooled))
            row(name, f"omc_store_autocorr {tag}, whole call", ms, f"FMA floor / time = {floor_ms / ms:.3f}; largest deviation from the torch route {dev:.1e} of g(0)")
            ms_t = timed(lambda: fft_route(torch, sel_of(), L, pooled))
            row(name, f"torch route {tag}: gather, centre, rfft, |.|^2, irfft (fp64, device)", ms_t, f"{ms_t / ms:.2f} x omc_store_autocorr")
        if not args.skip_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = sel_of().contiguous().cpu().numpy()
            t1 = time.perf_counter()
            part = host if host_elements is None else host[:, :, :host_elements]
            fft_route(np, part, L, True)
            t2 = time.perf_counter()
            row(name, "host route: gather of the selection and transfer (wall clock, once)", 1e3 * (t1 - t0))
            row(name, "host route: numpy FFT route, pooled" + ("" if host_elements is None else f", first {host_elements} elements only")
                + " (wall clock, once)", 1e3 * (t2 - t1))

    shapes = args.shapes.split(",")
    if "cfg3" in shapes:
        n, C, K = 10000, 1024, 128
        sw = GmrfSweep(n, C, seed=7, chain_offset=0, device=0, n_store=K)
        sw.run_fused(K + 8)
        torch.cuda.synchronize()
        idx = torch.arange(n // 4, n // 4 + 512, device=sw.store_b.device)
        shape_rows("cfg3", sw.eng, sw.store_b, idx, 100, (True, False))
        del sw
        torch.cuda.empty_cache()
    if "cfg4" in shapes:
        eng = Engine(512, seed=1)
        store = torch.randn((2000, 512, 500), dtype=torch.float64, device=eng.device, generator=torch.Generator(device=eng.device).manual_seed(4))
        shape_rows("cfg4", eng, store, None, 100, (True,), host_elements=32)
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
        shape_rows("thin", eng, store, None, 1000, (True, False))
        tau = eng.store_autocorr(store, 1000)[1].cpu().numpy()
        print(f"  thin  tau of the four elements {np.round(tau, 2).tolist()} ((1 + phi) / (1 - phi) = 19)")
        eng.close()
    print(json.dumps({"reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
