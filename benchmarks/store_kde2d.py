#!/usr/bin/env python3
"""Joint kernel density estimates of the device store (MCMC.kde2d: omc_store_minmax, omc_store_histogram2d, omc_kde2d_binned) on the
cfg3-shaped store and a reversible-jump-shaped one, beside the host route and a torch expression of the same convolution.

    python3 benchmarks/store_kde2d.py [--reps 5] [--iters 64] [--chains 1024] [--size 10000] [--pairs 512] [--chain-pairs 64]

Prints a table and one JSON line, in one process on one card:
  MCMC.kde2d end to end (wall clock around a call that ends with the results on the host) for --pairs neighbouring node pairs of a
    store of --iters x --chains x --size normal draws (5.2 GB by default) at 128 x 128, pooled, and for --chain-pairs pairs per chain
    (per chain all 512 pairs would be 524 288 grids: 69 GB of counts, as much of densities, and as much again on the host end to end), with its device parts timed alone by
    device events: the ranges (omc_store_minmax, both coordinates), the counts (omc_store_histogram2d over per-pair edges: the
    floor of any route, the counts must be made) and omc_kde2d_binned, which is split further by what it is asked for: H alone
    (the moments), H and density (+ the convolution), + mode, + levels (+ the sort of the densities and the level pass).  The
    figure in brackets behind a part is the DIFFERENCE of two such call medians, not a kernel's own time (no kernel trace is
    taken here); a difference below the calls' scatter -- the mode pass is a few microseconds -- is printed as "< scatter";
  one pooled pair at 256 x 256;
  a reversible-jump-shaped store (2000 x 512 x 20, NaN-padded) with pool_elements at 128 x 128;
  the convolution alone on 64 grids of 128 x 128 with 1 %, 5 %, 25 % and 100 % of the cells non-empty (what skipping empty cells
    gains), with the multiply-add rate of the full grid against the fp64 vector peak (78.6 TFLOP/s, AMD's figure for the MI355X);
  the same binned convolution as a torch expression on the device, by FFT (a (2 nx) x (2 ny) weight table per grid, rfft2,
    product, irfft2), with the kernel's H; and for one grid directly, a (nx ny) x (nx ny) weight matrix times the counts;
  the host route for one pooled pair: both columns to the host, scipy.stats.gaussian_kde evaluated on the same 128 x 128 centres.
Medians of --reps calls after a warm-up call (3 calls where a single one takes more than a second)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP64_VECTOR = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--chain-pairs", type=int, default=64)
    ap.add_argument("--skip-host", action="store_true")
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

    rows = []

    def row(label, ms, grids=None, extra=""):
        r = {"case": label, "ms": ms}
        if grids:
            r["us_per_grid"] = ms * 1e3 / grids
        rows.append(r)
        print(f"  {label:<92s} {ms:11.3f} ms" + (f" {r['us_per_grid']:10.3f} us/grid" if grids else "") + extra, flush=True)

    n_iter, C, size = args.iters, args.chains, args.size
    eng = Engine(C, seed=3)
    dev = eng.device
    from openmcmc_amd import _abi

    def binned_parts(counts, ends, label, grids, probs=(0.5, 0.9)):
        """omc_kde2d_binned by what it is asked for, every output allocated once"""
        lead, (nx, ny) = tuple(counts.shape[:-2]), counts.shape[-2:]
        n = int(np.prod(lead, dtype=np.int64))
        e = [eng.to_device(np.array(np.broadcast_to(v, lead))) for v in ends]
        p = eng.to_device(np.array(probs))
        out = dict(density=torch.empty(lead + (nx, ny), dtype=torch.float64, device=dev), bw=eng.empty(lead + (3,)), mode=eng.empty(lead + (2,)),
                   level=eng.empty(lead + (len(probs),)), level_pos=torch.empty(lead + (len(probs),), dtype=torch.int64, device=dev),
                   flag=torch.empty(lead, dtype=torch.int32, device=dev))

        def call(keep):
            q = {k: (out[k].data_ptr() if k in keep else None) for k in out}
            st = _abi.lib.omc_kde2d_binned(eng._ctx, n, nx, ny, counts.data_ptr(), *(v.data_ptr() for v in e), 1, None, 1.0, len(probs),
                                           p.data_ptr(), q["density"], q["bw"], q["mode"], q["level"], q["level_pos"], q["flag"])
            assert st == _abi.OK

        def diff(a, b):  # difference of two call medians; what is below 2 % of the larger call is within their scatter
            return f"{a - b:.3f} ms by difference" if a - b > 0.02 * a else "< scatter"

        t_h = timed(lambda: call(("bw", "flag")))
        t_d = timed(lambda: call(("bw", "flag", "density")))
        t_m = timed(lambda: call(("bw", "flag", "density", "mode")))
        t_l = timed(lambda: call(("bw", "flag", "density", "mode", "level", "level_pos")))
        row(f"  part: omc_kde2d_binned, {label}: H and flag alone (check, moments)", t_h, grids)
        row(f"  part: omc_kde2d_binned, {label}: + density (the convolution: {diff(t_d, t_h)})", t_d, grids)
        row(f"  part: omc_kde2d_binned, {label}: + mode ({diff(t_m, t_d)})", t_m, grids)
        row(f"  part: omc_kde2d_binned, {label}: + levels (keys, sort, level pass: {diff(t_l, t_m)})", t_l, grids)
        filled = float((counts > 0).double().mean())
        print(f"      (non-empty cells: {100 * filled:.2f} %; flags: {int((out['flag'] == 0).sum())} ok, {int((out['flag'] == 2).sum())} degenerate)", flush=True)
        return out, t_d - t_h

    def fft_route(counts, ends, H):
        """the same convolution by FFT, H (.., 3) given: weights on the (2 nx) x (2 ny) torus of offsets"""
        nx, ny = counts.shape[-2:]
        dx, dy = ((ends[1] - ends[0]) / nx)[..., None, None], ((ends[3] - ends[2]) / ny)[..., None, None]
        det = H[..., 0] * H[..., 2] - H[..., 1] ** 2
        A, B, Cc = (H[..., 2] / det)[..., None, None], (-H[..., 1] / det)[..., None, None], (H[..., 0] / det)[..., None, None]
        di = torch.arange(2 * nx, dtype=torch.float64, device=dev)
        dj = torch.arange(2 * ny, dtype=torch.float64, device=dev)
        u = torch.where(di < nx, di, di - 2 * nx)[:, None] * dx
        v = torch.where(dj < ny, dj, dj - 2 * ny)[None, :] * dy
        W = torch.exp(-0.5 * (A * u * u + 2 * B * u * v + Cc * v * v))
        c = torch.zeros(counts.shape[:-2] + (2 * nx, 2 * ny), dtype=torch.float64, device=dev)
        c[..., :nx, :ny] = counts
        f = torch.fft.irfft2(torch.fft.rfft2(c) * torch.fft.rfft2(W), s=(2 * nx, 2 * ny))[..., :nx, :ny]
        N = counts.sum(dim=(-2, -1)).double()
        return f / (N * 2 * np.pi * det.sqrt())[..., None, None]

    # ---- the cfg3-shaped store
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    shift = torch.linspace(-1, 1, size, dtype=torch.float64, device=dev)
    x = torch.empty((n_iter, C, size), dtype=torch.float64, device=dev)
    for i in range(n_iter):  # (slab by slab: no second store-sized temporary; neighbouring nodes correlated through a shared term)
        z = torch.randn((C, size), generator=g, dtype=torch.float64, device=dev)
        x[i] = 0.8 * z + 0.6 * torch.roll(z, 1, dims=1) + shift
    M = MCMC.__new__(MCMC)
    M.engine, M.store, M.store_ring, M.n_iter, M._n_dev = eng, {"x": x}, None, n_iter, n_iter
    print(f"store: {n_iter} iterations x {C} chains x {size} ({8.0 * n_iter * C * size / 1e9:.2f} GB)", flush=True)
    for pooled, n_pairs in ((True, args.pairs), (False, args.chain_pairs)):
        ix = np.arange(size // 4, size // 4 + n_pairs)
        iy = ix + 1
        grids = n_pairs * (1 if pooled else C)
        print(f"{n_pairs} node pairs at 128 x 128, " + (f"pooled ({grids} grids of {n_iter * C} draws)" if pooled else f"per chain ({grids} grids of {n_iter} draws)"), flush=True)
        row("MCMC.kde2d(grid_len=128), end to end, wall clock", timed(lambda: M.kde2d("x", index_x=ix, index_y=iy, pooled=pooled), wall=True), grids)
        row("  part: omc_store_minmax, both coordinates (the ranges, always pooled)",
            timed(lambda: (eng.store_minmax(x, index=ix), eng.store_minmax(x, index=iy))))
        ends = []
        for idx in (ix, iy):
            mn, mx, _ = (v.cpu().numpy() for v in eng.store_minmax(x, index=idx))
            ends += [mn - 0.1 * (mx - mn), mx + 0.1 * (mx - mn)]
        ex, ey = (eng.to_device(np.stack([np.linspace(p, q, 129) for p, q in zip(ends[k], ends[k + 1])])) for k in (0, 2))
        t_counts = timed(lambda: eng.store_histogram2d(x, x, ex, ey, index_x=ix, index_y=iy, pooled=pooled))
        row("  part: omc_store_histogram2d, 128 x 128, per-pair edges (the floor: the counts must be made)", t_counts, grids)
        counts, _ = eng.store_histogram2d(x, x, ex, ey, index_x=ix, index_y=iy, pooled=pooled)
        out, _ = binned_parts(counts, ends, "128 x 128", grids)
        if pooled:
            e_dev = [eng.to_device(v) for v in ends]
            f = fft_route(counts, e_dev, out["bw"])
            err = float((f - out["density"]).abs().max() / out["density"].max())
            row(f"  torch expression by FFT, given H (max abs. difference {err:.1e} of the peak)", timed(lambda: fft_route(counts, e_dev, out["bw"])), grids)
            one = [v[:1] for v in e_dev]

            def direct():
                k = torch.arange(128, dtype=torch.float64, device=dev)
                H = out["bw"][0]
                det = H[0] * H[2] - H[1] ** 2
                u = ((k[:, None] - k[None, :]) * (one[1] - one[0]) / 128)[:, None, :, None]
                v = ((k[:, None] - k[None, :]) * (one[3] - one[2]) / 128)[None, :, None, :]
                W = torch.exp(-0.5 * (H[2] / det * u * u - 2 * H[1] / det * u * v + H[0] / det * v * v)).reshape(128 * 128, 128 * 128)
                return (W @ counts[0].double().reshape(-1)).reshape(128, 128) / (counts[0].sum() * 2 * np.pi * det.sqrt())

            err = float(((direct() - out["density"][0]).abs() / out["density"][0].clamp_min(1e-300)).max())
            row(f"  torch expression, direct, ONE grid (a 2 GiB weight matrix; max rel. difference {err:.1e})", timed(direct), 1)
        del counts, out
        torch.cuda.empty_cache()

    # ---- one pooled pair at 256 x 256
    print("one pooled pair at 256 x 256", flush=True)
    ix, iy = np.array([size // 2]), np.array([size // 2 + 1])
    row("MCMC.kde2d(grid_len=256), end to end, wall clock", timed(lambda: M.kde2d("x", index_x=ix, index_y=iy, grid_len=256), wall=True), 1)
    ends = []
    for idx in (ix, iy):
        mn, mx, _ = (v.cpu().numpy() for v in eng.store_minmax(x, index=idx))
        ends += [mn - 0.1 * (mx - mn), mx + 0.1 * (mx - mn)]
    ex, ey = (eng.to_device(np.stack([np.linspace(p, q, 257) for p, q in zip(ends[k], ends[k + 1])])) for k in (0, 2))
    row("  part: omc_store_histogram2d, 256 x 256", timed(lambda: eng.store_histogram2d(x, x, ex, ey, index_x=ix, index_y=iy)), 1)
    counts, _ = eng.store_histogram2d(x, x, ex, ey, index_x=ix, index_y=iy)
    out, _ = binned_parts(counts, ends, "256 x 256", 1)
    e_dev = [eng.to_device(v) for v in ends]
    f = fft_route(counts, e_dev, out["bw"])
    err = float((f - out["density"]).abs().max() / out["density"].max())
    row(f"  torch expression by FFT, given H (max abs. difference {err:.1e} of the peak)", timed(lambda: fft_route(counts, e_dev, out["bw"])), 1)
    dense = torch.ones_like(counts)
    out_d, t_conv = binned_parts(dense, ends, "256 x 256, every cell non-empty", 1)
    print(f"      (the full 256 x 256 convolution: {2 * 65536.0**2 / t_conv / 1e9:.2f} TFLOP/s = {100 * 2 * 65536.0**2 / (t_conv * 1e-3) / PEAK_FP64_VECTOR:.1f} % of the fp64 vector peak, from the difference of call medians; one grid is 64 workgroups on 256 CUs)", flush=True)
    row("  torch expression by FFT, every cell non-empty", timed(lambda: fft_route(dense, e_dev, out_d["bw"])), 1)

    # ---- the host route, one pooled pair at 128 x 128
    if not args.skip_host:
        from scipy.stats import gaussian_kde

        got = M.kde2d("x", index_x=ix, index_y=iy)
        gx, gy = np.meshgrid(got["grid_x"][0], got["grid_y"][0], indexing="ij")

        def host_route():
            cols = x[:, :, int(ix[0]):int(ix[0]) + 2].reshape(-1, 2).cpu().numpy()
            return gaussian_kde(cols.T)(np.vstack([gx.ravel(), gy.ravel()])).reshape(128, 128)

        t0 = time.perf_counter()
        f = host_route()
        t_host = (time.perf_counter() - t0) * 1e3
        err = float(np.abs(f - got["density"][0]).max() / got["density"][0].max())
        row(f"transfer + scipy.stats.gaussian_kde on 128 x 128 centres, one pooled pair, one call (unbinned: differs by {err:.1e} of the peak)", t_host, 1)
    del x, M
    torch.cuda.empty_cache()

    # ---- what skipping empty cells gains
    print("the convolution alone, 64 grids of 128 x 128, by the share of non-empty cells", flush=True)
    rng = np.random.default_rng(2)
    ends = [np.full(64, -3.0), np.full(64, 3.0), np.full(64, -2.0), np.full(64, 2.0)]
    gi, gj = np.meshgrid(np.arange(128), np.arange(128), indexing="ij")
    bump = np.exp(-0.5 * (((gi - 60) / 25.0) ** 2 + ((gj - 70) / 20.0) ** 2 - 1.2 * (gi - 60) / 25.0 * (gj - 70) / 20.0))
    for share in (0.01, 0.05, 0.25, 1.0):
        c = (1 + (1000 * bump).astype(np.int64)) * (rng.random((64, 128, 128)) < share)
        out, t_conv = binned_parts(torch.as_tensor(c, device=dev), ends, f"{100 * share:g} % of the cells", 64)
        if share == 1.0:
            rate = 64 * 2 * 16384.0**2 / (t_conv * 1e-3)
            print(f"      (the full grids: {rate / 1e12:.2f} TFLOP/s = {100 * rate / PEAK_FP64_VECTOR:.1f} % of the fp64 vector peak, from the difference of call medians)", flush=True)

    # ---- a reversible-jump-shaped store
    n_it, Cr, K = 2000, 512, 20
    eng2 = Engine(Cr, seed=4)
    g.manual_seed(9)
    loc = torch.rand((n_it, Cr, K), generator=g, dtype=torch.float64, device=dev)
    centre = torch.where(loc < 0.5, 0.25, 0.75)
    loc = centre + 0.05 * torch.randn((n_it, Cr, K), generator=g, dtype=torch.float64, device=dev)
    coef = torch.where(centre < 0.5, -1.0, 2.0) + 0.4 * torch.randn((n_it, Cr, K), generator=g, dtype=torch.float64, device=dev)
    k_active = torch.randint(1, K + 1, (n_it, Cr, 1), generator=g, device=dev)
    pad = torch.arange(K, device=dev)[None, None, :] >= k_active
    loc[pad], coef[pad] = float("nan"), float("nan")
    R = MCMC.__new__(MCMC)
    R.engine, R.store, R.store_ring, R.n_iter, R._n_dev = eng2, {"loc": loc, "coef": coef}, None, n_it, n_it
    print(f"reversible-jump-shaped store: {n_it} x {Cr} x {K}, NaN-padded, pool_elements at 128 x 128", flush=True)
    for bw in ("scott", "marginal"):
        row(f"MCMC.kde2d('loc', 'coef', pool_elements=True, bw='{bw}'), end to end, wall clock",
            timed(lambda: R.kde2d("loc", "coef", pool_elements=True, bw=bw), wall=True), 1)
    ex, ey = eng2.to_device(np.linspace(0.0, 1.0, 129)), eng2.to_device(np.linspace(-3.0, 4.0, 129))
    row("  part: omc_store_histogram2d, pooled pairs, 128 x 128", timed(lambda: eng2.store_histogram2d(loc, coef, ex, ey, pool_pairs=True)), 1)
    eng.check_status()
    eng2.check_status()
    eng.close()
    eng2.close()
    print(json.dumps({"reps": args.reps, "store": f"{n_iter} x {C} x {size}", "pairs": args.pairs, "rows": rows}))


if __name__ == "__main__":
    main()
