#!/usr/bin/env python3
"""Do two builds of libomcmc_hip.so give the same bits in every summary of the device store?

    bash benchmarks/build_rev.sh HEAD~1 before
    python3 benchmarks/store_same_bits.py [--before build/ab/libomcmc_hip_before.so]

One fresh child process per library (the other build through OMC_HIP_LIB, the in-tree build without it) runs every Engine.store_*
entry point and kde_binned on the same stores and saves what comes back; this process compares the two files array by array with
np.array_equal(equal_nan=True) and prints one line per entry point and store shape.  The stores are made on the host from a numpy
seed and uploaded: both children see the same bytes.  Shapes (n_iter, C, size) = (5, 3, 17) and (130, 2, 33): R = 260 pooled
rows are two slices of the column moments, n_iter is odd for the split diagnostics, and size is one element past a 16-wide and a
32-wide tile.  Column 0 holds a NaN, column 1 an infinity, column 2 ties with -0.0 and +0.0.  Every entry point runs pooled and
per chain where it has both forms, without an index and with one of 19 entries that has repeats and is not sorted.  The summaries
whose workspace goes by chunks run with the library's own chunk and with option "rank_chunk" = 3; the likelihood routes
(store_loglik, store_psis, store_loo_expect: every f, every output, tail_max as a number and as a vector, from a log-likelihood
entry and from a mean entry) run over the selection as it is -- columns 0 and 1 give their NaN outputs -- and over its finite
columns alone.
Also checked, on the in-tree build alone: an identity index gives the bits of no index in store_cov and store_minmax.
Exit status 1 if anything differs.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(5, 3, 17), (130, 2, 33)]


def host_store(shape, seed):
    n_iter, C, size = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) * np.linspace(0.5, 2.0, size) + np.linspace(-1.0, 1.0, size)
    x[n_iter // 2, C - 1, 0] = np.nan
    x[1, 0, 1] = np.inf
    x[:, :, 2] = np.round(x[:, :, 2])  # ties, and zeros of both signs
    x[0, 0, 2], x[n_iter - 1, C - 1, 2] = -0.0, 0.0
    return x


def later_entry_points(eng, put, tag, iname, store, other, idx):
    """The summaries that came after the first pass, for one store and selection.  Every one whose workspace goes by chunks runs
    with the chunk the library picks and with option "rank_chunk" = 3 (several chunks, the last one short)."""
    n_iter, C, size = store.shape
    S = n_iter * C
    n = size if idx is None else idx.size
    rng = np.random.default_rng(23)
    k = f"{tag}/{{}}/{iname}"
    counts, _ = eng.store_histogram(store, np.linspace(-3.0, 3.0, 13), index=idx, pooled=True)
    lo, hi = np.full(n, -3.0), np.full(n, 3.0)
    for rule in eng.KDE_RULES:
        for reflect in ((False, False), (True, True)):
            put(k.format("kde_binned") + f"/{rule}/reflect{reflect[0]}",
                eng.kde_binned(counts, lo, hi, rule=rule, bw=np.linspace(0.2, 0.9, n) if rule == "given" else None, reflect=reflect))
    m = 3
    W, offset = rng.standard_normal((m, n)), rng.standard_normal(m)
    prec_one, prec_m = eng.to_device(rng.gamma(2.0, 1.0, (n_iter, C, 1))), eng.to_device(rng.gamma(2.0, 1.0, (n_iter, C, m)))
    for omit in (True, False):
        put(k.format("store_project") + f"/plain/omit{omit}", eng.store_project(store, W, index=idx, omit_nan=omit))
        put(k.format("store_project") + f"/offset/omit{omit}", eng.store_project(store, W, index=idx, offset=offset, omit_nan=omit))
    put(k.format("store_project") + "/prec1/stream", eng.store_project(store, W, index=idx, offset=offset, prec=prec_one, replicate=1))
    put(k.format("store_project") + "/precm/stream", eng.store_project(store, W[0], index=idx, prec=prec_m[:, :, :1].contiguous(), replicate=2))
    put(k.format("store_project") + "/precm/wide", eng.store_project(store, W, index=idx, prec=prec_m, replicate=3))
    pos = rng.integers(0, 2 * C * (n_iter // 2), size=(n, 3))  # inside the split column, the shorter of the two
    probs_hi, probs_lo = np.array([0.05, 0.5, 0.95]), np.array([-1.0, 0.25, 0.9])
    # the likelihood routes: over the selection as it is (columns 0 and 1 give the NaN outputs) and over its finite columns alone
    cols = np.arange(size) if idx is None else idx
    finite = cols[cols >= 3]
    selections = (("", idx, n), ("/finite", finite, finite.size))
    for chunk in (0, 3):
        eng.set_option("rank_chunk", chunk)
        c = f"/chunk{chunk}"
        for pname, pooled in (("pooled", True), ("chain", False)):
            put(k.format("store_autocorr") + f"/{pname}{c}", eng.store_autocorr(store, min(n_iter - 1, 40), index=idx, pooled=pooled))
            put(k.format("store_autocorr") + f"/{pname}/raw{c}", eng.store_autocorr(store, 2, index=idx, pooled=pooled, normalize=False))
        for algo in (1, 2):
            put(k.format("store_ess_indicator") + f"/upper/algo{algo}{c}", eng.store_ess_indicator(store, None, probs_hi, index=idx, counts=2, algo=algo))
            put(k.format("store_ess_indicator") + f"/lower/algo{algo}{c}",
                eng.store_ess_indicator(store, probs_lo, probs_hi, index=idx, counts=2, algo=algo))
        for split in (False, True):
            put(k.format("store_order_stats") + f"/split{split}{c}", eng.store_order_stats(store, pos, index=idx, split=split))
        for sname, sel, ns in selections:
            y, thr = np.linspace(-1.0, 1.0, ns), np.linspace(-0.5, 0.5, ns)
            tails = (("scalar", min(S - 1, 3)), ("vector", 1 + np.arange(ns) % (S - 1)))
            for prname, prec in (("prec1", prec_one), ("precn", eng.to_device(rng.gamma(2.0, 1.0, (n_iter, C, ns))))):
                e = f"{sname}/{prname}{c}"
                if chunk == 0:  # (one pass, no chunks)
                    put(k.format("store_loglik") + e, eng.store_loglik(store, y, prec, index=sel, lse=True, mean=True, var=True, ll=True))
                for tname, tm in tails:
                    put(k.format("store_psis") + f"/mean/{tname}{e}", eng.store_psis(store, tm, index=sel, y=y, prec=prec))
                    for f in ("mean", "cdf", "entry"):
                        got = eng.store_loo_expect(store, tm, index=sel, y=y, prec=prec, f=f, values=other if f == "entry" else None,
                                                   values_index=sel[::-1].copy() if f == "entry" and sel is not None else None, threshold=thr,
                                                   want=("mean", "var", "below", "ess", "invprec", "k", "tail"), lw=True)
                        put(k.format("store_loo_expect") + f"/mean/{f}/{tname}{e}", tuple(got[w] for w in sorted(got)))
            for tname, tm in tails:  # the entry holds the log-likelihoods themselves
                e = f"{sname}{c}"
                put(k.format("store_psis") + f"/ll/{tname}{e}", eng.store_psis(store, tm, index=sel))
                entry = dict(index=sel, f="entry", values=other, values_index=None if sel is None else sel[::-1].copy())
                got = eng.store_loo_expect(store, tm, threshold=thr, want=("mean", "var", "below", "ess", "k", "tail"), lw=True, **entry)
                put(k.format("store_loo_expect") + f"/ll/{tname}{e}", tuple(got[w] for w in sorted(got)))
                put(k.format("store_loo_expect") + f"/ll/lw_only/{tname}{e}", eng.store_loo_expect(store, tm, want=(), lw=True, **entry)["lw"])
                put(k.format("store_loo_expect") + f"/ll/k_only/{tname}{e}", eng.store_loo_expect(store, tm, want=("k",), **entry)["k"])
    eng.set_option("rank_chunk", 0)


def child(path):
    from openmcmc_amd.engine import Engine

    out = {}

    def put(key, result):
        for i, t in enumerate(result if isinstance(result, tuple) else (result,)):
            out[f"{key}#{i}"] = t.cpu().numpy()

    for shape in SHAPES:
        n_iter, C, size = shape
        tag = "x".join(map(str, shape))
        eng = Engine(C, seed=1)
        rng = np.random.default_rng(11)
        store, other = eng.to_device(host_store(shape, 5)), eng.to_device(host_store(shape, 6))
        index = np.concatenate([[2, 0, 1, size - 1, 2], rng.integers(0, size, 14)])
        assert index.size == 19 and np.unique(index).size < 19 and np.any(np.diff(index) < 0)
        for iname, idx in (("all", None), ("index", index)):
            n = size if idx is None else idx.size
            even, uneven = np.linspace(-3.0, 3.0, 13), np.array([-4.0, -1.5, -1.0, -0.25, 0.0, 0.125, 1.0, 2.5, 6.0])
            per = {"even": even[None, :] + 0.01 * np.arange(n)[:, None], "uneven": uneven[None, :] * (1.0 + 0.05 * np.arange(n)[:, None])}
            idy = None if idx is None else idx[::-1].copy()
            for pname, pooled in (("pooled", True), ("chain", False)):
                k = f"{tag}/{{}}/{iname}/{pname}"
                if idx is None:
                    put(k.format("store_moments"), eng.store_moments(store, pooled=pooled))
                    for omit in (True, False):
                        put(k.format("store_quantiles") + f"/omit{omit}", eng.store_quantiles(store, [0.05, 0.5, 0.95], pooled=pooled, omit_nan=omit))
                for corr in (False, True):
                    put(k.format("store_cov") + f"/corr{corr}", eng.store_cov(store, index_a=idx, pooled=pooled, correlation=corr))
                    put(k.format("store_cov") + f"/cross/corr{corr}", eng.store_cov(store, other, index_a=idx, index_b=idy, pooled=pooled, correlation=corr))
                put(k.format("store_minmax"), eng.store_minmax(store, index=idx, pooled=pooled))
                for ename, e in (("even", even), ("uneven", uneven)):
                    put(k.format("store_histogram") + f"/{ename}/shared", eng.store_histogram(store, e, index=idx, pooled=pooled))
                    put(k.format("store_histogram") + f"/{ename}/per", eng.store_histogram(store, per[ename], index=idx, pooled=pooled))
                    put(k.format("store_histogram2d") + f"/{ename}/shared", eng.store_histogram2d(store, other, e, uneven, index_x=idx, index_y=idy, pooled=pooled))
                    put(k.format("store_histogram2d") + f"/{ename}/per", eng.store_histogram2d(store, other, per[ename], per["uneven"], index_x=idx, index_y=idy, pooled=pooled))
                    put(k.format("store_histogram2d") + f"/{ename}/pool", eng.store_histogram2d(store, other, e, uneven, index_x=idx, index_y=idy, pooled=pooled, pool_pairs=True, occupancy=True))
                for omit in (True, False):
                    put(k.format("store_hdi") + f"/omit{omit}", eng.store_hdi(store, [0.5, 0.94], index=idx, pooled=pooled, omit_nan=omit))
            k = f"{tag}/{{}}/{iname}"
            for split in (False, True):
                put(k.format("store_ranks") + f"/split{split}", eng.store_ranks(store, index=idx, split=split))
            put(k.format("store_rank_diagnostics"), eng.store_rank_diagnostics(store, index=idx))
            a, b = np.linspace(-0.5, 0.5, n), np.linspace(0.5, 1.5, n)
            for op in Engine.REDUCE_OPS:
                for omit in (True, False):
                    put(k.format("store_reduce") + f"/{op}/omit{omit}", eng.store_reduce(store, op, index=idx, omit_nan=omit, a=a, b=b))
            later_entry_points(eng, put, tag, iname, store, other, idx)
        put(f"{tag}/store_rhat_ess/all", eng.store_rhat_ess(store))
        put(f"{tag}/store_thin/all", eng.store_thin(store, 2, first=1))
        for pname, pooled in (("pooled", True), ("chain", False)):
            put(f"{tag}/store_cov/identity/{pname}", eng.store_cov(store, index_a=np.arange(size), pooled=pooled))
            put(f"{tag}/store_minmax/identity/{pname}", eng.store_minmax(store, index=np.arange(size), pooled=pooled))
        eng.check_status()
        eng.close()
    np.savez(path, **out)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", default="build/ab/libomcmc_hip_before.so")
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, lib in (("before", os.path.join(ROOT, args.before)), ("after", None)):
            env = dict(os.environ)
            env.pop("OMC_HIP_LIB", None)
            if lib:
                env["OMC_HIP_LIB"] = lib
            path = os.path.join(tmp, name + ".npz")
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, timeout=600)
            if run.returncode != 0:
                print(f"the child of the {name} build ended with status {run.returncode}: nothing compared")
                return 2
            with np.load(path) as z:
                got[name] = {k: z[k] for k in z.files}
    before, after = got["before"], got["after"]
    assert sorted(before) == sorted(after)
    groups, unequal = {}, []
    for key in sorted(after):
        tag, entry = key.split("/")[:2]
        ok = same(before[key], after[key])
        groups.setdefault((entry, tag), []).append(ok)
        if not ok:
            unequal.append(key)
    print(f"before = {args.before}, after = the in-tree build; arrays compared with np.array_equal(equal_nan=True), integers exactly")
    for (entry, tag), oks in sorted(groups.items()):
        print(f"{entry:24s} {tag:10s} {'equal' if all(oks) else 'NOT EQUAL'}  ({sum(oks)} of {len(oks)} arrays)")
    for key in sorted(k for k in after if "/identity/" in k):
        ok = same(after[key], after[key.replace("/identity/", "/all/") if "minmax" in key else key.replace("/identity/", "/all/").replace("#", "/corrFalse#")])
        print(f"identity index against no index, {key:44s} {'equal' if ok else 'NOT EQUAL'}")
        if not ok:
            unequal.append(key)
    for key in unequal:
        print("NOT EQUAL:", key)
    print(f"{len(after)} arrays, {len(unequal)} unequal")
    return 1 if unequal else 0


if __name__ == "__main__":
    sys.exit(main())
