#!/usr/bin/env python3
"""Do two builds of libomcmc_hip.so give the same bits in the small per-chain kernels (ragged state, reversible jump, mixture
priors, truncated conditionals: omc_rj.hip, omc_scalar.hip, omc_truncated.hip, omc_truncmix.hip)?

    bash benchmarks/build_rev.sh HEAD~1 before
    python3 benchmarks/small_kernels_same_bits.py [--before build/ab/libomcmc_hip_before.so]

One fresh child process per library (the other build through OMC_HIP_LIB, the in-tree build without it) calls the entry points
below on the same inputs, with in-kernel draws and with injected ones, and saves every output; this process compares the two files
array by array with np.array_equal(equal_nan=True) and prints one line per entry point and shape.  Inputs come from a numpy seed on
the host: both children see the same bytes.  Shapes: chains C in {1, 5, 65} (65 crosses a 64-chain block of the lane-per-chain
kernels); order kmax / p in {1, 2, 7, 63, 64}, the dense scan also 65 and 130 (its lanes stride); band width w in {0, 1, 3} with
n in {1, 2, 70}; ragged counts 0, 1, kmax - 1 and kmax going round the chains (1, kmax - 1, kmax for the reversible-jump
transition, which needs a live column).  Exit status 1 if anything differs.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAINS = (1, 5, 65)
ORDERS = (1, 2, 7, 63, 64)
DENSE_ORDERS = ORDERS + (65, 130)
BAND = [(w, n) for w in (0, 1, 3) for n in (1, 2, 70)]


def spd(rng, k, m=None):
    A = rng.standard_normal(((m or k) + 3, k))
    return A.T @ A / max(k, 1) + 0.1 * np.eye(k)


def child(path):
    import torch

    from openmcmc_amd.engine import Engine

    out = {}

    def put(key, *tensors):
        for i, t in enumerate(tensors):
            if t is not None:
                out[f"{key}#{i}"] = t.cpu().numpy()

    for C in CHAINS:
        eng = Engine(C, seed=7)
        t = eng.to_device
        i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=eng.device)  # noqa: E731
        i64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int64, device=eng.device)  # noqa: E731
        for k in ORDERS:
            rng = np.random.default_rng(1000 * C + k)
            tag = f"C{C}/k{k}"
            counts = np.array([(0, 1, k - 1, k)[c % 4] for c in range(C)], dtype=np.float64)
            live = np.arange(k)[None, :] < counts[:, None]
            cnt = t(counts)
            x, grad = rng.standard_normal((C, k)), rng.standard_normal((C, k))
            u, z = rng.random((C, k)), rng.standard_normal((C, k))
            prec, mean = 0.5 + 2 * rng.random((C, k)), rng.standard_normal((C, k))
            lo_v, hi_v = np.full(k, -0.5), np.full(k, 1.5)
            # ---- omc_rw_propose, omc_mala_diag, omc_mh_accept
            x3, step = t(np.clip(x, -0.4, 1.4).reshape(C, k, 1)), t(0.1 + rng.random(k))
            for cname, cn in (("all", None), ("ragged", cnt)):
                for dname, inj_u, inj_z in (("stream", None, None), ("inject", t(u), t(z))):
                    zt, zn = eng.empty(C, k, 1), eng.empty(C, k, 1)
                    put(f"rw_propose/{tag}/truncated/{cname}/{dname}", zt, *eng.rw_propose(x3, zt, step, lower=t(lo_v), upper=t(hi_v), count=cn, inject=inj_u, draw_index=3, sub=2))
                    put(f"rw_propose/{tag}/plain/{cname}/{dname}", zn, *eng.rw_propose(x3, zn, step, count=cn, inject=inj_z, draw_index=3, sub=2))
                    xo, lq = eng.mala_diag(t(x), t(grad), t(prec), 0.3, count=cn, z=inj_z, draw_index=4, sub=1)
                    put(f"mala_diag/{tag}/propose/{cname}/{dname}", xo, lq)
                    put(f"mala_diag/{tag}/reverse/{cname}/{dname}", eng.mala_diag(xo, t(grad), t(prec), 0.3, count=cn, x_other=t(x)))
                    la = eng.empty(C)
                    acc = eng.mh_accept(t(x[:, 0]), t(grad[:, 0]), lq_fwd=t(z[:, 0]), lq_rev=t(u[:, 0]), count=cn, index=0,
                                        u=None if inj_u is None else t(u[:, 0]), draw_index=5, sub=3, log_alpha=la)
                    put(f"mh_accept/{tag}/{cname}/{dname}", acc, la)
            # ---- the small ragged operator: omc_small_sample_canonical, omc_small_gibbs_truncated, omc_small_spd_ops
            gram = np.zeros((C, k, k))
            for c in range(C):
                n_live = int(counts[c])
                gram[c, :n_live, :n_live] = spd(rng, n_live)
            g, rhs, tau = t(gram), t(rng.standard_normal((C, k))), t(0.5 + rng.random(C))
            for cname, cn, gg in (("all", None, t(np.stack([spd(rng, k) for _ in range(C)]))), ("ragged", cnt, g)):
                for dname, inj_u, inj_z in (("stream", None, None), ("inject", t(u), t(z))):
                    mu = eng.empty(C, k)
                    xs = eng.small_sample_canonical(gg, rhs, t(prec), lik_scale=tau, prior_mean=t(mean), count=cn, z=inj_z, draw_index=6, mean_out=mu)
                    put(f"small_sample_canonical/{tag}/{cname}/{dname}", xs, mu)
                    xg = t(np.abs(x))
                    eng.small_gibbs_truncated(gg, rhs, t(prec), xg, lower=0.0, lik_scale=tau, prior_mean=t(mean), count=cn, u=inj_u, draw_index=7)
                    put(f"small_gibbs_truncated/{tag}/{cname}/{dname}", xg)
            A = t(np.stack([spd(rng, k) for _ in range(C)]))
            put(f"small_spd_ops/{tag}/all", *eng.small_spd_ops(A, t(x), want_Av=True, want_quad=True, want_logdet=True))
            put(f"small_spd_ops/{tag}/logdet", *eng.small_spd_ops(A, want_logdet=True))
            # ---- omc_rj_matched_transition: birth and death, with and without limits
            rj_counts = np.array([(1, max(k - 1, 1), k)[c % 3] for c in range(C)], dtype=np.float64)
            G = t(np.stack([spd(rng, k, 2 * k) for _ in range(C)]))
            coef = np.where(np.arange(k)[None, :] < rj_counts[:, None], np.abs(x) + 0.1, 0.0)
            dele = (rng.integers(0, 1 << 30, C) % np.maximum(rj_counts, 1)).astype(np.int64)
            for bname, birth in (("birth", np.ones(C)), ("death", np.zeros(C))):
                for lname, limits in (("plain", None), ("limits", (0.0, np.inf))):
                    for dname, inj in (("stream", None), ("inject", t(u[:, 0] if limits else z[:, 0]))):
                        lqf, lqr = t(np.zeros(C)), t(np.zeros(C))
                        cp = eng.rj_matched_transition(G, G, t(rj_counts), i32(birth), i64(dele), t(coef), 0.7, limits, lqf, lqr, inject=inj, draw_index=8, sub=1)
                        put(f"rj_matched_transition/{tag}/{bname}/{lname}/{dname}", cp, lqf, lqr)
            # ---- omc_design_predict_batched: n even and aligned (two nodes per thread), n odd
            for n in (70, 71):
                B = t(rng.standard_normal((C, k, n)) * live[:, :, None])
                put(f"design_predict_batched/{tag}/n{n}", eng.design_predict_batched(B, t(x * live), add_chain=t(rng.standard_normal((C, n))),
                                                                                  add_shared=t(rng.standard_normal(n)), alpha=-1.5, chain_scale=tau))
                put(f"design_predict_batched/{tag}/n{n}/bare", eng.design_predict_batched(B, t(x * live)))
            # ---- log-densities, mixture allocation, prior draws, centred row product
            for cname, cn in (("all", None), ("ragged", cnt)):
                o0, o1, o2 = eng.empty(C), eng.empty(C), eng.empty(C)
                eng.diag_gauss_logpdf(t(x), t(prec), o0, mean=t(mean), count=cn)
                eng.diag_gauss_logpdf_limits(t(x), t(prec), o1, lower=-1.0, upper=np.inf, mean=t(mean), count=cn)
                eng.diag_gauss_logpdf_limits(t(x), t(prec), o2, lower=-np.inf, upper=np.inf, count=cn)
                put(f"diag_gauss_logpdf/{tag}/{cname}", o0)
                put(f"diag_gauss_logpdf_limits/{tag}/{cname}", o1, o2)
            K = 3
            prior = rng.random((k, K)) + 0.1
            for dname, inj in (("stream", None), ("inject", t(u))):
                put(f"mixture_allocation/{tag}/shared/{dname}", eng.mixture_allocation(t(x), t(prior[:1]), t(np.array([-1.0, 0.0, 1.0])), t(np.array([4.0, 1.0, 0.25])), u=inj, draw_index=9))
                put(f"mixture_allocation/{tag}/rows/{dname}", eng.mixture_allocation(t(x), t(prior), t(rng.standard_normal((C, K))), t(0.5 + rng.random((C, K))), u=inj, draw_index=9))
                put(f"uniform_draw/{tag}/{dname}", eng.uniform_draw(t(lo_v), t(hi_v - lo_v), inject=inj, draw_index=10, sub=4))
            M = spd(rng, k)
            m0 = rng.standard_normal(k)
            put(f"centered_rowdot/{tag}", eng.dense_quadform(t(M), t(x), center=t(m0), M_center=t(M @ m0)), eng.dense_quadform(t(M), t(x)))
        # ---- omc_poisson_draw: both generators (rate below and from 10), streams and a tape
        rng = np.random.default_rng(77 + C)
        rate = t(np.array([(0.0, 0.7, 9.5, 10.0, 48.0, 300.0)[c % 6] for c in range(C)]))
        tape = rng.random((C, 700))
        put(f"poisson_draw/C{C}/stream", eng.poisson_draw(rate, draw_index=11))
        put(f"poisson_draw/C{C}/inject", eng.poisson_draw(rate, u=t(tape), draw_index=11))
        eng.check_status()
        # ---- omc_dense_gibbs_truncated (with and without diag_chain), omc_band_gibbs_truncated
        for p in DENSE_ORDERS:
            rng = np.random.default_rng(2000 * C + p)
            terms = [{"mat": t(spd(rng, p)), "rhs": t(rng.standard_normal(p)), "scale": t(0.5 + rng.random(C))}, {"scale": t(0.1 + rng.random(C))}]
            lower = t(np.where(rng.random(p) < 0.5, 0.0, -np.inf))
            d, rc = t(0.5 + 3 * rng.random((C, p))), t(rng.standard_normal((C, p)))
            x0, u = np.abs(rng.standard_normal((C, p))), rng.random((C, p))
            for dname, inj in (("stream", None), ("inject", t(u))):
                for gname, diag in (("plain", None), ("diag_chain", d)):
                    x = t(x0)
                    eng.dense_gibbs_truncated(p, terms, x, lower=lower, u=inj, rhs_chain=rc, draw_index=12, diag_chain=diag)
                    put(f"dense_gibbs_truncated/C{C}/p{p}/{gname}/{dname}", x)
        for w, n in BAND:
            rng = np.random.default_rng(3000 * C + 10 * w + n)
            band = np.zeros((w + 1, n))
            band[0] = 2.0 * w + 1.0 + rng.random(n)
            band[1:] = -0.5 - 0.4 * rng.random((w, n))
            terms = [{"band": t(band), "rhs": t(rng.standard_normal(n)), "scale": t(0.5 + rng.random(C))}, {"scale": t(0.1 + rng.random(C))}]
            lower, upper = t(np.where(rng.random(n) < 0.5, 0.0, -np.inf)), t(np.full(n, 3.0))
            x0, u, rc = np.abs(rng.standard_normal((C, n))), rng.random((C, n)), t(rng.standard_normal((C, n)))
            for dname, inj in (("stream", None), ("inject", t(u))):
                x = t(x0)
                eng.band_gibbs_truncated(n, terms, x, lower=lower, upper=upper, u=inj, rhs_chain=rc, draw_index=13)
                put(f"band_gibbs_truncated/C{C}/w{w}n{n}/{dname}", x)
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
    groups, unequal, finite = {}, [], 0
    for key in sorted(after):
        entry, c, shape = key.split("/")[:3]
        ok = same(before[key], after[key])
        finite += int(np.isfinite(after[key].astype(np.float64)).sum())
        groups.setdefault((entry, c, shape.split("#")[0]), []).append(ok)
        if not ok:
            unequal.append(key)
    print(f"before = {args.before}, after = the in-tree build; arrays compared with np.array_equal(equal_nan=True), integers exactly")
    for (entry, c, shape), oks in sorted(groups.items()):
        print(f"{entry:26s} {c:4s} {shape:8s} {'equal' if all(oks) else 'NOT EQUAL'}  ({sum(oks)} of {len(oks)} arrays)")
    for key in unequal:
        print("NOT EQUAL:", key)
    total = sum(a.size for a in after.values())
    print(f"{len(after)} arrays, {total} numbers ({finite} finite), {len(unequal)} arrays unequal")
    return 1 if unequal else 0


if __name__ == "__main__":
    sys.exit(main())
