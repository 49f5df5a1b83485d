#!/usr/bin/env python3
"""Do two revisions of the Python package give the same bits, through the same library calls, on every route of NormalNormal
(sampler/sampler.py) and on the two fused loops of MCMC (mcmc.py)?

    mkdir -p build/ab/parent && git archive HEAD~1 openmcmc_amd tests benchmarks bench.py oracle | tar -x -C build/ab/parent
    python3 benchmarks/normal_normal_same_bits.py [--before build/ab/parent]

One fresh child process per source tree, one after the other (the other tree goes first on sys.path, both load the in-tree
libomcmc_hip.so), runs the cases below through MCMC(...).run_mcmc() -- 2 burn-in and 4 stored sweeps, once with the chains' own
draws and once with draws injected through the samplers' `inject` hook -- and saves every store entry, log_post included, the
final per-chain state and the sequence of omc_* entry points the run called (the `lib` object engine.py imports is wrapped, in
the child only).  A case that raises is recorded as the exception's type and message.  This process compares the two files:
np.array_equal(equal_nan=True) for every array, the same call sequence (or the same exception) for every case; one line per
case, exit status 1 if anything differs.  The models are those of tests/normal_normal_models.py.  Chains C in {3, 65} (65 crosses
a 64-chain block), parameter size n = 70 (crosses a 64-site block) unless the case says otherwise -- the tridiagonal cases with a
per-chain centre also at n = 700, where the kernel takes the centre inside the launch; inputs come from a numpy seed on the
host: both children see the same bytes.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = (3, 65)
N = 70
N_CENTRE = 700
N_BURN, N_ITER = 2, 4
HOST_ERRORS = (NotImplementedError, ValueError, TypeError, KeyError, AttributeError, np.linalg.LinAlgError)


def cases():
    """(name, builder, its arguments, chains, modes, fuse)"""
    from normal_normal_models import full_spd, mixture, ragged, regression, rw1, rw2, smoother
    from openmcmc_amd.sampler.sampler import NormalNormal

    both, table = ("stream", "inject"), []
    tri = ["plain", "offset", "mean", "mean_lincomb", "mean+const", "mean_lincomb+const", "mean_first", "two_vectors", "offset+mean",
           "offset+two_vectors", "replicated+const", "trunc1", "trunc2"]
    for v in tri:
        table.append((f"tridiag/{v}", smoother, (rw1(N), v, N), CHAINS, both, True))
    table.append(("tridiag/plain/unfused", smoother, (rw1(N), "plain", N), CHAINS, both, False))
    # the workgroup-per-chain form of the tridiagonal kernel (more than 512 sites) takes a per-chain centre inside the launch: the
    # plan's center_chain, the quadratic-form factor of an unscaled constant-diagonal term and the skip of a form that a later
    # block invalidates exist only there
    for v in ["mean", "mean_first", "mean_lincomb", "mean+const", "mean_lincomb+const", "two_vectors", "offset+mean"]:
        table.append((f"tridiag/{v}/n{N_CENTRE}", smoother, (rw1(N_CENTRE), v, N_CENTRE), CHAINS, both, True))
    for v in ["plain", "offset", "mean", "mean_first", "replicated+const", "trunc1", "trunc2"]:
        table.append((f"band/{v}", smoother, (rw2(N), v, N), CHAINS, both, True))
    n_long = NormalNormal.TRIDIAG_WG_MAX + 1
    table.append((f"band/long_tridiagonal_n{n_long}", smoother, (rw1(n_long), "plain", n_long), (3,), both, True))
    for v in ["diag", "corr", "diag+offset", "corr+offset", "diag+trunc"]:
        table.append((f"dense/regression/{v}", regression, (v, N), CHAINS, both, True))
    for v in ["mean", "mean_first", "trunc1", "trunc2"]:
        table.append((f"dense/full_precision/{v}", smoother, (full_spd(N), v, N), CHAINS, both, True))
    table.append(("dense/spectral_n64", regression, ("diag", 64), CHAINS, ("stream",), True))
    table.append(("dense/spectral_off_n64", regression, ("diag+factorise", 64), CHAINS, ("stream",), True))
    table.append(("dense/mixture_prior", mixture, ("plain", N), CHAINS, both, True))
    table.append(("dense/mixture_prior_truncated", mixture, ("trunc", N), CHAINS, both, True))
    table.append(("ragged/plain", ragged, ("plain", N), CHAINS, both, True))
    table.append(("ragged/limits", ragged, ("limits", N), CHAINS, both, True))
    return table


class Recorder:
    """The library object with every call of an omc_* entry point noted in `log`."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("omc_"):
            return fn

        def call(*args):
            self._log.append(name)
            return fn(*args)
        return call


def child(path, tree):
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    sys.path.append(os.path.join(ROOT, "tests"))  # (the models of this revision, where the other tree has none)
    import openmcmc_amd
    import openmcmc_amd.engine as engine_module
    from openmcmc_amd.chains import is_chain
    from openmcmc_amd.mcmc import MCMC
    from openmcmc_amd.sampler.sampler import NormalGamma, NormalNormal

    assert os.path.dirname(os.path.dirname(os.path.abspath(openmcmc_amd.__file__))) == os.path.abspath(tree)
    log = []
    engine_module.lib = Recorder(engine_module.lib, log)
    out = {}
    for i_case, (name, builder, args, chains, modes, fuse) in enumerate(cases()):
        for C in chains:
            for mode in modes:
                tag = f"{name}|C{C}|{mode}"
                rng = np.random.default_rng(1000 * i_case + C)
                eng = engine_module.Engine(C, seed=11)
                del log[:]
                try:
                    mdl, st, samplers, uniform = builder(*args, C, rng, eng)
                    M = MCMC(st, samplers, model=mdl, n_burn=N_BURN, n_iter=N_ITER, n_chains=C, engine=eng, fuse=fuse)
                    if mode == "inject":
                        for smp in samplers:
                            if type(smp) is NormalNormal:
                                size = M.store[smp.param].shape[2]
                                draws = rng.random((N_BURN + N_ITER, C, size)) if smp.param in uniform else rng.standard_normal((N_BURN + N_ITER, C, size))
                                smp.inject = lambda s, it, d=draws: eng.to_device(d[it])
                            elif type(smp) is NormalGamma and M.store[smp.param].shape[2] == 1:
                                draws = rng.gamma(20.0, size=(N_BURN + N_ITER, C))
                                smp.inject = lambda s, it, d=draws: eng.to_device(d[it])
                    M.run_mcmc()
                    for key, t in M.store.items():
                        out[f"{tag}|store|{key}"] = t.cpu().numpy()
                    for key, v in M.state.items():
                        if is_chain(v):
                            out[f"{tag}|state|{key}"] = v.data.cpu().numpy()
                except HOST_ERRORS as e:  # (anything else, a device error above all, ends the child)
                    out[f"{tag}|raised"] = np.array(f"{type(e).__name__}: {e}")
                out[f"{tag}|calls"] = np.array("\n".join(log))
                eng.close()
    np.savez(path, **out)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def main(child=child, script=os.path.abspath(__file__)):
    """The driver and the comparison; another case table (benchmarks/mh_same_bits.py) passes its own `child` and file."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", default="build/ab/parent")
    ap.add_argument("--child")
    ap.add_argument("--tree")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.tree)
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, tree in (("before", os.path.join(ROOT, args.before)), ("after", ROOT)):
            env = dict(os.environ, OMC_HIP_LIB=os.path.join(ROOT, "openmcmc_amd", "libomcmc_hip.so"))
            path = os.path.join(tmp, name + ".npz")
            run = subprocess.run([sys.executable, script, "--child", path, "--tree", tree], env=env, timeout=900)
            if run.returncode != 0:
                print(f"the child of the {name} tree ended with status {run.returncode}: nothing compared")
                return 2
            with np.load(path) as z:
                got[name] = {k: z[k] for k in z.files}
    before, after = got["before"], got["after"]
    print(f"before = {args.before}, after = the working tree, one library; arrays compared with np.array_equal(equal_nan=True), "
          "call sequences and exceptions as text")
    groups, n_bad = {}, 0
    for key in sorted(set(before) | set(after)):
        ok = key in before and key in after and same(before[key], after[key])
        groups.setdefault(key.split("|")[0], []).append((key, ok))
    for name, found in sorted(groups.items()):
        arrays = [ok for key, ok in found if not key.endswith(("|calls", "|raised"))]
        calls = [(key, ok) for key, ok in found if key.endswith("|calls")]
        raised = sorted({str(after[key]) for key, _ in found if key.endswith("|raised") and key in after})
        n_calls = sum(len(str(after[key]).split("\n")) for key, _ in calls if key in after and str(after[key]))
        ok = all(ok for _, ok in found)
        n_bad += not ok
        print(f"{name:42s} {'equal' if ok else 'NOT EQUAL'}  ({sum(arrays)} of {len(arrays)} arrays, {sum(ok for _, ok in calls)} of {len(calls)} "
              f"call sequences, {n_calls} calls)" + (f"  raised in both: {'; '.join(raised)}" if raised and ok else ""))
        for key, ok in found:
            if not ok:
                print("    NOT EQUAL:", key)
    total = sum(a.size for k, a in after.items() if a.dtype.kind == "f")
    print(f"{len(groups)} cases, {len(after)} entries, {total} numbers, {n_bad} cases unequal")
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main())
