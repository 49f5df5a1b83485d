#!/usr/bin/env python3
"""Do two revisions of the Python package give the same bits, through the same library calls, on every route of the
Metropolis-Hastings samplers (sampler/metropolis_hastings.py, sampler/reversible_jump.py)?

    mkdir -p build/ab/parent && git archive HEAD~1 openmcmc_amd tests benchmarks bench.py oracle | tar -x -C build/ab/parent
    python3 benchmarks/mh_same_bits.py [--before build/ab/parent]

The method, the child-process driver, the recorder of omc_* entry points and the comparison are those of
benchmarks/normal_normal_same_bits.py (one fresh child per source tree, one after the other, both on the in-tree libomcmc_hip.so;
np.array_equal(equal_nan=True) for every array, the call sequence as text; one line per case, exit status 1 if anything differs).  Only
the case table is new.  Every case runs 2 burn-in and 4 stored sweeps, once with the chains' own draws and once with draws injected
through the samplers' hooks (then with `trace` switched on where the route keeps one), at C = 3 and 65 chains (65 crosses a 64-chain
block), and saves every store entry, the final per-chain state, the accept and proposal counters, `last_log_p` where set and the
trace.  The cases: the fused Gaussian steps (RandomWalk; ManifoldMALA whitened and on the products) at d = 1, 5, 24, as single steps,
through MCMC.run_mcmc with n_iter = 40 (blocks of steps: a 32-step block is crossed), once with a ring store, and in a run where the
library overwrites x and the state entry is replaced between steps; a generic RandomWalk with domain limits; RandomWalkLoop on the knots
of tests/rj_problem.py (n = 70, n_max = 6) by the fused loop and launch by launch; ManifoldMALA on each of its other routes ("diag" on
the prior model of tests/rj_problem.py, "transform" at p = 5, "dense" at p = 5 under a scaled and under a mixture prior, "general" at
d = 5 and at d = 65, past the small kernels); the whole reversible-jump sweep of tests/rj_problem.py with matched transitions, with and
without limits.  Inputs come from a numpy seed on the host: both children see the same bytes.
"""
import os
import sys

import numpy as np
from normal_normal_same_bits import HOST_ERRORS, ROOT, Recorder, main

CHAINS = (3, 65)
N_BURN, N_ITER = 2, 4
N_SWEEPS = N_BURN + N_ITER
N_KNOT, N_MAX = 70, 6


def spd(d, rng):
    A = rng.standard_normal((d, 2 * d))
    Q = np.linalg.inv(A @ A.T / (2 * d))
    return (Q + Q.T) / 2


class Run:
    """One case on one engine: the samplers whose hooks take injected draws, what is run and what is saved of it."""

    def __init__(self, C, rng, eng, inject):
        import torch

        self.C, self.rng, self.eng, self.inject, self.torch = C, rng, eng, inject, torch
        self.store, self.state, self.samplers = {}, {}, []

    def hooks(self, smp, size, uniform=False, columns=None, trace=True, sweeps=N_SWEEPS):
        """Injected draws for `inject` ((C, size); (C, 1) per column of a loop) and `inject_uniform`, and the trace, in inject mode."""
        self.samplers.append(smp)
        if not self.inject:
            return smp
        shape = (sweeps, self.C, size) if columns is None else (sweeps, columns, self.C, 1)
        z = self.rng.uniform(0.05, 0.95, shape) if uniform else self.rng.standard_normal(shape)
        u = self.rng.uniform(0.05, 0.95, shape[:-1])
        dev = self.eng.to_device
        smp.inject = lambda s, it, *j: dev(z[(it, *j)])
        smp.inject_uniform = lambda s, it, *j: dev(u[(it, *j)])
        if trace:
            smp.trace = {}
        return smp

    def loop(self, smp, state, n=N_SWEEPS, between=None):
        """n sweeps of one sampler on its own; the parameter after every stored sweep is the store."""
        kept = []
        for i in range(n):
            state = smp.sample(state if between is None else between(i, state))
            if i >= n - N_ITER:
                kept.append(state[smp.param].data.clone())
        self.store, self.state = {smp.param: self.torch.stack(kept)}, state

    def mcmc(self, state, samplers, mdl, n_iter=N_ITER, **kw):
        from openmcmc_amd.mcmc import MCMC

        M = MCMC(state, samplers, model=mdl, n_burn=N_BURN, n_iter=n_iter, n_chains=self.C, engine=self.eng, **kw)
        return M

    def run_mcmc(self, M):
        M.run_mcmc()
        self.store, self.state = M.collect(), M.state


def gaussian(d, C, rng, eng):
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model

    mdl = Model([Normal("x", mean="mu", precision="Q")])
    x0 = 0.5 * rng.standard_normal((C, d, 1))
    return mdl, {"x": ChainArray(eng.to_device(x0)), "mu": 0.3 * rng.standard_normal((d, 1)), "Q": spd(d, rng)}, x0


def fused_sampler(kind, mdl):
    from openmcmc_amd.sampler.metropolis_hastings import ManifoldMALA, RandomWalk

    if kind == "rw":
        return RandomWalk("x", mdl, step=np.array([[0.1]]))
    return ManifoldMALA("x", mdl, step=np.array([[0.5]]), whitened=kind == "mala_white")


def case_fused(R, kind, d):
    mdl, state, _ = gaussian(d, R.C, R.rng, R.eng)
    R.loop(R.hooks(fused_sampler(kind, mdl).bind(R.eng), d), state)


def case_fused_mcmc(R, d, ring):
    mdl, state, _ = gaussian(d, R.C, R.rng, R.eng)
    smp = fused_sampler("mala_white", mdl)
    M = R.mcmc(state, [smp], mdl, n_iter=40, store_ring=ring)
    R.hooks(smp, d, trace=False, sweeps=N_BURN + 40)
    R.run_mcmc(M)


def case_fused_disturbed(R, kind):
    """tests/test_mh_gpu.py::test_cached_whitened_state_notices_library_writes: the library overwrites x, then a fresh state entry"""
    from openmcmc_amd.chains import ChainArray

    d = 24
    mdl, state, x0 = gaussian(d, R.C, R.rng, R.eng)
    other = R.eng.to_device(R.rng.standard_normal((R.C, d)))

    def between(i, st):
        if i == 2:
            R.eng.chain_copy(other, st["x"].vector())
        if i == 4:
            st["x"] = ChainArray(R.eng.to_device(x0))
        return st
    R.loop(R.hooks(fused_sampler(kind, mdl).bind(R.eng), d), state, between=between)


def case_rw_limits(R):
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.sampler.metropolis_hastings import RandomWalk

    d = 5
    mdl, state, x0 = gaussian(d, R.C, R.rng, R.eng)
    state["x"] = ChainArray(R.eng.to_device(np.clip(x0, -0.9, 0.9)))
    smp = RandomWalk("x", mdl, step=np.array([[0.3]]), domain_limits=np.tile([-1.0, 1.0], (d, 1))).bind(R.eng)
    R.loop(R.hooks(smp, d, uniform=True), state)


def knot_problem(R, fused=True):
    """(model, state, samplers) of tests/rj_problem.py at n = 70, n_max = 6, one to four knots per chain"""
    from rj_problem import build
    from scipy import sparse

    n, rng = N_KNOT, R.rng
    X = np.linspace(-9.0, 9.0, n)
    y = np.sin(X / 2.0) + 0.2 * rng.standard_normal(n)
    diag = np.full(n, 2.0)
    diag[0] = diag[-1] = 1.0 + 1e-3
    P = sparse.diags((-np.ones(n - 1), diag, -np.ones(n - 1)), offsets=[-1, 0, 1]).toarray()
    k0 = rng.integers(1, 5, R.C)
    theta = [rng.uniform(-8.0, 8.0, int(k)) for k in k0]
    beta = [rng.standard_normal(int(k)) for k in k0]
    return build(y, X, P, N_MAX, R.eng, theta, beta, k0, fused=fused)


def case_knots(R, fused):
    mdl, state, samplers = knot_problem(R, fused)
    M = R.mcmc(state, samplers, mdl)  # (binds the samplers and puts the scalars on the chains)
    R.loop(R.hooks(samplers[4], 1, uniform=True, columns=N_MAX, trace=not fused), M.state)


def case_rj(R, limits):
    mdl, state, samplers = knot_problem(R)
    rw, rj = samplers[4], samplers[5]
    if not limits:
        rj.matching_params["limits"] = None
    M = R.mcmc(state, samplers, mdl)
    R.hooks(rw, 1, uniform=True, columns=N_MAX, trace=False)
    R.hooks(rj, 1, uniform=True)
    if R.inject:
        dev, C, rng = R.eng.to_device, R.C, R.rng
        move, assoc = rng.uniform(0.05, 0.95, (N_SWEEPS, C)), rng.uniform(0.05, 0.95, (N_SWEEPS, C, 1))
        match = rng.uniform(0.05, 0.95, (N_SWEEPS, C)) if limits else rng.standard_normal((N_SWEEPS, C))
        first = R.torch.zeros(C, dtype=R.torch.int64, device=R.eng.device)  # (a death deletes the first knot: there always is one)
        rj.inject_move = lambda s, it: (dev(move[it]), first)
        rj.inject_associated = lambda s, it: {"theta": dev(assoc[it])}
        rj.inject_match = lambda s, it: dev(match[it])
    R.run_mcmc(M)


def case_diag(R):
    from rj_problem import build_prior_model

    rng = R.rng
    k0 = rng.integers(1, 5, R.C)
    lists = lambda draw: [draw(int(k)) for k in k0]  # noqa: E731
    mdl, state, samplers = build_prior_model(np.linspace(-9.0, 9.0, N_KNOT), N_MAX, R.eng, lists(lambda k: rng.uniform(-8.0, 8.0, k)),
                                             lists(lambda k: rng.uniform(0.8, 1.5, k)), lists(rng.standard_normal), k0)
    M = R.mcmc(state, samplers, mdl)
    assert getattr(samplers[0], "route", lambda s: "diag")(M.state) == "diag"
    R.loop(R.hooks(samplers[0], N_MAX), M.state)


def regression(R, p, prior, lognormal=False):
    """y ~ N(A beta, (tau W)^-1) under a scaled Normal, a mixture Normal or a LogNormal prior on the per-chain (p, 1) vector"""
    from scipy import sparse

    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.location_scale import LogNormal, Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombination, MixtureParameterMatrix, MixtureParameterVector, ScaledMatrix

    rng, eng, C, n = R.rng, R.eng, R.C, p + 7
    A = np.vstack([2.0 * np.eye(p), 0.3 * rng.standard_normal((n - p, p))])
    truth = 1.0 + 0.2 * rng.standard_normal(p)
    full = lambda v: ChainArray(eng.full((C, 1, 1), float(v)))  # noqa: E731
    B = rng.standard_normal((p, p + 3))
    state = {"y": (A @ truth + 0.1 * rng.standard_normal(n)).reshape(n, 1), "A": A, "W": sparse.diags(rng.uniform(0.5, 1.5, n), format="csc"),
             "tau": full(10.0), "beta": ChainArray(eng.to_device(1.0 + 0.1 * rng.uniform(-1.0, 1.0, (C, p, 1)))), "lam": full(2.0),
             "mu": np.full((p, 1), 0.5), "P": B @ B.T / p + np.eye(p), "prior_mean": np.array([[0.0], [1.0], [2.0]]),
             "prior_prec": np.array([[0.5], [1.0], [4.0]]), "alloc": ChainArray(eng.to_device(rng.integers(0, 3, (C, p, 1)).astype(np.float64))),
             "Q_s": 0.5 * np.eye(p)}
    priors = {"scaled": lambda: Normal("beta", mean="mu", precision=ScaledMatrix("P", "lam")),
              "mixture": lambda: Normal("beta", mean=MixtureParameterVector("prior_mean", "alloc"),
                                        precision=MixtureParameterMatrix("prior_prec", "alloc")),
              "lognormal": lambda: LogNormal("beta", mean="mu", precision="Q_s")}
    return Model([Normal("y", mean=LinearCombination({"beta": "A"}), precision=ScaledMatrix("W", "tau")), priors[prior]()]), state


def case_mala_route(R, route, p, prior):
    from openmcmc_amd.sampler.metropolis_hastings import ManifoldMALA

    mdl, state = regression(R, p, prior)
    smp = ManifoldMALA("beta", mdl, step=np.array(0.4)).bind(R.eng)
    assert getattr(smp, "route", lambda s: route)(state) == route
    R.loop(R.hooks(smp, p), state)


def case_transform(R):
    from scipy import sparse

    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombinationWithTransform, ScaledMatrix
    from openmcmc_amd.sampler.metropolis_hastings import ManifoldMALA

    rng, eng, C, p, n = R.rng, R.eng, R.C, 5, 12
    A = rng.uniform(0.2, 1.0, (n, p))
    mdl = Model([Normal("y", mean=LinearCombinationWithTransform(form={"s": "A"}, transform={"s": True}), precision=ScaledMatrix("W", "tau")),
                 Normal("s", mean="m0", precision="P0")])
    state = {"A": A, "y": np.tile((A @ np.exp(0.2 * rng.standard_normal(p))).reshape(n, 1), (1, 2)) + 0.05 * rng.standard_normal((n, 2)),
             "s": ChainArray(eng.to_device(0.1 * rng.standard_normal((C, p, 1)))), "W": sparse.diags(rng.uniform(0.5, 1.5, n), format="csc"),
             "tau": ChainArray(eng.full((C, 1, 1), 4.0)), "m0": 0.1 * rng.standard_normal((p, 1)), "P0": np.eye(p)}
    smp = ManifoldMALA("s", mdl, step=np.array(0.3)).bind(eng)
    assert smp._transform_plan(state) is not None
    R.loop(R.hooks(smp, p), state)


def cases():
    """(name, function of a Run, its further arguments)"""
    table = []
    for kind in ("rw", "mala_white", "mala_products"):
        table += [(f"fused/{kind}/d{d}", case_fused, (kind, d)) for d in (1, 5, 24)]
    table += [(f"fused/mala_white/run_mcmc_n40/d{d}", case_fused_mcmc, (d, 0)) for d in (1, 5, 24)]
    table.append(("fused/mala_white/run_mcmc_n40/ring16/d5", case_fused_mcmc, (5, 16)))
    table += [(f"fused/{kind}/library_write_and_new_entry", case_fused_disturbed, (kind,)) for kind in ("rw", "mala_white")]
    table.append(("generic/rw_limits/d5", case_rw_limits, ()))
    table += [(f"knots/{'fused' if fused else 'launches'}", case_knots, (fused,)) for fused in (True, False)]
    table.append(("mala/diag", case_diag, ()))
    table.append(("mala/transform/p5", case_transform, ()))
    table += [(f"mala/dense/{prior}/p5", case_mala_route, ("dense", 5, prior)) for prior in ("scaled", "mixture")]
    table += [(f"mala/general/d{d}", case_mala_route, ("general", d, "lognormal")) for d in (5, 65)]
    table += [(f"rj_sweep/{'limits' if limits else 'no_limits'}", case_rj, (limits,)) for limits in (True, False)]
    return table


def flatten(prefix, node, out):
    """The tensors of a trace (dicts and lists of them) as arrays under their path."""
    if isinstance(node, dict):
        for k, v in node.items():
            flatten(f"{prefix}/{k}", v, out)
    elif isinstance(node, (list, tuple)):
        for i, v in enumerate(node):
            flatten(f"{prefix}/{i}", v, out)
    elif hasattr(node, "cpu"):
        out[prefix] = node.cpu().numpy()


def child(path, tree):
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    sys.path.append(os.path.join(ROOT, "tests"))
    import openmcmc_amd
    import openmcmc_amd.engine as engine_module
    from openmcmc_amd.chains import is_chain

    assert os.path.dirname(os.path.dirname(os.path.abspath(openmcmc_amd.__file__))) == os.path.abspath(tree)
    log = []
    engine_module.lib = Recorder(engine_module.lib, log)
    out = {}
    for i_case, (name, fn, args) in enumerate(cases()):
        for C in CHAINS:
            for inject in (False, True):
                tag = f"{name}|C{C}|{'inject' if inject else 'stream'}"
                eng = engine_module.Engine(C, seed=11)
                R = Run(C, np.random.default_rng(1000 * i_case + C), eng, inject)
                del log[:]
                try:
                    fn(R, *args)
                    eng.check_status()
                    for key, t in R.store.items():
                        out[f"{tag}|store|{key}"] = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
                    for key, v in R.state.items():
                        if is_chain(v):
                            out[f"{tag}|state|{key}"] = v.data.cpu().numpy()
                    for smp in R.samplers:
                        out[f"{tag}|accept|{smp.param}"] = smp.accept_rate.accept.cpu().numpy()
                        out[f"{tag}|proposal|{smp.param}"] = smp.accept_rate.proposal.cpu().numpy()
                        if getattr(smp, "last_log_p", None) is not None:
                            out[f"{tag}|last_log_p|{smp.param}"] = smp.last_log_p[0].cpu().numpy()
                        if smp.trace is not None:
                            flatten(f"{tag}|trace|{smp.param}", smp.trace, out)
                except HOST_ERRORS as e:  # (anything else, a device error above all, ends the child)
                    out[f"{tag}|raised"] = np.array(f"{type(e).__name__}: {e}")
                out[f"{tag}|calls"] = np.array("\n".join(log))
                eng.close()
    np.savez(path, **out)


if __name__ == "__main__":
    sys.exit(main(child, os.path.abspath(__file__)))
