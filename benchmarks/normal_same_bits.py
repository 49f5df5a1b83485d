#!/usr/bin/env python3
"""Do two revisions of the Python package give the same bits, through the same library calls, on every path of Normal
(distribution/location_scale.py) and of the engine's per-model caches under it?

    mkdir -p build/ab/parent && git archive HEAD~1 openmcmc_amd tests benchmarks bench.py oracle | tar -x -C build/ab/parent
    python3 benchmarks/normal_same_bits.py [--before build/ab/parent]

The method, the child-process driver, the recorder of omc_* entry points and the comparison are those of
benchmarks/normal_normal_same_bits.py (one fresh child per source tree, one after the other, both on the in-tree libomcmc_hip.so;
np.array_equal(equal_nan=True) for every array, the call sequence as text, set-up calls included; one line per case, exit status 1 if
anything differs).  Only the case table and what a case calls are new.  A case builds a model of tests/normal_normal_models.py, puts
its state on the chains (MCMC's constructor; the chains are then moved apart on the host) and calls the methods of every Normal of
the model DIRECTLY, on a state no draw has touched: the engine's quadratic-form cache is empty, so residual_quad takes its own path.
In this order per distribution: residual_quad with replicates False and True, log_p, log_p(out=..., accumulate=True), log_p_piece,
grad_log_p and grad_terms for every per-chain parameter in the mean, rvs with injected normals, Engine.matrix_logdet; then one
NormalNormal.sample of the model's main block and residual_quad of every distribution again (what the draw left in the cache, or a
pass over the new state).  A call that raises is recorded as the exception's type and message and the case goes on.  The cases:
`smoother` over rw1, rw2 and full_spd (the tridiagonal, the band and the dense route) with a shared centre, both sides sampled,
replicates and a per-chain offset; `regression` with a diagonal and a correlated response precision (the weighted residual kernel
and the residual formed on the device); the long tridiagonal chain that takes the band route (two parts of one cache entry); the
exp-transformed mean with three replicates of tests/test_transform_gpu.py under its diagonal, a dense and a tridiagonal W.
Chains C in {3, 65}, n = 70; inputs come from a numpy seed on the host: both children see the same bytes.
"""
import os
import sys

import numpy as np
from normal_normal_same_bits import CHAINS, HOST_ERRORS, N, ROOT, Recorder, main


def transformed(W_kind, C, rng, eng):
    """The replicated response under an exp-transformed mean of tests/test_transform_gpu.py (three chains), W as asked"""
    from normal_normal_models import full_spd, rw1
    from test_transform_gpu import _param_setup

    from openmcmc_amd.model import Model

    G = np.load(os.path.join(ROOT, "tests", "golden", "transform_parameter.npz"))
    _, dist, state = _param_setup(G, "nrep3", eng)
    n_obs = state["y"].shape[0]
    if W_kind != "diag":
        state["W"] = full_spd(n_obs) if W_kind == "dense" else rw1(n_obs)
    return Model([dist]), state, [], set()


def cases():
    """(name, builder, its arguments, chains)"""
    from normal_normal_models import full_spd, regression, rw1, rw2, smoother
    from openmcmc_amd.sampler.sampler import NormalNormal

    table = []
    for route, P in (("tridiag", rw1), ("band", rw2), ("dense", full_spd)):
        for v in ["plain", "mean", "mean_first", "mean_lincomb", "replicated+const", "offset"]:
            table.append((f"{route}/{v}", smoother, (P(N), v, N), CHAINS))
    for v in ["diag", "corr", "corr+offset"]:
        table.append((f"regression/{v}", regression, (v, N), CHAINS))
    n_long = NormalNormal.TRIDIAG_WG_MAX + 1
    table.append((f"band/long_tridiagonal_n{n_long}", smoother, (rw1(n_long), "plain", n_long), (3,)))
    for W_kind in ["diag", "dense", "tridiag"]:
        table.append((f"transformed/nrep3/W_{W_kind}", transformed, (W_kind,), (3,)))
    return table


def save(out, tag, value):
    """The numbers of what a Normal method returned, under `tag`: tensors, ChainArrays, host arrays and sparse matrices, scalars,
    and tuples / lists / dicts of them (a ScaledHessian, the piece of log_p_piece, the terms of grad_terms)."""
    if value is None or isinstance(value, str):
        out[tag] = np.array(str(value))
    elif hasattr(value, "cpu"):
        out[tag] = value.cpu().numpy()
    elif hasattr(value, "data") and hasattr(value.data, "cpu"):
        out[tag] = value.data.cpu().numpy()
    elif hasattr(value, "tocoo"):  # (never densified: the Hessian of the long chain has 16385 rows)
        coo = value.tocoo()
        save(out, tag, {"shape": coo.shape, "row": coo.row, "col": coo.col, "data": coo.data})
    elif isinstance(value, dict):
        for k, v in value.items():
            save(out, f"{tag}/{k}", v)
    elif isinstance(value, (tuple, list)):
        for i, v in enumerate(value):
            save(out, f"{tag}/{i}", v)
    else:
        out[tag] = np.asarray(value)


def spread(state, rng):
    """The per-chain entries moved apart on the host, as tests/test_normal_normal_routes_gpu.py does: precision scalars stay positive"""
    import torch

    from openmcmc_amd.chains import is_chain

    for key, v in state.items():
        if is_chain(v):
            a = v.data.cpu().numpy()
            a = a * (0.5 + rng.random(a.shape)) if a.shape[1:] == (1, 1) else a + 0.3 * rng.standard_normal(a.shape)
            v.data.copy_(torch.as_tensor(a, device=v.data.device))


def child(path, tree):
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    sys.path.append(os.path.join(ROOT, "tests"))  # (the models of this revision, where the other tree has none)
    import openmcmc_amd
    import openmcmc_amd.engine as engine_module
    from openmcmc_amd.chains import is_chain
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.mcmc import MCMC
    from openmcmc_amd.sampler.sampler import NormalNormal

    assert os.path.dirname(os.path.dirname(os.path.abspath(openmcmc_amd.__file__))) == os.path.abspath(tree)
    log = []
    engine_module.lib = Recorder(engine_module.lib, log)
    out = {}
    for i_case, (name, builder, args, chains) in enumerate(cases()):
        for C in chains:
            tag = f"{name}|C{C}"
            rng = np.random.default_rng(1000 * i_case + C)
            eng = engine_module.Engine(C, seed=11)
            del log[:]

            def record(what, call):
                try:
                    save(out, f"{tag}|{what}", call())
                except HOST_ERRORS as e:  # (anything else, a device error above all, ends the child)
                    out[f"{tag}|{what}|raised"] = np.array(f"{type(e).__name__}: {e}")

            mdl, st, samplers, _ = builder(*args, C, rng, eng)
            state = MCMC(st, samplers, model=mdl, n_burn=0, n_iter=1, n_chains=C, engine=eng).state if samplers else st
            spread(state, rng)
            normals = [(key, dist) for key, dist in mdl.items() if isinstance(dist, Normal) and not dist.is_mixture]
            for key, dist in normals:
                size = dist.structure(state).n
                record(f"{key}.residual_quad", lambda: dist.residual_quad(state, eng, replicates=False))
                record(f"{key}.residual_quad(replicates)", lambda: dist.residual_quad(state, eng, replicates=True))
                record(f"{key}.log_p", lambda: dist.log_p(state, engine=eng))
                record(f"{key}.log_p(accumulate)", lambda: dist.log_p(state, engine=eng, out=eng.full((C,), 1.0), accumulate=True))
                record(f"{key}.log_p_piece", lambda: dist.log_p_piece(state, eng))
                for param in dist.mean.get_grad_param_list():
                    if param != key and is_chain(state[param]):
                        record(f"{key}.grad_log_p({param})", lambda: dist.grad_log_p(state, param, engine=eng))
                        record(f"{key}.grad_terms({param})", lambda: dist.grad_terms(state, param, eng))
                z = rng.standard_normal((C, size))
                record(f"{key}.rvs", lambda: dist.rvs(state, engine=eng, inject=z))
                record(f"{key}.matrix_logdet", lambda: eng.matrix_logdet(dist.structure(state)))
            blocks = [smp for smp in samplers if type(smp) is NormalNormal]
            if blocks:
                main_block = next((smp for smp in blocks if smp.param in ("b", "beta")), blocks[0])
                try:
                    state = main_block.sample(state)
                    save(out, f"{tag}|draw|{main_block.param}", state[main_block.param])
                    for key, dist in normals:
                        record(f"{key}.residual_quad(after the draw)", lambda: dist.residual_quad(state, eng, replicates=True))
                except HOST_ERRORS as e:
                    out[f"{tag}|draw|raised"] = np.array(f"{type(e).__name__}: {e}")
            eng.check_status()
            out[f"{tag}|calls"] = np.array("\n".join(log))
            eng.close()
    np.savez(path, **out)


if __name__ == "__main__":
    sys.exit(main(child, os.path.abspath(__file__)))
