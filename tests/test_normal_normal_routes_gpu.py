"""NormalNormal routes that no other GPU test reaches through `NormalNormal.sample`: one draw of the block with injected
draws on per-chain state, against a float64 host evaluation of Q_c^-1 b_c + L_c^-T z_c with Q_c and b_c assembled from the model
as the reference does (sampler/sampler.py:176-192) -- for a truncated prior the same single-site scan with the same uniforms
(oracle/gmrf_ref.py).  The models are those of tests/normal_normal_models.py: n = 70 crosses a 64-site
block, 65 chains cross a 64-chain block.  Bars: those of the existing tests of the same route (test_hier_gpu.py,
test_band_gpu.py, test_dense_gpu.py, test_truncated_gpu.py)."""

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu
N = 70


def relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def host(state, key, c):
    """state[key] as chain c sees it, a 2-D float64 array"""
    from openmcmc_amd.chains import is_chain

    v = state[key]
    if is_chain(v):
        return v.data[c].cpu().numpy().astype(np.float64)
    return v.toarray() if sparse.issparse(v) else np.asarray(v, dtype=np.float64)


def unscaled(dist, state, c):
    from openmcmc_amd.parameter import ScaledMatrix

    if isinstance(dist.precision, ScaledMatrix):
        return host(state, dist.precision.matrix, c), host(state, dist.precision.scalar, c).item()
    return host(state, dist.precision.form, c), 1.0


def mean_of(dist, state, c, exclude=None):
    from openmcmc_amd.parameter import Identity

    if isinstance(dist.mean, Identity):
        return host(state, dist.mean.form, c)
    return sum(host(state, A, c) @ host(state, k, c) for k, A in dist.mean.form.items() if k != exclude)


def assemble(smp, state, c):
    """(Q_c, b_c) of the conditional of smp.param, term by term as sampler/sampler.py:176-192"""
    from openmcmc_amd.parameter import Identity

    n = host(state, smp.param, c).shape[0]
    Q, b = np.zeros((n, n)), np.zeros((n, 1))
    for key, dist in smp.model.items():
        M, s = unscaled(dist, state, c)
        if key == smp.param:
            Q += s * M
            b += s * M @ mean_of(dist, state, c)
        elif isinstance(dist.mean, Identity):
            y = host(state, key, c)
            Q += y.shape[1] * s * M
            b += s * M @ y.sum(axis=1, keepdims=True)
        else:
            A = host(state, dist.mean.form[smp.param], c)
            rest = mean_of(dist, state, c, exclude=smp.param)
            Q += s * A.T @ M @ A
            b += s * A.T @ M @ (host(state, key, c) - rest)
    return Q, b


def prepare(builder, args, C, param, limits=None):
    """(MCMC, the sampler of `param`) on per-chain state: scalars, vectors and the start differ from chain to chain"""
    import torch

    from openmcmc_amd.chains import is_chain
    from openmcmc_amd.engine import Engine
    from openmcmc_amd.mcmc import MCMC

    rng = np.random.default_rng(C)
    eng = Engine(C, seed=3)
    mdl, st, samplers, _ = builder(*args, C, rng, eng)
    M = MCMC(st, samplers, model=mdl, n_burn=0, n_iter=1, n_chains=C, engine=eng)
    for key, v in M.state.items():
        if not is_chain(v):
            continue
        a = v.data.cpu().numpy()
        if key == param:
            a = a + 0.1 * rng.random(a.shape)
            if limits is not None:
                a = np.clip(a, limits[0] + 0.05, limits[1] - 0.05)
        elif a.shape[1:] == (1, 1):
            a = a * (0.5 + rng.random(a.shape))  # (the precision scalars stay positive)
        else:
            a = a + 0.3 * rng.standard_normal(a.shape)
        v.data.copy_(torch.as_tensor(a, device=v.data.device))
    return M, next(s for s in samplers if s.param == param), rng


def chains_checked(C):
    return sorted({0, 1, C // 2, 63 % C, C - 1})


def check_quadratic_forms(smp, state, eng, C, tol):
    """What the draw left in the engine's cache (or a pass over the state) is r'Mr of every term for the new state"""
    for key, dist in smp.model.items():
        got = dist.residual_quad(state, eng).cpu().numpy()
        for c in chains_checked(C):
            M, _ = unscaled(dist, state, c)
            r = host(state, key, c) - mean_of(dist, state, c)
            assert abs(got[c] - (r.T @ M @ r).item()) < tol * max(1.0, abs(got[c])), (key, c)


COLD = [(P, v) for P in ("rw1", "rw2", "full_spd") for v in ("plain", "mean", "replicated+const")] + [("regression", "diag"),
                                                                                                      ("regression", "corr")]


@pytest.mark.parametrize("C", [3, 65])
@pytest.mark.parametrize("matrix,variant", COLD)
def test_residual_quad_on_a_state_no_draw_has_touched(matrix, variant, C):
    """The checks above run after a draw and mostly read the engine's cache.  Here nothing has been drawn: residual_quad of every
    Normal of the model takes its own path -- a shared centre, both sides sampled and three replicates of the response on the
    tridiagonal, the band and the dense route; the weighted residual kernel and the residual formed on the device under a design
    matrix -- against sum over the columns of r'Mr on the host.  Bar: check_quadratic_forms' 1e-10."""
    import normal_normal_models as models

    if matrix == "regression":
        M, smp, _ = prepare(models.regression, (variant, N), C, "beta")
    else:
        M, smp, _ = prepare(models.smoother, (getattr(models, matrix)(N), variant, N), C, "b")
    eng, state = M.engine, M.state
    for key, dist in smp.model.items():
        if not hasattr(dist, "residual_quad"):
            continue  # (the Gamma priors of the scalars)
        got = dist.residual_quad(state, eng, replicates=True).cpu().numpy()
        eng.check_status()
        for c in chains_checked(C):
            P, _ = unscaled(dist, state, c)
            r = host(state, key, c) - mean_of(dist, state, c)  # (n, n_rep): the mean is one column
            assert abs(got[c] - np.sum(r * (P @ r))) < 1e-10 * max(1.0, abs(got[c])), (key, c)
    eng.close()


TRIDIAGONAL = ["mean_lincomb", "mean+const", "mean_lincomb+const", "two_vectors", "offset+mean", "offset+two_vectors", "replicated+const"]
# (at n = 700 a workgroup serves a chain, the form of the kernel that takes the per-chain centre inside the launch)
TRIDIAGONAL = [(v, N) for v in TRIDIAGONAL] + [(v, 700) for v in TRIDIAGONAL[:3]]


@pytest.mark.parametrize("C", [3, 65])
@pytest.mark.parametrize("variant,n", TRIDIAGONAL)
def test_tridiagonal_block_with_per_chain_terms(variant, n, C):
    """A sampled prior mean through a LinearCombination, next to an unscaled constant-diagonal term (the cached quadratic form
    carries its factor), two per-chain vectors in one block (the second product accumulates into the first), an offset with
    one and with two vectors, three replicates of the response.  Bar: test_hier_gpu.py's 1e-10."""
    from normal_normal_models import rw1, smoother
    from oracle import gmrf_ref

    M, smp, rng = prepare(smoother, (rw1(n), variant, n), C, "b")
    eng = M.engine
    z = rng.standard_normal((C, n))
    smp.inject = lambda s, t: eng.to_device(z)
    want = {c: assemble(smp, M.state, c) for c in chains_checked(C)}
    M.state = smp.sample(M.state)
    eng.check_status()
    x = M.state["b"].vector().cpu().numpy()
    for c, (Q, b) in want.items():
        ref, _, _ = gmrf_ref.draw_canonical(b, sparse.csc_matrix(Q), z[c])
        assert relerr(x[c], np.asarray(ref).ravel()) < 1e-10, c
    if "replicated" not in variant:
        check_quadratic_forms(smp, M.state, eng, C, 1e-10)
    eng.close()


@pytest.mark.parametrize("C", [3, 65])
@pytest.mark.parametrize("route,variant", [("tridiag", "trunc2"), ("band", "trunc1"), ("band", "trunc2")])
def test_truncated_prior_scans(route, variant, C):
    """A two-sided truncation on the tridiagonal route, a one- and a two-sided one on the band route: the one scan from the
    current value with injected uniforms.  Bars: test_truncated_gpu.py's 1e-10 (NormalNormal with a truncated prior) and, for
    the band scan, its 1e-9 * max(1, |x|)."""
    from normal_normal_models import rw1, rw2, smoother
    from oracle import gmrf_ref

    lo, hi = 0.5, (4.5 if variant == "trunc2" else np.inf)
    M, smp, rng = prepare(smoother, ((rw1 if route == "tridiag" else rw2)(N), variant, N), C, "b", limits=(lo, min(hi, 4.5)))
    eng = M.engine
    u = rng.random((C, N))
    smp.inject = lambda s, t: eng.to_device(u)
    x0 = M.state["b"].vector().cpu().numpy().copy()
    want = {c: assemble(smp, M.state, c) for c in chains_checked(C)}
    M.state = smp.sample(M.state)
    eng.check_status()
    x = M.state["b"].vector().cpu().numpy()
    assert x.min() >= lo and x.max() <= hi
    for c, (Q, b) in want.items():
        ref = gmrf_ref.gibbs_truncated_scan(b, Q, x0[c], lo, hi, u[c]).ravel()
        if route == "tridiag":
            assert np.max(np.abs(x[c] - ref) / np.maximum(1.0, np.abs(ref))) < 1e-10, c
        else:
            assert np.max(np.abs(x[c] - ref)) < 1e-9 * max(1.0, np.max(np.abs(ref))), c
    eng.close()


@pytest.mark.parametrize("C", [3, 65])
@pytest.mark.parametrize("variant,p,param", [("corr", N, "beta"), ("corr+offset", N, "beta"), ("corr+offset", N, "gamma"),
                                             ("diag+factorise", 64, "beta")])
def test_dense_regression_blocks(variant, p, param, C):
    """A correlated (tridiagonal) response precision under a design matrix, alone and with the other block's per-chain offset
    (both blocks), and the factorisation route at the order where the spectral route would start.  Bar: the 1e-9 of
    test_dense_gpu.py's run through the samplers and of test_hier_gpu.py's two-block model."""
    from normal_normal_models import regression
    from oracle import gmrf_ref

    M, smp, rng = prepare(regression, (variant, p), C, param)
    eng = M.engine
    n = M.state[param].shape[0]
    z = rng.standard_normal((C, n))
    smp.inject = lambda s, t: eng.to_device(z)
    want = {c: assemble(smp, M.state, c) for c in chains_checked(C)}
    M.state = smp.sample(M.state)
    eng.check_status()
    x = M.state[param].vector().cpu().numpy()
    for c, (Q, b) in want.items():
        ref, _, _ = gmrf_ref.draw_canonical(b, Q, z[c])
        assert relerr(x[c], np.asarray(ref).ravel()) < 1e-9, c
    eng.close()


@pytest.mark.parametrize("C", [3, 65])
def test_spectral_route_through_the_sampler(C):
    """Order 64, `scaled identity + one shared matrix`, the chains' own draws: the block takes the spectral route, once, and
    its draw is the library's spectral draw for the same terms and draw index, whose mean is Q_c^-1 b_c.  Bars:
    test_dense_gpu.py's spectral test, 1e-11 between two device evaluations and 1e-10 against the host mean."""
    from normal_normal_models import regression

    p = 64
    M, smp, _ = prepare(regression, ("diag", p), C, "beta")
    eng, st = M.engine, M.state
    calls = []
    spectral_sample = eng.dense_spectral_sample
    eng.dense_spectral_sample = lambda *a, **k: (calls.append(1), spectral_sample(*a, **k))[1]
    want = {c: assemble(smp, st, c) for c in chains_checked(C)}
    index = smp._draw_index()
    M.state = smp.sample(st)
    eng.dense_spectral_sample = spectral_sample
    assert len(calls) == 1
    X, w = eng.to_device(np.asarray(st["X"])), eng.to_device(st["P_tau"].diagonal())
    G = eng.gram(X, w)
    terms = [{"mat": G, "rhs": eng.design_rhs(X, eng.to_device(np.asarray(st["y"]).ravel()), w), "scale": st["tau"].scalar()},
             {"mat": None, "scale": st["lambda"].scalar()}]
    x2, mean = eng.empty(C, p), eng.empty(C, p)
    eng.dense_spectral_sample(p, terms, 0, *eng.dense_spectral_prepare(G), x2, draw_index=index, mean_out=mean)
    eng.check_status()
    assert relerr(M.state["beta"].vector().cpu().numpy(), x2.cpu().numpy()) < 1e-11
    for c, (Q, b) in want.items():
        mu = np.linalg.solve(Q, b).ravel()
        assert np.max(np.abs(mean[c].cpu().numpy() - mu)) < 1e-10 * np.max(np.abs(mu)), c
    eng.close()
