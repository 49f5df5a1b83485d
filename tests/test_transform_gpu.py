"""LinearCombinationWithTransform on the GPU: omc_transform_predict / omc_transform_grad_hess against numpy and the reference
(tests/golden/transform_parameter.npz), and ManifoldMALA on a parameter under the transform -- the fused step
(omc_mala_transform_step) and the launch-by-launch route -- replaying the reference's chains (tests/golden/transform_mala.npz).

Bounds: 1e-13 for the predictor, per output and relative to sum_j |X_ij| exp(x_j) (+ |extras|), the scale of that output's own
rounding error (an index-order fp64 sum against numpy's), 1e-10 relative for fp64 quantities against
the reference, and for the chain replays max(1e-9, 100 sens[t]) max(1, |ref|) with sens[t] the reference's own response to
last-bit noise in its inputs (make_golden_r6.py).  Observed maxima are printed (pytest -s) and recorded in DESIGN.md."""

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu


def make_engine(C, **kw):
    from openmcmc_amd.engine import Engine

    return Engine(C, **kw)


# ----------------------------------------------------------------------------- omc_transform_predict
@pytest.mark.parametrize("n", [1, 7, 1000])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 500])
def test_transform_predict_against_numpy(p, n):
    rng = np.random.default_rng(1000 * p + n)
    C = 5  # not a multiple of anything the kernel blocks by
    eng = make_engine(C)
    X, x = rng.standard_normal((n, p)), 0.5 * rng.standard_normal((C, p))
    add_c, add_s, cs = rng.standard_normal((C, n)), rng.standard_normal(n), rng.random(C) + 0.5
    ref0 = np.exp(x) @ X.T
    Xd, xd = eng.to_device(X), eng.to_device(x)

    mag0 = np.exp(x) @ np.abs(X).T   # sum_j |X_ij| exp(x_j): what each output's own rounding error scales with

    def rel(got, ref, alpha=1.0, sc=None, ac=None, as_=None):
        mag = abs(alpha) * (1.0 if sc is None else sc[:, None]) * mag0 + (0.0 if ac is None else np.abs(ac)) + (0.0 if as_ is None else np.abs(as_))
        return float(np.max(np.abs(got - ref) / mag))

    worst = rel(eng.transform_predict(Xd, xd).cpu().numpy(), ref0)
    # every nullable extra, alone and together
    for ac, as_, alpha, sc in [(add_c, None, 1.0, None), (None, add_s, 1.0, None), (None, None, -0.5, None), (None, None, 1.0, cs),
                               (add_c, add_s, -1.0, cs)]:
        got = eng.transform_predict(Xd, xd, add_chain=None if ac is None else eng.to_device(ac),
                                    add_shared=None if as_ is None else eng.to_device(as_), alpha=alpha,
                                    chain_scale=None if sc is None else eng.to_device(sc)).cpu().numpy()
        ref = alpha * (1.0 if sc is None else sc[:, None]) * ref0 + (0.0 if ac is None else ac) + (0.0 if as_ is None else as_)
        worst = max(worst, rel(got, ref, alpha, sc, ac, as_))
    # strided operands: X, x, add_chain and out are the leading columns of wider tensors
    Xw, xw = eng.to_device(np.hstack([X, rng.standard_normal((n, 3))])), eng.to_device(np.hstack([x, rng.standard_normal((C, 2))]))
    aw, ow = eng.to_device(np.hstack([add_c, rng.standard_normal((C, 5))])), eng.full((C, n + 4), 7.0)
    eng.transform_predict(Xw[:, :p], xw[:, :p], add_chain=aw[:, :n], out=ow[:, :n])
    worst = max(worst, rel(ow[:, :n].cpu().numpy(), ref0 + add_c, ac=add_c))
    assert np.all(ow[:, n:].cpu().numpy() == 7.0)
    print(f"transform_predict p={p} n={n}: max relative error {worst:.2e}")
    assert worst <= 1e-13
    # exp overflows to inf as numpy's does
    x_inf = x.copy()
    x_inf[2, p // 2] = 710.0
    Xpos = np.abs(X) + 0.1
    with np.errstate(over="ignore"):
        ref = np.exp(x_inf) @ Xpos.T
    got = eng.transform_predict(eng.to_device(Xpos), eng.to_device(x_inf)).cpu().numpy()
    assert np.all(np.isposinf(got[2])) and np.all(np.isposinf(ref[2]))
    assert np.all(np.isfinite(got[[0, 1, 3, 4]]))
    eng.close()


# ----------------------------------------------------------------------------- the parameter and the Normal around it
CASES = ["all", "none", "mixed", "sparseA", "nrep3", "scaled"]


def _param_setup(G, tag, eng):
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.parameter import LinearCombinationWithTransform, ScaledMatrix

    A = G[f"{tag}_A"]
    n, p = A.shape
    form, transform = {"s": "A"}, {"s": bool(G[f"{tag}_tr_s"])}
    if G[f"{tag}_second"]:
        form["g"], transform["g"] = "B", False
    mean = LinearCombinationWithTransform(form=form, transform=transform)
    tau = float(G[f"{tag}_tau"])
    dist = Normal("y", mean=mean, precision="W" if np.isnan(tau) else ScaledMatrix("W", "tau"))
    state = {"A": sparse.csc_matrix(A) if G[f"{tag}_sparse_A"] else A, "B": G[f"{tag}_B"], "g": G[f"{tag}_g"].reshape(-1, 1),
             "s": ChainArray(eng.to_device(G[f"{tag}_S"])), "y": G[f"{tag}_y"], "W": sparse.diags(G[f"{tag}_w"], format="csc"),
             "tau": ChainArray(eng.full((3, 1, 1), 1.0 if np.isnan(tau) else tau))}
    return mean, dist, state


def _rel(got, ref):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(ref))) / max(np.max(np.abs(ref)), 1e-300))


@pytest.mark.parametrize("tag", CASES)
def test_predictor_logp_and_gradients_match_the_reference(golden, tag):
    import torch

    from openmcmc_amd.distribution.location_scale import ScaledHessian
    from openmcmc_amd.parameter import LinearCombination

    G = golden("transform_parameter")
    eng = make_engine(3)
    mean, dist, state = _param_setup(G, tag, eng)
    errs = {"pred": _rel(mean.predictor_device(state, eng).cpu().numpy(), G[f"{tag}_pred"])}
    if tag == "none":  # all transforms False: LinearCombination, bit for bit
        plain = LinearCombination(dict(mean.form)).predictor_device(state, eng)
        assert torch.equal(plain, mean.predictor_device(state, eng))
    errs["logp"] = _rel(dist.log_p(state, engine=eng).cpu().numpy(), G[f"{tag}_logp"])
    obs = dist.log_p(state, by_observation=True, engine=eng).cpu().numpy()
    assert G[f"{tag}_logp_obs"].shape == obs.shape, (obs.shape, G[f"{tag}_logp_obs"].shape)
    errs["logp_obs"] = _rel(obs, G[f"{tag}_logp_obs"])
    grad, H = dist.grad_log_p(state, "s", hessian_required=True, engine=eng)
    errs["grad"] = _rel(grad.numpy()[:, :, 0], G[f"{tag}_glp_grad"])
    if isinstance(H, torch.Tensor):
        Hh = H.cpu().numpy()
    elif isinstance(H, ScaledHessian):
        Hh = H.scale.cpu().numpy()[:, None, None] * np.asarray(H.matrix)[None]
    else:
        Hh = np.broadcast_to(H.toarray() if sparse.issparse(H) else np.asarray(H), G[f"{tag}_glp_hess"].shape)
    assert bool(G[f"{tag}_tr_s"]) == isinstance(H, torch.Tensor)  # the per-chain Hessian exactly where the reference's moves
    errs["hess"] = _rel(Hh, G[f"{tag}_glp_hess"])
    print(tag, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-10, errs
    eng.check_status()
    eng.close()


def test_transform_grad_hess_against_numpy():
    rng = np.random.default_rng(5)
    for p, C in [(1, 3), (7, 5), (64, 4), (130, 3)]:   # any p: beyond one wave's 64 columns too
        eng = make_engine(C)
        x, u, sc = 0.5 * rng.standard_normal((C, p)), rng.standard_normal((C, p)), rng.random(C) + 0.5
        R = rng.standard_normal((p, p))
        Gm = R @ R.T
        s = np.exp(x)
        for scale in (None, sc):
            k = np.ones(C) if scale is None else scale
            g, H = eng.transform_grad_hess(eng.to_device(x), eng.to_device(Gm), u=eng.to_device(u),
                                           scale=None if scale is None else eng.to_device(scale))
            assert _rel(g.cpu().numpy(), k[:, None] * s * u) <= 1e-10
            assert _rel(H.cpu().numpy(), k[:, None, None] * s[:, :, None] * s[:, None, :] * Gm[None]) <= 1e-10
        g, H = eng.transform_grad_hess(eng.to_device(x), eng.to_device(Gm), u=None)
        assert g is None and H is not None
        g, H = eng.transform_grad_hess(eng.to_device(x), eng.to_device(Gm), u=eng.to_device(u), want_hess=False)
        assert H is None and _rel(g.cpu().numpy(), s * u) <= 1e-10
        eng.close()


# ----------------------------------------------------------------------------- chain replays
def _mala_setup(G, tag, eng, C, fused):
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombinationWithTransform, ScaledMatrix
    from openmcmc_amd.sampler.metropolis_hastings import ManifoldMALA

    A = G[f"{tag}_A"]
    d = A.shape[1]
    form, transform = {"s": "A"}, {"s": True}
    if G[f"{tag}_second"]:
        form["g"], transform["g"] = "B", False
    tau = float(G[f"{tag}_tau"])
    lik = Normal("y", mean=LinearCombinationWithTransform(form=form, transform=transform),
                 precision="W" if np.isnan(tau) else ScaledMatrix("W", "tau"))
    mdl = Model([lik, Normal("s", mean="m0", precision="P0")])
    state = {"A": sparse.csc_matrix(A) if G[f"{tag}_sparse_A"] else A, "B": G[f"{tag}_B"], "g": G[f"{tag}_g"].reshape(-1, 1),
             "y": G[f"{tag}_y"], "s": ChainArray(eng.to_device(np.tile(G[f"{tag}_x0"], (C, 1)))),
             "W": sparse.diags(G[f"{tag}_w"], format="csc"), "tau": ChainArray(eng.full((C, 1, 1), 1.0 if np.isnan(tau) else tau)),
             "m0": G[f"{tag}_m0"].reshape(d, 1), "P0": G[f"{tag}_P0"]}
    smp = ManifoldMALA("s", mdl, step=np.array(float(G[f"{tag}_step"])), fused=fused).bind(eng)
    return smp, state


@pytest.mark.parametrize("tag,fused", [("a", True), ("a", False), ("b", True), ("b", False), ("c", True), ("c", False), ("d", False),
                                       ("e", True), ("e", False)])
def test_chain_replays_the_reference(golden, tag, fused):
    """The reference's chain with its z and u injected, three chains in lock-step: accept flags equal at every step; states,
    proposals and the two proposal log-densities within max(1e-9, 100 sens[t]) (relative to max(1, |ref|) for the vectors)."""
    G = golden("transform_mala")
    C = 3
    eng = make_engine(C)
    smp, state = _mala_setup(G, tag, eng, C, fused)
    took = []
    if fused:
        assert smp.route(state) == "transform"
        inner = smp._transform_step
        smp._transform_step = lambda *a, **k: (took.append(1), inner(*a, **k))[1]
    else:
        assert smp._transform_plan(state) is None
    smp.inject = lambda s, it: eng.to_device(np.tile(G[f"{tag}_z"][it], (C, 1)))
    smp.inject_uniform = lambda s, it: eng.full((C,), float(G[f"{tag}_u"][it]))
    smp.trace = {}
    n_steps = G[f"{tag}_x"].shape[0]
    worst = {"x": 0.0, "prop": 0.0, "lq": 0.0}
    for it in range(n_steps):
        before = smp.accept_rate.accept.clone()
        state = smp.sample(state)
        eng.check_status()
        tr = smp.trace["steps"][-1]
        bound = max(1e-9, 100.0 * float(G[f"{tag}_sens"][it]))
        assert (smp.accept_rate.accept - before).cpu().numpy().tolist() == [int(G[f"{tag}_accept"][it])] * C, (tag, it)
        for name, got, ref in (("x", state["s"].numpy()[:, :, 0], G[f"{tag}_x"][it]), ("prop", tr["prop"].cpu().numpy(), G[f"{tag}_prop"][it])):
            err = float(np.max(np.abs(got - ref[None, :]) / np.maximum(1.0, np.abs(ref))[None, :]))
            worst[name] = max(worst[name], err)
            assert err <= bound, (tag, fused, it, name, err, bound)
        for name in ("lq_fwd", "lq_rev"):
            err = float(np.max(np.abs(tr[name].cpu().numpy() - float(G[f"{tag}_{name}"][it]))))
            worst["lq"] = max(worst["lq"], err)
            assert err <= bound, (tag, fused, it, name, err, bound)
    assert smp.accept_rate.count["proposal"] == C * n_steps
    assert len(took) == (n_steps if fused else 0)
    print(f"chain {tag} {'fused' if fused else 'general'}: max deviation state {worst['x']:.2e}, proposal {worst['prop']:.2e}, "
          f"log q {worst['lq']:.2e}")
    eng.close()


def test_chain_d_is_beyond_the_fused_route(golden):
    G = golden("transform_mala")
    eng = make_engine(3)
    smp, state = _mala_setup(G, "d", eng, 3, True)
    assert state["s"].shape[0] == 80 and smp._transform_plan(state) is None
    eng.close()


# ----------------------------------------------------------------------------- the fused kernel on its own
def _numpy_step(Gm, cv, P, m0, tau, lam, step, x, z, u):
    """One update of omc_mala_transform_step for one chain, in numpy."""
    def point(v):
        t, d = np.exp(v), v - m0
        g = tau * t * (cv - Gm @ t) - lam * (P @ d)
        L = np.linalg.cholesky((tau * np.outer(t, t) * Gm + lam * P) / step**2)
        mu = v + 0.5 * np.linalg.solve(L.T, np.linalg.solve(L, g))
        return mu, L, tau * (t @ cv - 0.5 * t @ Gm @ t) - 0.5 * lam * d @ P @ d

    def lq(L, r):
        w = L.T @ r
        return np.sum(np.log(np.diag(L))) - 0.5 * w @ w

    mu, L, tg = point(x)
    xp = mu + np.linalg.solve(L.T, z)
    mu_p, L_p, tg_p = point(xp)
    lf, lr = lq(L, xp - mu), lq(L_p, x - mu_p)
    la = tg_p - tg + lr - lf
    return xp, lf, lr, la, np.log(u) < la


def _random_target(rng, p, n=None):
    n = n or max(4 * p, 20)
    A = (rng.random((n, p)) + 0.1) * (rng.random((n, p)) < max(0.15, 2.0 / p))
    A[np.arange(n), np.arange(n) % p] += 0.5
    truth = 0.3 * rng.standard_normal(p)
    w = 40.0 * (rng.random(n) + 0.5)
    y = A @ np.exp(truth) + rng.standard_normal(n) / np.sqrt(w)
    R = rng.standard_normal((p, 2 * p))
    P = R @ R.T / (2 * p) + 0.5 * np.eye(p)
    return dict(A=A, w=w, y=y, truth=truth, P=0.5 * (P + P.T), m0=np.full(p, 0.1))


@pytest.mark.parametrize("p", [1, 7, 33, 64])
def test_fused_step_against_numpy(p):
    """Every argument of the kernel: per-chain tau and lam, a prior mean, injected draws, all optional outputs; C odd, so the
    last workgroup is partly empty."""
    import torch

    rng = np.random.default_rng(70 + p)
    C, step = 7, 0.6
    T = _random_target(rng, p)
    A, w = T["A"], T["w"]
    Gm, cv = A.T @ (w[:, None] * A), A.T @ (w * T["y"])
    tau, lam = rng.random(C) + 0.5, rng.random(C) + 0.5
    x0 = T["truth"][None, :] + 0.03 * rng.standard_normal((C, p))
    z, u = rng.standard_normal((C, p)), rng.random(C)
    eng = make_engine(C)
    x = eng.to_device(x0)
    acc = torch.zeros(C, dtype=torch.int64, device=eng.device)
    prp = torch.full((C,), 5, dtype=torch.int64, device=eng.device)
    prop, lf, lr, lp = eng.empty(C, p), eng.empty(C), eng.empty(C), eng.empty(C)
    eng.mala_transform_step(eng.to_device(Gm), eng.to_device(cv), eng.to_device(T["P"]), step, x, m0=eng.to_device(T["m0"]),
                            tau=eng.to_device(tau), lam=eng.to_device(lam), z=eng.to_device(z), u=eng.to_device(u),
                            accept_count=acc, proposal_count=prp, prop_out=prop, lq_fwd_out=lf, lq_rev_out=lr, log_p_out=lp)
    eng.check_status()
    assert prp.cpu().tolist() == [6] * C
    for c in range(C):
        xp, rf, rr, la, ok = _numpy_step(Gm, cv, T["P"], T["m0"], tau[c], lam[c], step, x0[c], z[c], u[c])
        assert np.max(np.abs(prop[c].cpu().numpy() - xp) / np.maximum(1.0, np.abs(xp))) <= 1e-9
        assert abs(float(lf[c]) - rf) <= 1e-9 * max(1.0, abs(rf)) and abs(float(lr[c]) - rr) <= 1e-9 * max(1.0, abs(rr))
        if abs(np.log(u[c]) - la) > 1e-6:  # (a decision this close to the line may go either way in other arithmetic)
            assert int(acc[c]) == int(ok), (c, la, u[c])
        want = xp if int(acc[c]) else x0[c]
        assert np.max(np.abs(x[c].cpu().numpy() - want) / np.maximum(1.0, np.abs(want))) <= 1e-9
    eng.close()


# ----------------------------------------------------------------------------- the two routes from one seed
def _routes_setup(p, C, fused, seed):
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombinationWithTransform, ScaledMatrix
    from openmcmc_amd.sampler.metropolis_hastings import ManifoldMALA

    rng = np.random.default_rng(900 + p)
    T = _random_target(rng, p)
    n = T["A"].shape[0]
    eng = make_engine(C, seed=seed)
    lik = Normal("y", mean=LinearCombinationWithTransform(form={"s": "A"}, transform={"s": True}), precision=ScaledMatrix("W", "tau"))
    mdl = Model([lik, Normal("s", mean="m0", precision="P0")])
    x0 = T["truth"][None, :] + 0.03 * rng.standard_normal((C, p))
    state = {"A": T["A"], "y": T["y"].reshape(n, 1), "s": ChainArray(eng.to_device(x0)), "W": sparse.diags(T["w"], format="csc"),
             "tau": ChainArray(eng.to_device(0.8 + 0.4 * rng.random(C)).reshape(C, 1, 1)), "m0": T["m0"].reshape(p, 1), "P0": T["P"]}
    smp = ManifoldMALA("s", mdl, step=np.array(0.5), fused=fused).bind(eng)
    return eng, smp, state


@pytest.mark.parametrize("p", [1, 5, 33, 64])
def test_fused_and_general_route_agree_from_one_seed(p):
    """No injected draws: both routes read the same Philox streams, so they make the same decisions in every chain."""
    C, steps = 257, 30
    res = {}
    for fused in (True, False):
        eng, smp, state = _routes_setup(p, C, fused, seed=11)
        assert (smp._transform_plan(state) is not None) == fused
        for _ in range(steps):
            state = smp.sample(state)
        eng.check_status()
        res[fused] = (state["s"].numpy()[:, :, 0].copy(), smp.accept_rate.accept.cpu().numpy().copy(),
                      smp.accept_rate.proposal.cpu().numpy().copy())
        eng.close()
    assert np.array_equal(res[True][1], res[False][1]) and np.array_equal(res[True][2], res[False][2])
    assert 0 < res[True][1].sum() < C * steps
    ref = res[False][0]
    err = float(np.max(np.abs(res[True][0] - ref) / np.maximum(1.0, np.abs(ref))))
    print(f"fused vs general, p={p}: max relative deviation after {steps} steps {err:.2e}, accepted {int(res[True][1].sum())} of {C * steps}")
    assert err <= 1e-9


def test_fused_route_is_reproducible():
    out = []
    for _ in range(2):
        eng, smp, state = _routes_setup(33, 70, True, seed=3)
        for _ in range(10):
            state = smp.sample(state)
        eng.check_status()
        out.append((state["s"].numpy().copy(), smp.accept_rate.accept.cpu().numpy().copy()))
        eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_non_spd_prior_latches_the_chain():
    """A prior precision that is not positive definite: the factorisation fails in every chain, the lowest one is reported
    through check_status as on the other routes, and the state is left as it was."""
    eng, smp, state = _routes_setup(5, 6, True, seed=1)
    state["P0"] = -50000.0 * np.eye(5)
    before = state["s"].numpy().copy()
    state = smp.sample(state)
    with pytest.raises(np.linalg.LinAlgError, match="chain 0"):
        eng.check_status()
    assert np.array_equal(state["s"].numpy(), before)
    eng.close()


def test_unsupported_forms_raise():
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombinationWithTransform
    from openmcmc_amd.sampler.sampler import NormalNormal

    eng = make_engine(2)
    mean = LinearCombinationWithTransform(form={"s": "A"}, transform={"s": True})
    state = {"A": np.eye(3), "s": ChainArray(eng.zeros(2, 3, 1)), "y": np.ones((3, 1)), "W": np.eye(3), "m0": np.zeros((3, 1)), "P0": np.eye(3)}
    mdl = Model([Normal("y", mean=mean, precision="W"), Normal("s", mean="m0", precision="P0")])
    with pytest.raises(NotImplementedError):   # the conditional of a transformed term is not Gaussian
        NormalNormal("s", mdl).bind(eng).sample(state)
    with pytest.raises(NotImplementedError):   # the dense route needs a constant Hessian
        mdl["y"].grad_terms(state, "s", eng)
    per_chain_design = dict(state, A=ChainArray(eng.zeros(2, 3, 3)))
    with pytest.raises(NotImplementedError):
        mean.predictor_device(per_chain_design, eng)
    eng.close()


# ----------------------------------------------------------------------------- through MCMC, and next to other samplers
def test_run_mcmc_replays_the_reference(golden):
    """[ManifoldMALA(s), NormalGamma(tau)] through MCMC.run_mcmc with a fitted-value store, on both routes: tau changes between
    the mMALA steps, the draw index runs over two samplers, log_post comes from the model (no fused log density).  40 iterations
    of the reference (tests/golden/transform_mcmc.npz) with its z, u and gamma draws injected: stores within 1e-9."""
    from openmcmc_amd.distribution.distribution import Gamma
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.mcmc import MCMC
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombinationWithTransform, ScaledMatrix
    from openmcmc_amd.sampler.metropolis_hastings import ManifoldMALA
    from openmcmc_amd.sampler.sampler import NormalGamma

    G = golden("transform_mcmc")
    d, C, n_iter = G["s0"].size, 3, int(G["n_iter"])
    for fused in (True, False):
        mdl = Model([Normal("y", mean=LinearCombinationWithTransform(form={"s": "A"}, transform={"s": True}),
                            precision=ScaledMatrix("W", "tau")),
                     Normal("s", mean="m0", precision="P0"), Gamma("tau", shape="a_tau", rate="b_tau")], response={"y": "mean"})
        state = {"A": G["A"], "y": G["y"], "s": G["s0"].reshape(d, 1), "W": sparse.diags(G["w"], format="csc"), "tau": float(G["tau0"]),
                 "m0": G["m0"].reshape(d, 1), "P0": G["P0"], "a_tau": float(G["a_tau"]), "b_tau": float(G["b_tau"])}
        samplers = [ManifoldMALA("s", mdl, step=np.array(float(G["step"])), fused=fused), NormalGamma("tau", mdl)]
        M = MCMC(state, samplers, model=mdl, n_burn=0, n_iter=n_iter, n_chains=C)
        eng = M.engine
        assert (samplers[0]._transform_plan(M.state) is not None) == fused
        samplers[0].inject = lambda smp, t: eng.to_device(np.tile(G["z"][t], (C, 1)))
        samplers[0].inject_uniform = lambda smp, t: eng.full((C,), float(G["u"][t]))
        samplers[1].inject = lambda smp, t: eng.full((C,), float(G["g"][t]))
        M.run_mcmc()
        eng.check_status()
        out = M.collect()
        worst = {}
        for key in ("s", "tau", "log_post", "y"):
            ref = G["store_" + key]
            for c in range(C):
                got = np.asarray(out[key][c])
                assert got.shape == ref.shape, (key, got.shape, ref.shape)
                worst[key] = max(worst.get(key, 0.0), float(np.max(np.abs(got - ref)) / np.max(np.abs(ref))))
        print(f"run_mcmc {'fused' if fused else 'general'}:", {k: f"{v:.1e}" for k, v in worst.items()})
        assert max(worst.values()) <= 1e-9, worst
        assert samplers[0].accept_rate.count == {"accept": C * int(G["n_accept"]), "proposal": C * n_iter}
        eng.close()


def test_normal_normal_next_to_a_transformed_term(golden):
    """NormalNormal on the untransformed term g of chain (b)'s model: the transformed term A exp(s_c) is a per-chain offset of the
    response (predictor_device with exclude=, alpha=-1).  Three chains at three values of s against three draws of the
    reference with one injected z."""
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombinationWithTransform
    from openmcmc_amd.sampler.sampler import NormalNormal

    G = golden("transform_mala")
    C, d = 3, G["b_A"].shape[1]
    eng = make_engine(C)
    mean = LinearCombinationWithTransform(form={"s": "A", "g": "B"}, transform={"s": True, "g": False})
    mdl = Model([Normal("y", mean=mean, precision="W"), Normal("s", mean="m0", precision="P0"), Normal("g", mean="mg", precision="Pg")])
    state = {"A": G["b_A"], "B": G["b_B"], "g": ChainArray(eng.zeros(C, 2, 1)), "y": G["b_y"], "s": ChainArray(eng.to_device(G["nn_S"])),
             "W": sparse.diags(G["b_w"], format="csc"), "m0": G["b_m0"].reshape(d, 1), "P0": G["b_P0"], "mg": G["nn_mg"].reshape(2, 1),
             "Pg": G["nn_Pg"]}
    nn = NormalNormal("g", mdl).bind(eng)
    nn.inject = lambda smp, t: eng.to_device(np.tile(G["nn_z"], (C, 1)))
    state = nn.sample(state)
    eng.check_status()
    got = state["g"].numpy()[:, :, 0]
    err = _rel(got, G["nn_g"])
    print(f"NormalNormal next to a transformed term: {err:.1e}")
    assert err <= 1e-10
    assert np.max(np.abs(G["nn_g"][0] - G["nn_g"][1])) > 1e-3  # (the offset does differ between the chains)
    # the scaled per-chain offset on its own, and with a per-chain scale: alpha c_s (A exp(s)) for the terms but g
    cs = np.array([0.5, 1.5, 2.5])
    off = mean.predictor_device(state, eng, exclude="g", alpha=-1.0, chain_scale=eng.to_device(cs)).cpu().numpy()
    assert _rel(off, -cs[:, None] * (np.exp(G["nn_S"]) @ G["b_A"].T)) <= 1e-13
    full = mean.predictor_device(state, eng, alpha=-1.0, chain_scale=eng.to_device(cs)).cpu().numpy()   # both kinds of per-chain term
    assert _rel(full, -cs[:, None] * (np.exp(G["nn_S"]) @ G["b_A"].T + got @ G["b_B"].T)) <= 1e-13
    eng.close()


def test_fused_sweep_steps_aside_for_a_transformed_offset():
    """x ~ GMRF next to A exp(s_c) in the mean of y: [NormalNormal(x), NormalGamma, NormalGamma] would be one fused launch,
    which knows nothing of per-chain offsets.  The plan is not made; the sampler-by-sampler draw sees y - A exp(s_c)."""
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.distribution import Gamma
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.mcmc import MCMC
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombination, LinearCombinationWithTransform, ScaledMatrix
    from openmcmc_amd.sampler.sampler import NormalGamma, NormalNormal

    rng = np.random.default_rng(8)
    n, p, C = 30, 4, 3
    A, S, y = rng.random((n, p)), 0.3 * rng.standard_normal((C, p)), rng.standard_normal((n, 1)) + 3.0
    Prw = sparse.diags([-np.ones(n - 1), np.r_[1.001, 2 * np.ones(n - 2), 1.0], -np.ones(n - 1)], [-1, 0, 1], format="csc")
    eng = make_engine(C)

    def build(mean, state_extra):
        mdl = Model([Normal("y", mean=mean, precision=ScaledMatrix("W", "tau")), Normal("x", mean="mx", precision=ScaledMatrix("Prw", "lam")),
                     Gamma("tau", shape="a", rate="b"), Gamma("lam", shape="a", rate="b")])
        state = dict({"I": sparse.identity(n, format="csc"), "y": y, "x": np.zeros((n, 1)), "W": sparse.identity(n, format="csc"), "tau": 2.0,
                      "Prw": Prw, "lam": 5.0, "mx": np.zeros((n, 1)), "a": 1.0, "b": 1.0}, **state_extra)
        samplers = [NormalNormal("x", mdl), NormalGamma("tau", mdl), NormalGamma("lam", mdl)]
        return MCMC(state, samplers, model=mdl, n_burn=0, n_iter=2, n_chains=C, engine=eng), samplers

    M0, _ = build(LinearCombination({"x": "I"}), {})
    assert M0._fused is not None    # the same model without the transformed term is fused
    mean = LinearCombinationWithTransform(form={"x": "I", "s": "A"}, transform={"x": False, "s": True})
    M, samplers = build(mean, {"A": A, "s": ChainArray(eng.to_device(S))})
    assert M._fused is None
    z = rng.standard_normal(n)
    samplers[0].inject = lambda smp, t: eng.to_device(np.tile(z, (C, 1)))
    state = samplers[0].sample(M.state)
    eng.check_status()
    got = state["x"].numpy()[:, :, 0]
    Q = (5.0 * Prw + 2.0 * sparse.identity(n)).toarray()
    L = np.linalg.cholesky(Q)
    for c in range(C):
        b = 2.0 * (y.ravel() - A @ np.exp(S[c]))
        ref = np.linalg.solve(Q, b) + np.linalg.solve(L.T, z)
        assert np.max(np.abs(got[c] - ref)) <= 1e-10 * np.max(np.abs(ref)), c
    eng.close()
