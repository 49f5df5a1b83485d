"""Golden vectors for LinearCombinationWithTransform (reference parameter.py:231-297) and ManifoldMALA on a parameter
under it (metropolis_hastings.py:301-373 with the state-dependent Hessian of location_scale.py:234-242), made by RUNNING
the reference (openMCMC v1.0.7) in the build container:

    PYTHONPATH=/root/reference/src python3 tests/golden/make_golden_r6.py

Writes transform_parameter.npz, transform_mala.npz and transform_mcmc.npz (pass names to regenerate a subset).  Fixtures hold data only: inputs,
the draws the reference consumed (stats.norm.rvs / stats.uniform.rvs patched, as in make_golden_rj.py) and what it produced.

Every chain of transform_mala.npz must accept between 20 % and 90 % of its steps, so that a replay takes both branches of the
decision; the generator asserts it.  Each chain is also run a second time with A and y multiplied element-wise by
1 + 1e-16 eps (eps standard normal; the factor rounds to 1 or 1 +- 2.2e-16) under the same draws: sens[t] is the largest
deviation of the state at step t relative to max(1, |x|) -- the reference's own amplification of last-bit noise, which a
replay on other arithmetic cannot be held below.
"""

import os
import sys

import numpy as np
from scipy import sparse, stats

REF_SRC = "/root/reference/src"
if REF_SRC not in sys.path:
    sys.path.insert(0, REF_SRC)

from openmcmc import parameter  # noqa: E402
from openmcmc.distribution.distribution import Gamma  # noqa: E402
from openmcmc.distribution.location_scale import Normal  # noqa: E402
from openmcmc.mcmc import MCMC  # noqa: E402
from openmcmc.model import Model  # noqa: E402
from openmcmc.sampler.metropolis_hastings import ManifoldMALA  # noqa: E402
from openmcmc.sampler.sampler import NormalGamma, NormalNormal  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def _dense(M):
    return M.toarray() if sparse.issparse(M) else np.asarray(M, dtype=float)


# ----------------------------------------------------------------------------- the parameter and the Normal around it
def gen_transform_parameter():
    rng = np.random.default_rng(61)
    n, p, q = 25, 6, 3
    cases = {"all": dict(tr_s=True, second=False), "none": dict(tr_s=False, second=True), "mixed": dict(tr_s=True, second=True),
             "sparseA": dict(tr_s=True, second=False, sparse_A=True), "nrep3": dict(tr_s=True, second=True, n_rep=3),
             "scaled": dict(tr_s=True, second=False, tau=1.7)}
    out = {"cases": np.array(sorted(cases))}
    for tag, cfg in cases.items():
        A = rng.random((n, p)) * (rng.random((n, p)) < 0.4 if cfg.get("sparse_A") else 1.0)
        B = rng.standard_normal((n, q))
        S = 0.4 * rng.standard_normal((3, p))
        g = rng.standard_normal((q, 1))
        w = rng.random(n) + 0.5
        n_rep, tau = cfg.get("n_rep", 1), cfg.get("tau")
        y = A @ np.exp(S[0]).reshape(p, 1) + (B @ g if cfg["second"] else 0.0) + 0.3 * rng.standard_normal((n, n_rep))
        form, transform = {"s": "A"}, {"s": cfg["tr_s"]}
        if cfg["second"]:
            form["g"], transform["g"] = "B", False
        mean = parameter.LinearCombinationWithTransform(form=form, transform=transform)
        prec = parameter.ScaledMatrix("W", "tau") if tau is not None else parameter.Identity("W")
        dist = Normal("y", mean=mean, precision=prec)
        out.update({f"{tag}_A": A, f"{tag}_B": B, f"{tag}_S": S, f"{tag}_g": g.ravel(), f"{tag}_w": w, f"{tag}_y": y,
                    f"{tag}_tr_s": float(cfg["tr_s"]), f"{tag}_second": float(cfg["second"]),
                    f"{tag}_sparse_A": float(bool(cfg.get("sparse_A"))), f"{tag}_tau": np.nan if tau is None else tau})
        res = {k: [] for k in ("pred", "pred_cond", "grad", "logp", "logp_obs", "glp_grad", "glp_hess")}
        for k in range(3):
            st = {"A": sparse.csc_matrix(A) if cfg.get("sparse_A") else A, "B": B, "s": S[k].reshape(p, 1).copy(), "g": g, "y": y,
                  "W": sparse.diags(w, format="csc"), "tau": np.array([[tau if tau is not None else 1.0]])}
            res["pred"].append(np.asarray(mean.predictor(st)).ravel())
            res["pred_cond"].append(np.asarray(mean.predictor_conditional(st, term_to_exclude="s")).ravel() * np.ones(n))
            res["grad"].append(_dense(mean.grad(st, "s")))
            res["logp"].append(float(np.sum(dist.log_p(st))))
            res["logp_obs"].append(np.asarray(dist.log_p(st, by_observation=True), dtype=float).ravel())
            gr, he = dist.grad_log_p(st, "s", hessian_required=True)
            res["glp_grad"].append(np.asarray(gr).ravel())
            res["glp_hess"].append(_dense(he))
        for k, v in res.items():
            out[f"{tag}_{k}"] = np.array(v)
    np.savez_compressed(os.path.join(OUT, "transform_parameter.npz"), **out)


# ----------------------------------------------------------------------------- mMALA chains
def _mala_model(rng, d, n, sparse_A=False, second=False, n_rep=1, tau=None, wscale=40.0):
    A = rng.random((n, d)) + 0.1
    if sparse_A:
        A = A * (rng.random((n, d)) < 0.15)
        A[np.arange(n), np.arange(n) % d] += 0.5   # every column observed
    truth = 0.3 * rng.standard_normal(d)
    B = rng.standard_normal((n, 2))
    g = np.array([[0.7], [-0.4]])
    w = wscale * (rng.random(n) + 0.5)   # informative data: the posterior of s is narrow, hence close to Gaussian
    noise = rng.standard_normal((n, n_rep)) / np.sqrt(w).reshape(n, 1)
    y = A @ np.exp(truth).reshape(d, 1) + (B @ g if second else 0.0) + noise
    R = rng.standard_normal((d, 2 * d))
    P0 = R @ R.T / (2 * d) + 0.5 * np.eye(d)
    P0 = 0.5 * (P0 + P0.T)
    return dict(A=A, truth=truth, B=B, g=g, w=w, y=y, P0=P0, m0=np.full(d, 0.1), second=second, sparse_A=sparse_A, tau=tau)


def _run_chain(m, x0, step, n_steps, zs=None, us=None, perturb=None):
    """One reference chain.  zs / us None: fresh draws are recorded; given: replayed.  perturb: (fA, fy) factors."""
    d = x0.size
    A, y = m["A"], m["y"]
    if perturb is not None:
        A, y = A * perturb[0], y * perturb[1]
    form, transform = {"s": "A"}, {"s": True}
    if m["second"]:
        form["g"], transform["g"] = "B", False
    mean = parameter.LinearCombinationWithTransform(form=form, transform=transform)
    prec = parameter.ScaledMatrix("W", "tau") if m["tau"] is not None else parameter.Identity("W")
    mdl = Model([Normal("y", mean=mean, precision=prec), Normal("s", mean="m0", precision="P0")])
    st = {"A": sparse.csc_matrix(A) if m["sparse_A"] else A, "B": m["B"], "g": m["g"], "y": y, "s": x0.reshape(d, 1).copy(),
          "W": sparse.diags(m["w"], format="csc"), "tau": np.array([[m["tau"] if m["tau"] is not None else 1.0]]),
          "m0": m["m0"].reshape(d, 1), "P0": m["P0"]}
    smp = ManifoldMALA("s", mdl, step=np.array(step))
    rd = np.random.default_rng(600 + d)
    rec = dict(z=[], u=[], x=[], prop=[], lq_fwd=[], lq_rev=[], accept=[])
    it = {"z": 0, "u": 0}

    def _norm(loc=0, scale=1, size=None, **_):
        if zs is None:
            z = np.asarray(rd.standard_normal(size), dtype=float)
        else:
            z = np.asarray(zs[it["z"]], dtype=float).reshape(size)
        it["z"] += 1
        rec["z"].append(z.reshape(-1).copy())
        return loc + z * scale

    def _uniform(loc=0, scale=1, size=None, **_):
        u = float(rd.random(size)) if us is None else float(us[it["u"]])
        it["u"] += 1
        rec["u"].append(u)
        return loc + u * scale

    inner = smp.proposal

    def _proposal(current_state, param_index=None):
        prop_state, lf, lr = inner(current_state, param_index)
        rec["prop"].append(prop_state["s"].ravel().copy())
        rec["lq_fwd"].append(float(np.asarray(lf).item()))
        rec["lq_rev"].append(float(np.asarray(lr).item()))
        return prop_state, lf, lr

    smp.proposal = _proposal
    saved = (stats.norm.rvs, stats.uniform.rvs)
    stats.norm.rvs, stats.uniform.rvs = _norm, _uniform
    try:
        for _ in range(n_steps):
            before = smp.accept_rate.count["accept"]
            st = smp.sample(st)
            rec["x"].append(st["s"].ravel().copy())
            rec["accept"].append(float(smp.accept_rate.count["accept"] - before))
    finally:
        stats.norm.rvs, stats.uniform.rvs = saved
    return {k: np.array(v) for k, v in rec.items()}


def gen_transform_mala():
    rng = np.random.default_rng(62)
    chains = {
        "a": dict(d=5, n=40, step=0.7, n_steps=60, start="zero"),
        "b": dict(d=5, n=40, step=0.7, n_steps=60, start="zero", second=True, like="a"),
        "c": dict(d=32, n=200, step=0.5, n_steps=60, start="near", sparse_A=True),
        "d": dict(d=80, n=400, step=0.5, n_steps=40, start="near", sparse_A=True),
        "e": dict(d=5, n=40, step=1.1, n_steps=60, start="zero", n_rep=3, tau=1.3),   # (step 0.7 accepts > 90 % here)
    }
    out = {"chains": np.array(sorted(chains))}
    models = {}
    for tag, cfg in chains.items():
        d = cfg["d"]
        if cfg.get("like"):
            m = dict(models[cfg["like"]])
            m["second"] = True
            m["y"] = m["y"] + m["B"] @ m["g"]
        else:
            m = _mala_model(rng, d, cfg["n"], sparse_A=cfg.get("sparse_A", False), n_rep=cfg.get("n_rep", 1), tau=cfg.get("tau"),
                            wscale=cfg.get("wscale", 40.0))
        models[tag] = m
        x0 = np.zeros(d) if cfg["start"] == "zero" else m["truth"] + 0.05 * (2.0 * rng.random(d) - 1.0)
        ref = _run_chain(m, x0, cfg["step"], cfg["n_steps"])
        rate = ref["accept"].mean()
        print(f"chain {tag}: d = {d}, step {cfg['step']}: accepted {int(ref['accept'].sum())} of {cfg['n_steps']}")
        assert 0.2 <= rate <= 0.9, (tag, rate)
        eps = np.random.default_rng(63)
        fA = 1.0 + 1e-16 * eps.standard_normal(m["A"].shape)
        fy = 1.0 + 1e-16 * eps.standard_normal(m["y"].shape)
        per = _run_chain(m, x0, cfg["step"], cfg["n_steps"], zs=ref["z"], us=ref["u"], perturb=(fA, fy))
        sens = np.max(np.abs(per["x"] - ref["x"]) / np.maximum(1.0, np.abs(ref["x"])), axis=1)
        print(f"          sens: max {sens.max():.3e}, decisions equal: {bool(np.array_equal(per['accept'], ref['accept']))}")
        out.update({f"{tag}_A": m["A"], f"{tag}_B": m["B"], f"{tag}_g": m["g"].ravel(), f"{tag}_w": m["w"], f"{tag}_y": m["y"],
                    f"{tag}_P0": m["P0"], f"{tag}_m0": m["m0"], f"{tag}_second": float(m["second"]),
                    f"{tag}_sparse_A": float(m["sparse_A"]), f"{tag}_tau": np.nan if m["tau"] is None else m["tau"],
                    f"{tag}_x0": x0, f"{tag}_step": cfg["step"], f"{tag}_sens": sens})
        for k, v in ref.items():
            out[f"{tag}_{k}"] = v
    out.update(_normal_normal_next_to_transform(models["b"], out["b_x"][[5, 20, 50]]))
    np.savez_compressed(os.path.join(OUT, "transform_mala.npz"), **out)


def _normal_normal_next_to_transform(m, S):
    """NormalNormal (sampler.py:154-207) on the untransformed term g of chain (b)'s model, g ~ N(mg, Pg), at three values of the
    transformed term s (rows of S), one recorded z for all three."""
    mean = parameter.LinearCombinationWithTransform(form={"s": "A", "g": "B"}, transform={"s": True, "g": False})
    mdl = Model([Normal("y", mean=mean, precision=parameter.Identity("W")), Normal("s", mean="m0", precision="P0"),
                 Normal("g", mean="mg", precision="Pg")])
    d = m["A"].shape[1]
    mg, Pg = np.array([[0.2], [-0.1]]), np.array([[2.0, 0.3], [0.3, 1.5]])
    z = np.random.default_rng(64).standard_normal(2)
    draws = []
    saved = stats.norm.rvs
    stats.norm.rvs = lambda loc=0, scale=1, size=None, **_: loc + z.reshape(size) * scale
    try:
        for s in S:
            st = {"A": m["A"], "B": m["B"], "g": np.zeros((2, 1)), "y": m["y"], "s": s.reshape(d, 1).copy(),
                  "W": sparse.diags(m["w"], format="csc"), "m0": m["m0"].reshape(d, 1), "P0": m["P0"], "mg": mg, "Pg": Pg}
            draws.append(NormalNormal("g", mdl).sample(st)["g"].ravel().copy())
    finally:
        stats.norm.rvs = saved
    return {"nn_S": np.array(S), "nn_z": z, "nn_mg": mg.ravel(), "nn_Pg": Pg, "nn_g": np.array(draws)}


# ----------------------------------------------------------------------------- through MCMC
def gen_transform_mcmc():
    """y ~ N(A exp(s), tau I), s ~ N(m0, P0), tau ~ Gamma(a, b); [ManifoldMALA(s), NormalGamma(tau)] through MCMC.run_mcmc with
    response={'y': 'mean'}, 40 iterations; the stores and the tape of draws (z and u of every mMALA step, the gamma draw)."""
    rng = np.random.default_rng(65)
    d, n, n_iter, step = 5, 40, 40, 0.7
    m = _mala_model(rng, d, n)
    mean = parameter.LinearCombinationWithTransform(form={"s": "A"}, transform={"s": True})
    mdl = Model([Normal("y", mean=mean, precision=parameter.ScaledMatrix("W", "tau")), Normal("s", mean="m0", precision="P0"),
                 Gamma("tau", shape="a_tau", rate="b_tau")], response={"y": "mean"})
    s0 = m["truth"] + 0.05 * (2.0 * rng.random(d) - 1.0)
    w = m["w"] / 40.0   # the weights of _mala_model without their scale: tau carries it (truth: 40)
    st = {"A": m["A"], "y": m["y"], "s": s0.reshape(d, 1).copy(), "W": sparse.diags(w, format="csc"), "tau": 30.0,
          "m0": m["m0"].reshape(d, 1), "P0": m["P0"], "a_tau": 2.0, "b_tau": 0.05}
    samplers = [ManifoldMALA("s", mdl, step=np.array(step)), NormalGamma("tau", mdl)]
    rd = np.random.default_rng(650)
    tape = dict(z=[], u=[], g=[])

    def _norm(loc=0, scale=1, size=None, **_):
        z = np.asarray(rd.standard_normal(size), dtype=float)
        tape["z"].append(z.reshape(-1).copy())
        return loc + z * scale

    def _uniform(loc=0, scale=1, size=None, **_):
        u = float(rd.random(size))
        tape["u"].append(u)
        return loc + u * scale

    def _gamma(a, loc=0, scale=1, size=None, **_):
        g = rd.standard_gamma(np.asarray(a, dtype=float), size=size)
        tape["g"].append(float(np.asarray(g).reshape(-1)[0]))
        return loc + g * scale

    saved = (stats.norm.rvs, stats.uniform.rvs, stats.gamma.rvs)
    stats.norm.rvs, stats.uniform.rvs, stats.gamma.rvs = _norm, _uniform, _gamma
    try:
        M = MCMC(st, samplers, model=mdl, n_burn=0, n_iter=n_iter)
        M.run_mcmc()
    finally:
        stats.norm.rvs, stats.uniform.rvs, stats.gamma.rvs = saved
    acc = samplers[0].accept_rate.count
    print(f"mcmc: accepted {acc['accept']} of {acc['proposal']}")
    assert len(tape["z"]) == len(tape["u"]) == len(tape["g"]) == n_iter and acc["proposal"] == n_iter
    assert 0.2 <= acc["accept"] / acc["proposal"] <= 0.9
    out = {"A": m["A"], "y": m["y"], "w": w, "s0": s0, "tau0": 30.0, "m0": m["m0"], "P0": m["P0"], "a_tau": 2.0, "b_tau": 0.05,
           "step": step, "n_iter": n_iter, "z": np.array(tape["z"]), "u": np.array(tape["u"]), "g": np.array(tape["g"]),
           "n_accept": float(acc["accept"])}
    for key in ("s", "tau", "log_post", "y"):
        out["store_" + key] = np.asarray(M.store[key])
    np.savez_compressed(os.path.join(OUT, "transform_mcmc.npz"), **out)


GENERATORS = {"transform_parameter": gen_transform_parameter, "transform_mala": gen_transform_mala, "transform_mcmc": gen_transform_mcmc}

if __name__ == "__main__":
    which = sys.argv[1:] or list(GENERATORS)
    for name in which:
        GENERATORS[name]()
        print(name + ".npz", os.path.getsize(os.path.join(OUT, name + ".npz")))
