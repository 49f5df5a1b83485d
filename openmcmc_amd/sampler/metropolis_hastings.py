"""Metropolis-Hastings samplers on chain-batched state (reference sampler/metropolis_hastings.py).

Routes:
  * fused Gaussian: RandomWalk (untruncated) and ManifoldMALA for a parameter whose conditional model is one Normal with
    the parameter as response, a shared mean and a shared dense precision (Normal("x", mean="mu", precision="Q")
    -- BASELINE configs[3]).  The Hessian of that target is constant, so chol(H/step^2) is factorised once per sampler instead of
    five times per update and every chain advances with level-3 BLAS on the d x C state matrix: in the whitened
    coordinates a = L'(x - mu) (omc_rw_step_white, omc_mala_step_white, blocks of steps through omc_mala_run_white; one protocol
    for the library's cached a, `_fused_gaussian_step`) or, ManifoldMALA(whitened=False), on the products of omc_mala_step.
  * generic: any model whose log_p the device can evaluate.  The proposal (omc_rw_propose: Gaussian or truncated
    Gaussian random walk), the model log-density of the current and the proposed state, the accept test
    (omc_mh_accept) and the per-chain merge of the two states (omc_chain_select) are separate launches over all
    chains; `state_update_function` callbacks receive and return chain-batched state.  This is the route of
    RandomWalkLoop over the knots of a basis and of ReversibleJump (BASELINE configs[4]).
  * knot loop: RandomWalkLoop over the knots of a library basis as one launch (omc_knot_loop) when `_knot_plan` allows.
  * ManifoldMALA beyond the Gaussian target, named by `ManifoldMALA.route(state)`: "diag" (a per-chain diagonal Hessian: omc_mala_diag
    does both halves of the proposal), "transform" (a parameter under the exponential transform: the whole update in
    omc_mala_transform_step), "dense" (a constant Hessian of shared matrices with per-chain scales) and "general" (a per-chain
    (C, d, d) Hessian); the last two are one proposal skeleton (`_mmala_step`) over two precision objects.
"""

from dataclasses import dataclass, field
from functools import partial
from typing import Callable

import numpy as np

from openmcmc_amd.chains import ChainArray, is_chain
from openmcmc_amd.distribution.location_scale import Normal, NullDistribution
from openmcmc_amd.parameter import Identity
from openmcmc_amd.sampler.sampler import MCMCSampler


class AcceptRate:
    """Acceptance counters (metropolis_hastings.py:25-66), one pair per chain on the device (int64);
    `count` reports the totals over chains, as the reference's dict does for its single chain."""

    def __init__(self):
        self.accept = None
        self.proposal = None

    def attach(self, engine):
        import torch

        self.accept = torch.zeros(engine.n_chains, dtype=torch.int64, device=engine.device)
        self.proposal = torch.zeros(engine.n_chains, dtype=torch.int64, device=engine.device)

    @property
    def count(self):
        if self.accept is None:
            return {"accept": 0, "proposal": 0}
        return {"accept": int(self.accept.sum().item()), "proposal": int(self.proposal.sum().item())}

    @property
    def acceptance_rate(self) -> float:
        c = self.count
        return c["accept"] / c["proposal"] * 100

    def get_acceptance_rate(self) -> str:
        if self.count["proposal"] == 0:
            return "No proposals"
        return f"Acceptance rate {self.acceptance_rate:.0f}%"


@dataclass
class MetropolisHastings(MCMCSampler):
    """Base class (metropolis_hastings.py:69-173): `step`, `accept_rate`."""

    step: np.ndarray = field(default_factory=lambda: np.array([0.2], ndmin=2), init=True)
    accept_rate: AcceptRate = field(default_factory=lambda: AcceptRate(), init=False)

    def _init_runtime(self):
        """(every `__post_init__` of the family comes here: RandomWalk and ReversibleJump skip the base's on purpose)"""
        super()._init_runtime()
        # empty caches: what the fused routes' factor was made from and where they leave log p; the members and the value of the generic
        # route's last log-density; _transform_plan's (host objects, statistics made from them); proposal's device steps and limits
        self._plan_key = self._log_p_buf = self._lp_members = self._lp_state = self._transform_memo = None
        self._dev_consts = {}
        self.step = np.array(self.step, ndmin=2)
        self._init_hooks()

    def _init_hooks(self):
        self.inject_uniform = None  # test hook like `inject`, for the accept/reject uniforms
        self.trace = None  # test hook: a dict that receives the internals of the last proposal / decision

    def _hook(self, name, *extra):
        """The draws a test hook injects for this sweep (and column, ...), None when the hook is unset."""
        hook = getattr(self, name)
        return None if hook is None else hook(self, self._sweep, *extra)

    def bind(self, engine, position=0, n_samplers=1):
        super().bind(engine, position, n_samplers)
        self.accept_rate.attach(engine)
        self._white_tag, self._white_serial = None, 0  # a sampler object taken into another run starts without a cached state
        return self

    def _blocks_per_proposal(self, p):
        return (p + 1) // 2 + 1  # Philox blocks for p proposal draws, plus one for the accept uniform

    _accept_block = _blocks_per_proposal  # ... which a whole-vector proposal takes from the block behind those

    def _white_state_tag(self, state, x, L, mu):
        """What the library's cached whitened state a = L'(x - mu) of the fused steps belongs to: this state entry (the object,
        not only its address -- a fresh tensor can land on a recycled address with the same version), its contents as far as
        torch sees them (version counter), the factor and the mean."""
        return (id(state[self.param]), x.data_ptr(), x._version, L.data_ptr(), L._version,
                None if mu is None else (mu.data_ptr(), mu._version))

    def _white_state_is_current(self, engine, x, tag):
        """... and as far as the library's own writes go, which torch's version counter does not see (Engine.note_write)."""
        return self._white_tag == tag and not engine.written_since(x, self._white_serial)

    def _fused_gaussian_step(self, state, entry, scale, **extras):
        """One call of a fused whitened entry point of the engine (rw_step_white, mala_step_white, mala_run_white; `extras` are its own
        arguments) with L = chol(scale * Q), and the whole protocol around it.  The step is element-wise in a = L'(x - mu); the library
        keeps a for the x it wrote last and may reuse it if this is still that state entry, factor and mean (`_white_state_tag`) and
        nobody else has written x since.  Leaves the target's log density at the state just left in x in `last_log_p` (MCMC.run_mcmc)."""
        eng = self._need_engine()
        Q, mu = self._target(state)
        L, sl = self._factor_plan(eng, state, Q, scale)
        x = self._x(state)
        tag = self._white_state_tag(state, x, L, mu)
        if self._log_p_buf is None or self._log_p_buf.shape[0] != eng.n_chains:
            self._log_p_buf = eng.empty(eng.n_chains)
        entry(mu, L, sl, float(self.step.item()), x, state_is_current=self._white_state_is_current(eng, x, tag),
              accept_count=self.accept_rate.accept, proposal_count=self.accept_rate.proposal, log_p_out=self._log_p_buf, **extras)
        self._white_tag, self._white_serial = tag, eng._write_serial
        self.last_log_p = (self._log_p_buf, x)

    def _gaussian_target(self, state):
        """Does the fused route apply?  (one Normal with the parameter as response, shared mean and precision)"""
        if list(self.model.keys()) != [self.param] or np.size(self.step) != 1:
            return False
        dist = self.model[self.param]
        if not isinstance(dist, Normal) or not isinstance(dist.precision, Identity) or not isinstance(dist.mean, Identity):
            return False
        return not (is_chain(state[dist.precision.form]) or is_chain(state[dist.mean.form]))

    def _target(self, state):
        """(Q device, mu device or None) of the Gaussian target of the fused route (the caller has asked `_gaussian_target`)."""
        eng = self._need_engine()
        dist = self.model[self.param]
        Q, mu = state[dist.precision.form], state[dist.mean.form]
        # device copies are cached by the identity of the STATE ENTRY (a reshaped copy would be a new object every step:
        # one upload per step, and a new address for everything the library derives from the mean)
        return eng.shared(Q), eng.shared(mu).reshape(-1) if np.any(mu) else None

    def _factor_plan(self, eng, state, Q, scale):
        """chol(scale * Q) of the fused routes, kept from step to step (the reference refactorises every step,
        metropolis_hastings.py:345-346) but rebuilt whenever what it was made from changes: another precision array in
        the state, or another step size.  The library keeps matrices derived from the factor (drift matrix, L^-T) keyed
        by device addresses; a rebuilt factor may land on a recycled address, so that cache is dropped as well."""
        key = (float(scale), id(state[self.model[self.param].precision.form]), int(Q.data_ptr()), int(Q._version))
        if self._plan is None or self._plan_key != key:
            eng.mh_invalidate()
            self._plan = eng.dense_cholesky(Q, scale)
            self._plan_key = key
        return self._plan

    def _x(self, state):
        v = state[self.param]
        if not is_chain(v) or v.shape[1] != 1:
            raise NotImplementedError("MH samplers need a per-chain (d, 1) parameter")
        return v.vector()

    # ------------------------------------------------------------------ generic route
    def _accept_reject_proposal(self, current_state: dict, prop_state: dict, logp_pr_g_cr, logp_cr_g_pr, count=None,
                                index=0, u=None, sub=0, trace=None, lp_cur=None) -> dict:
        """metropolis_hastings.py:127-173 for every chain at once: log_alpha = lp' + q_rev - (lp + q_fwd), accept iff
        log U < log_alpha, then current_state takes the proposed value of every entry that differs, chain by chain.
        `count`/`index` gate the chains taking part (a loop over the columns of a ragged parameter).
        `lp_cur`: the model log-density of current_state if the caller already has it (the reference recomputes it
        for every proposal; inside a loop over columns it is the value selected at the previous step); it is
        updated in place to the log-density of the returned state and kept in self._lp_state."""
        eng = self._need_engine()
        # Only distributions that read an entry the proposal replaced can differ between the two states; the others
        # contribute the same number to both log-densities (the reference sums them all and subtracts,
        # metropolis_hastings.py:150-155).  Proposals and callbacks must REPLACE state entries, never mutate them.
        changed = [k for k, v in prop_state.items() if v is not current_state.get(k)]
        members = self.model.affected_by(changed)
        if lp_cur is None or self._lp_members != members:
            lp_cur = self.model.log_p(current_state, engine=eng, members=members)
        self._lp_members = members
        lp_prop = self.model.log_p(prop_state, engine=eng, members=members)
        log_alpha = eng.empty(eng.n_chains) if trace is not None else None
        acc = eng.mh_accept(lp_cur, lp_prop, _as_chain_tensor(eng, logp_pr_g_cr), _as_chain_tensor(eng, logp_cr_g_pr),
                            count=count, index=index, u=u, draw_index=self._draw_index(), sub=sub,
                            accept_count=self.accept_rate.accept, proposal_count=self.accept_rate.proposal,
                            log_alpha=log_alpha)
        if trace is not None:
            trace.update(log_alpha=log_alpha, accept=acc, lp_cur=lp_cur.clone(), lp_prop=lp_prop)
        pairs = []
        for key, value in prop_state.items():
            cur = current_state.get(key)
            if value is cur or not is_chain(value):
                continue
            if not is_chain(cur) or cur.data.shape != value.data.shape:
                raise NotImplementedError(f"proposed state entry '{key}' changes kind or padded shape")
            pairs.append((value.storage(), cur.storage()))
        pairs.append((lp_prop, lp_cur))
        eng.chain_select_many(acc, pairs)  # every changed entry and the log-density in one launch
        self._lp_state = lp_cur
        return current_state


def _as_chain_tensor(engine, value):
    """Proposal log-density contributions may be Python floats (0.0 from a callback) or (C,) tensors."""
    if value is None or hasattr(value, "data_ptr"):
        return value
    v = float(value)
    return None if v == 0.0 else engine.full((engine.n_chains,), v)


def _lin(engine, a, x, b, y):
    """a x + b y per chain by the library's own kernel (omc_chain_lincomb); x, y: (C, n) or (C,) tensors.  With a, b in
    {+-1, +-0.5} both products are exact, so this is the one-rounding sum an element-wise a*x + b*y gives."""
    if x.dim() == 1:
        return engine.chain_lincomb(a, x.reshape(-1, 1), b, y.reshape(-1, 1)).reshape(-1)
    return engine.chain_lincomb(a, x if x.stride(1) == 1 else x.contiguous(), b, y if y.stride(1) == 1 else y.contiguous())


def _add_contribution(engine, total, extra):
    """total (a (C,) tensor) += extra (float or (C,) tensor)."""
    if hasattr(extra, "data_ptr"):
        total += extra
    elif float(extra) != 0.0:
        total += float(extra)
    return total


class _SharedPrecision:
    """Lambda_c = (sum_k s_kc M_k + diag(d_c)) / step^2 for ManifoldMALA._mmala_step, from the shared matrices, per-chain scales and
    per-chain diagonal of Model.grad_terms.  Constant in the parameter: one object serves both points of a step."""

    def __init__(self, eng, terms, diag, s2, shape, draw_index):
        Cn, p = shape
        self.eng, self.shape, self.draw_index, self.logdet = eng, shape, draw_index, None
        self.terms = [{"mat": None if t["mat"] is None else eng.shared(t["mat"]),
                       "scale": eng.full((Cn,), 1.0 / s2) if t["scale"] is None else t["scale"] / s2} for t in terms]
        if not self.terms:
            self.terms.append({"mat": None, "scale": eng.zeros(Cn)})
        self.diag = None if diag is None else diag / s2
        self.T = eng.dense_terms(self.terms, p)

    def times(self, v):  # Lambda_c v_c for every chain
        out = None if self.diag is None else self.diag * v
        for t in self.terms:
            part = (v if t["mat"] is None else self.eng.design_predict(t["mat"], v.contiguous())) * t["scale"].unsqueeze(1)
            out = part if out is None else out + part
        return out

    def quad(self, d):  # d_c' Lambda_c d_c
        out = None if self.diag is None else (self.diag * d * d).sum(dim=1)
        for t in self.terms:
            q = (d * d).sum(dim=1) if t["mat"] is None else self.eng.dense_quadform(t["mat"], d.contiguous())
            out = q * t["scale"] if out is None else out + q * t["scale"]
        return out

    def draw(self, b, z):
        """(m + L^-T z, m = Lambda^-1 b) in one launch; the first draw takes the stream's index and leaves log det Lambda"""
        eng, first = self.eng, self.logdet is None
        out, mean, self.logdet = eng.empty(*self.shape), eng.empty(*self.shape), eng.empty(self.shape[0]) if first else self.logdet
        eng.dense_sample_canonical(self.shape[1], self.T, out, z=z, rhs_chain=b, draw_index=self.draw_index if first else 0,
                                   mean_out=mean, logdet_out=self.logdet if first else None, diag_chain=self.diag)
        return out, mean


class _ChainPrecision:
    """Lambda_c as a (C, d, d) tensor for ManifoldMALA._mmala_step.  Up to one wave's 64 columns the library's small-matrix kernels
    (one wave per chain); beyond, the same operations as batched dense factorisations (Engine.chain_spd_ops / chain_sample_canonical):
    the reference has no size limit here (metropolis_hastings.py:325-348).  `logdet` comes with the product of `times` (one launch)."""

    def __init__(self, eng, Lam, zero, draw_index):
        self.eng, self.Lam, self.logdet = eng, Lam, None
        if Lam.shape[1] <= 64:
            self.ops, self.sample = eng.small_spd_ops, partial(eng.small_sample_canonical, prior_prec=zero, draw_index=draw_index)
        else:
            self.ops, self.sample = eng.chain_spd_ops, partial(eng.chain_sample_canonical, draw_index=draw_index)

    def times(self, v):
        Av, _, self.logdet = self.ops(self.Lam, v, want_Av=True, want_logdet=True)
        return Av

    def quad(self, d):
        return self.ops(self.Lam, d, want_quad=True)[1]

    def draw(self, b, z):
        """(m + L^-T z, m = Lambda^-1 b) in one launch"""
        mean = self.eng.empty(*b.shape)
        return self.sample(self.Lam, b, z=z, mean_out=mean), mean


@dataclass
class RandomWalk(MetropolisHastings):
    """(Truncated) Gaussian random-walk proposal (metropolis_hastings.py:176-269).

    `state_update_function(prop_state, param_index) -> (prop_state, logq_fwd_extra, logq_rev_extra)` is called with
    chain-batched state (ChainArray entries) and may return floats or (C,) tensors for the two extras."""

    domain_limits: np.ndarray = None
    state_update_function: Callable = None

    def __post_init__(self):
        # metropolis_hastings.py:201-210: keep the FULL model when a state_update_function may change other entries
        if self.state_update_function is None:
            self.model = self.model.conditional(self.param)
        self._init_runtime()

    def _column(self, state, param_index):
        """(column (0 for None: the whole vector), are the columns ragged, their live number per chain if so, proposal and accept blocks)"""
        x = state[self.param]
        p = x.shape[0]
        col = 0 if param_index is None else int(param_index)
        ragged_cols = x.ragged is not None and x.ragged[1] == 1
        sub = col * self._blocks_per_proposal(p)
        return col, ragged_cols, x.count(state) if ragged_cols else None, sub, sub + (p + 1) // 2

    def proposal(self, current_state: dict, param_index: int = None, inject=None):
        """metropolis_hastings.py:212-269 for every chain; returns (prop_state, logq_fwd (C,), logq_rev (C,))."""
        eng = self._need_engine()
        x = current_state[self.param]
        if not is_chain(x):
            raise NotImplementedError("RandomWalk needs a per-chain parameter")
        p, n_rep = x.shape
        if param_index is None and n_rep != 1:
            raise NotImplementedError("whole-matrix proposals for a replicated parameter: use RandomWalkLoop")
        step = self.step
        if step.shape[1] != 1:
            if param_index is None:
                raise NotImplementedError("(p, n) step sizes without a column index")
            step = step[:, [param_index]]
        cache = self._dev_consts
        skey = ("step", 0 if self.step.shape[1] == 1 else param_index)
        if skey not in cache:
            cache[skey] = eng.to_device(np.ascontiguousarray(step.reshape(-1)))
        if self.domain_limits is not None and "lim" not in cache:
            lim = np.asarray(self.domain_limits, dtype=np.float64).reshape(-1, 2)
            if lim.shape[0] != p:
                raise ValueError("domain_limits must have one (lower, upper) row per element of the parameter")
            cache["lim"] = (eng.to_device(lim[:, 0].copy()), eng.to_device(lim[:, 1].copy()))
        lower, upper = cache.get("lim", (None, None))
        col, ragged_cols, count, sub, _ = self._column(current_state, param_index)
        data = x.data if x.data.is_contiguous() else x.data.contiguous()
        z = data.clone()
        lq_f, lq_r = eng.rw_propose(data, z, cache[skey], lower, upper, column=col if n_rep > 1 or ragged_cols else None,
                                    count=count, inject=inject, draw_index=self._draw_index(), sub=sub)
        prop_state = {**current_state, self.param: x.like(z)}  # shallow: only the entries a proposal replaces are new objects
        if callable(self.state_update_function):
            prop_state, f_extra, r_extra = self.state_update_function(prop_state, param_index)
            lq_f, lq_r = _add_contribution(eng, lq_f, f_extra), _add_contribution(eng, lq_r, r_extra)
        return prop_state, lq_f, lq_r

    def _generic_step(self, current_state, param_index=None, lp_cur=None):
        inject, u = self._hook("inject", param_index), self._hook("inject_uniform", param_index)
        prop_state, lq_f, lq_r = self.proposal(current_state, param_index, inject=inject)
        col, _, count, _, sub_accept = self._column(current_state, param_index)
        trace = None
        if self.trace is not None:
            trace = {"z": prop_state[self.param].data.clone(), "lq_fwd": lq_f.clone(), "lq_rev": lq_r.clone()}
            self.trace.setdefault("steps", []).append(trace)
        return self._accept_reject_proposal(current_state, prop_state, lq_f, lq_r, count=count, index=col, u=u, sub=sub_accept,
                                            trace=trace, lp_cur=lp_cur)

    def sample(self, current_state: dict) -> dict:
        self.last_log_p = None  # set again by the fused whitened steps only
        eng = self._need_engine()
        if self.domain_limits is None and self.state_update_function is None and self._gaussian_target(current_state):  # (gmrf.py:339)
            self._fused_gaussian_step(current_state, eng.rw_step_white, 1.0, z=self._hook("inject"), u=self._hook("inject_uniform"),
                                      draw_index=self._draw_index())
        else:
            current_state = self._generic_step(current_state)
        self._sweep += 1
        return current_state


@dataclass
class RandomWalkLoop(RandomWalk):
    """One random-walk step per column of the parameter (metropolis_hastings.py:272-289).  For a ragged parameter
    the loop runs to the largest live length over the chains; chains with fewer columns sit the extra steps out.
    `fused` (default True): let one kernel launch run the whole loop when the model allows it (`_knot_plan`)."""

    fused: bool = True

    def _knot_plan(self, state):
        """Can the whole loop go to omc_knot_loop?  Yes when the sampler moves the knots of a library basis
        (state_update_function is a GaussianKnotBasis on this parameter) and the only distributions a move can change
        are the knots' own Uniform prior (constant over the proposal's domain) and ONE Normal regression likelihood
        whose mean carries the basis: shared response, diagonal precision with a per-chain scalar, mean =
        basis @ coefficients + at most one per-chain offset + shared terms.  Returns the kernel's arguments, or None
        (then the loop runs launch by launch through the callback)."""
        from openmcmc_amd.basis import GaussianKnotBasis
        from openmcmc_amd.distribution.distribution import Uniform
        from openmcmc_amd.parameter import LinearCombination, LinearCombinationWithTransform, _is_identity

        basis = self.state_update_function
        if not isinstance(basis, GaussianKnotBasis) or basis.knots != self.param or self.trace is not None:
            return None
        x = state[self.param]
        if (not is_chain(x) or x.ragged is None or x.ragged[1] != 1 or x.shape[0] != 1 or not x.data.is_contiguous()
                or self.step.size != 1 or self.domain_limits is None):
            return None
        lim = np.asarray(self.domain_limits, dtype=np.float64).reshape(-1, 2)
        if lim.shape[0] != 1:
            return None
        lower, upper = float(lim[0, 0]), float(lim[0, 1])
        Bm = state.get(basis.matrix)
        if (not is_chain(Bm) or Bm.shape[1] != x.shape[1] or not Bm.data.transpose(1, 2).is_contiguous()
                or Bm.shape[0] > 10240):  # omc_knot_loop keeps a chain's residual in registers: n <= 10 240
            return None
        lik = None
        for key in self.model.affected_by([self.param, basis.matrix]):
            dist = self.model[key]
            if isinstance(dist, Uniform) and key == self.param:
                if not (np.all(dist.domain_response_lower <= lower) and np.all(dist.domain_response_upper >= upper)):
                    return None
            elif isinstance(dist, Normal) and not dist.is_mixture and lik is None and self.param not in dist.param_list:
                lik = dist
            else:
                return None
        if lik is None or not isinstance(lik.mean, LinearCombination):
            return None
        if isinstance(lik.mean, LinearCombinationWithTransform) and lik.mean.is_transformed():
            return None  # the kernel sums basis x coefficients itself: an exp-transformed term goes launch by launch through log_p
        resp = state[lik.response]
        if is_chain(resp) or resp.shape[1] != 1:
            return None
        host_sum, offset, coef = 0, None, None
        for prm, pre in lik.mean.form.items():
            A, v = state[pre], state[prm]
            if pre == basis.matrix:
                if coef is not None or not is_chain(v) or v.shape[1] != 1:
                    return None
                coef = v.vector()
            elif is_chain(A):
                return None
            elif not is_chain(v):
                host_sum = host_sum + A @ v
            elif v.shape[1] == 1 and _is_identity(A, v.shape[0]) and offset is None:
                offset = v.vector()
            else:
                return None
        if coef is None:
            return None
        st = lik.structure(state)
        if not st.diagonal_only or (st.scale_key is not None and not is_chain(state[st.scale_key])):
            return None
        eng = self._need_engine()
        return {"basis": basis, "x": x, "B": Bm, "coef": coef, "offset": offset, "lower": lower, "upper": upper,
                "y": eng.shared(resp).reshape(-1), "w": None if st.diag is None else eng.shared(st.diag),
                "shared": None if isinstance(host_sum, int) else eng.to_device(np.asarray(host_sum, dtype=np.float64).reshape(-1)),
                "tau": state[st.scale_key].scalar() if st.scale_key is not None else None}

    def _knot_loop(self, current_state, plan):
        eng = self.engine
        x, Bm = plan["x"], plan["B"]
        count = x.count(current_state)
        inj = {}
        if self.inject is not None or self.inject_uniform is not None:  # test hooks: one (C,) vector per column visited
            n_cols = int(count.max().item())
            for name, hook in (("inject_z", "inject"), ("inject_u", "inject_uniform")):
                if getattr(self, hook) is not None:
                    rows = eng.zeros(x.shape[1], eng.n_chains)
                    for j in range(n_cols):
                        rows[j] = self._hook(hook, j).reshape(-1)
                    inj[name] = rows
        eng.knot_loop(plan["basis"].X, plan["basis"].scale, plan["y"], Bm.data.transpose(1, 2), plan["coef"], x.data[:, 0, :],
                      count, float(self.step.item()), plan["lower"], plan["upper"], add_shared=plan["shared"],
                      add_chain=plan["offset"], w=plan["w"], tau=plan["tau"], draw_index=self._draw_index(),
                      accept_count=self.accept_rate.accept, proposal_count=self.accept_rate.proposal, **inj)
        # theta and the basis were updated in place; new wrappers, so that anything keyed on the identity of a state
        # entry sees them as replaced (the convention of every other sampler)
        current_state[self.param] = x.like(x.data)
        current_state[plan["basis"].matrix] = Bm.like(Bm.data)
        return current_state

    def sample(self, current_state: dict) -> dict:
        self.last_log_p = None  # set again by the fused whitened steps only
        plan = self._knot_plan(current_state) if self.fused else None
        if plan is not None:
            current_state = self._knot_loop(current_state, plan)
        else:
            _, ragged_cols, count, _, _ = self._column(current_state, 0)
            self._lp_state = None  # log-density of the current state, carried from one column to the next
            for param_index in range(int(count.max().item()) if ragged_cols else current_state[self.param].shape[1]):
                current_state = self._generic_step(current_state, param_index, lp_cur=self._lp_state)
        self._sweep += 1
        return current_state


@dataclass
class ManifoldMALA(MetropolisHastings):
    """Manifold MALA (Girolami & Calderhead 2011; metropolis_hastings.py:292-373).  `whitened` (default True): the fused
    route for a Gaussian target runs in the coordinates a = L'(x - mu), where the step is element-wise
    (omc_mala_step_white); False keeps it on the products of omc_mala_step.  `fused` (default True): a parameter under the
    exponential transform of a LinearCombinationWithTransform takes its whole update in one launch when the model allows it
    (`_transform_plan`); False keeps it on the launch-by-launch route (`_general_step`)."""

    whitened: bool = True
    fused: bool = True

    def _transform_plan(self, state):
        """Can the whole update go to omc_mala_transform_step?  Yes when the parameter is a fixed-size per-chain (p, 1) vector,
        p <= 64, without domain limits, that appears in exactly one likelihood Normal -- as an exp-transformed term of its
        LinearCombinationWithTransform mean with a shared design, every other term shared, a shared response (any number of
        replicates) and a shared precision matrix, optionally times a per-chain scalar -- and whose own distribution is a
        non-mixture Normal with shared mean and shared precision matrix, optionally times a per-chain scalar.  Then target,
        gradient and Hessian at any x need only G = n_rep A'WA, c = A'W sum_rep (y - shared terms) and the prior: computed
        once on the host and kept while the state entries they were made from are the same objects.  None otherwise (the
        launch-by-launch route takes the step)."""
        from scipy import sparse

        from openmcmc_amd.parameter import LinearCombinationWithTransform

        x = state[self.param]
        if (not self.fused or np.size(self.step) != 1 or not is_chain(x) or x.ragged is not None or x.shape[1] != 1
                or x.shape[0] > 64 or not x.data.is_contiguous()):
            return None
        prior, lik = self.model.get(self.param), None
        for key, dist in self.model.items():
            if key == self.param or self.param not in dist.param_list:
                continue
            if lik is not None:
                return None
            lik = dist
        if lik is None or not isinstance(prior, Normal) or type(lik) is not Normal or type(prior) is not Normal:
            return None
        if prior.is_mixture or lik.is_mixture or prior.domain_response_lower is not None or prior.domain_response_upper is not None:
            return None
        mean = lik.mean
        if (not isinstance(mean, LinearCombinationWithTransform) or self.param not in mean.form or not mean._transformed(self.param)
                or self.param in lik.precision.get_param_list() or mean.has_chain_terms(state, exclude=self.param)):
            return None
        A, resp = state[mean.form[self.param]], state[lik.response]
        if is_chain(A) or is_chain(resp) or any(is_chain(state[k]) for k in prior.mean.get_param_list()):
            return None
        try:
            st_l, st_p = lik.structure(state), prior.structure(state)
        except NotImplementedError:
            return None
        for st in (st_l, st_p):
            if st.scale_key is not None and not is_chain(state[st.scale_key]):
                return None
        # the host objects the statistics are made from: kept in the memo and compared with `is` (an id() alone can be reused)
        made_from = [A, resp, st_l.matrix, st_p.matrix] + [state[k] for k in mean.get_param_list() if k != self.param] \
            + [state[k] for k in prior.mean.get_param_list()]
        memo = self._transform_memo
        if memo is None or len(memo[0]) != len(made_from) or any(a is not b for a, b in zip(memo[0], made_from)):
            eng = self._need_engine()
            dense = lambda M: M.toarray() if sparse.issparse(M) else np.asarray(M, dtype=np.float64)  # noqa: E731
            Ad, Y = dense(A), np.asarray(resp, dtype=np.float64)
            rest = mean.predictor_conditional(state, term_to_exclude=self.param)
            ysum = (Y - (0.0 if isinstance(rest, int) else np.asarray(rest, dtype=np.float64))).sum(axis=1)
            WA = np.asarray(st_l.matrix @ Ad, dtype=np.float64)
            G = float(Y.shape[1]) * (Ad.T @ WA)
            m0 = np.asarray(prior.mean.predictor(state), dtype=np.float64).reshape(-1)
            # (the kernel reads element (i, j) at [j * p + i]: the transposes, so that it sees exactly these matrices)
            stats = {"G": eng.to_device(np.ascontiguousarray(G.T)), "c": eng.to_device(WA.T @ ysum),
                     "P": eng.to_device(np.ascontiguousarray(dense(st_p.matrix).T)),
                     "m0": eng.to_device(m0) if np.any(m0) else None}
            memo = self._transform_memo = (made_from, stats)
        plan = dict(memo[1])
        plan["tau"] = state[st_l.scale_key].scalar() if st_l.scale_key is not None else None
        plan["lam"] = state[st_p.scale_key].scalar() if st_p.scale_key is not None else None
        return plan

    def _transform_step(self, current_state: dict, plan: dict) -> dict:
        """metropolis_hastings.py:127-173 and :301-373 as one launch (omc_mala_transform_step): forward proposal, reverse
        proposal and the accept test on the p x p statistics of `_transform_plan`; x is updated in place."""
        eng = self.engine
        x = current_state[self.param]
        xv = x.vector()
        Cn, p = xv.shape
        z, u = self._hook("inject"), self._hook("inject_uniform")
        prop = lq_f = lq_r = None
        if self.trace is not None:
            prop, lq_f, lq_r = eng.empty(Cn, p), eng.empty(Cn), eng.empty(Cn)
            self.trace.setdefault("steps", []).append({"prop": prop, "lq_fwd": lq_f, "lq_rev": lq_r})
        eng.mala_transform_step(plan["G"], plan["c"], plan["P"], float(self.step.item()), xv, m0=plan["m0"], tau=plan["tau"],
                                lam=plan["lam"], z=None if z is None else z.reshape(Cn, p).contiguous(), u=u,
                                draw_index=self._draw_index(), accept_count=self.accept_rate.accept,
                                proposal_count=self.accept_rate.proposal, prop_out=prop, lq_fwd_out=lq_f, lq_rev_out=lq_r)
        # x was updated in place; a new wrapper, so that anything keyed on the identity of a state entry sees it as replaced
        current_state[self.param] = x.like(x.data)
        return current_state

    def _diag_step(self, current_state: dict) -> dict:
        """Generic route when the Hessian is diagonal per chain (e.g. the mixture-Normal prior of a variable-size
        coefficient vector under a null likelihood): metropolis_hastings.py:301-373 with omc_mala_diag for the proposal
        and its two densities, then the generic accept/reject with the sampler's model."""
        eng = self.engine
        x = current_state[self.param]
        if not is_chain(x) or x.shape[1] != 1:
            raise NotImplementedError("ManifoldMALA needs a per-chain (d, 1) parameter")
        step = float(self.step.item())
        count = x.count(current_state) if (x.ragged is not None and x.ragged[1] == 0) else None
        grad, h = self.model.grad_log_p_diag(current_state, self.param, eng)
        xp, lq_f = eng.mala_diag(x.vector(), grad, h, step, count=count, z=self._hook("inject"), draw_index=self._draw_index(), sub=0)
        prop_state = {**current_state, self.param: x.like(xp.unsqueeze(2))}
        grad_p, h_p = self.model.grad_log_p_diag(prop_state, self.param, eng)
        lq_r = eng.mala_diag(xp, grad_p, h_p, step, count=count, x_other=x.vector().contiguous())
        return self._accept_reject_proposal(current_state, prop_state, lq_f, lq_r, u=self._hook("inject_uniform"),
                                            sub=self._accept_block(x.shape[0]))

    def _dense_step(self, current_state: dict) -> dict:
        """Generic route for a Hessian that is a per-chain combination of shared matrices (+ a per-chain diagonal):
        regression coefficients under a Gaussian or a mixture prior (`_mmala_step` over `_SharedPrecision`)."""
        eng, s2 = self.engine, float(self.step.item()) ** 2

        def point(state, zero, forward):  # (the Hessian does not depend on the parameter: the proposed point keeps the forward object)
            grad, terms, diag = self.model.grad_terms(state, self.param, eng)
            return grad, forward or _SharedPrecision(eng, terms, diag, s2, zero.shape, self._draw_index())
        return self._mmala_step(current_state, point)

    def _mmala_step(self, current_state, point, trace=False):
        """The proposal of metropolis_hastings.py:301-373 and its accept test over Lambda_c = H_c / step^2 as an object (`_SharedPrecision`,
        `_ChainPrecision`): from x, b = Lambda x + g/2, x' = m + L^-T z with m = Lambda^-1 b, log q(x'|x) = (1/2) log det Lambda
        - (1/2)(x' - m)' Lambda (x' - m); the same from x' with z = 0 for log q(x|x').  `point(state, zero, forward)` -> (gradient
        (C, d), precision) at a state; `forward` is None at x and the precision found there at x'."""
        eng = self.engine
        x = current_state[self.param]
        xv = x.vector().contiguous()
        zero = eng.zeros(*xv.shape)

        def log_q(prec, start, grad, z, end=None):  # (the point drawn from `start` with noise z, log q(end or that point | start))
            drawn, mean = prec.draw(_lin(eng, 1.0, prec.times(start), 0.5, grad), z)
            dev = _lin(eng, 1.0, drawn if end is None else end, -1.0, mean)
            return drawn, _lin(eng, 0.5, prec.logdet, -0.5, prec.quad(dev))

        grad, prec = point(current_state, zero, None)
        xp, lq_f = log_q(prec, xv, grad, self._hook("inject"))
        prop_state = {**current_state, self.param: x.like(xp.unsqueeze(2))}
        grad_p, prec_p = point(prop_state, zero, prec)
        _, lq_r = log_q(prec_p, xp, grad_p, zero, end=xv)
        if trace and self.trace is not None:
            self.trace.setdefault("steps", []).append({"prop": xp.clone(), "lq_fwd": lq_f.clone(), "lq_rev": lq_r.clone()})
        return self._accept_reject_proposal(current_state, prop_state, lq_f, lq_r, u=self._hook("inject_uniform"),
                                            sub=self._accept_block(xv.shape[1]))

    def _grad_hess_per_chain(self, state):
        """(grad (C, d), H (C, d, d)) of the whole model w.r.t. the parameter, for every chain, whatever each member
        distribution returns (model.py:72-112): a shared matrix, a per-chain scalar x shared matrix (ScaledHessian) or the
        (C, d, d) tensor of the finite-difference default (distribution.py:124-198)."""
        import torch
        from scipy import sparse

        from openmcmc_amd.distribution.location_scale import ScaledHessian

        eng = self.engine
        x = state[self.param]
        Cn, d = x.n_chains, x.size
        grad, H = None, eng.zeros(Cn, d, d)
        for dist in self.model.values():
            if self.param not in dist.param_list:
                continue
            g, h = dist.grad_log_p(state, self.param, hessian_required=True, engine=eng)
            grad = g.data.reshape(Cn, d) if grad is None else grad + g.data.reshape(Cn, d)
            if isinstance(h, ScaledHessian):
                M = h.matrix.toarray() if sparse.issparse(h.matrix) else np.asarray(h.matrix, dtype=np.float64)
                H = H + h.scale.reshape(Cn, 1, 1) * eng.to_device(M).unsqueeze(0)
            elif isinstance(h, torch.Tensor):
                H = H + h.reshape(Cn, d, d)
            else:
                M = h.toarray() if sparse.issparse(h) else np.asarray(h, dtype=np.float64)
                H = H + eng.to_device(M).unsqueeze(0)
        if grad is None:
            raise ValueError(f"no distribution depends on '{self.param}'")
        return grad.contiguous(), H.contiguous()

    def _general_step(self, current_state: dict) -> dict:
        """Any model whose device log_p exists, for a fixed-size parameter: gradient and Hessian of every
        member as the reference's generic path computes them (analytic where a distribution has one, central differences
        otherwise, distribution.py:90-198), Lambda_c = H_c / step^2 factorised per chain (`_mmala_step` over `_ChainPrecision`)."""
        x = current_state[self.param]
        if x.ragged is not None or x.shape[1] != 1:
            raise NotImplementedError("generic ManifoldMALA route: fixed-size (d, 1) parameter")
        eng, s2 = self.engine, float(self.step.item()) ** 2

        def point(state, zero, forward):  # (the Hessian moves with the state: evaluated and factorised again at the proposed point)
            grad, H = self._grad_hess_per_chain(state)
            return grad, _ChainPrecision(eng, H / s2, zero, self._draw_index())
        return self._mmala_step(current_state, point, trace=True)

    def can_run_block(self, state) -> bool:
        """May MCMC.run_mcmc hand this sampler whole blocks of iterations (omc_mala_run_white)?  The fused whitened route, no
        injected draws, no trace, and `sample` not replaced by the caller."""
        return (self.whitened and self.inject is None and self.inject_uniform is None and self.trace is None
                and getattr(self.sample, "__func__", None) is ManifoldMALA.sample and self._gaussian_target(state))

    def run_block(self, current_state: dict, n_steps: int, x_store=None, logp_store=None) -> dict:
        """n_steps calls of `sample` as one library call: blocks of 32 steps per launch, the state of every step into
        x_store (n_steps, C, d) and the target's log density there into logp_store (n_steps, C) when given (what
        sampler.store and mcmc.py:108 keep per iteration).  Same streams, same decisions, same states as the single steps."""
        if not self._gaussian_target(current_state):
            raise NotImplementedError("fused MH route needs Normal(param, mean=<shared>, precision=<shared matrix>) and a scalar step")
        self._fused_gaussian_step(current_state, self._need_engine().mala_run_white, 1.0 / float(self.step.item()) ** 2,
                                  n_steps=int(n_steps), draw_index0=self._draw_index(), draw_stride=self._n_samplers, x_store=x_store,
                                  logp_store=logp_store)
        self._sweep += int(n_steps)
        return current_state

    def _route(self, state):
        """(the route `sample` takes in this state, the plan of the "transform" route or None)"""
        if self._gaussian_target(state):
            return ("white" if self.whitened else "products"), None
        # a per-chain diagonal Hessian: a variable-size parameter, or nothing but the parameter's own mixture prior and null distributions
        if state[self.param].ragged is not None or all((getattr(d, "is_mixture", False) and k == self.param)
                                                       or isinstance(d, NullDistribution) for k, d in self.model.items()):
            return "diag", None
        plan = self._transform_plan(state)
        if plan is not None:
            return "transform", plan
        structured = all(hasattr(d, "grad_terms") and d.constant_hessian(self.param)
                         for d in self.model.values() if self.param in d.param_list)
        return ("dense" if structured else "general"), None  # a constant Hessian of shared matrices, or one per chain and point

    def route(self, state) -> str:
        """Which of "white", "products", "diag", "transform", "dense", "general" does `sample` take in this state?"""
        return self._route(state)[0]

    def sample(self, current_state: dict) -> dict:
        self.last_log_p = None  # set again by the fused whitened steps only
        eng = self._need_engine()
        route, plan = self._route(current_state)
        step = float(self.step.item())
        if route == "white":  # L = chol(H/step^2), H = Q (metropolis_hastings.py:345-346)
            self._fused_gaussian_step(current_state, eng.mala_step_white, 1.0 / step**2, z=self._hook("inject"),
                                      u=self._hook("inject_uniform"), draw_index=self._draw_index())
        elif route == "products":
            Q, mu = self._target(current_state)
            L, sl = self._factor_plan(eng, current_state, Q, 1.0 / step**2)
            eng.mala_step(Q, mu, L, sl, step, self._x(current_state), z=self._hook("inject"), u=self._hook("inject_uniform"),
                          draw_index=self._draw_index(), accept_count=self.accept_rate.accept, proposal_count=self.accept_rate.proposal)
        else:
            current_state = {"diag": self._diag_step, "transform": partial(self._transform_step, plan=plan), "dense": self._dense_step,
                             "general": self._general_step}[route](current_state)
        self._sweep += 1
        return current_state
