"""MCMC driver on chain-batched state (reference mcmc.py:19-115).

Same fields and loop as the reference plus `n_chains`, `seed`, `device`, `chain_id_offset`: C
independent chains advance together, one HIP launch per sampler per sweep -- or ONE launch per
sweep when the sampler list is the Gaussian-block pattern [NormalNormal(x), NormalGamma(s)...],
which `fuse=True` (default) recognises and hands to omc_gmrf_sweep.  Both routes draw from the
same random streams and give identical results.

store[param] is a device tensor (n_iter, C, size); `collect()` returns host arrays shaped
(C, size, n_iter), i.e. the reference's store per chain.

The store is the step directly behind the sampler loop (mcmc.py:105-111): it stays on the device,
`summary()` / `quantiles()` reduce it there, `collect(every=k)` / `gather(every=k)` move a thinned part only, and with
`store_ring=R` the device keeps a ring of R iteration slabs that a second stream drains -- to pinned host memory, or to the
root rank through the run's one collective (parallel.GatherSink) -- while the chains keep sampling: a run is then not bounded by
what 288 GB hold (about 3 400 stored iterations at cfg3).
"""

from copy import copy
from dataclasses import dataclass, field

import numpy as np
from scipy import sparse

from openmcmc_amd.chains import ChainArray, host_2d, is_chain
from openmcmc_amd.model import Model
from openmcmc_amd.parameter import LinearCombination, ScaledMatrix
from openmcmc_amd.sampler.sampler import MCMCSampler, MixtureAllocation, NormalGamma, NormalNormal


@dataclass
class MCMC:
    state: dict
    samplers: list
    model: Model
    n_burn: int = 5000
    n_iter: int = 5000
    n_thin: int = 1
    n_chains: int = 1
    seed: int = 0
    device: int = 0
    chain_id_offset: int = 0
    fuse: bool = True
    engine: object = None  # an existing Engine (e.g. one that user callbacks already hold); default: a new one
    store_ring: int = 0    # > 0: the device store is a ring of this many iteration slabs, drained in halves while sampling goes on
    sink: object = None    # ring mode: callable(key, it0, it1, device_block) run under the drain stream; default: pinned host arrays
    store: dict = field(default_factory=dict, init=False)

    def __post_init__(self):
        from openmcmc_amd.engine import Engine

        self.state = copy(self.state)
        for key, term in self.state.items():  # mcmc.py:65-76
            if sparse.issparse(term) or is_chain(term):
                continue
            self.state[key] = host_2d(term)
        if self.engine is None:
            self.engine = Engine(self.n_chains, seed=self.seed, device=self.device, chain_id_offset=self.chain_id_offset)
        elif self.engine.n_chains != self.n_chains:
            raise ValueError("engine holds a different number of chains")
        eng, C = self.engine, self.n_chains
        ns = len(self.samplers)
        # iteration slabs resident on the device: all of them, or a ring of two halves (one being filled, one being drained)
        self._n_dev, self._half, self._drain = self.n_iter, self.n_iter, None
        if self.store_ring:
            if int(self.store_ring) < 2:
                raise ValueError("store_ring must be at least 2 (two halves)")
            half = int(self.store_ring) // 2
            self._half, self._n_dev = (half, 2 * half) if 2 * half < self.n_iter else (max(1, self.n_iter), max(1, self.n_iter))
        for pos, sampler in enumerate(self.samplers):
            sampler.bind(eng, pos, ns)
            # what the rest of the sweep samples after this block (a Normal-Normal block does not take the fused quadratic
            # form of a term whose other side is about to be replaced)
            sampler._later_params = frozenset(s.param for s in self.samplers[pos + 1:])
            if sampler.param not in self.state:  # mcmc.py:79-80: draw the start from the prior
                self.state[sampler.param] = sampler.model[sampler.param].rvs(
                    self.state, engine=eng, draw_index=(1 << 40) + pos)
            elif not is_chain(self.state[sampler.param]):
                v = np.asarray(self.state[sampler.param], dtype=np.float64)
                self.state[sampler.param] = ChainArray(eng.to_device(np.broadcast_to(v, (C,) + v.shape).copy()))
            self.store = sampler.init_store(current_state=self.state, store=self.store, n_iterations=self._n_dev)
        if self.model.response is not None:
            for response in self.model.response.keys():
                self.store[response] = eng.full((self._n_dev, C, self.state[response].size), float("nan"))
        self.store["log_post"] = eng.full((self._n_dev, C), float("nan"))
        self._fused = self._fusion_plan() if self.fuse else None
        self._sweeps_done = 0
        self._derived = set()  # names of the store entries `derive` made
        if self.store_ring:
            self._drain = _RingDrain(self)

    def _check_stream(self):
        """The context issues every library call on the stream it was created with; the mirror's own torch operations run
        on torch's current stream.  Sampling under another current stream would let the two race."""
        import torch

        if torch.cuda.current_stream(self.engine.device).cuda_stream != self.engine._stream.cuda_stream:
            raise RuntimeError("the current torch stream is not the one the Engine was created under: create the Engine (or "
                               "the MCMC object) and call run_mcmc under the same torch.cuda.stream")

    # ------------------------------------------------------------------ fusion
    def _fusion_plan(self):
        """[NormalNormal(x), NormalGamma(s_1), ...] with every s_j the ScaledMatrix scalar of one of
        x's Gaussian terms, no fitted-value store, and the full model made of exactly those pieces."""
        if len(self.samplers) < 2 or self.model.response is not None:
            return None
        nn = self.samplers[0]
        if type(nn) is not NormalNormal or nn.inject is not None:
            return None
        gammas = self.samplers[1:]
        if any(type(g) is not NormalGamma for g in gammas):
            return None
        try:
            plan = nn.plan(self.state)
        except NotImplementedError:
            return None
        if plan.kind != "tridiag" or plan.chain_terms or plan.center_chain or plan.replicated or plan.limits is not None:
            return None
        term_of = {}
        for k, key in enumerate(plan.keys):
            prec = nn.model[key].precision
            if isinstance(prec, ScaledMatrix):
                term_of[prec.scalar] = k
        blocks = [None] * len(plan.keys)
        for pos, g in enumerate(gammas, start=1):
            k = term_of.get(g.param)
            if k is None or g.normal_param != plan.keys[k] or blocks[k] is not None:
                return None
            blocks[k] = (pos, g)
        expected = set(plan.keys) | {g.param for g in gammas}
        full_model = set(self.model.keys()) == expected
        return {"nn": nn, "plan": plan, "blocks": blocks, "log_post": full_model}

    def _gamma_specs(self, draw_index0, rows):
        """One spec per term of the fused plan for the library's Gamma blocks: the block of sampler `pos` draws from index
        draw_index0 + pos and writes into the rows `rows` of its store (None: nowhere)."""
        f = self._fused
        nn, plan = f["nn"], f["plan"]
        specs = []
        for k, key in enumerate(plan.keys):
            spec = {"enabled": False, "logdet": plan.logdets[k]}
            if f["blocks"][k] is not None:
                pos, g = f["blocks"][k]
                a0, b0 = g.prior_shape_rate(self.state)
                spec.update(enabled=True, a0=a0, b0=b0, n_pos=nn.model[key].structure(self.state).n_pos, draw_index=draw_index0 + pos,
                            g=g.inject(g, g._sweep) if g.inject is not None else None,
                            store=None if rows is None else self.store[g.param][rows, :, 0])
            specs.append(spec)
        return specs

    def _fused_sweep(self, store_it):
        eng, f = self.engine, self._fused
        nn, plan = f["nn"], f["plan"]
        ns, t, n = len(self.samplers), nn._sweep, plan.n
        specs = self._gamma_specs(t * ns, store_it)
        x_out = self.store[nn.param][store_it] if store_it is not None else self._scratch(n)
        lp = self.store["log_post"][store_it] if (store_it is not None and f["log_post"]) else None
        z = nn.inject(nn, nn._sweep) if getattr(nn, "inject", None) is not None else None  # (test hook set after construction)
        eng.gmrf_sweep(n, plan.terms, specs, x_out, z=z, draw_index=t * ns, log_post_out=lp)
        self.state[nn.param] = ChainArray(x_out)
        for s in self.samplers:
            s._sweep += 1

    def _direct_slab(self, sampler, i_it):
        """The store slab of this iteration if `sampler` can draw straight into it (a fixed-size NormalNormal block whose
        store is the plain (n_iter, C, n) tensor): the store step then has nothing to copy."""
        if type(sampler) is not NormalNormal or sampler.max_variable_size is not None:
            return None
        if getattr(sampler.sample, "__func__", None) is not NormalNormal.sample:
            return None  # a replaced sample method (tests count the calls): it gets the reference's signature
        cur = self.state.get(sampler.param)
        st = self.store.get(sampler.param)
        if not is_chain(cur) or cur.ragged is not None or cur.shape[1] != 1 or st is None or st.dim() != 3 or st.shape[2] != cur.shape[0]:
            return None
        return st[i_it]

    def _scratch(self, n):
        if getattr(self, "_scratch_x", None) is None or self._scratch_x.shape[1] != n:
            self._scratch_x = self.engine.empty(self.n_chains, n)
        return self._scratch_x

    # ------------------------------------------------------------------ the loop (mcmc.py:87-115)
    def _run_fused_in_c(self):
        """The whole loop as one omc_gmrf_run call: possible when no draws are injected."""
        eng, f = self.engine, self._fused
        nn, plan = f["nn"], f["plan"]
        ns, n = len(self.samplers), plan.n
        specs = self._gamma_specs(0, slice(None))  # (a block's offset inside a sweep's draw indices; its whole store)
        # one library call for the whole run -- or, with a ring store, one per half of the ring: the drain stream empties
        # the half just filled while the next call fills the other (same draw indices, same results as the single call)
        it, burn = 0, self.n_burn
        while it < self.n_iter:
            k = min(self._half, self.n_iter - it)
            if self._drain is not None:
                self._drain.acquire(it)
            eng.gmrf_run(n, plan.terms, specs, burn, k, self.n_thin, self.store[nn.param],
                         self._scratch(n), draw_index0=nn._sweep * ns, draws_per_sweep=ns, first_slot=it % self._n_dev,
                         log_post_store=self.store["log_post"] if f["log_post"] else None)
            for s in self.samplers:
                s._sweep += (burn + k) * self.n_thin
            if self._drain is not None:
                self._drain.release(it, it + k)
            it, burn = it + k, 0
        last = self.store[nn.param][(self.n_iter - 1) % self._n_dev] if self.n_iter > 0 else self._scratch(n)
        self.state[nn.param] = ChainArray(last)

    def _early_freeze_plan(self):
        """{sampler index: [(response key, predictor parameter)]}: stored LinearCombination predictors that may be evaluated
        right after that sampler because nothing later in the sweep changes their inputs.  Only when every later sampler is a
        conjugate one (it replaces its own parameter and nothing else) whose parameter the predictor does not use."""
        plan = {}
        if self._fused is not None or self.model.response is None:
            return plan
        for response, predictor in self.model.response.items():
            par = getattr(self.model[response], predictor)
            if not isinstance(par, LinearCombination):
                continue
            used = set(par.form.keys()) | set(par.form.values())
            touching = [k for k, s in enumerate(self.samplers)
                        if s.param in used or not isinstance(s, (NormalNormal, NormalGamma, MixtureAllocation))]
            if not touching:
                continue
            k = max(touching)
            if k == len(self.samplers) - 1 or self.samplers[k].param not in used:
                continue  # nothing to gain, or the last sampler that matters is one that may change anything
            if not isinstance(self.samplers[k], (NormalNormal, NormalGamma, MixtureAllocation)):
                continue
            plan.setdefault(k, []).append((response, par))
        return plan

    def run_mcmc(self):
        eng = self.engine
        self._check_stream()
        if not self.store_ring:  # (a caller may have re-sized n_iter and the store after construction)
            self._n_dev = self._half = self.n_iter
        if (self._fused is not None and self._fused["log_post"] and self.n_iter > 0
                and all(getattr(s, "inject", None) is None for s in self.samplers)):
            self._run_fused_in_c()
            return self._finish()
        if self._mala_block_route():
            self._run_mala_blocks()
            return self._finish()
        early = self._early_freeze_plan()
        for i_it in range(-self.n_burn, self.n_iter):
            storing = i_it >= 0
            slot = i_it % self._n_dev if storing else None  # the iteration's slab on the device (a ring with store_ring)
            if storing and self._drain is not None and i_it % self._half == 0:
                self._drain.acquire(i_it)
            for i_thin in range(self.n_thin):
                last = i_thin == self.n_thin - 1
                if self._fused is not None:
                    self._fused_sweep(slot if (storing and last) else None)
                else:
                    for k, sampler in enumerate(self.samplers):
                        slab = self._direct_slab(sampler, slot) if (storing and last) else None
                        self.state = sampler.sample(self.state) if slab is None else sampler.sample(self.state, out=slab)
                        if storing and last:
                            # a stored predictor whose inputs no later sampler of the sweep touches: evaluated here, into
                            # its store slab, and reused by the samplers that follow (a NormalGamma's residual), by the store
                            # and by log_post
                            for response, par in early.get(k, ()):
                                par._frozen = {}
                                par.predictor_device(self.state, eng, out=self.store[response][slot])
            if not storing:
                continue
            if self._fused is None:
                for sampler in self.samplers:
                    self.store = sampler.store(current_state=self.state, store=self.store, iteration=slot)
            # The state does not change any more in this sweep: the fitted values go straight into their store slab and
            # log_post's residual reads them from there (mcmc.py:99-111 evaluates the predictor once for each; for cfg2 that
            # is a 5 GFLOP product per evaluation)
            frozen = []
            if self.model.response is not None:
                for response, predictor in self.model.response.items():
                    par = getattr(self.model[response], predictor)
                    if hasattr(par, "predictor_device") and any(is_chain(self.state[k]) for k in par.form):
                        if getattr(par, "_frozen", None) is None:
                            par._frozen = {}
                        frozen.append(par)
                        par.predictor_device(self.state, eng, out=self.store[response][slot])  # (a no-op when evaluated early)
                        continue
                    fitted = par.predictor(self.state)
                    if is_chain(fitted):
                        eng.chain_copy(fitted.data.reshape(self.n_chains, -1), self.store[response][slot])
                    else:
                        self.store[response][slot].copy_(eng.to_device(np.asarray(fitted).reshape(1, -1)).expand(self.n_chains, -1))
            try:
                if self._fused is None or not self._fused["log_post"]:
                    # one sampler on a one-distribution model whose fused step has just left the target's log density of
                    # this very state behind (the whitened MALA / random-walk steps): that IS the model's log_p
                    lp = getattr(self.samplers[0], "last_log_p", None) if len(self.samplers) == 1 and len(self.model) == 1 else None
                    cur = self.state.get(self.samplers[0].param) if lp is not None else None
                    if lp is not None and is_chain(cur) and cur.data.data_ptr() == lp[1].data_ptr():
                        self.store["log_post"][slot].copy_(lp[0])
                    else:
                        self.model.log_p(self.state, engine=eng, out=self.store["log_post"][slot])
            finally:
                for par in frozen:
                    par._frozen = None
            if self._drain is not None and ((i_it + 1) % self._half == 0 or i_it == self.n_iter - 1):
                self._drain.release(i_it - i_it % self._half, i_it + 1)
        self._finish()

    def _finish(self):
        """The end of run_mcmc: like the reference it returns with the whole store where the user reads it."""
        self.engine.check_status()  # raises numpy.linalg.LinAlgError like gmrf.py:518 if a factorisation failed
        if self._drain is not None:
            self._drain.wait()
        self._print_acceptance()

    def _print_acceptance(self):
        from openmcmc_amd.sampler.metropolis_hastings import MetropolisHastings

        for sampler in self.samplers:  # mcmc.py:113-115
            if isinstance(sampler, MetropolisHastings):
                print(f"{sampler.param}: {sampler.accept_rate.get_acceptance_rate()}")

    # ------------------------------------------------------------------ one ManifoldMALA sampler on a Gaussian target (cfg4)
    def _mala_block_route(self):
        """[ManifoldMALA(x)] alone on the one-Normal model of the fused whitened step, every iteration stored: the loop is then
        blocks of steps issued by the library (omc_mala_run_white), the store slabs written by one product per block."""
        from openmcmc_amd.sampler.metropolis_hastings import ManifoldMALA

        if len(self.samplers) != 1 or self.n_thin != 1 or self.model.response is not None or len(self.model) != 1:
            return False
        smp = self.samplers[0]
        if type(smp) is not ManifoldMALA or smp.max_variable_size is not None or not smp.can_run_block(self.state):
            return False
        cur, st = self.state.get(smp.param), self.store.get(smp.param)
        return (is_chain(cur) and cur.ragged is None and cur.shape[1] == 1 and st is not None and st.dim() == 3
                and st.shape[2] == cur.shape[0] and st.is_contiguous())

    def _run_mala_blocks(self):
        smp = self.samplers[0]
        if self.n_burn > 0:
            self.state = smp.run_block(self.state, self.n_burn)  # nothing stored: no product until the last step
        it = 0
        while it < self.n_iter:
            k = min(self._half, self.n_iter - it)
            if self._drain is not None:
                self._drain.acquire(it)
            lo = it % self._n_dev
            self.state = smp.run_block(self.state, k, x_store=self.store[smp.param][lo: lo + k],
                                       logp_store=self.store["log_post"][lo: lo + k])
            if self._drain is not None:
                self._drain.release(it, it + k)
            it += k

    # ------------------------------------------------------------------ results
    def _whole_store_on_device(self, what):
        if self.store_ring and self._n_dev != self.n_iter:
            raise ValueError(f"{what} reduces the device store, and with store_ring the device holds the last {self._n_dev} of "
                             f"{self.n_iter} iterations only: reduce the drained store (host_store) instead")

    def summary(self, key, pooled=True):
        """Posterior mean and variance of store[key] computed on the device (no gather of the store):
        pooled over chains and iterations -> ((size,), (size,)), else per chain -> ((C, size), (C, size))."""
        self._whole_store_on_device("summary")
        t = self.store[key]
        t = t.unsqueeze(-1) if t.dim() == 2 else t.reshape(t.shape[0], t.shape[1], -1)
        mean, var = self.engine.store_moments(t.contiguous(), pooled=pooled)
        return mean.cpu().numpy(), var.cpu().numpy()

    def quantiles(self, key, q, pooled=True, omit_nan=True):
        """np.quantile(..., q) of store[key] over the stored iterations, computed on the device (exact order statistics by
        radix refinement, numpy's default "linear" interpolation; the store is neither sorted nor moved):
        pooled over chains and iterations -> (len(q), size), else per chain -> (len(q), C, size) -- what a user of the
        reference gets from np.quantile(mcmc.store[key], q, axis=-1) per chain.  omit_nan: the NaN padding of variable-size
        parameters is left out (np.nanquantile); False propagates NaN like np.quantile."""
        self._whole_store_on_device("quantiles")
        t = self.store[key]
        t = t.unsqueeze(-1) if t.dim() == 2 else t.reshape(t.shape[0], t.shape[1], -1)
        return self.engine.store_quantiles(t.contiguous(), q, pooled=pooled, omit_nan=omit_nan).cpu().numpy()

    def diagnostics(self, key):
        """Convergence diagnostics of store[key], computed on the device (no gather of the store): a dict of host arrays
        of shape (size,) -- "rhat" (split R-hat), "ess" (effective sample size, Geyer's initial monotone sequence as
        ArviZ's ess(method="mean")) and "mcse_mean" (pooled sd / sqrt(ess)).  Every chain is split into its first and last
        halves; an element with a NaN draw (the padding of variable-size parameters) gives NaN.  Under a sharded multi-GPU
        run these are diagnostics of this rank's chains only."""
        self._whole_store_on_device("diagnostics")
        t = self.store[key]
        t = (t.unsqueeze(-1) if t.dim() == 2 else t.reshape(t.shape[0], t.shape[1], -1)).contiguous()
        rhat, ess, _ = self.engine.store_rhat_ess(t)
        _, var = self.engine.store_moments(t, pooled=True)
        rhat, ess, var = rhat.cpu().numpy(), ess.cpu().numpy(), var.cpu().numpy()
        return {"rhat": rhat, "ess": ess, "mcse_mean": np.sqrt(var) / np.sqrt(ess)}

    def rank_diagnostics(self, key, index=None):
        """Rank-normalised convergence diagnostics of store[key] (Vehtari et al. 2021, the defaults of Stan and ArviZ),
        computed on the device (no gather of the store): a dict of host arrays of shape (n_idx,) -- "rhat" (the larger of
        the rank-normalised split R-hat of the draws and of the draws folded around their median), "ess_bulk" and
        "ess_tail" (the smaller ESS of the indicators of the 5 % and 95 % quantiles).  They see differences in scale and
        in the tails that `diagnostics` (means and variances of the raw draws) does not.  index selects elements (in that
        order, repeats allowed); a 2-D entry ("log_post") counts as one element.  An element with a NaN or infinite draw
        gives NaN.  Every element is sorted: meant for the elements one inspects.  Under a sharded multi-GPU run these are
        diagnostics of this rank's chains only."""
        self._whole_store_on_device("rank diagnostics")
        rhat, bulk, tail = self.engine.store_rank_diagnostics(self._store_3d(key), index=index)
        return {"rhat": rhat.cpu().numpy(), "ess_bulk": bulk.cpu().numpy(), "ess_tail": tail.cpu().numpy()}

    def _selected_columns(self, key, index):
        """(store (n_iter, C, size), selection as a host int64 array or None, n_idx); an entry outside [0, size) raises"""
        t = self._store_3d(key)
        if index is None:
            return t, None, t.shape[2]
        idx, n = self.engine._store_index(index, t.shape[2])
        cols = idx.cpu().numpy()
        if cols.min() < 0 or cols.max() >= t.shape[2]:
            raise ValueError(f"index outside [0, {t.shape[2]})")
        return t, cols, n

    def _column_chunks(self, t, cols, n):
        """(first, last, contiguous sub-store (n_iter, C, last - first)) over the selected columns, each at most 1 GiB"""
        import torch

        step = max(1, (1 << 30) // (8 * t.shape[0] * t.shape[1]))
        for a in range(0, n, step):
            b = min(n, a + step)
            if cols is None:
                yield a, b, (t if (a, b) == (0, t.shape[2]) else t[:, :, a:b].contiguous())
            else:
                yield a, b, t.index_select(2, torch.as_tensor(cols[a:b], device=t.device)).contiguous()

    def _mean_sd_ess(self, key, index, squared):
        """pooled mean, pooled sd (ddof 1) and E(.) of omc_store_rhat_ess -- of the draws, or with `squared` of (x - pooled mean)^2
        -- of the selected columns, as host arrays (n_idx,)"""
        t, cols, n = self._selected_columns(key, index)
        mean, sd, ess = np.empty(n), np.empty(n), np.empty(n)
        for a, b, sub in self._column_chunks(t, cols, n):
            m, v = self.engine.store_moments(sub, pooled=True)
            if squared:
                sub = (sub - m).square_()  # the chunk's one temporary
            mean[a:b], sd[a:b] = m.cpu().numpy(), np.sqrt(v.cpu().numpy())
            ess[a:b] = self.engine.store_rhat_ess(sub)[1].cpu().numpy()
        return mean, sd, ess

    @staticmethod
    def _probs(prob, method):
        """(prob_lo or None, prob_hi, squeeze) of the `prob` of ess / mcse"""
        if prob is None:
            raise ValueError(f'method="{method}" needs prob')
        p = np.asarray(prob, dtype=np.float64)
        if method == "local":
            if p.ndim not in (1, 2) or p.shape[-1] != 2 or p.size < 2:
                raise ValueError('method="local" takes prob = (lo, hi) or a sequence of such pairs')
            pairs = p.reshape(-1, 2)
            if not np.all((pairs[:, 0] >= 0) & (pairs[:, 0] <= pairs[:, 1]) & (pairs[:, 1] <= 1)):
                raise ValueError("every pair must satisfy 0 <= lo <= hi <= 1")
            return pairs[:, 0].copy(), pairs[:, 1].copy(), p.ndim == 1
        if p.ndim > 1 or p.size < 1:
            raise ValueError("prob must be a number or a non-empty one-dimensional sequence")
        flat = np.atleast_1d(p)
        if not np.all((flat >= 0) & (flat <= 1)):
            raise ValueError("every prob must lie inside [0, 1]")
        return None, flat, p.ndim == 0

    def ess(self, key, method="bulk", prob=None, index=None):
        """Effective sample size of store[key], computed on the device (no gather of the store): the family of ArviZ's
        az.ess(method=...), a host array (n_idx,).  "bulk" and "tail" are those of `rank_diagnostics`; "mean" the ESS of the
        draws (`diagnostics`); "sd" that of (x - pooled mean)^2; "quantile" the ESS of the indicator x <= q_prob -- whether a
        reported quantile has converged --, with prob a number or a sequence (then (n_prob, n_idx)); "median" is quantile 0.5;
        "local" the ESS of q_lo <= x <= q_hi for prob = (lo, hi) or a sequence of pairs (then (n_pairs, n_idx)): np.linspace
        pairs give the profile of az.plot_ess(kind="local"), twenty probabilities that of kind="quantile".  The quantiles are
        np.quantile of the split draws (first and last n_iter // 2 iterations of every chain).  index selects elements (in that
        order, repeats allowed); a 2-D entry ("log_post") counts as one element.  An element with a NaN or infinite draw gives
        NaN.  "quantile", "median", "local", "bulk" and "tail" sort every element: meant for the elements one inspects.  Under
        a sharded multi-GPU run these are this rank's chains only."""
        self._whole_store_on_device("ess")
        if method in ("bulk", "tail"):
            return self.rank_diagnostics(key, index=index)["ess_" + method]
        if method in ("mean", "sd"):
            return self._mean_sd_ess(key, index, squared=method == "sd")[2]
        if method == "median":
            prob = 0.5
        elif method not in ("quantile", "local"):
            raise ValueError(f"unknown method {method!r}: one of bulk, tail, mean, sd, quantile, median, local")
        lo, hi, squeeze = self._probs(prob, method)
        out = self.engine.store_ess_indicator(self._store_3d(key), lo, hi, index=index)[0].cpu().numpy()
        return out[0] if squeeze else out

    def mcse(self, key, method="mean", prob=None, index=None):
        """Monte Carlo standard error of a posterior summary of store[key], computed on the device (no gather of the store): the
        family of ArviZ's az.mcse(method=...), a host array (n_idx,).  "mean": sd / sqrt(ess_mean), sd the pooled standard
        deviation (ddof 1); "sd": sd sqrt(e (1 - 1 / ess_sd)^(ess_sd - 1) - 1); "quantile" (prob a number, or a sequence: then
        (n_prob, n_idx)) and "median": half the distance between the order statistics of the split draws at the 16 % and 84 %
        points of Beta(ess p + 1, ess (1 - p) + 1), ess = ess(method="quantile", prob=p) -- the beta quantiles on the host, the
        order statistics on the device.  index as in `ess`.  An element with a NaN or infinite draw gives NaN.  Under a sharded
        multi-GPU run these are this rank's chains only."""
        self._whole_store_on_device("mcse")
        if method in ("mean", "sd"):
            _, sd, ess = self._mean_sd_ess(key, index, squared=method == "sd")
            if method == "mean":
                return sd / np.sqrt(ess)
            return sd * np.sqrt(np.exp(1.0) * (1.0 - 1.0 / ess) ** (ess - 1.0) - 1.0)
        if method == "median":
            prob = 0.5
        elif method != "quantile":
            raise ValueError(f"unknown method {method!r}: one of mean, sd, quantile, median")
        from scipy import stats

        _, p, squeeze = self._probs(prob, method)
        t = self._store_3d(key)
        S = 2 * t.shape[1] * (t.shape[0] // 2)
        ess = self.engine.store_ess_indicator(t, None, p, index=index)[0].cpu().numpy()  # (n_p, n_idx)
        bad = ~np.isfinite(ess)
        e = np.where(bad, 1.0, ess)
        a = stats.beta.ppf(0.1586553, e * p[:, None] + 1, e * (1 - p[:, None]) + 1)
        b = stats.beta.ppf(0.8413447, e * p[:, None] + 1, e * (1 - p[:, None]) + 1)
        lower = np.floor(np.maximum(a * S - 1, 0)).astype(np.int64)
        upper = np.ceil(np.minimum(b * S - 1, S - 1)).astype(np.int64)
        pos = np.ascontiguousarray(np.concatenate([lower, upper], axis=0).T)  # (n_idx, 2 n_p)
        x = self.engine.store_order_stats(t, pos, index=index, split=True).cpu().numpy().T  # (2 n_p, n_idx)
        out = (x[p.size:] - x[:p.size]) / 2
        out[bad] = np.nan
        return out[0] if squeeze else out

    def summarize(self, key, index=None, hdi_prob=0.94):
        """The columns of az.summary for store[key], computed on the device (no gather of the store): a dict of host arrays
        (n_idx,) -- "mean", "sd" (pooled, ddof 1), "hdi_lo", "hdi_hi" (`hdi` at hdi_prob), "mcse_mean", "mcse_sd" (`mcse`),
        "ess_bulk", "ess_tail", "r_hat" (`rank_diagnostics`).  index as in `ess`.  Under a sharded multi-GPU run these are this
        rank's chains only."""
        self._whole_store_on_device("summarize")
        mean, sd, ess_mean = self._mean_sd_ess(key, index, squared=False)
        hdi = self.hdi(key, prob=float(hdi_prob), index=index)
        rank = self.rank_diagnostics(key, index=index)
        return {"mean": mean, "sd": sd, "hdi_lo": hdi[:, 0], "hdi_hi": hdi[:, 1], "mcse_mean": sd / np.sqrt(ess_mean),
                "mcse_sd": self.mcse(key, method="sd", index=index), "ess_bulk": rank["ess_bulk"], "ess_tail": rank["ess_tail"],
                "r_hat": rank["rhat"]}

    def ranks(self, key, index=None, split=False):
        """Average ranks of the stored draws of every selected element of store[key] among all chains and iterations
        (scipy.stats.rankdata(method="average") per element), computed on the device: a host array (n_iter, C, n_idx), the
        store's own layout -- ranks[:, c, i] is what a rank histogram of chain c shows.  split=True ranks among the split
        draws the diagnostics use (NaN in the dropped middle row of an odd n_iter).  An element with a NaN draw gives NaN."""
        self._whole_store_on_device("ranks")
        return self.engine.store_ranks(self._store_3d(key), index=index, split=split).cpu().numpy()

    def hdi(self, key, prob=0.94, index=None, pooled=True, omit_nan=True):
        """Highest-density intervals of store[key], computed on the device (no gather of the store): per element the
        shortest interval between two stored draws that holds floor(prob * n) + 1 of its n draws -- ArviZ's default
        (unimodal) hdi, what az.summary prints as hdi_3% / hdi_97% at prob = 0.94.  For a skewed posterior it differs
        visibly from the equal-tailed interval of `quantiles`.  A host array (n_prob, n_idx, 2) pooled over chains and
        iterations, else (n_prob, C, n_idx, 2) per chain, [..., 0] the lower and [..., 1] the upper limit; for a scalar prob
        the leading axis is dropped.  Any number of probabilities, each inside (0, 1).  index selects elements (in that
        order, repeats allowed); a 2-D entry ("log_post") counts as one element.  omit_nan: the NaN padding of variable-size
        parameters is left out; False gives NaN for a column with a NaN.  A column with an infinite draw or without a valid
        draw gives NaN.  Every column is sorted: meant for the elements one inspects.  Under a sharded multi-GPU run these
        are intervals of this rank's chains only."""
        self._whole_store_on_device("hdi")
        probs = np.asarray(prob, dtype=np.float64)
        if probs.ndim > 1 or probs.size < 1:
            raise ValueError("prob must be a number or a non-empty one-dimensional sequence")
        flat = np.atleast_1d(probs)
        t = self._store_3d(key)
        parts = [self.engine.store_hdi(t, flat[i: i + 8], index=index, pooled=pooled, omit_nan=omit_nan)[0].cpu().numpy()
                 for i in range(0, flat.size, 8)]  # at most 8 probabilities per call of omc_store_hdi
        out = np.concatenate(parts, axis=0)
        return out[0] if probs.ndim == 0 else out

    def derive(self, key, reduce, index=None, weights=None, threshold=None, center=None, scale=None, omit_nan=True, name=None):
        """A per-draw derived quantity of store[key], computed on the device (one read of the store, no gather): every stored
        state (iteration, chain) is reduced over the selected elements of its row, as Stan's generated quantities are -- a
        host array (n_iter, C), shaped like log_post.  reduce, with x the elements at the selected positions:
        "sum" (np.nansum; with weights w the contrast or regional total sum of w[k] * x[k]), "mean" (np.nanmean: sum / count,
        NaN where nothing is left), "count" (the elements that are not NaN: the live size of a variable-size parameter),
        "min", "max", "argmin", "argmax" (the position in the selection of the first extreme), "count_above" (the number with
        x[k] > threshold[k]: the area above a level), "supnorm" (the largest |x[k] - center[k]| / scale[k]; a term 0 / 0 counts as
        NaN).  weights, threshold, center and scale are scalars or hold one value per SELECTED element.  index selects
        elements (in that order, repeats allowed); a 2-D entry ("log_post") counts as one element.  omit_nan: NaN terms (the
        padding of variable-size parameters) are left out; False propagates them like numpy's plain reductions ("argmin" /
        "argmax" then give the first NaN).  "sum" and "mean" are within n 2^-53 sum|terms| of the exact sum, the rest is exact.
        With name the device result is kept as store[name], shaped (n_iter, C, 1): `summary`, `quantiles`, `diagnostics`,
        `rank_diagnostics`, `hdi`, `histogram` ... accept it as a key (R-hat and ESS of a derived quantity), and `collect()` /
        `gather()` carry it as a scalar parameter (C, 1, n_iter).  A derived entry describes the store AT THE TIME OF THE CALL:
        it is not updated by a later run.  A name may be derived again, but a name that is a store entry of the run raises
        ValueError.  Under a sharded multi-GPU run every rank must derive the same names before `gather`."""
        self._whole_store_on_device("derive")
        if name is not None and name in self.store and name not in self._derived:
            raise ValueError(f"{name!r} is a store entry of the run: choose another name for the derived quantity")
        ops = {"sum": "sum", "mean": "sum", "count": "sum", "min": "min", "max": "max", "argmin": "argmin", "argmax": "argmax",
               "count_above": "count_above", "supnorm": "supnorm"}
        if reduce not in ops:
            raise ValueError(f"unknown reduce {reduce!r}: one of {', '.join(ops)}")
        takes = {"sum": ("weights",), "mean": ("weights",), "count_above": ("threshold",), "supnorm": ("center", "scale")}
        given = {"weights": weights, "threshold": threshold, "center": center, "scale": scale}
        for arg, v in given.items():
            if v is not None and arg not in takes.get(reduce, ()):
                raise ValueError(f"{arg} does not apply to reduce={reduce!r}")
        a = {"sum": weights, "mean": weights, "count_above": threshold, "supnorm": center}.get(reduce)
        out, cnt = self.engine.store_reduce(self._store_3d(key), ops[reduce], index=index, omit_nan=omit_nan, a=a, b=scale)
        if reduce == "count":
            out = cnt.to(out.dtype)
        elif reduce == "mean":
            out = out / cnt  # (0 / 0: NaN where no term is left)
        if name is not None:
            self.store[name] = out.unsqueeze(-1).contiguous()
            self._derived.add(name)
        return out.cpu().numpy()

    def project(self, key, matrix, index=None, offset=None, base=None, omit_nan=True, name=None, noise_precision=None, replicate=0):
        """Linear maps of store[key], computed on the device (one read of the store for up to 128 outputs, no gather): every
        stored state (iteration, chain) gives m numbers, out[it, c, j] = base[it, c, j] + offset[j] + sum_k matrix[j, k] * x[k]
        with x the elements at the selected positions of its row -- the fitted curve A beta at the observations or on a new grid,
        a set of contrasts or regional totals, the predictor of a variable-size parameter summed over its live components.  A
        host array (n_iter, C, m), the store's own layout.  matrix is (m, n_idx), host array or device tensor, a 1-D matrix one
        output; offset holds m values.  index selects elements (in that order, repeats allowed); a 2-D entry ("log_post")
        counts as one element.  base and noise_precision are store keys: base an entry of m elements that is added,
        noise_precision an entry of 1 or m elements tau, with which z / sqrt(tau) is added for z ~ N(0, 1) -- the
        posterior-predictive replicate y_rep = A beta + eps / sqrt(tau) of every stored draw.  z is element j of the chain's own
        normal stream under a draw index no sweep uses, one stream per replicate 0 .. 15: the same seed gives the same
        replicates, also when the chains are sharded over GPUs.  omit_nan: NaN elements (the padding of variable-size
        parameters: "component absent") are left out, their terms are 0, and a row with nothing left gives base + offset;
        False follows IEEE as numpy's matmul does (a NaN element makes the row's m outputs NaN).  The linear part is within
        (n_idx + 2) 2^-53 (|base| + |offset| + sum|terms|) of the exact value.
        With name the result stays on the device as store[name], shaped (n_iter, C, m), and None is returned (the entry can be
        as large as the store: no silent transfer): `summary`, `quantiles`, `hdi`, `diagnostics`, `simultaneous_band`,
        `histogram` ... accept it as a key (pointwise intervals and a simultaneous band of a fitted curve, R-hat and ESS of a
        prediction), and `collect()` / `gather()` carry it as a vector parameter (C, m, n_iter).  base=name with the same name
        accumulates in place, the way to add the blocks of one mean: project("beta", A, name="f"); project("gamma", B, base="f",
        name="f").  A projected entry describes the store AT THE TIME OF THE CALL; a name may be made again, but a name that is
        a store entry of the run raises ValueError.  Under a sharded multi-GPU run every rank must make the same names before
        `gather`."""
        self._whole_store_on_device("project")
        if name is not None and name in self.store and name not in self._derived:
            raise ValueError(f"{name!r} is a store entry of the run: choose another name for the projected quantity")
        if name is not None and base == name and key == name:
            raise ValueError(f"{name!r} cannot be accumulated into while it is the entry the map reads")
        t = self._store_3d(key)
        b = None if base is None else self._store_3d(base)
        prec = None if noise_precision is None else self._store_3d(noise_precision)
        out = b if (base is not None and base == name) else None  # accumulate in place
        out = self.engine.store_project(t, matrix, index=index, offset=offset, base=b, omit_nan=omit_nan, prec=prec,
                                        replicate=replicate, out=out)
        if name is None:
            return out.cpu().numpy()
        self.store[name] = out
        self._derived.add(name)
        return None

    def _predictive_precision(self, dist, m, what="posterior_predictive"):
        """store key of the noise precision of a Normal response of m elements: an entry of 1 or m elements"""
        from openmcmc_amd.parameter import Identity

        prec = dist.precision
        if isinstance(prec, Identity):
            scalar, diag = prec.form, None
        elif isinstance(prec, ScaledMatrix):
            M = self.state[prec.matrix]
            M = sparse.csr_matrix(M) if not sparse.issparse(M) else M.tocsr()
            diag = np.asarray(M.diagonal(), dtype=np.float64)
            if M.shape != (m, m) or (M - sparse.diags(diag)).count_nonzero():
                raise NotImplementedError(f"{what}: the precision matrix {prec.matrix!r} is not diagonal")
            scalar = prec.scalar
            if np.all(diag == 1.0):
                diag = None
        else:
            raise NotImplementedError(f"{what}: a precision of type {type(prec).__name__}")
        if scalar in self.store:
            t = self._store_3d(scalar)
            key = scalar
        else:  # a constant of the state, broadcast to a device entry once
            key = f"_precision_{scalar}"
            if key not in self._derived:
                v = self.state[scalar]
                if sparse.issparse(v) or is_chain(v):
                    raise NotImplementedError(f"{what}: the precision {scalar!r} is neither stored nor a constant vector")
                v = np.asarray(v, dtype=np.float64)
                if v.size != max(v.shape, default=1):
                    raise NotImplementedError(f"{what}: the precision {scalar!r} is a matrix")
                self.store[key] = self.engine.to_device(v.reshape(-1)).expand(self._n_dev, self.n_chains, v.size).contiguous()
                self._derived.add(key)
            t = self.store[key]
        if t.shape[2] not in (1, m):
            raise NotImplementedError(f"{what}: the precision {scalar!r} holds {t.shape[2]} values, the response {m}")
        if diag is None:
            return key
        key = f"_precision_of_{dist.response}"  # the scalar times the matrix's diagonal, made anew by every call
        self.store[key] = (t * self.engine.to_device(diag)).contiguous()
        self._derived.add(key)
        return key

    def _normal_response(self, response, what):
        """(dist, blocks, m) of a Normal response whose mean the store holds: blocks [(stored parameter, shared design matrix as
        a dense host array)], or [(stored parameter, None)] for a mean that is the entry itself; m its length.  What
        `posterior_predictive`, `log_likelihood`, `waic` and `loo` can read of a model; anything else raises NotImplementedError
        naming the part."""
        from openmcmc_amd.distribution.location_scale import Normal
        from openmcmc_amd.parameter import Identity, LinearCombinationWithTransform

        self._whole_store_on_device(what)
        dist = self.model[response]
        if type(dist) is not Normal:
            raise NotImplementedError(f"{what}: a response of type {type(dist).__name__}")
        mean = dist.mean
        if isinstance(mean, Identity):
            if mean.form not in self.store:
                raise NotImplementedError(f"{what}: the mean {mean.form!r} is not in the store")
            blocks = [(mean.form, None)]
        elif isinstance(mean, LinearCombinationWithTransform):
            raise NotImplementedError(f"{what}: a mean of type LinearCombinationWithTransform")
        elif isinstance(mean, LinearCombination):
            blocks = []
            for prm, prefactor in mean.form.items():
                if prm not in self.store:
                    raise NotImplementedError(f"{what}: the term {prm!r} is not in the store")
                A = self.state[prefactor]
                if is_chain(A):
                    raise NotImplementedError(f"{what}: the design matrix {prefactor!r} is per chain")
                blocks.append((prm, A.toarray() if sparse.issparse(A) else np.asarray(A, dtype=np.float64)))
        else:
            raise NotImplementedError(f"{what}: a mean of type {type(mean).__name__}")
        identity = blocks[0][1] is None
        m = self._store_3d(blocks[0][0]).shape[2] if identity else blocks[0][1].shape[0]
        return dist, blocks, m

    def posterior_predictive(self, response, name=None, replicate=0, noise=True):
        """Posterior-predictive replicates of a Normal response of the model, one per stored draw, computed on the device:
        y_rep = mean + eps / sqrt(precision) with the mean and the precision of self.model[response] evaluated at every stored
        state -- what Normal.rvs of the reference gives in a loop over the store.  noise=False gives the fitted values (the
        mean alone).  Supported: a mean that is a stored parameter (Identity) or a LinearCombination of stored parameters with
        shared design matrices in the state (dense or scipy-sparse, densified); a precision that is a stored or constant scalar
        or vector of the response's length (Identity), or a scalar times a diagonal matrix (ScaledMatrix).  Anything else
        raises NotImplementedError naming the part: per-chain designs, LinearCombinationWithTransform, precisions that are
        not diagonal, a term that is not in the store.  name, replicate, the layout (n_iter, C, m), the NaN rule (padding
        left out) and the sharding remark as `project`, which does the work.  A constant precision is
        broadcast once to the store entry "_precision_<its name>", a scalar times a diagonal to "_precision_of_<response>"."""
        dist, blocks, m = self._normal_response(response, "posterior_predictive")
        identity = blocks[0][1] is None
        prec_key = self._predictive_precision(dist, m) if noise else None
        work = name if name is not None else f"_predictive_of_{response}"
        if work in self.store and work not in self._derived:
            raise ValueError(f"{work!r} is a store entry of the run: choose another name for the replicates")
        if identity:  # the entry itself is the mean: it goes in as the base of a map with zero weights on its first element
            # (NaN padding stays NaN as the base carries it; an infinite first element would make its draw's row NaN by inf * 0)
            self.project(blocks[0][0], np.zeros((m, 1)), index=[0], base=blocks[0][0], name=work, noise_precision=prec_key,
                         replicate=replicate)
        for i, (prm, A) in enumerate(blocks if not identity else []):  # the noise goes in with the last block
            last = i == len(blocks) - 1
            self.project(prm, A, base=work if i else None, name=work, noise_precision=prec_key if last else None, replicate=replicate)
        if name is not None:
            return None
        self._derived.discard(work)
        return self.store.pop(work).cpu().numpy()

    pointwise_work_bytes = 1 << 30  # the work entry of a LinearCombination mean in log_likelihood / waic / loo: observations per chunk

    def _pointwise_chunks(self, response, what):
        """The pointwise Normal log-density of self.model[response] as the library reads it: yields (j0, j1, m, mean, y, prec) per
        chunk [j0, j1) of the m observations -- mean a device entry (n_iter, C, j1 - j0) of the fitted mean of every stored draw,
        y the observations (host, (j1 - j0,)), prec a device entry (n_iter, C, 1) or (n_iter, C, j1 - j0).  An Identity mean is the
        store entry itself, in one chunk; a LinearCombination goes through store_project in chunks of observations whose work
        entry stays within pointwise_work_bytes."""
        dist, blocks, m = self._normal_response(response, what)
        y = self.state[response]
        if is_chain(y):
            raise NotImplementedError(f"{what}: the response {response!r} is per chain")
        y = np.asarray(y.toarray() if sparse.issparse(y) else y, dtype=np.float64)
        if y.ndim > 1 and y.shape[1] != 1:
            raise NotImplementedError(f"{what}: the response {response!r} is replicated ({y.shape[1]} columns)")
        y = y.reshape(-1)
        if y.size != m:
            raise NotImplementedError(f"{what}: the response {response!r} holds {y.size} values, its mean {m}")
        prec = self.store[self._predictive_precision(dist, m, what)]
        if blocks[0][1] is None:
            yield 0, m, m, self._store_3d(blocks[0][0]), y, prec
            return
        rows = self._n_dev * self.n_chains
        step = max(1, int(self.pointwise_work_bytes) // (8 * rows))
        for j0 in range(0, m, step):
            j1 = min(m, j0 + step)
            work = None
            for prm, A in blocks:
                work = self.engine.store_project(self._store_3d(prm), A[j0:j1], base=work, out=work)
            yield j0, j1, m, work, y[j0:j1], prec if prec.shape[2] == 1 else prec[:, :, j0:j1].contiguous()

    def log_likelihood(self, response, name=None):
        """The pointwise log-likelihood of a Normal response of the model, computed on the device: for every stored draw and every
        observation i, log N(y_i | mean_i, 1 / precision_i) with the mean and the precision of self.model[response] evaluated at
        that draw -- what Normal.log_p(..., by_observation=True) of the reference gives in a loop over the store, and what
        ArviZ keeps as the log_likelihood group.  A host array (n_iter, C, m), the store's own layout; with name the entry stays
        on the device as store[name] and None is returned, under the rules of `project(name=...)`: `summary`, `quantiles`,
        `diagnostics` ... accept it as a key, `collect()` / `gather()` carry it.  The models read are those of
        `posterior_predictive` (a mean that is a stored parameter or a LinearCombination of stored parameters with shared
        designs; a stored or constant scalar or vector precision, or a scalar times a diagonal matrix), with observations
        state[response] shared across chains in one column; anything else raises NotImplementedError naming the part.  Under
        a sharded multi-GPU run these are this rank's chains only."""
        if name is not None and name in self.store and name not in self._derived:
            raise ValueError(f"{name!r} is a store entry of the run: choose another name for the log-likelihood")
        out = None
        for j0, j1, m, mean, y, prec in self._pointwise_chunks(response, "log_likelihood"):
            ll = self.engine.store_loglik(mean, y, prec, lse=False, mean=False, var=False, ll=True)[3]
            if (j0, j1) == (0, m):
                out = ll
            else:
                if out is None:
                    out = self.engine.empty(self._n_dev, self.n_chains, m)
                out[:, :, j0:j1] = ll
        if name is None:
            return out.cpu().numpy()
        self.store[name] = out
        self._derived.add(name)
        return None

    def waic(self, response, pointwise=False):
        """The widely applicable information criterion of a Normal response of the model (Watanabe 2010; az.waic), computed on
        the device without writing the pointwise log-likelihood: a dict with "elpd_waic", "se", "p_waic", "lppd" (floats) and
        "n_high_var".  With S = n_iter * C stored draws and ll_si the log-likelihood of observation i under draw s:
        lppd_i = logsumexp_s(ll_si) - log S, p_i = the unbiased variance of ll_si over s, elpd_i = lppd_i - p_i; the totals are
        sums over the m observations, se = sqrt(m * np.var(elpd_i)), and n_high_var is the number of p_i > 0.4 (where WAIC is
        unreliable: use `loo`).  Higher elpd_waic predicts better; pointwise=True adds the arrays "elpd_i", "p_i" and
        "lppd_i" (m,).  The models read and the sharding remark as `log_likelihood`.  An observation with a log-likelihood that
        is not finite under some draw gives NaN."""
        lse = var = None
        for j0, j1, m, mean, y, prec in self._pointwise_chunks(response, "waic"):
            if lse is None:
                lse, var = np.empty(m), np.empty(m)
            a, _, b, _ = self.engine.store_loglik(mean, y, prec, lse=True, mean=False, var=True)
            lse[j0:j1], var[j0:j1] = a.cpu().numpy(), b.cpu().numpy()
        lppd_i = lse - np.log(self._n_dev * self.n_chains)
        elpd_i = lppd_i - var
        out = {"elpd_waic": float(elpd_i.sum()), "se": float(np.sqrt(m * np.var(elpd_i))), "p_waic": float(var.sum()),
               "lppd": float(lppd_i.sum()), "n_high_var": int(np.sum(var > 0.4))}
        if pointwise:
            out.update({"elpd_i": elpd_i, "p_i": var, "lppd_i": lppd_i})
        return out

    def loo(self, response, pointwise=False, reff=1.0):
        """Pareto-smoothed importance-sampling leave-one-out cross-validation of a Normal response of the model (Vehtari et
        al. 2024; az.loo), computed on the device without writing the pointwise log-likelihood: a dict with "elpd_loo", "se",
        "p_loo" (floats), "pareto_k" (m,), "n_bad_k" and "tail" (m,).  Per observation the importance ratios 1 / p(y_i | draw) of
        the S = n_iter * C stored draws are sorted, a generalised Pareto distribution is fitted to their upper tail (Zhang and
        Stephens 2009) and the tail replaced by the fit's expected order statistics; elpd_i is the log of the weighted mean
        likelihood, elpd_loo their sum, se = sqrt(m * np.var(elpd_i)), p_loo = lppd - elpd_loo.  pareto_k is the fit's shape: the
        estimate of an observation with k > 0.7 is unreliable, n_bad_k counts them; k is +inf where the tail holds 4 draws or
        fewer.  tail is the number of draws in each tail, at most ceil(min(S / 5, 3 sqrt(S / reff))); reff, a scalar or one value
        per observation, is the relative efficiency of the draws (ess / S of `diagnostics`).  pointwise=True adds "elpd_i" and
        "lppd_i".  The models read and the sharding remark as `log_likelihood`.  An observation with a log-likelihood that is
        not finite under some draw gives NaN, and -1 in tail."""
        S = self._n_dev * self.n_chains
        lse = None
        for j0, j1, m, mean, y, prec in self._pointwise_chunks(response, "loo"):
            if lse is None:
                tail_max = self._loo_tail_max(reff, m)
                lse, elpd_i, k, tail = np.empty(m), np.empty(m), np.empty(m), np.empty(m, dtype=np.int64)
            lse[j0:j1] = self.engine.store_loglik(mean, y, prec, lse=True, mean=False, var=False)[0].cpu().numpy()
            e, kk, t = self.engine.store_psis(mean, tail_max[j0:j1], y=y, prec=prec)
            elpd_i[j0:j1], k[j0:j1], tail[j0:j1] = e.cpu().numpy(), kk.cpu().numpy(), t.cpu().numpy()
        lppd_i = lse - np.log(S)
        out = {"elpd_loo": float(elpd_i.sum()), "se": float(np.sqrt(m * np.var(elpd_i))), "p_loo": float(lppd_i.sum() - elpd_i.sum()),
               "pareto_k": k, "n_bad_k": int(np.sum(k > 0.7)), "tail": tail}
        if pointwise:
            out.update({"elpd_i": elpd_i, "lppd_i": lppd_i})
        return out

    def _loo_tail_max(self, reff, m):
        """the longest tail of each of the m observations, ceil(min(S / 5, 3 sqrt(S / reff))) within 1 .. S - 1"""
        S = self._n_dev * self.n_chains
        r = np.asarray(reff, dtype=np.float64).reshape(-1)
        r = np.broadcast_to(r, (m,)) if r.size == 1 else r
        if r.shape != (m,) or not np.all(r > 0):
            raise ValueError(f"reff must be a positive number or hold one per observation ({m})")
        return np.clip(np.ceil(np.minimum(S / 5.0, 3.0 * np.sqrt(S / r))), 1, S - 1).astype(np.int64)

    def _loo_expect(self, what, response, reff, f, want, values=None, index=None, threshold=None, lw=False):
        """omc_store_loo_expect over the chunks of `_pointwise_chunks`: ({name: host array (m,)}, the observations (m,), the
        device entry (n_iter, C, m) of the log weights or None).  values is a store key (f = "entry"), index selects m of its
        elements, threshold is a scalar, holds one value per observation, or is True for the observations themselves."""
        out = lw_out = ys = None
        for j0, j1, m, mean, y, prec in self._pointwise_chunks(response, what):
            if out is None:
                tail_max = self._loo_tail_max(reff, m)
                out = {w: np.empty(m, dtype=np.int64 if w == "tail" else np.float64) for w in want}
                ys = np.empty(m)
                vt = vi = thr = None
                if values is not None:
                    vt = self._store_3d(values)
                    if index is not None:
                        vi = np.asarray(index)
                        if vi.ndim != 1 or (vi.size and vi.dtype.kind not in "iu"):
                            raise ValueError("index must be a one-dimensional sequence of integers")
                    if (vt.shape[2] if vi is None else vi.size) != m:
                        raise ValueError(f"{values!r} holds or selects {vt.shape[2] if vi is None else vi.size} elements, the "
                                         f"response {response!r} {m} observations")
                if threshold is not None and threshold is not True:
                    thr = np.asarray(threshold, dtype=np.float64).reshape(-1)
                    thr = np.broadcast_to(thr, (m,)) if thr.size == 1 else thr
                    if thr.shape != (m,):
                        raise ValueError(f"threshold must be a number or hold one per observation ({m})")
            whole = (j0, j1) == (0, m)
            sel = None
            if vt is not None and not (whole and vi is None):
                sel = np.arange(j0, j1) if vi is None else vi[j0:j1]
            got = self.engine.store_loo_expect(mean, tail_max[j0:j1], y=y, prec=prec, f=f, values=vt, values_index=sel,
                                               threshold=y if threshold is True else None if thr is None else thr[j0:j1], want=want,
                                               lw=lw)
            ys[j0:j1] = y
            for w in want:
                out[w][j0:j1] = got[w].cpu().numpy()
            if lw and whole:
                lw_out = got["lw"]
            elif lw:
                if lw_out is None:
                    lw_out = self.engine.empty(self._n_dev, self.n_chains, m)
                lw_out[:, :, j0:j1] = got["lw"]
        return out, ys, lw_out

    def loo_expectation(self, response, values, index=None, threshold=None, reff=1.0):
        """Leave-one-out expectations of a stored quantity under the PSIS weights of a Normal response of the model, computed on
        the device (omc_store_loo_expect; neither the pointwise log-likelihood nor the weights are written): a dict of host
        arrays (m,) -- "mean" and "sd", the weighted mean and population standard deviation of store[values][..., i] over the
        stored draws with observation i left out, "ess" the effective sample size of the weights (sum w)^2 / sum w^2,
        "pareto_k" as `loo`, and with a threshold "below", the weighted share of draws with value <= threshold[i].  What a loop of
        weighted averages over az.psislw(-log_likelihood) gives.  values is a store key whose last dimension matches the m
        observations, or of which index selects m elements (in that order, repeats allowed); threshold a number or one per
        observation.  Every draw has the smoothed weight of its position among the sorted importance ratios; tied tail draws
        share theirs evenly.  reff as `loo`.  The models read and the sharding remark (this rank's chains only) as
        `log_likelihood`.  An observation with a log-likelihood that is not finite under some draw gives NaN; a value that is
        not finite gives what IEEE gives in "mean" and "sd" and leaves "ess" and "pareto_k" alone."""
        want = ("mean", "var", "ess", "k") + (("below",) if threshold is not None else ())
        got, _, _ = self._loo_expect("loo_expectation", response, reff, "entry", want, values=values, index=index, threshold=threshold)
        out = {"mean": got["mean"], "sd": np.sqrt(got["var"]), "ess": got["ess"], "pareto_k": got["k"]}
        if threshold is not None:
            out["below"] = got["below"]
        return out

    def loo_predictive(self, response, reff=1.0):
        """Leave-one-out predictive means and standard deviations of a Normal response of the model, computed on the device
        (omc_store_loo_expect, one pass): a dict with "mean" (m,), E_loo[mu_i], the PSIS-weighted mean of the fitted mean of
        observation i with that observation left out; "sd" (m,), sqrt(E_loo[1 / precision_i] + Var_loo[mu_i]), the standard
        deviation of the leave-one-out predictive distribution; "residual" = y - mean; "z" = residual / sd; "r2", the LOO-R^2
        1 - np.var(residual) / np.var(y) (a float); and "pareto_k" (m,) as `loo`.  reff as `loo`; the models read and the
        sharding remark (this rank's chains only) as `log_likelihood`.  An observation with a log-likelihood that is not
        finite under some draw gives NaN (and a NaN "r2")."""
        got, y, _ = self._loo_expect("loo_predictive", response, reff, "mean", ("mean", "var", "invprec", "k"))
        sd = np.sqrt(got["invprec"] + got["var"])
        res = y - got["mean"]
        return {"mean": got["mean"], "sd": sd, "residual": res, "z": res / sd, "r2": float(1.0 - np.var(res) / np.var(y)),
                "pareto_k": got["k"]}

    def loo_pit(self, response, y_rep=None, reff=1.0):
        """Leave-one-out probability integral transform of a Normal response of the model (az.loo_pit), computed on the
        device: a host array (m,), uniform on [0, 1] for a calibrated model.  With y_rep=None the analytic value, the
        PSIS-weighted mean over the stored draws of the Normal distribution function of observation i under the draw's mean
        and precision; with y_rep a store key made by `posterior_predictive(name=...)` the weighted share of replicates
        y_rep[..., i] <= y_i, az.loo_pit's own definition.  reff as `loo`; the models read and the sharding remark (this rank's
        chains only) as `log_likelihood`.  An observation with a log-likelihood that is not finite under some draw gives
        NaN; a NaN replicate counts as not below."""
        if y_rep is None:
            return self._loo_expect("loo_pit", response, reff, "cdf", ("mean",))[0]["mean"]
        return self._loo_expect("loo_pit", response, reff, "entry", ("below",), values=y_rep, threshold=True)[0]["below"]

    def loo_weights(self, response, name=None, reff=1.0):
        """The normalised Pareto-smoothed log importance weights of a Normal response of the model (the first result of
        az.psislw(-log_likelihood)), computed on the device: a host array (n_iter, C, m), the store's own layout, whose
        exponentials sum to 1 over the draws of every observation -- the weights with which any other stored quantity is
        averaged leave-one-out.  With name the entry stays on the device as store[name] and None is returned, under the rules
        of `log_likelihood(name=...)`.  Tied tail draws share the weight of their sorted positions evenly.  reff as `loo`; the
        models read and the sharding remark (this rank's chains only) as `log_likelihood`.  An observation with a
        log-likelihood that is not finite under some draw gives a NaN column."""
        if name is not None and name in self.store and name not in self._derived:
            raise ValueError(f"{name!r} is a store entry of the run: choose another name for the weights")
        lw = self._loo_expect("loo_weights", response, reff, "mean", (), lw=True)[2]
        if name is None:
            return lw.cpu().numpy()
        self.store[name] = lw
        self._derived.add(name)
        return None

    def simultaneous_band(self, key, prob=0.95, index=None):
        """A simultaneous credible band of the selected elements of store[key], computed on the device (two reads of the
        store, no gather): a dict of host arrays "lower", "upper", "mean", "sd" of shape (n_idx,) and "critical" (a float).
        The band of the maximal standardised deviation, as the simultaneous bands of Ruppert, Wand and Carroll
        (Semiparametric Regression, 2003, section 6.5): with the pooled posterior mean and standard deviation (the root of
        the unbiased variance) of every element, m = max_k |x[k] - mean[k]| / sd[k] is taken in every stored draw,
        critical = np.quantile(m, prob) over all draws, and the band is mean -/+ critical * sd.  It holds WHOLE posterior curves
        with probability prob: a share prob of the stored draws lies inside it at every selected element at once.  The
        intervals of `hdi` and `quantiles` are pointwise -- each holds its own element's draws with probability prob -- and
        drawn as a band they cover a whole curve far less often; critical is accordingly larger than the pointwise normal
        quantile (1.96 at 0.95).  An element that never moved (sd = 0) or that holds a NaN draw (the padding of a
        variable-size parameter) does not enter m and gets a degenerate or NaN band of its own.  index selects elements (in
        that order, repeats allowed).  Under a sharded multi-GPU run this is the band of this rank's chains only."""
        self._whole_store_on_device("simultaneous_band")
        if not 0.0 < float(prob) < 1.0:
            raise ValueError("prob must lie inside (0, 1)")
        t = self._store_3d(key)
        mean, var = self.engine.store_moments(t, pooled=True)
        idx, _ = self.engine._store_index(index, t.shape[2])
        if idx is not None:
            if int(idx.min()) < 0 or int(idx.max()) >= t.shape[2]:
                raise ValueError("index out of range")
            mean, var = mean[idx], var[idx]
        mean, sd = mean.cpu().numpy(), np.sqrt(var.cpu().numpy())  # (n_idx values: the root is numpy's, on the host)
        m, _ = self.engine.store_reduce(t, "supnorm", index=idx, a=mean, b=sd, omit_nan=True)
        critical = float(self.engine.store_quantiles(m.unsqueeze(-1).contiguous(), float(prob), pooled=True, omit_nan=True).cpu().numpy()[0, 0])
        return {"lower": mean - critical * sd, "upper": mean + critical * sd, "mean": mean, "sd": sd, "critical": critical}

    def autocorrelation(self, key, max_lag=None, index=None, pooled=True, normalize=True):
        """Autocorrelation function and integrated autocorrelation time of store[key], computed on the device (no gather of the
        store): a dict of host arrays "acf" (n_idx, max_lag + 1), "tau" (n_idx,) and "window" (n_idx,), or per chain
        (pooled=False) (C, n_idx, max_lag + 1), (C, n_idx), (C, n_idx).  The estimator: g(t) = sum_i (x_i - m)(x_{i+t} - m) / n_iter
        around each chain's own mean m, averaged over the chains when pooled, "acf" = g(t) / g(0) (normalize=False: g(t), the
        autocovariance), and tau = -1 + 2 sum of the pairs rho(2k) + rho(2k+1) while they are positive (Geyer's initial positive
        sequence).  ceil(tau) is the thinning at which stored draws are roughly independent: the way to choose n_thin.
        "window" is the number of lags the sum used; a window that reaches max_lag (max_lag - 1 for an even max_lag) means
        the sequence was cut off and tau is a lower bound: raise max_lag.  max_lag defaults to min(100, n_iter - 1).  index
        selects elements (in that order, repeats allowed); a 2-D entry ("log_post") counts as one element, and an entry made
        by derive(name=...) is a key like any other.  An element with a NaN or infinite draw gives NaN; one that never moved
        gives tau NaN and window 0.  Under a sharded multi-GPU run this summarises this rank's chains only."""
        self._whole_store_on_device("autocorrelation")
        t = self._store_3d(key)
        if max_lag is None:
            max_lag = min(100, t.shape[0] - 1)
        acf, tau, window, _ = self.engine.store_autocorr(t, max_lag, index=index, pooled=pooled, normalize=normalize)
        return {"acf": acf.cpu().numpy(), "tau": tau.cpu().numpy(), "window": window.cpu().numpy()}

    def _store_3d(self, key):
        t = self.store[key]
        return (t.unsqueeze(-1) if t.dim() == 2 else t.reshape(t.shape[0], t.shape[1], -1)).contiguous()

    def covariance(self, key, other=None, index=None, other_index=None, pooled=True, correlation=False):
        """Posterior covariance matrix of the elements of store[key] -- np.cov of the stored draws -- or, with `other`, of
        its elements against those of store[other] (the off-diagonal block of np.cov of the stacked variables), computed on
        the device (no gather of the store): pooled over chains and iterations -> (n_a, n_b), else per chain ->
        (C, n_a, n_b).  index / other_index select elements (in that order, repeats allowed); a 2-D entry ("log_post") counts
        as one element.  An element with a NaN draw (the padding of variable-size parameters) gives NaN in its row and
        column; a single stored draw gives 0.  Under a sharded multi-GPU run this is the covariance over this rank's
        chains only."""
        self._whole_store_on_device("covariance")
        a = self._store_3d(key)
        b = None if other is None else self._store_3d(other)
        return self.engine.store_cov(a, b, index_a=index, index_b=other_index, pooled=pooled, correlation=correlation).cpu().numpy()

    def correlation(self, key, other=None, index=None, other_index=None, pooled=True):
        """Posterior correlation matrix -- np.corrcoef of the stored draws: `covariance` scaled by the standard deviations
        and clipped to [-1, 1]; an element that never moved gives NaN in its row and column."""
        return self.covariance(key, other=other, index=index, other_index=other_index, pooled=pooled, correlation=True)

    def _allocation_labels(self, key, n_labels):
        """K of the allocation entry store[key]: n_labels, or the last dimension of the prob of the model's Categorical on key"""
        if n_labels is not None:
            return self.engine._n_labels(n_labels)
        from openmcmc_amd.distribution.distribution import Categorical

        dist = self.model.get(key) if self.model is not None else None
        if not isinstance(dist, Categorical):
            raise ValueError(f"'{key}' is not the response of a Categorical of the model: give n_labels")
        return self.engine._n_labels(np.shape(dist.prob.predictor(self.state))[-1])

    def _coallocation(self, key, n_labels, index, pooled, per_label):
        t = self._store_3d(key)
        K = self._allocation_labels(key, n_labels)
        counts, flags = self.engine.store_coalloc(t, K, index=index, pooled=pooled, per_label=per_label)
        flags = flags.cpu().numpy()
        if flags[..., 1].any():
            per_element = flags[..., 1].reshape(-1, flags.shape[-2]).sum(axis=0)
            first = int(np.flatnonzero(per_element)[0])
            el = first if index is None else int(self.engine._store_index(index, t.shape[2])[0][first])
            raise ValueError(f"'{key}' is not an allocation in [0, {K}): element {el} holds {int(per_element[first])} draws that are "
                             f"neither an integer label below {K} nor NaN")
        return t, K, counts, flags

    def coallocation(self, key, n_labels=None, index=None, pooled=True, per_label=False):
        """Posterior similarity (co-clustering) matrix of the allocation vector store[key] -- labels 0 .. K - 1 as MixtureAllocation
        draws them -- computed on the device (no gather of the store): a dict of host arrays "prob" (n, n) = P(z_i = z_j), the
        share of the stored draws in which elements i and j carry the same label, "counts" (int64, prob = counts / rows),
        "absent" (n,) the NaN draws of every element (the padding of variable-size parameters; such a draw matches nothing, so
        the diagonal of counts is rows - absent) and "rows"; per chain (pooled=False) (C, n, n), (C, n) and rows = n_iter.
        per_label=True: (K, n, n) or (C, K, n, n), entry (k, i, j) = P(z_i = k and z_j = k) -- for spike-and-slab the joint
        inclusion probability of two coefficients; its diagonal is the marginal P(z_i = k) and its sum over k the plain form.
        The matrix does not change when the labels are permuted (label switching), which mean, quantiles or kde of a label do.
        n_labels defaults to the number of categories of the model's Categorical on key.  A draw that is neither NaN nor an
        integer in [0, K) raises ValueError.  index selects elements (in that order, repeats allowed).  Under a sharded
        multi-GPU run these are this rank's chains only; counts of several ranks can simply be added."""
        self._whole_store_on_device("coallocation")
        t, _, counts, flags = self._coallocation(key, n_labels, index, pooled, per_label)
        rows = t.shape[0] * (t.shape[1] if pooled else 1)
        counts = counts.cpu().numpy()
        return {"prob": counts / float(rows), "counts": counts, "absent": flags[..., 0], "rows": rows}

    def partition(self, key, n_labels=None, index=None, pooled=True):
        """Point estimate of the partition behind the allocation vector store[key]: the stored draw whose co-membership matrix
        is nearest (least squares) to the posterior similarity matrix of `coallocation` -- Dahl's (2006) least-squares
        clustering, the stored draw of least posterior expected Binder loss --, found on the device (no gather of the store).
        A dict of host arrays: "labels" int64 (n,) the draw, relabelled in order of first appearance (0, 1, ..), -1 for an
        absent (NaN) element; "iteration", "chain" where it is stored (the first of equals); "score" its score and "scores"
        (n_iter, C) int64 those of all stored draws, sum over i < j of [z_i = z_j] (rows - 2 counts_ij): rows times the squared
        distance up to a constant.  pooled=False: one estimate per chain against that chain's own matrix -- "labels" (C, n),
        "iteration" (C,), "chain" = 0 .. C - 1, "score" (C,).  Unlike the element-wise mode of the labels it is not misled by
        label switching.  n_labels, index and the ValueError as in `coallocation`.  Under a sharded multi-GPU run this is the
        estimate from this rank's chains only."""
        import torch

        self._whole_store_on_device("partition")
        t, K, counts, _ = self._coallocation(key, n_labels, index, pooled, False)
        score, best = self.engine.store_partition_score(t, K, counts, index=index, pooled=pooled)
        best = best.cpu().numpy()
        C = t.shape[1]
        if pooled:
            it, ch = np.int64(best[0] // C), np.int64(best[0] % C)
            draws = t[int(it), int(ch)]
        else:
            it, ch = best[:, 0].copy(), np.arange(C, dtype=np.int64)
            draws = t[torch.as_tensor(it, device=t.device), torch.arange(C, device=t.device)]
        draws = draws.cpu().numpy()  # (size,) or (C, size): the chosen rows alone leave the device
        if index is not None:
            draws = draws[..., self.engine._store_index(index, t.shape[2])[0].cpu().numpy()]

        def canonical(z):
            out, seen = np.full(z.shape, -1, dtype=np.int64), {}
            for i, v in enumerate(z):
                if v == v:
                    out[i] = seen.setdefault(int(v), len(seen))
            return out

        labels = canonical(draws) if pooled else np.stack([canonical(z) for z in draws])
        return {"labels": labels, "iteration": it, "chain": ch, "score": best[..., 1].copy() if not pooled else np.int64(best[1]),
                "scores": score.cpu().numpy()}

    def histogram(self, key, bins=10, range=None, index=None, pooled=True, density=False):
        """np.histogram of the stored draws of every selected element of store[key] at once, counted on the device (one read
        of the store, no gather): (hist, edges) as host arrays.  hist is (n_idx, n_bins) pooled over chains and iterations,
        else (C, n_idx, n_bins); int64 counts, or with density=True hist / (hist.sum() * np.diff(edges)) per row in fp64, divided
        in np.histogram's order (by the widths, then by the sum), so that the densities are bit-equal to numpy's.
        bins: an array of shared edges (n_bins + 1,) or of per-element edges (n_idx, n_bins + 1), which is returned as given;
        or an int: with range=(lo, hi) the shared edges np.linspace(lo, hi, bins + 1), without a range every element gets
        the edges numpy would give it, np.linspace over its own minimum and maximum (widened by 0.5 either way when they are
        equal, (0, 1) for an element without a draw; an infinite draw raises ValueError as in numpy) -- edges (n_idx, bins + 1).
        That range is the element's over ALL chains also with pooled=False, so that one element's chains share their edges.
        NaN draws (the padding of variable-size parameters) are left out.  index selects elements (in that order, repeats
        allowed); a 2-D entry ("log_post") counts as one element.  Under a sharded multi-GPU run these are the counts of this
        rank's chains only; counts of several ranks over the same edges can simply be added."""
        self._whole_store_on_device("histogram")
        t = self._store_3d(key)
        if np.ndim(bins) == 0:
            n_bins = int(bins)
            if n_bins != bins or not 1 <= n_bins <= 1024:
                raise ValueError("bins must be an integer between 1 and 1024 or an array of edges")
            if range is not None:
                lo, hi = (float(v) for v in range)
                if lo > hi:
                    raise ValueError("max must be larger than min in range parameter.")  # np.histogram's own messages
                if not (np.isfinite(lo) and np.isfinite(hi)):
                    raise ValueError(f"supplied range of [{lo}, {hi}] is not finite")
                if lo == hi:
                    lo, hi = lo - 0.5, hi + 0.5
                edges = np.linspace(lo, hi, n_bins + 1)
            else:
                mn, mx, cnt = (v.cpu().numpy() for v in self.engine.store_minmax(t, index=index, pooled=True))
                lo, hi = np.where(cnt > 0, mn, 0.0), np.where(cnt > 0, mx, 1.0)
                if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
                    raise ValueError("autodetected range is not finite")
                same = lo == hi
                lo, hi = np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)
                edges = np.stack([np.linspace(a, b, n_bins + 1) for a, b in zip(lo, hi)])
        else:
            edges = np.array(bins, dtype=np.float64)
            if edges.ndim not in (1, 2) or edges.shape[-1] < 2:
                raise ValueError("bins must be an integer, (n_bins + 1,) edges or (n_idx, n_bins + 1) edges")
            if np.isnan(edges).any() or (np.diff(edges, axis=-1) < 0).any():
                raise ValueError("`bins` must increase monotonically, when an array")
        counts, _ = self.engine.store_histogram(t, edges, index=index, pooled=pooled)
        hist = counts.cpu().numpy()
        if density:
            hist = hist / np.diff(edges, axis=-1) / hist.sum(axis=-1, keepdims=True)  # (np.histogram's order of operations)
        return hist, edges

    def kde(self, key, index=None, pooled=True, grid_len=512, bw="experimental", bw_fct=1.0, extend=0.1, bounds=None):
        """Kernel density estimate of the marginal posterior of every selected element of store[key] -- the curve of
        az.plot_posterior / plot_density -- from one histogram pass over the store and a per-element kernel on the device (no
        gather): a dict of host arrays "grid" (.., G), "density" (.., G), "bw", "mode", "flag" (int32), "n" (draws counted) and
        "outside" (draws left out: NaN, or beyond a bound), the leading shape (n_idx,) pooled over chains and iterations, else
        (C, n_idx).  G = grid_len (8..1024).  The grid of an element spans its minimum and maximum over ALL chains (also with
        pooled=False, so that its chains share a grid), widened by extend (max - min) either way; an element that never moved
        is widened by 0.5 as `histogram` does and comes out with flag 2 under a bandwidth rule.  bounds=(L, U), either may be
        None, are the ends of the parameter's support: the grid is clamped to and starts (ends) exactly at a bound, and the mass
        a Gaussian kernel would put beyond it is reflected back.  The draws are counted into the G bins with the edges
        np.linspace(a, b, G + 1) (counts equal np.histogram(x, G, (a, b))); "grid" holds the bin centres, the midpoints of
        neighbouring edges; the density is the binned Gaussian convolution at those centres.  bw: "experimental" (ArviZ's
        default: the mean of Silverman's rule and the improved Sheather-Jones rule), "isj", "silverman", "scott", or a
        bandwidth -- a float or an (n_idx,) array; every bandwidth is multiplied by bw_fct.  "mode" is the grid point of the
        largest density (the lowest of equal ones).  flag: 0 ok; 1 the Sheather-Jones equation had no root and Silverman's
        bandwidth stands in; 2 degenerate (fewer than two draws or than two non-empty bins; density, bw and mode are NaN).
        NaN draws (the padding of variable-size parameters) are left out; an infinite draw raises ValueError as in
        `histogram`.  index selects elements (in that order, repeats allowed); a 2-D entry ("log_post") counts as one
        element.  Under a sharded multi-GPU run this covers this rank's chains only; the estimate is a function of the counts
        and the grid alone, so counts of several ranks over the same edges can be added and handed to `engine.kde_binned`, which
        gives the estimate of all ranks' chains."""
        self._whole_store_on_device("kde")
        t = self._store_3d(key)
        G = int(grid_len)
        if G != grid_len or not 8 <= G <= 1024:
            raise ValueError("grid_len must be an integer between 8 and 1024")
        if not (np.ndim(extend) == 0 and extend >= 0 and np.isfinite(extend)):
            raise ValueError("extend must be a finite non-negative number")
        L, U = (None, None) if bounds is None else bounds
        mn, mx, cnt = (v.cpu().numpy() for v in self.engine.store_minmax(t, index=index, pooled=True))
        lo, hi = np.where(cnt > 0, mn, 0.0), np.where(cnt > 0, mx, 1.0)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError("autodetected range is not finite")
        same = lo == hi
        pad = extend * (hi - lo)
        a, b = np.where(same, lo - 0.5, lo - pad), np.where(same, hi + 0.5, hi + pad)
        if L is not None:
            a = np.full_like(a, float(L))
        if U is not None:
            b = np.full_like(b, float(U))
        if not (np.isfinite(a).all() and np.isfinite(b).all() and (a < b).all()):
            raise ValueError("bounds leave an element without a range")
        n_idx = a.shape[0]
        edges = np.stack([np.linspace(x, y, G + 1) for x, y in zip(a, b)])
        counts, outside = self.engine.store_histogram(t, edges, index=index, pooled=pooled)
        lead = tuple(counts.shape[:-1])
        rule, given = bw, None
        if not isinstance(bw, str):
            if np.ndim(bw) > 1 or (np.ndim(bw) == 1 and len(bw) != n_idx):
                raise ValueError("bw must be a rule's name, a float or an (n_idx,) array")
            rule, given = "given", np.array(np.broadcast_to(np.asarray(bw, dtype=np.float64), lead))
        density, h, mode, flag = self.engine.kde_binned(counts, np.array(np.broadcast_to(a, lead)),
                                                        np.array(np.broadcast_to(b, lead)), rule=rule, bw=given,
                                                        bw_fct=bw_fct, reflect=(L is not None, U is not None))
        grid = 0.5 * (edges[:, :-1] + edges[:, 1:])
        return {"grid": np.ascontiguousarray(np.broadcast_to(grid, lead + (G,))), "density": density.cpu().numpy(),
                "bw": h.cpu().numpy(), "mode": mode.cpu().numpy(), "flag": flag.cpu().numpy(),
                "n": counts.sum(dim=-1).cpu().numpy(), "outside": outside.sum(dim=-1).cpu().numpy()}

    def mode(self, key, index=None, pooled=True, **kde_args):
        """Posterior mode of every selected element of store[key]: the grid point of the largest kernel density estimate,
        kde(key, index=index, pooled=pooled, **kde_args)["mode"] -- what az.plot_posterior(point_estimate="mode") shows."""
        return self.kde(key, index=index, pooled=pooled, **kde_args)["mode"]

    def exceedance(self, key, thresholds, index=None, pooled=True):
        """P(x > t) of every selected element of store[key] for every threshold t, from one histogram pass on the device:
        (n_t, n_idx) pooled over chains and iterations, else (n_t, C, n_idx).  The numerator counts the draws strictly greater
        than t, the denominator the non-NaN draws; NaN where an element has none.  thresholds: a scalar or a sequence in any
        order (at most 1024, no NaN).  Under a sharded multi-GPU run: this rank's chains only."""
        self._whole_store_on_device("exceedance")
        t = self._store_3d(key)
        th = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        if th.ndim != 1 or not 1 <= th.size <= 1024 or np.isnan(th).any():
            raise ValueError("thresholds must be a scalar or a sequence of at most 1024 values without NaN")
        order = np.argsort(th, kind="stable")
        # v >= nextafter(t, +inf) is exactly v > t: bin j holds the draws in (t_j, t_{j+1}], the last one those above the largest t
        edges = np.concatenate([np.nextafter(th[order], np.inf), [np.inf]])
        counts, outside = self.engine.store_histogram(t, edges, index=index, pooled=pooled)
        counts, outside = counts.cpu().numpy(), outside.cpu().numpy()
        above = np.cumsum(counts[..., ::-1], axis=-1)[..., ::-1]  # suffix sums: draws > t_j
        above[..., np.isposinf(th[order])] = 0  # (the closed last bin holds the +inf draws: none of them exceeds +inf)
        valid = counts.sum(axis=-1) + outside[..., 0] + outside[..., 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            p = np.where(valid[..., None] > 0, above / valid[..., None], np.nan)
        out = np.empty_like(p)
        out[..., order] = p
        return np.moveaxis(out, -1, 0)

    def _axis_edges(self, t, index, bins, rng, pool_elements):
        """Edges of one axis of histogram2d: (n + 1,) shared by all pairs or (n_pairs, n + 1), by np.histogramdd's rules"""
        if np.ndim(bins) == 0:
            n = int(bins)
            if n != bins or not 1 <= n <= 1024:
                raise ValueError("bins must be integers between 1 and 1024 or arrays of edges")
            if rng is not None:
                lo, hi = (float(v) for v in rng)
                if lo > hi:
                    raise ValueError("max must be larger than min in range parameter.")  # np.histogramdd's own messages
                if not (np.isfinite(lo) and np.isfinite(hi)):
                    raise ValueError(f"supplied range of [{lo}, {hi}] is not finite")
                lo, hi = np.array([lo]), np.array([hi])
            else:
                mn, mx, cnt = (v.cpu().numpy() for v in self.engine.store_minmax(t, index=index, pooled=True))
                lo, hi = np.where(cnt > 0, mn, 0.0), np.where(cnt > 0, mx, 1.0)
                if pool_elements:  # one range over all selected elements: that of the flattened draws
                    have = cnt > 0
                    lo, hi = (np.array([lo[have].min()]), np.array([hi[have].max()])) if have.any() else (np.zeros(1), np.ones(1))
                if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
                    raise ValueError("autodetected range is not finite")
            same = lo == hi
            lo, hi = np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)
            edges = np.stack([np.linspace(a, b, n + 1) for a, b in zip(lo, hi)])
            return edges[0] if (rng is not None or pool_elements) else edges
        edges = np.array(bins, dtype=np.float64)
        if edges.ndim not in (1, 2) or edges.shape[-1] < 2 or (edges.ndim == 2 and pool_elements):
            raise ValueError("bins must be integers, (n + 1,) edges or, without pool_elements, (n_pairs, n + 1) edges")
        if np.isnan(edges).any() or (np.diff(edges, axis=-1) < 0).any():
            raise ValueError("`bins` must increase monotonically, when an array")
        return edges

    def _hist2d(self, key_x, key_y, index_x, index_y, bins, range, pooled, pool_elements, occupancy):
        tx = self._store_3d(key_x)
        ty = tx if key_y is None else self._store_3d(key_y)
        try:
            n_given = len(bins)
        except TypeError:
            n_given = 1
        if n_given != 2:  # (np.histogram2d: an int, or one array of edges for both axes)
            bins = [bins, bins]
        rngs = [None, None] if range is None else list(range)
        if len(rngs) != 2:
            raise ValueError("range must be [[xlo, xhi], [ylo, yhi]]")
        ex = self._axis_edges(tx, index_x, bins[0], rngs[0], pool_elements)
        ey = self._axis_edges(ty, index_y, bins[1], rngs[1], pool_elements)
        gx, gy = ex, ey
        if ex.ndim != ey.ndim:  # per-pair edges on one axis only: the other axis' edges for every pair
            n = max(ex.shape[0] if ex.ndim == 2 else 0, ey.shape[0] if ey.ndim == 2 else 0)
            gx = ex if ex.ndim == 2 else np.broadcast_to(ex, (n, ex.size))
            gy = ey if ey.ndim == 2 else np.broadcast_to(ey, (n, ey.size))
        out = self.engine.store_histogram2d(tx, ty, gx, gy, index_x=index_x, index_y=index_y, pooled=pooled,
                                            pool_pairs=pool_elements, occupancy=occupancy)
        return [v.cpu().numpy() for v in out], ex, ey, tx.shape[0] * (tx.shape[1] if pooled else 1)

    def histogram2d(self, key_x, key_y=None, index_x=None, index_y=None, bins=10, range=None, pooled=True, pool_elements=False,
                    density=False):
        """np.histogram2d of the stored draws of pairs of elements, counted on the device (one read of the selected columns, no
        gather): (hist, xedges, yedges) as host arrays.  Pair k is element index_x[k] of store[key_x] against element index_y[k]
        of store[key_y] in the same (iteration, chain) state (key_y=None: two elements of store[key_x]; index None: all elements;
        in that order, repeats allowed; a 2-D entry ("log_post") counts as one element; both sides equally many).  hist is
        (n_pairs, nx, ny) pooled over chains and iterations, else (C, n_pairs, nx, ny); with pool_elements=True all pairs are
        counted into one map, (nx, ny) or (C, nx, ny) -- the joint map of a variable-size parameter, locations against
        coefficients.  int64 counts, or with density=True fp64, divided in np.histogramdd's order (by the x widths, by the y
        widths, then by the sum), so that the densities are bit-equal to numpy's.
        bins, as numpy takes them: an int, (nx, ny), one array of edges for both axes, or [xedges, yedges]; an axis' edges are
        (n + 1,) shared by all pairs or (n_pairs, n + 1) per pair (not with pool_elements) and are returned as given.  An int
        axis with range=[[xlo, xhi], [ylo, yhi]] gets the shared edges np.linspace(lo, hi, n + 1); without a range (or with None
        in its place) every coordinate gets the edges numpy would give it, np.linspace over its own non-NaN minimum and maximum
        over ALL chains (widened by 0.5 either way when they are equal, (0, 1) without a draw; an infinite draw raises ValueError
        as in numpy) -- edges (n_pairs, n + 1), or with pool_elements (n + 1,) over all selected elements.
        A pair with a NaN coordinate (the padding of variable-size parameters) is left out.  Under a sharded multi-GPU run these
        are the counts of this rank's chains only; counts of several ranks over the same edges can simply be added."""
        self._whole_store_on_device("histogram2d")
        (counts, _), ex, ey, _ = self._hist2d(key_x, key_y, index_x, index_y, bins, range, pooled, pool_elements, False)
        hist = counts
        if density:  # (np.histogramdd's order of operations)
            s = counts.sum(axis=(-2, -1), keepdims=True).astype(np.float64)
            hist = counts.astype(np.float64) / np.diff(ex, axis=-1)[..., :, None] / np.diff(ey, axis=-1)[..., None, :]
            hist /= s
        return hist, ex, ey

    def occupancy(self, key_x, key_y=None, index_x=None, index_y=None, bins=10, range=None, pooled=True):
        """In what share of the stored states a cell of the (x, y) grid holds at least one of the selected pairs: (prob, xedges,
        yedges), prob fp64 (nx, ny) over all chains and iterations, else (C, nx, ny) -- per state np.histogram2d(...)[0] > 0,
        averaged over the states, counted on the device.  What a variable-size parameter has in place of marginals: where its
        components (knots, sources) lie, location against coefficient or x against y.  Pairs, bins and range as `histogram2d`
        with pool_elements=True (the elements always share their edges); at most 256 pairs; NaN-padded components are left
        out.  Under a sharded multi-GPU run: this rank's chains only; prob times the states adds across ranks over the same
        edges."""
        self._whole_store_on_device("occupancy")
        (_, _, occupied), ex, ey, rows = self._hist2d(key_x, key_y, index_x, index_y, bins, range, pooled, True, True)
        return occupied / rows, ex, ey

    def kde2d(self, key_x, key_y=None, index_x=None, index_y=None, pooled=True, grid_len=128, bw="scott", bw_fct=1.0, extend=0.1,
              probs=(0.5, 0.9), pool_elements=False):
        """Joint kernel density estimate of pairs of elements -- the surface, the contour levels and the joint mode of
        az.plot_pair(kind="kde") / az.plot_kde(x, y, hdi_probs=...) -- from one joint histogram pass over the store and a
        full-covariance binned Gaussian convolution on the device (no gather): a dict of host arrays "grid_x" (.., nx), "grid_y"
        (.., ny) (the bin centres), "density" (.., nx, ny), "bw" (.., 3) = the kernel covariance (h_xx, h_xy, h_yy), "mode" (.., 2),
        "probs", "levels" (.., n_probs), "flag" (int32), "n" (pairs counted) and "outside" (pairs left out: a NaN coordinate).
        Pairs are selected as in `histogram2d`: pair k is element index_x[k] of store[key_x] against element index_y[k] of
        store[key_y] in the same state (key_y=None: two elements of store[key_x]); the leading shape is (n_pairs,) pooled over
        chains and iterations, else (C, n_pairs); with pool_elements=True all pairs go into one density, () or (C,) -- the joint
        density of a NaN-padded variable-size parameter, locations against coefficients.  grid_len: an int or (nx, ny), each
        8..256.  The grid of a coordinate spans its minimum and maximum over ALL chains (with pool_elements: over all selected
        elements), widened by extend (max - min) either way; a coordinate that never moved is widened by 0.5 as in `kde` and
        leaves its pair with flag 2 under a rule.  The pairs are counted into the cells with the edges np.linspace(a, b, n + 1)
        (counts equal np.histogram2d); the density is the binned convolution at the bin centres, without reflection at bounds.
        bw: "scott" or "silverman" (one rule in two dimensions, H = N^(-1/3) S, S the covariance of the binned pairs: what
        scipy.stats.gaussian_kde and ArviZ use); "marginal", the product kernel H = diag(h_x^2, h_y^2), h the coordinate's own
        `kde(..., bw="experimental")` bandwidth on the marginal counts times N^(1/30) (the 1-D rate N^(-1/5) moved to the 2-D
        rate N^(-1/6)) -- the choice for the bimodal joints of mixture-prior and reversible-jump models, which Scott's rule
        oversmooths; or a symmetric 2 x 2 matrix, or (n_pairs, 2, 2).  Every H is multiplied by bw_fct^2.  "levels": for every
        prob the density level whose region {density >= level} is the highest-density region holding that share of the mass
        (ArviZ's _find_hdi_contours); "mode": the grid point of the largest density, the lowest flat index of equal ones.
        flag: 0 ok; 1 ("marginal") the Sheather-Jones equation of a coordinate had no root and Silverman's bandwidth stands in; 2
        degenerate (fewer than two pairs, non-empty rows or columns, a singular or nearly singular H; density, bw, mode and levels
        are NaN).  An infinite draw raises ValueError as in `histogram2d`.  Under a sharded multi-GPU run this covers this rank's
        chains only; the estimate is a function of the counts and the grid alone, so counts of several ranks over the same edges
        can be added and handed to `engine.kde2d_binned`, which gives the estimate of all ranks' chains."""
        self._whole_store_on_device("kde2d")
        tx = self._store_3d(key_x)
        ty = tx if key_y is None else self._store_3d(key_y)
        try:
            nx, ny = grid_len
        except TypeError:
            nx = ny = grid_len
        if int(nx) != nx or int(ny) != ny or not (8 <= nx <= 256 and 8 <= ny <= 256):
            raise ValueError("grid_len must be an integer or (nx, ny), each between 8 and 256")
        nx, ny = int(nx), int(ny)
        if not (np.ndim(extend) == 0 and extend >= 0 and np.isfinite(extend)):
            raise ValueError("extend must be a finite non-negative number")
        # every argument is judged before the store is read
        if not (np.ndim(bw_fct) == 0 and bw_fct > 0 and np.isfinite(bw_fct)):
            raise ValueError("bw_fct must be a finite positive number")
        p = np.zeros(0) if probs is None else np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if p.ndim != 1 or p.size > 16 or not np.all((p > 0) & (p < 1)):
            raise ValueError("probs must be at most 16 shares of mass, each in (0, 1)")
        H = None
        if not isinstance(bw, str):
            H = np.asarray(bw, dtype=np.float64)
            n_sel = tx.shape[2] if index_x is None else len(index_x)
            if H.shape not in ((2, 2), (n_sel, 2, 2)) or (H.ndim == 3 and pool_elements):
                raise ValueError("bw must be a rule's name, a 2 x 2 matrix or, without pool_elements, an (n_pairs, 2, 2) array")
            if not np.array_equal(H[..., 0, 1], H[..., 1, 0]):
                raise ValueError("bw must be symmetric")
        elif bw not in ("scott", "silverman", "marginal"):
            raise ValueError('bw must be "scott", "silverman", "marginal" or a symmetric 2 x 2 matrix')

        def axis(t, index, n):  # (a, b, edges) of a coordinate: per pair, or one for all with pool_elements
            mn, mx, cnt = (v.cpu().numpy() for v in self.engine.store_minmax(t, index=index, pooled=True))
            lo, hi = np.where(cnt > 0, mn, 0.0), np.where(cnt > 0, mx, 1.0)
            if pool_elements:
                have = cnt > 0
                lo, hi = (np.array([lo[have].min()]), np.array([hi[have].max()])) if have.any() else (np.zeros(1), np.ones(1))
            if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
                raise ValueError("autodetected range is not finite")
            same = lo == hi
            pad = extend * (hi - lo)
            a, b = np.where(same, lo - 0.5, lo - pad), np.where(same, hi + 0.5, hi + pad)
            edges = np.stack([np.linspace(p, q, n + 1) for p, q in zip(a, b)])
            return (a[0], b[0], edges[0]) if pool_elements else (a, b, edges)

        ax, bx, ex = axis(tx, index_x, nx)
        ay, by, ey = axis(ty, index_y, ny)
        counts, outside = self.engine.store_histogram2d(tx, ty, ex, ey, index_x=index_x, index_y=index_y, pooled=pooled,
                                                        pool_pairs=pool_elements)
        lead = tuple(counts.shape[:-2])
        # (device tensors of the leading shape, () with pooled elements, which a host array would not keep)
        ends = [self.engine.to_device(np.array(np.broadcast_to(v, lead))).reshape(lead) for v in (ax, bx, ay, by)]
        rule, given, flag1 = bw, None, None
        if isinstance(bw, str) and bw == "marginal":
            n_pairs = counts.sum(dim=(-2, -1)).double()
            _, hx, _, fx = self.engine.kde_binned(counts.sum(dim=-1), ends[0], ends[1], rule="experimental")
            _, hy, _, fy = self.engine.kde_binned(counts.sum(dim=-2), ends[2], ends[3], rule="experimental")
            up = n_pairs ** (1.0 / 30.0)
            hx, hy = hx * up, hy * up
            given = self.engine.full(lead + (3,), 0.0)
            given[..., 0], given[..., 2] = hx * hx, hy * hy
            rule, flag1 = "given", ((fx == 1) | (fy == 1)).cpu().numpy()
        elif H is not None:
            rule = "given"
            given = np.array(np.broadcast_to(np.stack([H[..., 0, 0], H[..., 0, 1], H[..., 1, 1]], axis=-1), lead + (3,)))
        density, h, mode, level, _, flag = self.engine.kde2d_binned(counts, *ends, rule=rule, bw=given, bw_fct=bw_fct, probs=p)
        flag = flag.cpu().numpy()
        if flag1 is not None:
            flag = np.where((flag == 0) & flag1, np.int32(1), flag).astype(np.int32)
        gx, gy = 0.5 * (ex[..., :-1] + ex[..., 1:]), 0.5 * (ey[..., :-1] + ey[..., 1:])
        return {"grid_x": np.ascontiguousarray(np.broadcast_to(gx, lead + (nx,))),
                "grid_y": np.ascontiguousarray(np.broadcast_to(gy, lead + (ny,))), "density": density.cpu().numpy(),
                "bw": h.cpu().numpy(), "mode": mode.cpu().numpy(),
                "probs": p,
                "levels": level.cpu().numpy(), "flag": flag, "n": counts.sum(dim=(-2, -1)).cpu().numpy(),
                "outside": outside.sum(dim=-1).cpu().numpy()}

    def joint_mode(self, key_x, key_y=None, index_x=None, index_y=None, pooled=True, **kde2d_args):
        """Joint posterior mode of pairs of elements: the grid point of the largest joint kernel density estimate,
        kde2d(key_x, key_y, index_x, index_y, pooled, **kde2d_args)["mode"], (.., 2).  The pair of marginal `mode`s is no joint
        mode: a ridge or a second cluster moves a marginal's peak to where the joint density has none."""
        return self.kde2d(key_x, key_y, index_x, index_y, pooled, **kde2d_args)["mode"]

    def density_region(self, key_x, key_y=None, index_x=None, index_y=None, prob=0.9, pooled=True, **kde2d_args):
        """The highest-density region of pairs of elements that holds the share `prob` of the mass: (mask, grid_x, grid_y), mask
        bool (.., nx, ny) = density >= level of kde2d(..., probs=(prob,)) -- the cells inside az.plot_kde's contour at
        hdi_probs=[prob]; all False for a degenerate pair (flag 2)."""
        out = self.kde2d(key_x, key_y, index_x, index_y, pooled, probs=(prob,), **kde2d_args)
        with np.errstate(invalid="ignore"):
            mask = out["density"] >= out["levels"][..., 0, None, None]
        return mask, out["grid_x"], out["grid_y"]

    def _thinned(self, every):
        """{key: device tensor (ceil(n_iter / every), C, ...)}: every `every`-th stored iteration, packed on the device"""
        self._whole_store_on_device("a thinned transfer")
        if int(every) <= 1:
            return self.store
        return {key: self.engine.store_thin(t.contiguous(), every) for key, t in self.store.items()}

    def collect(self, every=1):
        """Host copy of the store in the reference's per-chain layout: {key: (C, size, n_iter)},
        log_post: (C, n_iter, 1).  every=k: iterations 0, k, 2k, ... only (thinned on the device before the transfer).
        With store_ring: the drained store (every stored iteration, from pinned host memory)."""
        from openmcmc_amd.parallel import store_to_reference_layout

        if self._drain is not None and self._n_dev != self.n_iter:
            host = self.host_store
            return {key: store_to_reference_layout(key, t.numpy()[:: int(every)]) for key, t in host.items()}
        return {key: store_to_reference_layout(key, t.detach().cpu().numpy()) for key, t in self._thinned(every).items()}

    @property
    def host_store(self):
        """store_ring with the default sink: {key: pinned host tensor (n_iter, C, ...)} once run_mcmc has returned"""
        if self._drain is None or self._drain.host is None:
            raise ValueError("no drained store: run with store_ring and the default sink")
        self._drain.wait()
        return self._drain.host

    def gather(self, dst=0, comm=None, group=None, every=1):
        """The one collective of the path: gather every rank's store on rank `dst` over RCCL (xGMI).
        Returns the host dict of `collect()` for all chains on dst, None elsewhere.  `comm`: the library's own
        communicator (parallel.make_communicator(self.engine)) -> omc_gather_samples; "auto" makes one when the
        process group runs on RCCL; None -> torch.distributed's gather on the group's backend.  every=k: a thinned gather
        (iterations 0, k, 2k, ...: 1/k of the bytes over the links).  A run with store_ring gathers WHILE it samples:
        give it sink=parallel.GatherSink(...) instead."""
        import torch.distributed as dist

        from openmcmc_amd.parallel import gather_store, make_communicator

        if comm == "auto":
            comm = None
            if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1 and dist.get_backend(group) == "nccl":
                comm = make_communicator(self.engine, group)
        return gather_store(self._thinned(every), dst=dst, group=group, comm=comm)


class _RingDrain:
    """The ring store's second stream.  Iterations are cut into chunks of `half` slabs; chunk j lives in half j % 2 of the ring.
    release(): the chunk just filled is handed to the sink on the drain stream (behind an event of the sampling stream);
    acquire(): before the sampling stream writes into a half again it waits -- on the device, not on the host -- for the
    event that closed that half's drain.  The host never blocks inside the loop."""

    def __init__(self, mcmc):
        import torch

        self.m = mcmc
        self.dev = mcmc.engine.device
        self.stream = torch.cuda.Stream(device=self.dev)
        self.done = [None, None]
        self.sink = mcmc.sink
        self.host = None
        if self.sink is None:
            self.host = {key: torch.empty((mcmc.n_iter,) + tuple(t.shape[1:]), dtype=t.dtype, pin_memory=True)
                         for key, t in mcmc.store.items()}
        if self.sink is not None and hasattr(self.sink, "bind"):
            self.sink.bind(mcmc, self.stream)
        # entries whose slabs rely on the NaN fill beyond the live part (variable-size parameters, sampler.py:81-87, 105-116)
        self.refill = [s.param for s in mcmc.samplers if getattr(s, "max_variable_size", None) is not None]

    def acquire(self, it0):
        import torch

        h = (it0 // self.m._half) % 2
        ev = self.done[h]
        if ev is None:
            return
        torch.cuda.current_stream(self.dev).wait_event(ev)
        lo = it0 % self.m._n_dev
        for key in self.refill:  # a reused slab starts as the reference's fresh store does: NaN
            self.m.store[key][lo: lo + self.m._half].fill_(float("nan"))

    def release(self, it0, it1):
        import torch

        m = self.m
        h = (it0 // m._half) % 2
        filled = torch.cuda.Event()
        filled.record(torch.cuda.current_stream(self.dev))
        lo = it0 % m._n_dev
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(filled)
            for key, t in m.store.items():
                block = t[lo: lo + (it1 - it0)]
                if self.sink is None:
                    self.host[key][it0:it1].copy_(block, non_blocking=True)
                else:
                    self.sink(key, it0, it1, block)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.done[h] = ev

    def wait(self):
        self.stream.synchronize()
