"""Every kernel that draws its own random numbers, held to the stream map of csrc/omc_common.h and to chain sharding.

A. Shard invariance.  130 chains in one context against the same chains in three contexts of 1, 64 and 65 (every chain but the
   first changes its lane, chains 65-128 their workgroup, chain 64 goes from the first lane of a second group to the last lane
   of a first): everything a call writes must be equal bit for bit.  The contexts start at global chain 2^32 - 3, so chains
   0-2 have a zero high word in their chain id and the rest have 1, and the draw index has a non-zero high word as well: a
   kernel that keyed its counter by the local chain gives other numbers on the shards.  One that dropped the chain id's high
   word would not (every context drops it alike): chain 3, global id 2^32, is therefore run once more with the same inputs at
   global id 0 and must draw other numbers.
B. Stream identity.  Five chains at the same offset: the call with its draws made in the kernel against the same call with
   the draws injected -- uniforms from the host model (philox_model.uniforms: integer arithmetic and an exact scaling, so bit
   for bit), normals from the device's own omc_fill_normal of the same seed, offset and draw index.

The route of every row is fixed through the context's options: what the automatic choice picks may depend on the number of
chains in the context (band_algo 0 looks at C <= 3072, the segment count of k_band_seg is costed from the groups of 64
chains, the form of k_band_blocked from chains against CUs), and then results agree to rounding only.

Which bar a row's part B is held to:
  bits    every row but the two below: the kernels evaluate omc_normal_pair / omc_u53 on the words of the same Philox block
          as omc_fill_normal and the host model, and the scans run the same code on the same u either way.
  1e-12   normal_gamma_update and mixture_normal_gamma, element by element: their injected gammas come from the host model of
          omc_standard_gamma (philox_model.standard_gamma: from block 0, and from a component's block offset), whose
          logarithms and square roots are NumPy's: libm-level differences, the constant of
          tests/test_mixture_ragged_kernels_gpu.py.  The gammas that the gmrf_sweep row injects are device draws of
          normal_gamma_update at the same shape and draw index (bits): it is the row above that ties them to the host model.
Rows without part B (no argument to inject through): the index of rj_move / rj_move_densities (its uniform is injected, the
index then still comes from the stream in both runs), chain_sample_canonical (z=None is omc_fill_normal by construction).
"""

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import philox_model as pm

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0123_4567_89AB
OFFSET = 2**32 - 3           # chains 0-2: high word 0; from chain 3 on: 1
DRAW = (5 << 32) | 7         # a draw index with a non-zero high word
C_ALL = 130
SHARDS = ((0, 1), (1, 65), (65, 130))
C_B = 5                      # part B: chains 0-4, two of them past 2^32
RTOL = 1e-10                 # tests/test_truncated_gpu.py
SENTINEL = -7.25             # what a kernel must leave alone (an exact binary fraction no kernel here produces)
COUNTERS = ("tridiag_join_fallbacks", "band_join_retries", "band_join_fallbacks")


def make_engine(C, lo=0, opts=(), offset=OFFSET):
    from openmcmc_amd.engine import Engine

    eng = Engine(C, seed=SEED, chain_id_offset=offset + lo)
    for name, value in dict(opts).items():
        eng.set_option(name, value)
    return eng


def host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()) if hasattr(t, "detach") else np.asarray(t)


def i64(eng, a):
    import torch

    return torch.as_tensor(np.asarray(a, dtype=np.int64), device=eng.device)


def run(row, lo, hi, inject=False, offset=OFFSET):
    eng = make_engine(hi - lo, lo, row.opts, offset)
    out = row.fn(eng, lo, hi, inject)
    eng.check_status()  # no chain failed
    for name in COUNTERS:
        assert eng.counter(name) == 0, (row.name, name)
    res = {k: host(v) for k, v in out.items()}
    eng.close()
    return res


def host_uniforms(lo, hi, n, draw=DRAW, sub=0):
    return np.stack([pm.uniforms(SEED, draw, OFFSET + c, n, sub=sub) for c in range(lo, hi)])


# ---------------------------------------------------------------------------------------------------------------- inputs
# Built once for all 130 chains and never modified; a context for chains [lo, hi) takes rows lo .. hi - 1.
@functools.lru_cache(maxsize=None)
def tri_inputs(n):
    rng = np.random.default_rng(1000 + n)
    d = np.full(n, 2.0)
    d[0] = d[-1] = 1.0
    d[0] += 1e-3
    return SimpleNamespace(d=d, off=-np.ones(n - 1), y=rng.standard_normal(n), lam=20.0 + 0.5 * np.arange(C_ALL),
                           tau=1.0 + 0.01 * np.arange(C_ALL), rc=0.3 * rng.standard_normal((C_ALL, n)))


def band_rows(M, w):
    n = M.shape[0]
    band = np.zeros((w + 1, n))
    for d in range(min(w, n - 1) + 1):
        band[d, : n - d] = np.diag(M, -d)
    return band


def band_spd(rng, n, w, bw=None):
    """Symmetric, bandwidth bw <= w, strictly diagonally dominant (so positive definite, and with a short memory: the joins of
    the segmented kernel close after a few columns)."""
    bw = w if bw is None else bw
    M = np.zeros((n, n))
    for d in range(1, min(bw, n - 1) + 1):
        v = rng.uniform(-1.0, 1.0, n - d) / bw
        M += np.diag(v, d) + np.diag(v, -d)
    M += np.diag(1.5 + np.abs(M).sum(axis=1) + rng.random(n))
    return M


@functools.lru_cache(maxsize=None)
def band_inputs(n, w):
    rng = np.random.default_rng(2000 + 7 * n + w)
    return SimpleNamespace(band=band_rows(band_spd(rng, n, w), w), y=rng.standard_normal(n), lam=1.0 + 2.0 * rng.random(C_ALL),
                           tau=0.5 + rng.random(C_ALL), rc=0.3 * rng.standard_normal((C_ALL, n)))


def random_spd(rng, p):
    A = rng.standard_normal((p, 2 * p))
    M = A @ A.T / (2 * p) + 0.5 * np.eye(p)
    return 0.5 * (M + M.T)


@functools.lru_cache(maxsize=None)
def dense_inputs(p):
    rng = np.random.default_rng(3000 + p)
    return SimpleNamespace(M=random_spd(rng, p), r=rng.standard_normal(p), s1=0.5 + rng.random(C_ALL), s2=0.5 + rng.random(C_ALL),
                           rc=0.3 * rng.standard_normal((C_ALL, p)), dc=0.2 + rng.random((C_ALL, p)))


@functools.lru_cache(maxsize=None)
def small_inputs(kmax):
    rng = np.random.default_rng(4000 + kmax)
    A = rng.standard_normal((C_ALL, kmax, 2 * kmax))
    gram = A @ A.transpose(0, 2, 1) / (2 * kmax)
    count = 1 + (np.arange(C_ALL) * 5) % kmax  # every live length 1 .. kmax
    count[0] = kmax
    return SimpleNamespace(gram=gram, rhs=rng.standard_normal((C_ALL, kmax)), prec=0.5 + rng.random((C_ALL, kmax)),
                           pmean=0.2 * rng.standard_normal((C_ALL, kmax)), tau=0.5 + rng.random(C_ALL), count=count.astype(float),
                           x0=rng.uniform(-0.3, 0.3, (C_ALL, kmax)))


def limits(rng, n):
    """Limits that bite at some sites (the near-limit quantile) and are far at others (the Phi^-1 route)."""
    lower = np.where(rng.random(n) < 0.5, -0.2, -30.0)
    upper = np.where(rng.random(n) < 0.3, 0.4, 40.0)
    return lower, upper


@functools.lru_cache(maxsize=None)
def scan_inputs(n):
    rng = np.random.default_rng(5000 + n)
    lower, upper = limits(rng, n)
    return SimpleNamespace(d1=2.0 + rng.random(n), o1=-0.8 * rng.random(max(n - 1, 0)), lam=1.0 + 3.0 * rng.random(C_ALL),
                           tau=0.5 + rng.random(C_ALL), y=rng.standard_normal(n), rc=0.5 * rng.standard_normal((C_ALL, n)),
                           lower=lower, upper=upper, x0=np.clip(rng.standard_normal((C_ALL, n)), lower + 0.01, upper - 0.01),
                           M3=band_spd(rng, n, 3), M=random_spd(rng, n), dc=0.2 + rng.random((C_ALL, n)))


@functools.lru_cache(maxsize=None)
def mh_inputs(d):
    rng = np.random.default_rng(6000 + d)
    A = rng.standard_normal((d, 2 * d))
    Q = np.linalg.inv(A @ A.T / (2 * d))
    Q = 0.5 * (Q + Q.T)
    mu = rng.standard_normal(d)
    x0 = mu + np.linalg.solve(np.linalg.cholesky(Q).T, rng.standard_normal((d, C_ALL))).T  # draws from the target
    return SimpleNamespace(Q=Q, mu=mu, x0=x0)


def factor(eng, Q, scale):
    """(L, sum log L_ii) of scale * Q made on the host: the same bits in every context."""
    L = np.linalg.cholesky(scale * Q)
    return eng.to_device(L), eng.to_device(np.array([np.log(np.diag(L)).sum()]))


# ------------------------------------------------------------------------------------------------------------------ rows
ROWS = {}


def row(name, opts=(), stream="bits", primary="x"):
    def deco(fn):
        ROWS[name] = SimpleNamespace(name=name, fn=fn, opts=dict(opts), stream=stream, primary=primary)
        return fn
    return deco


def tridiag_row(name, n, opts, with_rc=True):
    @row(name, opts)
    def fn(eng, lo, hi, inject):
        I, C, dev = tri_inputs(n), hi - lo, eng.to_device
        terms = [{"diag": dev(I.d), "off": dev(I.off), "scale": dev(I.lam[lo:hi])},
                 {"rhs": dev(I.y), "center": dev(I.y), "scale": dev(I.tau[lo:hi])}]
        x, mean, quad, ld = eng.empty(C, n), eng.empty(C, n), eng.empty(2, C), eng.empty(C)
        eng.tridiag_sample_canonical(n, terms, x, z=eng.fill_normal(n, DRAW) if inject else None,
                                     rhs_chain=dev(I.rc[lo:hi]) if with_rc else None, draw_index=DRAW, mean_out=mean, quad_out=quad,
                                     logdet_out=ld)
        return {"x": x, "mean": mean, "quad": quad.T, "logdet": ld}


# takes_specialised (omc_tridiag.hip) for smoother-shaped terms at tridiag_seg 8: 2 * threads > 1024 with threads = 64 ceil(S / 64),
# S = ceil(n / 8) segments, i.e. S >= 513: n = 4097 is the smallest
tridiag_row("tridiag/serial", 70, {"tridiag_algo": 1})
tridiag_row("tridiag/seg-wave", 300, {"tridiag_algo": 2, "tridiag_seg": 8})
tridiag_row("tridiag/seg-workgroup-generic", 700, {"tridiag_algo": 2, "tridiag_seg": 8, "tridiag_generic": 1})
tridiag_row("tridiag/seg-workgroup-specialised", 4097, {"tridiag_algo": 2, "tridiag_seg": 8}, with_rc=False)
# n > 16 384 under the automatic tridiag_algo goes to the band route at bandwidth 1: its segmented kernel, the count fixed
tridiag_row("tridiag/long-chain", 16400, {"tridiag_algo": 0, "band_algo": 0, "band_seg_count": 8}, with_rc=False)


@row("gmrf_sweep", {"tridiag_algo": 2, "tridiag_seg": 8})
def _gmrf_sweep(eng, lo, hi, inject):
    n = 700
    I, C, dev = tri_inputs(n), hi - lo, eng.to_device
    d, off, y = dev(I.d), dev(I.off), dev(I.y)
    lam, tau = dev(I.lam[lo:hi]), dev(I.tau[lo:hi])
    terms = eng.tridiag_terms([{"diag": d, "off": off, "scale": lam}, {"rhs": y, "center": y, "scale": tau}], n)
    logdets = (eng.tridiag_logdet(n, d, off), eng.zeros(1))
    x, lp = eng.empty(C, n), eng.empty(C)
    out = {}
    for s in range(2):  # sweep s: normals at DRAW + 3 s, the gammas of its two blocks at DRAW + 3 s + 1 and + 2
        di = DRAW + 3 * s
        blocks = [{"a0": 10.0, "b0": 1.0, "n_pos": n, "logdet": logdets[0]}, {"a0": 1.0, "b0": 1.0, "n_pos": n, "logdet": logdets[1]}]
        if inject:
            for k, b in enumerate(blocks):  # rate 1 + 0 / 2: the update returns the Gamma(a0 + n / 2) draw itself
                b["g"] = eng.empty(C)
                eng.normal_gamma_update(b["a0"], 1.0, n, eng.zeros(C), b["g"], draw_index=di + 1 + k)
        eng.gmrf_sweep(n, terms, blocks, x, z=eng.fill_normal(n, di) if inject else None, draw_index=di, log_post_out=lp,
                       gamma_draw_base=di + 1)
        out.update({f"x{s}": x.clone(), f"lam{s}": lam.clone(), f"tau{s}": tau.clone(), f"log_post{s}": lp.clone()})
    out["x"] = out["x1"]
    return out


def band_row(name, n, w, opts, with_rc):
    @row(name, opts)
    def fn(eng, lo, hi, inject):
        I, C, dev = band_inputs(n, w), hi - lo, eng.to_device
        terms = [{"band": dev(I.band), "scale": dev(I.lam[lo:hi])}, {"rhs": dev(I.y), "scale": dev(I.tau[lo:hi])}]
        x, mean, ld = eng.empty(C, n), eng.empty(C, n), eng.empty(C)
        eng.band_sample_canonical(n, terms, x, z=eng.fill_normal(n, DRAW) if inject else None,
                                  rhs_chain=dev(I.rc[lo:hi]) if with_rc else None, draw_index=DRAW, mean_out=mean, logdet_out=ld)
        return {"x": x, "mean": mean, "logdet": ld}


band_row("band/k_band_lane", 70, 2, {"band_algo": 1}, with_rc=True)
band_row("band/k_band_seg", 200, 2, {"band_algo": 0, "band_seg_count": 2, "band_seg_overlap": 64}, with_rc=False)
band_row("band/k_band_sample", 70, 5, {"band_algo": 2}, with_rc=True)
# band_blocked_choose at w = 12 and two terms: 4 -> (16 columns, 256 threads, four waves a SIMD), 16 -> (16, 256, one),
# 8 -> (8, 512, four), 512 -> (16, 512, one)
for _form in (4, 16, 8, 512):
    band_row(f"band/k_band_blocked-{_form}", 70, 12, {"band_algo": 3, "band_blocked_threads": _form}, with_rc=_form == 512)


def dense_row(name, p, opts):
    @row(name, opts)
    def fn(eng, lo, hi, inject):
        I, C, dev = dense_inputs(p), hi - lo, eng.to_device
        terms = [{"mat": dev(I.M), "scale": dev(I.s1[lo:hi])}, {"rhs": dev(I.r), "scale": dev(I.s2[lo:hi])}]
        x, mean, ld = eng.empty(C, p), eng.empty(C, p), eng.empty(C)
        eng.dense_sample_canonical(p, terms, x, z=eng.fill_normal(p, DRAW) if inject else None, rhs_chain=dev(I.rc[lo:hi]),
                                   draw_index=DRAW, mean_out=mean, logdet_out=ld)
        return {"x": x, "mean": mean, "logdet": ld}


# dense_overlap 0: with it on, contexts of 64 chains and more factorise their chains as two halves on two streams
dense_row("dense/p40", 40, {"dense_overlap": 0})
dense_row("dense/p65-blocked", 65, {"dense_overlap": 0, "dense_blocked_min": 64})  # past the first 64-column block


@functools.lru_cache(maxsize=None)
def spectral_inputs(p):
    """M = V diag(ev) V' of dense_inputs(p) made on the host: every context is handed the same bits.  The library keeps V
    column-major (eigenvector j in memory row j, as omc_dense_spectral_prepare leaves it)."""
    ev, V = np.linalg.eigh(dense_inputs(p).M)
    return SimpleNamespace(V=np.ascontiguousarray(V.T), ev=ev)


@row("dense_spectral_sample")
def _spectral(eng, lo, hi, inject):
    p = 70  # two 64-row tiles of the products, the second one partly empty
    I, C, dev = dense_inputs(p), hi - lo, eng.to_device
    E = spectral_inputs(p)
    terms = [{"mat": dev(I.M), "scale": dev(I.s1[lo:hi])}, {"rhs": dev(I.r), "scale": dev(I.s2[lo:hi])}]
    x, mean, ld = eng.empty(C, p), eng.empty(C, p), eng.empty(C)
    eng.dense_spectral_sample(p, terms, 0, dev(E.V), dev(E.ev), x, z=eng.fill_normal(p, DRAW) if inject else None,
                              rhs_chain=dev(I.rc[lo:hi]), draw_index=DRAW, mean_out=mean, logdet_out=ld)
    return {"x": x, "mean": mean, "logdet": ld}


@row("small_sample_canonical")
def _small_sample(eng, lo, hi, inject):
    kmax = 7
    I, C, dev = small_inputs(kmax), hi - lo, eng.to_device
    mean = eng.empty(C, kmax)
    x = eng.small_sample_canonical(dev(I.gram[lo:hi]), dev(I.rhs[lo:hi]), dev(I.prec[lo:hi]), lik_scale=dev(I.tau[lo:hi]),
                                   prior_mean=dev(I.pmean[lo:hi]), count=dev(I.count[lo:hi]),
                                   z=eng.fill_normal(kmax, DRAW) if inject else None, draw_index=DRAW, mean_out=mean)
    return {"x": x, "mean": mean}


@row("chain_sample_canonical", stream=None)
def _chain_sample(eng, lo, hi, inject):
    k = 70  # the entry point serves orders beyond the 64 of small_sample_canonical
    I, dev = small_inputs(k), eng.to_device
    A = I.gram[lo:hi] + np.eye(k)
    mean = eng.empty(hi - lo, k)
    x = eng.chain_sample_canonical(dev(A), dev(I.rhs[lo:hi]), draw_index=DRAW, mean_out=mean)
    return {"x": x, "mean": mean}


def scan_u(lo, hi, n, inject, eng):
    return eng.to_device(host_uniforms(lo, hi, n)) if inject else None


def tridiag_scan_row(n):
    @row(f"tridiag_gibbs_truncated/n{n}")
    def fn(eng, lo, hi, inject):
        I, dev = scan_inputs(n), eng.to_device
        terms = [{"diag": dev(I.d1), "off": dev(I.o1), "scale": dev(I.lam[lo:hi])}, {"rhs": dev(I.y), "scale": dev(I.tau[lo:hi])}]
        x = dev(I.x0[lo:hi])
        eng.tridiag_gibbs_truncated(n, terms, x, lower=dev(I.lower), upper=dev(I.upper), u=scan_u(lo, hi, n, inject, eng),
                                    rhs_chain=dev(I.rc[lo:hi]), draw_index=DRAW)
        return {"x": x}


tridiag_scan_row(130)  # blocks of 64 + 64 + 2 sites: Philox blocks pair across the block boundaries
tridiag_scan_row(67)   # odd: the last site is the first half of a block


@row("band_gibbs_truncated")
def _band_scan(eng, lo, hi, inject):
    n, w = 67, 3
    I, dev = scan_inputs(n), eng.to_device
    terms = [{"band": dev(band_rows(I.M3, w)), "scale": dev(I.lam[lo:hi])}, {"rhs": dev(I.y), "scale": dev(I.tau[lo:hi])}]
    x = dev(I.x0[lo:hi])
    eng.band_gibbs_truncated(n, terms, x, lower=dev(I.lower), upper=dev(I.upper), u=scan_u(lo, hi, n, inject, eng),
                             rhs_chain=dev(I.rc[lo:hi]), draw_index=DRAW)
    return {"x": x}


def dense_scan_row(name, with_diag):
    @row(name)
    def fn(eng, lo, hi, inject):
        p = 67
        I, dev = scan_inputs(p), eng.to_device
        terms = [{"mat": dev(I.M), "scale": dev(I.lam[lo:hi])}, {"rhs": dev(I.y), "scale": dev(I.tau[lo:hi])}]
        x = dev(I.x0[lo:hi])
        eng.dense_gibbs_truncated(p, terms, x, lower=dev(I.lower), upper=dev(I.upper), u=scan_u(lo, hi, p, inject, eng),
                                  rhs_chain=dev(I.rc[lo:hi]), draw_index=DRAW, diag_chain=dev(I.dc[lo:hi]) if with_diag else None)
        return {"x": x}


dense_scan_row("dense_gibbs_truncated", False)
dense_scan_row("dense_gibbs_truncated/diag_chain", True)


@row("small_gibbs_truncated")
def _small_scan(eng, lo, hi, inject):
    kmax = 9
    I, dev = small_inputs(kmax), eng.to_device
    x = dev(I.x0[lo:hi])
    eng.small_gibbs_truncated(dev(I.gram[lo:hi]), dev(I.rhs[lo:hi]), dev(I.prec[lo:hi]), x, lower=-0.4, upper=0.5,
                              lik_scale=dev(I.tau[lo:hi]), prior_mean=dev(I.pmean[lo:hi]), count=dev(I.count[lo:hi]),
                              u=scan_u(lo, hi, kmax, inject, eng), draw_index=DRAW)
    return {"x": x}


# ---- the Metropolis-Hastings family of omc_mala.hip: z is the chain's normal stream, u half 0 of block 0 of its uniform stream
def mh_counts(eng, C):
    return i64(eng, np.zeros(C)), i64(eng, np.full(C, 5))


def mh_row(kind, d):
    @row(f"{kind}/d{d}")
    def fn(eng, lo, hi, inject):
        I, C, dev = mh_inputs(d), hi - lo, eng.to_device
        mala = kind.startswith("mala")
        step = 0.5 if mala else 0.05
        L, sl = factor(eng, I.Q, 1.0 / step**2 if mala else 1.0)
        x, mu = dev(I.x0[lo:hi]), dev(I.mu)
        acc, prp = mh_counts(eng, C)
        kw = dict(z=eng.fill_normal(d, DRAW) if inject else None, u=dev(host_uniforms(lo, hi, 1)[:, 0]) if inject else None,
                  draw_index=DRAW, accept_count=acc, proposal_count=prp)
        out = {}
        if kind == "mala_step":
            eng.mala_step(dev(I.Q), mu, L, sl, step, x, **kw)
        elif kind == "rw_step":
            eng.rw_step(mu, L, sl, step, x, **kw)
        else:
            out["log_p"] = eng.empty(C)
            (eng.mala_step_white if mala else eng.rw_step_white)(mu, L, sl, step, x, log_p_out=out["log_p"], **kw)
        out.update(x=x, accept=acc, proposals=prp)
        return out


def mala_run_row(d):
    @row(f"mala_run_white/d{d}")
    def fn(eng, lo, hi, inject):
        I, C, dev = mh_inputs(d), hi - lo, eng.to_device
        step, steps, stride = 0.5, 3, 3
        L, sl = factor(eng, I.Q, 1.0 / step**2)
        x = dev(I.x0[lo:hi])
        acc, prp = mh_counts(eng, C)
        xs, lps, lp = eng.empty(steps, C, d), eng.empty(steps, C), eng.empty(C)
        z = u = None
        if inject:  # step k reads the streams of draw index DRAW + k * stride
            import torch

            z = torch.stack([eng.fill_normal(d, DRAW + k * stride) for k in range(steps)]).contiguous()
            u = dev(np.stack([host_uniforms(lo, hi, 1, draw=DRAW + k * stride)[:, 0] for k in range(steps)]))
        eng.mala_run_white(dev(I.mu), L, sl, step, x, steps, z=z, u=u, draw_index0=DRAW, draw_stride=stride, x_store=xs,
                           logp_store=lps, accept_count=acc, proposal_count=prp, log_p_out=lp)
        return {"x": x, "x_store": xs.transpose(0, 1), "logp_store": lps.T, "log_p": lp, "accept": acc, "proposals": prp}


for _d in (17, 65):
    for _kind in ("mala_step", "mala_step_white", "rw_step", "rw_step_white"):
        mh_row(_kind, _d)
    mala_run_row(_d)


@functools.lru_cache(maxsize=None)
def transform_inputs(p):
    rng = np.random.default_rng(7000 + p)
    n = 4 * p
    A = (rng.random((n, p)) + 0.1) * (rng.random((n, p)) < max(0.15, 2.0 / p))
    A[np.arange(n), np.arange(n) % p] += 0.5
    truth = 0.3 * rng.standard_normal(p)
    w = 40.0 * (rng.random(n) + 0.5)
    y = A @ np.exp(truth) + rng.standard_normal(n) / np.sqrt(w)
    return SimpleNamespace(G=A.T @ (w[:, None] * A), cv=A.T @ (w * y), P=random_spd(rng, p), m0=np.full(p, 0.1),
                           tau=0.5 + rng.random(C_ALL), lam=0.5 + rng.random(C_ALL),
                           x0=truth[None, :] + 0.03 * rng.standard_normal((C_ALL, p)))


@row("mala_transform_step", primary="proposal")  # (a rejected step leaves x where it was, whatever the draws)
def _mala_transform(eng, lo, hi, inject):
    p = 33
    I, C, dev = transform_inputs(p), hi - lo, eng.to_device
    x = dev(I.x0[lo:hi])
    acc, prp = mh_counts(eng, C)
    prop, lf, lr, lp = eng.empty(C, p), eng.empty(C), eng.empty(C), eng.empty(C)
    # the step's uniform: half 0 of block (p + 1) / 2 + 1 of the uniform stream (k_mala_transform, omc_transform.hip)
    u = dev(host_uniforms(lo, hi, 1, sub=(p + 1) // 2 + 1)[:, 0]) if inject else None
    eng.mala_transform_step(dev(I.G), dev(I.cv), dev(I.P), 0.6, x, m0=dev(I.m0), tau=dev(I.tau[lo:hi]), lam=dev(I.lam[lo:hi]),
                            z=eng.fill_normal(p, DRAW) if inject else None, u=u, draw_index=DRAW, accept_count=acc,
                            proposal_count=prp, prop_out=prop, lq_fwd_out=lf, lq_rev_out=lr, log_p_out=lp)
    return {"x": x, "proposal": prop, "lq_fwd": lf, "lq_rev": lr, "log_p": lp, "accept": acc, "proposals": prp}


@functools.lru_cache(maxsize=None)
def ragged_inputs(kmax):
    rng = np.random.default_rng(8000 + kmax)
    count = (np.arange(C_ALL) * 3) % (kmax + 1)
    count[0] = kmax
    return SimpleNamespace(count=count.astype(float), x=rng.standard_normal((C_ALL, kmax)), grad=3 * rng.standard_normal((C_ALL, kmax)),
                           h=rng.uniform(0.2, 5.0, (C_ALL, kmax)))


@row("mala_diag")
def _mala_diag(eng, lo, hi, inject):
    kmax, sub = 7, 3
    I, dev = ragged_inputs(kmax), eng.to_device
    z = eng.fill_normal(2 * sub + kmax, DRAW)[:, 2 * sub:].contiguous() if inject else None  # entry j: normal 2 sub + j
    prop, lq = eng.mala_diag(dev(I.x[lo:hi]), dev(I.grad[lo:hi]), dev(I.h[lo:hi]), 0.7, count=dev(I.count[lo:hi]), z=z,
                             draw_index=DRAW, sub=sub)
    return {"x": prop, "lq": lq}


@functools.lru_cache(maxsize=None)
def propose_inputs(p):
    rng = np.random.default_rng(9000 + p)
    return SimpleNamespace(step=rng.uniform(0.2, 1.5, p), lower=-1.0 - rng.random(p), upper=1.0 + rng.random(p),
                           x=rng.uniform(-1, 1, (C_ALL, p, 1)))


def propose_row(name, with_limits, sub):
    @row(name)
    def fn(eng, lo, hi, inject):
        p = 5
        I, C, dev = propose_inputs(p), hi - lo, eng.to_device
        z = eng.full((C, p, 1), np.nan)
        inj = None
        if inject and with_limits:     # element e: half e & 1 of block sub + (e >> 1) of the uniform stream
            inj = dev(host_uniforms(lo, hi, p, sub=sub))
        elif inject:                   # ... of the normal stream
            inj = eng.fill_normal(2 * sub + p, DRAW)[:, 2 * sub:].contiguous()
        lim = (dev(I.lower), dev(I.upper)) if with_limits else (None, None)
        f, r = eng.rw_propose(dev(I.x[lo:hi]), z, dev(I.step), lim[0], lim[1], inject=inj, draw_index=DRAW, sub=sub)
        return {"x": z, "lq_fwd": f, "lq_rev": r}


propose_row("rw_propose/limits", True, 0)
propose_row("rw_propose/limits-sub", True, 2)
propose_row("rw_propose/free-sub", False, 2)


@functools.lru_cache(maxsize=None)
def scalar_inputs():
    rng = np.random.default_rng(10000)
    n = 1 + (np.arange(C_ALL) * 7) % 20  # counts 1 .. 20 with n_max = 20: forced births, forced deaths and free moves
    return SimpleNamespace(lp_cur=rng.standard_normal(C_ALL), lp_prop=rng.standard_normal(C_ALL), lqf=0.3 * rng.standard_normal(C_ALL),
                           lqr=0.3 * rng.standard_normal(C_ALL), n=n, dens=rng.standard_normal(C_ALL),
                           rate=np.where(np.arange(C_ALL) % 3 == 0, 25.0 + np.arange(C_ALL), 0.5 + (np.arange(C_ALL) % 8)),
                           quad=10.0 * rng.random(C_ALL))


@row("mh_accept/sub", primary=None)
def _mh_accept(eng, lo, hi, inject):
    I, C, dev, sub = scalar_inputs(), hi - lo, eng.to_device, 2
    acc_n, prp_n = mh_counts(eng, C)
    la = eng.empty(C)
    u = dev(host_uniforms(lo, hi, 1, sub=sub)[:, 0]) if inject else None  # half 0 of block `sub`
    acc = eng.mh_accept(dev(I.lp_cur[lo:hi]), dev(I.lp_prop[lo:hi]), dev(I.lqf[lo:hi]), dev(I.lqr[lo:hi]), u=u, draw_index=DRAW,
                        sub=sub, accept_count=acc_n, proposal_count=prp_n, log_alpha=la)
    return {"accept": acc, "log_alpha": la, "accept_count": acc_n, "proposals": prp_n}


@row("uniform_draw")
def _uniform_draw(eng, lo, hi, inject):
    p, sub = 9, 3
    rng = np.random.default_rng(11000)
    lower, width = rng.standard_normal(p), rng.uniform(0.5, 3.0, p)
    inj = eng.to_device(host_uniforms(lo, hi, p, sub=sub)) if inject else None
    return {"x": eng.uniform_draw(eng.to_device(lower), eng.to_device(width), inject=inj, draw_index=DRAW, sub=sub)}


@row("poisson_draw", primary=None)
def _poisson_draw(eng, lo, hi, inject):
    I = scalar_inputs()
    u = eng.to_device(host_uniforms(lo, hi, 256)) if inject else None  # a tape far longer than any of these draws reads
    return {"x": eng.poisson_draw(eng.to_device(I.rate[lo:hi]), u=u, draw_index=DRAW)}


@row("rj_move", primary=None)
def _rj_move(eng, lo, hi, inject):
    I = scalar_inputs()
    u = eng.to_device(host_uniforms(lo, hi, 1)[:, 0]) if inject else None
    birth, pb, pd, dele = eng.rj_move(i64(eng, I.n[lo:hi]), 20, 0.4, u=u, draw_index=DRAW)
    return {"birth": birth, "p_birth": pb, "p_death": pd, "del_index": dele}


@row("rj_move_densities", primary=None)
def _rj_move_densities(eng, lo, hi, inject):
    I, dev = scalar_inputs(), eng.to_device
    u = dev(host_uniforms(lo, hi, 1)[:, 0]) if inject else None
    birth, dele, cp, lf, lr = eng.rj_move_densities(dev(I.n[lo:hi].astype(float)), 20, 0.4, density_chain=dev(I.dens[lo:hi]),
                                                    density_const=-0.7, u=u, draw_index=DRAW)
    return {"birth": birth, "del_index": dele, "count_prop": cp, "lq_fwd": lf, "lq_rev": lr}


@row("normal_gamma_update", stream="1e-12")
def _normal_gamma(eng, lo, hi, inject):
    """Two shapes: 0.3 + 1 / 2 = 0.8 (below 1: the boost block as well) and 10 + 700 / 2, the shape of the gmrf_sweep row's
    first block, whose injected gammas are device draws of this entry point.  Injected: the host model of the gamma stream
    from block 0."""
    I, C, dev = scalar_inputs(), hi - lo, eng.to_device
    out = eng.empty(2, C)
    for j, (a0, n_pos) in enumerate(((0.3, 1), (10.0, 700))):
        g = None
        if inject:
            g = dev(np.array([pm.standard_gamma(SEED, DRAW + j, OFFSET + c, a0 + 0.5 * n_pos) for c in range(lo, hi)]))
        eng.normal_gamma_update(a0, 2.0, n_pos, dev(I.quad[lo:hi]), out[j], g=g, draw_index=DRAW + j)
    return {"x": out.T}


@functools.lru_cache(maxsize=None)
def mixture_inputs():
    rng = np.random.default_rng(12000)
    p, K = 21, 4
    alloc = rng.integers(0, K - 1, (C_ALL, p)).astype(float)  # component K - 1 stays empty
    return SimpleNamespace(p=p, K=K, y=3 * rng.standard_normal((C_ALL, p)), prior=rng.dirichlet(np.ones(K), p),
                           mean=2 * rng.standard_normal(K), prec=rng.uniform(0.2, 3.0, K), alloc=alloc,
                           resid=rng.standard_normal((C_ALL, p)), a0=np.array([0.3, 2.0, 1.0, 0.5]), b0=np.array([1.0, 0.5, 2.0, 1.5]))


@row("mixture_allocation")
def _mixture_allocation(eng, lo, hi, inject):
    I, dev = mixture_inputs(), eng.to_device
    u = dev(host_uniforms(lo, hi, I.p)) if inject else None
    return {"x": eng.mixture_allocation(dev(I.y[lo:hi]), dev(I.prior), dev(I.mean), dev(I.prec), u=u, draw_index=DRAW)}


@row("mixture_normal_gamma", stream="1e-12")
def _mixture_normal_gamma(eng, lo, hi, inject):
    I, dev = mixture_inputs(), eng.to_device
    g = None
    if inject:  # component k: the gamma stream of the draw index from block (k + 1) << 24 on
        g = np.empty((hi - lo, I.K))
        for c in range(lo, hi):
            for k in range(I.K):
                g[c - lo, k] = pm.standard_gamma(SEED, DRAW, OFFSET + c, I.a0[k] + 0.5 * np.sum(I.alloc[c] == k),
                                                 block0=pm.mixture_component_block0(k))
        g = dev(g)
    return {"x": eng.mixture_normal_gamma(dev(I.resid[lo:hi]), dev(I.alloc[lo:hi]), dev(I.a0), dev(I.b0), g=g, draw_index=DRAW)}


# ---------------------------------------------------------------------------------------------------------------- part A
@pytest.mark.parametrize("name", list(ROWS))
def test_shards_give_the_bits_of_one_context(name):
    r = ROWS[name]
    whole = run(r, 0, C_ALL)
    parts = [run(r, lo, hi) for lo, hi in SHARDS]
    for key, want in whole.items():
        got = np.concatenate([p[key] for p in parts])
        assert want.shape[0] == C_ALL and got.shape == want.shape, (name, key)
        assert not np.any(np.isnan(want)), (name, key)
        differ = np.flatnonzero(np.any((got != want).reshape(C_ALL, -1), axis=1))
        assert differ.size == 0, (name, key, "chains that differ", differ[:10].tolist(), differ.size)
    # the chains are different streams: a kernel that ignored the chain id altogether would pass the comparison above
    # (rows whose outputs are a few integers have no such check: part B holds them to the host model)
    if r.primary is not None:
        prim = whole[r.primary].reshape(C_ALL, -1)
        assert len({row_.tobytes() for row_ in prim}) > C_ALL // 2, (name, "chains share their draws")
        # ... and so are two chains whose ids differ in the high word alone: chain 3 (global id 2^32) with its own inputs
        # in a context at global id 0.  A kernel that dropped the high word of the chain id passes every comparison above.
        alias = run(r, 3, 4, offset=OFFSET - 2**32)[r.primary].reshape(-1)
        assert not np.array_equal(alias, prim[3]), (name, "global chains 0 and 2^32 share their draws")


# ---------------------------------------------------------------------------------------------------------------- part B
@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r.stream is not None])
def test_draws_made_in_the_kernel_are_the_streams_of_the_map(name):
    r = ROWS[name]
    drawn = run(r, 0, C_B)
    injected = run(r, 0, C_B, inject=True)
    for key, want in injected.items():
        got = drawn[key]
        if r.stream == "bits":
            assert np.array_equal(got, want), (name, key, float(np.max(np.abs(got.astype(float) - want.astype(float)))))
        else:
            assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (name, key, float(np.max(np.abs(got - want) / np.abs(want))))


def test_tridiagonal_and_band_scan_read_the_same_uniforms():
    """k_tridiag_gibbs_truncated restates Philox inline (two sites per block, c3 assembled by hand), k_band_gibbs_truncated goes
    through omc_elem_uniform: on the same matrix (tridiagonal terms / band storage with w = 1), seed, draw index and offset both
    equal their own run with the host model's uniforms injected (bits), and each other to RTOL (their arithmetic differs)."""
    n = 130
    I = scan_inputs(n)
    eng = make_engine(C_B)
    dev = eng.to_device
    band = np.zeros((2, n))
    band[0], band[1, : n - 1] = I.d1, I.o1
    tri = [{"diag": dev(I.d1), "off": dev(I.o1), "scale": dev(I.lam[:C_B])}, {"rhs": dev(I.y), "scale": dev(I.tau[:C_B])}]
    bnd = [{"band": dev(band), "scale": dev(I.lam[:C_B])}, {"rhs": dev(I.y), "scale": dev(I.tau[:C_B])}]
    kw = dict(lower=dev(I.lower), upper=dev(I.upper), rhs_chain=dev(I.rc[:C_B]), draw_index=DRAW)
    u = dev(host_uniforms(0, C_B, n))
    res = {}
    for tag, inj in (("drawn", None), ("injected", u)):
        res["tri", tag] = host(eng.tridiag_gibbs_truncated(n, tri, dev(I.x0[:C_B]), u=inj, **kw))
        res["band", tag] = host(eng.band_gibbs_truncated(n, bnd, dev(I.x0[:C_B]), u=inj, **kw))
    eng.check_status()
    eng.close()
    assert np.array_equal(res["tri", "drawn"], res["tri", "injected"])
    assert np.array_equal(res["band", "drawn"], res["band", "injected"])
    a, b = res["tri", "drawn"], res["band", "drawn"]
    assert np.max(np.abs(a - b) / np.maximum(1e-3, np.abs(b))) < RTOL
    assert not np.array_equal(a[0], a[1])


# ------------------------------------------------------------------- the band and dense scans against the reference's scan
def padded(eng, a, pad=3):
    """(view of the first n columns, the whole tensor): rows of stride n + pad, the padding filled with SENTINEL."""
    full = eng.full((a.shape[0], a.shape[1] + pad), SENTINEL)
    full[:, : a.shape[1]] = eng.to_device(a)
    return full[:, : a.shape[1]], full


def padding_untouched(full, n):
    return bool((full[:, n:] == SENTINEL).all().item())


def scan_error(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(1e-3, np.abs(ref))))


@pytest.mark.parametrize("C", [3, 65])
@pytest.mark.parametrize("n,w", [(1, 0), (2, 1), (3, 5), (7, 2), (70, 5)])
def test_band_scan_with_several_terms_against_the_reference(n, w, C):
    """Three terms of different bandwidth (identity, bw <= 2, bw <= 5, each capped at w) and a term that is a right-hand side
    only, per-chain scales, per-site limits, rhs_chain / u / x as row-padded views: against oracle.gmrf_ref.gibbs_truncated_scan
    with the same uniforms."""
    from oracle import gmrf_ref

    rng = np.random.default_rng(100 * n + 10 * w + C)
    eng = make_engine(C)
    dev = eng.to_device
    bws = (min(2, w), min(5, w))
    Ms = [band_spd(rng, n, w, bw) if bw else np.diag(1.0 + rng.random(n)) for bw in bws]
    s = 0.5 + rng.random((4, C))
    y0, y3 = rng.standard_normal(n), rng.standard_normal(n)
    lower, upper = limits(rng, n)
    x0 = np.clip(rng.standard_normal((C, n)), lower + 0.01, upper - 0.01)
    u, rc = rng.random((C, n)), 0.5 * rng.standard_normal((C, n))
    terms = [{"rhs": dev(y0), "scale": dev(s[0])},  # identity
             {"band": dev(band_rows(Ms[0], bws[0])), "scale": dev(s[1])},
             {"band": dev(band_rows(Ms[1], bws[1])), "scale": dev(s[2])},
             {"band": eng.zeros(1, n), "rhs": dev(y3), "scale": dev(s[3])}]  # a right-hand side only: a zero matrix
    T, w_terms = eng.band_terms(terms, n)
    assert w_terms == max(bws)
    (xv, xf), (uv, uf), (rv, rf) = padded(eng, x0), padded(eng, u), padded(eng, rc)
    eng.band_gibbs_truncated(n, (T, w), xv, lower=dev(lower), upper=dev(upper), u=uv, rhs_chain=rv)
    eng.check_status()
    got = host(xv)
    assert padding_untouched(xf, n) and padding_untouched(uf, n) and padding_untouched(rf, n)
    assert np.array_equal(host(uv), u) and np.array_equal(host(rv), rc)
    worst = 0.0
    for c in sorted({*range(0, C, max(1, C // 5)), C - 1}):  # (C = 65: chain 64 is alone in the second block of 64 lanes)
        Q = s[0, c] * np.eye(n) + s[1, c] * Ms[0] + s[2, c] * Ms[1]
        b = rc[c] + s[0, c] * y0 + s[3, c] * y3
        worst = max(worst, scan_error(got[c], gmrf_ref.gibbs_truncated_scan(b, Q, x0[c], lower, upper, u[c]).ravel()))
    assert worst < RTOL, worst
    assert np.all(got >= lower) and np.all(got <= upper)
    eng.close()


@pytest.mark.parametrize("p", [1, 63, 64, 65, 130])
def test_dense_scan_with_two_terms_against_the_reference(p):
    """A matrix term and an identity term (mat=None), per-chain scales, per-site limits, rhs_chain / u / x row-padded."""
    from oracle import gmrf_ref

    C = 3
    rng = np.random.default_rng(200 + p)
    eng = make_engine(C)
    dev = eng.to_device
    M = random_spd(rng, p)
    s = 0.5 + rng.random((2, C))
    y0, y1 = rng.standard_normal(p), rng.standard_normal(p)
    lower, upper = limits(rng, p)
    x0 = np.clip(rng.standard_normal((C, p)), lower + 0.01, upper - 0.01)
    u, rc = rng.random((C, p)), 0.5 * rng.standard_normal((C, p))
    terms = [{"mat": dev(M), "rhs": dev(y0), "scale": dev(s[0])}, {"rhs": dev(y1), "scale": dev(s[1])}]
    (xv, xf), (uv, uf), (rv, rf) = padded(eng, x0), padded(eng, u), padded(eng, rc)
    eng.dense_gibbs_truncated(p, terms, xv, lower=dev(lower), upper=dev(upper), u=uv, rhs_chain=rv)
    eng.check_status()
    got = host(xv)
    assert padding_untouched(xf, p) and padding_untouched(uf, p) and padding_untouched(rf, p)
    for c in range(C):
        Q = s[0, c] * M + s[1, c] * np.eye(p)
        b = rc[c] + s[0, c] * y0 + s[1, c] * y1
        err = scan_error(got[c], gmrf_ref.gibbs_truncated_scan(b, Q, x0[c], lower, upper, u[c]).ravel())
        assert err < RTOL, (c, err)
    assert np.all(got >= lower) and np.all(got <= upper)
    eng.close()


@pytest.mark.parametrize("p", [6145, 8192])
def test_dense_scan_at_large_orders(p):
    """p = 6145: the first order whose LDS request (8 p bytes) passes 48 KB; p = 8192: the entry point's limit.  A matrix that
    is sparse in value (a tridiagonal plus the identity term), written into a dense array on the device; two chains.  The
    reference's scan takes 0.4 ms a site on the host, so the two chains are given the same inputs: chain 1 (the one whose rows
    do not start at the base pointers) is compared with the reference, chain 0 must equal chain 1 bit for bit."""
    import torch
    from scipy import sparse

    from oracle import gmrf_ref

    C = 2
    rng = np.random.default_rng(300 + p)
    eng = make_engine(C)
    dev = eng.to_device
    d = 2.0 + rng.random(p)
    o = -0.8 * rng.random(p - 1)
    M = eng.zeros(p, p)
    idx = torch.arange(p, device=eng.device)
    M[idx, idx] = dev(d)
    M[idx[:-1], idx[1:]] = dev(o)
    M[idx[1:], idx[:-1]] = dev(o)
    s = np.tile(0.5 + rng.random((2, 1)), (1, C))
    y = rng.standard_normal(p)
    lower, upper = limits(rng, p)
    x0 = np.tile(np.clip(rng.standard_normal(p), lower + 0.01, upper - 0.01), (C, 1))
    u = np.tile(rng.random(p), (C, 1))
    x = dev(x0)
    eng.dense_gibbs_truncated(p, [{"mat": M, "scale": dev(s[0])}, {"rhs": dev(y), "scale": dev(s[1])}], x, lower=dev(lower),
                              upper=dev(upper), u=dev(u))
    eng.check_status()
    got = host(x)
    P = sparse.diags((o, d, o), offsets=[-1, 0, 1], format="csr")
    assert np.array_equal(got[0], got[1])
    c = 1
    Q = (s[0, c] * P + s[1, c] * sparse.identity(p, format="csr")).tocsr()
    err = scan_error(got[c], gmrf_ref.gibbs_truncated_scan(s[1, c] * y, Q, x0[c], lower, upper, u[c]).ravel())
    assert err < RTOL, err
    assert np.all(got >= lower) and np.all(got <= upper)
    eng.close()


@pytest.mark.parametrize("kind", ["tridiag", "band", "dense"])
def test_scan_failure_latch_names_the_chain(kind):
    """One chain of five has a negative scale on its matrix term, so its Q_ii <= 0: check_status raises LinAlgError naming
    it, and the other four chains still equal the reference."""
    from oracle import gmrf_ref

    n, C, bad = 40, 5, 3
    rng = np.random.default_rng(400)
    eng = make_engine(C)
    dev = eng.to_device
    d, o = 2.0 + rng.random(n), -0.8 * rng.random(n - 1)
    Q1 = np.diag(d) + np.diag(o, 1) + np.diag(o, -1)
    lam, tau = 1.0 + rng.random(C), 0.5 + rng.random(C)
    lam[bad] = -2.0
    y = rng.standard_normal(n)
    lower, upper = limits(rng, n)
    x0 = np.clip(rng.standard_normal((C, n)), lower + 0.01, upper - 0.01)
    u = rng.random((C, n))
    x = dev(x0)
    kw = dict(lower=dev(lower), upper=dev(upper), u=dev(u))
    rhs = {"rhs": dev(y), "scale": dev(tau)}
    if kind == "tridiag":
        eng.tridiag_gibbs_truncated(n, [{"diag": dev(d), "off": dev(o), "scale": dev(lam)}, rhs], x, **kw)
    elif kind == "band":
        eng.band_gibbs_truncated(n, [{"band": dev(band_rows(Q1, 1)), "scale": dev(lam)}, rhs], x, **kw)
    else:
        eng.dense_gibbs_truncated(n, [{"mat": dev(Q1), "scale": dev(lam)}, rhs], x, **kw)
    with pytest.raises(np.linalg.LinAlgError, match=rf"chain {bad}\b"):
        eng.check_status()
    eng.check_status()  # the latch is cleared by reading it
    got = host(x)
    for c in range(C):
        if c != bad:
            Q = lam[c] * Q1 + tau[c] * np.eye(n)
            assert scan_error(got[c], gmrf_ref.gibbs_truncated_scan(tau[c] * y, Q, x0[c], lower, upper, u[c]).ravel()) < RTOL, c
    eng.close()


def test_scan_argument_checks_leave_x_alone():
    import ctypes

    from openmcmc_amd import _abi

    n, C = 12, 3
    eng = make_engine(C)
    x0 = np.random.default_rng(500).standard_normal((C, n))

    def refused(error, call):
        """OMC_INVALID_ARG surfaces as ValueError, OMC_UNSUPPORTED as NotImplementedError (_abi.check)."""
        x = eng.to_device(x0)
        with pytest.raises(error):
            call(x)
        eng.check_status()
        assert np.array_equal(host(x), x0)

    ones = eng.full((n,), 2.0)
    # a per-chain centre on a tridiagonal term: the exact draw only
    refused(NotImplementedError, lambda x: eng.tridiag_gibbs_truncated(n, [{"diag": ones, "center_chain": eng.zeros(C, n)}], x))
    # a band term wider than w
    T, _ = eng.band_terms([{"band": eng.full((3, n), 1.0)}], n)
    refused(ValueError, lambda x: eng.band_gibbs_truncated(n, (T, 1), x))
    # w > 128
    T0, _ = eng.band_terms([{"band": eng.full((1, n), 2.0)}], n)
    refused(ValueError, lambda x: eng.band_gibbs_truncated(n, (T0, 129), x))
    # a row stride below n, in each of the three entry points (through the C ABI: the Python layer has no way to say it)
    tri = eng.tridiag_terms([{"diag": ones}], n)
    dns = eng.dense_terms([{"mat": None}], n)

    def short_stride(which):
        def call(x):
            p, nul = ctypes.c_void_p(x.data_ptr()), None
            if which == "tridiag":
                st = _abi.lib.omc_tridiag_gibbs_truncated(eng._ctx, n, ctypes.byref(tri), nul, 0, nul, nul, nul, 0, 0, p, n - 1)
            elif which == "band":
                st = _abi.lib.omc_band_gibbs_truncated(eng._ctx, n, 0, ctypes.byref(T0), nul, 0, nul, nul, nul, 0, 0, p, n - 1)
            else:
                st = _abi.lib.omc_dense_gibbs_truncated(eng._ctx, n, ctypes.byref(dns), nul, 0, nul, nul, nul, 0, 0, p, n - 1)
            _abi.check(st)
        return call

    for which in ("tridiag", "band", "dense"):
        refused(ValueError, short_stride(which))
    # p > 8192: refused before anything is read (x of one row's length is enough: nothing is written)
    big = eng.dense_terms([{"mat": None}], 8193)
    xb = eng.zeros(C, 8193)
    with pytest.raises(ValueError):
        eng.dense_gibbs_truncated(8193, big, xb)
    assert not xb.any().item()
    eng.close()
