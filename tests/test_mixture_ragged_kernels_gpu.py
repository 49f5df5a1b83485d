"""Kernels of the mixture, reversible-jump and ragged-parameter models, called directly through Engine at the shapes where
their launch maths and wave loops change (chains not a multiple of four, lengths around the stride of 64, counts 0, 1,
kmax - 1 and kmax, K up to the entry-point limit of 255), against plain float64 / SciPy restatements of the reference
operations.  The in-kernel draws are recomputed from tests/philox_model.py, or tested in law where the arithmetic is
libm-deep (the Gamma draws of the mixture precisions).

Tolerances: 1e-13 relative to the size of the terms summed (a sum of terms of mixed sign is only as exact as its largest
term), 1e-12 for the long reductions (n up to 40 000); integer-valued results exactly."""

import math

import numpy as np
import pytest
import torch
from scipy import stats

import philox_model as pm

pytestmark = pytest.mark.gpu

LOG2PI = 1.8378770664093453
EPS = np.finfo(np.float64).eps
CHAINS = [1, 3, 4, 5, 257]
LENGTHS = [1, 2, 63, 64, 65, 130, 1000]


def make_engine(C, seed=0, offset=0):
    from openmcmc_amd.engine import Engine

    return Engine(C, seed=seed, chain_id_offset=offset)


def host(t):
    return t.cpu().numpy()


def assert_close(got, ref, scale, rtol=1e-13):
    """Equal infinities and NaNs in place; finite entries within rtol * scale (scale: the size of the terms)."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    scale = np.broadcast_to(np.asarray(scale, dtype=float), ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), (got, ref)
    err = np.abs(got[fin] - ref[fin])
    bar = rtol * np.maximum(np.abs(scale[fin]), np.abs(ref[fin])) + 1e-300
    assert np.all(err <= bar), f"max err / bar {np.max(err / bar)}"


def edge_counts(rng, C, kmax):
    """Per-chain live lengths: 0, 1, kmax - 1 and kmax first, then random."""
    base = [0, 1, max(kmax - 1, 0), kmax]
    cnt = np.array([base[c] if c < 4 else rng.integers(0, kmax + 1) for c in range(C)], dtype=float)
    return cnt


# ---------------------------------------------------------------------------------------------------- A. densities
@pytest.mark.parametrize("C", CHAINS)
@pytest.mark.parametrize("kmax", LENGTHS)
def test_diag_gauss_logpdf_and_grad(C, kmax):
    rng = np.random.default_rng(100 * C + kmax)
    x, m = rng.standard_normal((C, kmax)), rng.standard_normal((C, kmax))
    prec = rng.uniform(0.1, 10.0, (C, kmax))
    cnt = edge_counts(rng, C, kmax)
    eng = make_engine(C)
    X, M, P, N = (eng.to_device(a) for a in (x, m, prec, cnt))
    prev = rng.standard_normal(C)
    for mean in (None, M):
        for count in (None, N):
            k = cnt if count is not None else np.full(C, kmax)
            live = np.arange(kmax)[None, :] < k[:, None]
            r = x - (m if mean is not None else 0.0)
            terms = np.where(live, np.log(prec) - LOG2PI - prec * r * r, 0.0)
            ref = 0.5 * terms.sum(axis=1)
            scale = 0.5 * np.abs(terms).sum(axis=1) + 1.0
            for acc in (False, True):
                out = eng.to_device(prev)
                eng.diag_gauss_logpdf(X, P, out, mean=mean, count=count, accumulate=acc)
                assert_close(host(out), ref + (prev if acc else 0.0), scale + (np.abs(prev) if acc else 0.0))
            g = host(eng.diag_gauss_grad(X, P, mean=mean, count=count))
            assert np.all(g[~live] == 0.0)  # padding reads exactly 0
            assert_close(g[live], (-prec * r)[live], np.abs(prec * r)[live], rtol=2 * EPS)
    eng.check_status()
    eng.close()


GAMMA_X = np.array([0.0, -1.0, -0.0, 5e-324, 1e-310, 1e-300, 0.25, 1.0, 3.5, 1e300])
GAMMA_SHAPES = [1e-3, 0.5, 1.0, 2.0, 1e6]


def gamma_ref(x, a, b):
    """stats.gamma.logpdf and the size of its terms (lnorm, (a - 1) log x, b x).  SciPy evaluates at x b, which underflows
    for a subnormal x and a small rate: there the same sum is restated without the rescaling."""
    from scipy import special

    x = np.asarray(x, dtype=float)
    ref = stats.gamma.logpdf(x, a, scale=1.0 / b)
    with np.errstate(divide="ignore", invalid="ignore"):
        direct = a * math.log(b) - math.lgamma(a) + special.xlogy(a - 1.0, x) - b * x
        ref = np.where((x > 0) & (np.abs(x * b) < 2.3e-308), direct, ref)
        scale = abs(a * math.log(b)) + abs(math.lgamma(a)) + np.abs((a - 1.0) * np.log(np.abs(x))) + np.abs(b * x)
    return ref, np.where(np.isfinite(scale), scale, 0.0)


@pytest.mark.parametrize("rate", [2.0, 1e-3])
@pytest.mark.parametrize("shape", GAMMA_SHAPES)
def test_gamma_logpdf_matches_scipy_at_zero_and_extremes(shape, rate):
    """The density at x = 0 is +inf for shape < 1, log(rate) for shape 1, -inf above (scipy.stats.gamma.logpdf)."""
    C = GAMMA_X.size
    ref, scale = gamma_ref(GAMMA_X, shape, rate)
    eng = make_engine(C)
    x = eng.to_device(GAMMA_X)
    out = eng.empty(C)
    eng.gamma_logpdf(x, shape, rate, out)
    assert_close(host(out), ref, scale)
    out = eng.empty(C)
    eng.log_post_sum([("gamma", x, shape, rate)], 0.0, out)
    assert_close(host(out), ref, scale)
    # the same values through the vector form, one component per chain (K = 1) ...
    out = eng.empty(C)
    eng.gamma_logpdf_vec(x.reshape(C, 1), eng.to_device([shape]), eng.to_device([rate]), out)
    assert_close(host(out), ref, scale)
    # ... and through the ragged form, one live entry per chain
    out = eng.empty(C)
    eng.gamma_logpdf_ragged(x.reshape(C, 1), shape, rate, out, count=eng.to_device(np.ones(C)))
    assert_close(host(out), ref, scale)
    eng.check_status()
    eng.close()


@pytest.mark.parametrize("C", [1, 5, 257])
@pytest.mark.parametrize("kmax", [1, 2, 65])
def test_gamma_logpdf_ragged_and_last_only(C, kmax):
    rng = np.random.default_rng(7 * C + kmax)
    x = rng.gamma(2.0, 1.0, (C, kmax))
    x[0, 0] = 0.0  # density at 0 of shape 1: log(rate)
    cnt = edge_counts(rng, C, kmax)
    a, b = 1.0, 1.7
    ref_el, sc_el = gamma_ref(x, a, b)
    eng = make_engine(C)
    X, N = eng.to_device(x), eng.to_device(cnt)
    prev = rng.standard_normal(C)
    live = np.arange(kmax)[None, :] < cnt[:, None]
    full = np.where(live, ref_el, 0.0).sum(axis=1)
    idx = np.maximum(cnt.astype(int) - 1, 0)
    last = np.where(cnt > 0, ref_el[np.arange(C), idx], 0.0)
    for last_only, ref, sc in ((False, full, np.where(live, sc_el, 0.0).sum(axis=1)),
                               (True, last, np.where(cnt > 0, sc_el[np.arange(C), idx], 0.0))):
        for acc in (False, True):
            out = eng.to_device(prev)
            eng.gamma_logpdf_ragged(X, a, b, out, count=N, last_only=last_only, accumulate=acc)
            assert_close(host(out), ref + (prev if acc else 0.0), sc + 1.0 + (np.abs(prev) if acc else 0.0))
    out = eng.empty(C)
    eng.gamma_logpdf_ragged(X, a, b, out)  # count = NULL: every entry live
    assert_close(host(out), ref_el.sum(axis=1), sc_el.sum(axis=1) + 1.0)
    eng.check_status()
    eng.close()


@pytest.mark.parametrize("C", CHAINS)
@pytest.mark.parametrize("K", [1, 2, 3, 16, 17, 255])
def test_gamma_logpdf_vec(C, K):
    rng = np.random.default_rng(11 * C + K)
    shape, rate = rng.uniform(0.2, 5.0, K), rng.uniform(0.1, 4.0, K)
    x = rng.gamma(1.5, 1.0, (C, K))
    ref_el = np.stack([gamma_ref(x[:, k], shape[k], rate[k])[0] for k in range(K)], axis=1)
    sc_el = np.stack([gamma_ref(x[:, k], shape[k], rate[k])[1] for k in range(K)], axis=1)
    eng = make_engine(C)
    prev = rng.standard_normal(C)
    for acc in (False, True):
        out = eng.to_device(prev)
        eng.gamma_logpdf_vec(eng.to_device(x), eng.to_device(shape), eng.to_device(rate), out, accumulate=acc)
        assert_close(host(out), ref_el.sum(axis=1) + (prev if acc else 0.0), sc_el.sum(axis=1) + np.abs(prev))
    eng.close()


@pytest.mark.parametrize("rate", [1e-300, 1.0, 1e6])
def test_poisson_and_count_logpdf(rate):
    x = np.array([0.0, 1.0, 2.0, 7.0, 1000.0, 2.5, -1.0, -0.0, 1e6, 0.5])
    C = x.size
    ref = stats.poisson.logpmf(x, rate)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.abs(x * math.log(rate)) + np.abs([math.lgamma(v + 1.0) if v >= 0 else 0.0 for v in x]) + rate
    eng = make_engine(C)
    X = eng.to_device(x)
    prev = np.linspace(-1.0, 1.0, C)
    for acc in (False, True):
        out = eng.to_device(prev)
        eng.poisson_logpmf(X, rate, out, accumulate=acc)
        assert_close(host(out), ref + (prev if acc else 0.0), scale + 1.0)
        out = eng.to_device(prev)
        eng.count_logpdf(eng.to_device(np.abs(x)), -math.log(rate + 3.0), out, accumulate=acc)
        expect = -math.log(rate + 3.0) * np.abs(x)
        assert np.array_equal(host(out), expect + prev if acc else expect)  # one product (and one sum) per chain
    eng.close()


@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_log_transform_with_wide_rows(C, n):
    rng = np.random.default_rng(C + n)
    wide = rng.uniform(1e-3, 1e3, (C, n + 7))
    wide[:, n:] = -1.0  # beyond the row: log would be NaN if read
    eng = make_engine(C)
    W = eng.to_device(wide)
    out, sumlog = eng.log_transform(W[:, :n])
    lx = np.log(wide[:, :n])
    assert_close(host(out), lx, np.abs(lx), rtol=2 * EPS)
    assert_close(host(sumlog), np.array([math.fsum(r) for r in lx]), np.abs(lx).sum(axis=1))
    eng.close()


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_dense_quadform_with_and_without_centres(C, n):
    rng = np.random.default_rng(3 * C + n)
    A = rng.standard_normal((n, n))
    M = A @ A.T / n + np.eye(n)
    x, m = rng.standard_normal((C, n)), rng.standard_normal(n)
    eng = make_engine(C)
    Md, X = eng.to_device(M), eng.to_device(x)
    for centre in (False, True):
        mm = m if centre else np.zeros(n)
        r = (x - mm).astype(np.longdouble)
        ref = np.einsum("ci,ij,cj->c", r, M.astype(np.longdouble), r).astype(float)
        scale = np.einsum("ci,ij,cj->c", np.abs(x) + np.abs(mm), np.abs(M), np.abs(x) + np.abs(mm))
        if centre:
            got = eng.dense_quadform(Md, X, center=eng.to_device(m), M_center=eng.to_device(M @ m))
        else:
            got = eng.dense_quadform(Md, X)
        assert_close(host(got), ref, scale, rtol=1e-13 if n < 1000 else 1e-12)
    eng.close()


@pytest.mark.parametrize("C", [1, 3, 257])
@pytest.mark.parametrize("kmax", [1, 63, 64, 65, 130])
def test_mixture_gather_fill_and_latch(C, kmax):
    rng = np.random.default_rng(5 * C + kmax)
    m = 17
    alloc = rng.integers(0, m, (C, kmax)).astype(float)
    cnt = edge_counts(rng, C, kmax)
    pa, pb = rng.standard_normal((C, m)), rng.standard_normal(m)
    live = np.arange(kmax)[None, :] < cnt[:, None]
    eng = make_engine(C)
    A, N = eng.to_device(alloc), eng.to_device(cnt)
    out = host(eng.mixture_gather(eng.to_device(pb), A, count=N, fill=-7.5))
    assert np.array_equal(out, np.where(live, pb[alloc.astype(int)], -7.5))
    out = host(eng.mixture_gather(eng.to_device(pa), A))
    assert np.array_equal(out, np.take_along_axis(pa, alloc.astype(int), axis=1))
    oa, ob = eng.mixture_gather2(A, N, eng.to_device(pa), np.nan, eng.to_device(pb), 3.0)
    assert np.array_equal(host(oa), np.where(live, np.take_along_axis(pa, alloc.astype(int), axis=1), np.nan), equal_nan=True)
    assert np.array_equal(host(ob), np.where(live, pb[alloc.astype(int)], 3.0))
    eng.check_status()
    # out of range beyond the live length: ignored; at a live entry: the chain is reported
    bad = alloc.copy()
    dead = np.argwhere(~live)
    if dead.size:
        bad[tuple(dead[0])] = m
        eng.mixture_gather(eng.to_device(pb), eng.to_device(bad), count=N)
        eng.check_status()
    livepos = np.argwhere(live)
    if livepos.size:
        c_bad = int(livepos[-1][0])
        bad[tuple(livepos[-1])] = -1.0 if c_bad % 2 else float(m)
        eng.mixture_gather2(eng.to_device(bad), N, eng.to_device(pa), 0.0, eng.to_device(pb), 0.0)
        with pytest.raises(np.linalg.LinAlgError, match=f"chain {c_bad}\\)"):
            eng.check_status()
    eng.check_status()
    eng.close()


@pytest.mark.parametrize("C", [1, 4, 5])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("K", [1, 3, 17])
def test_categorical_logpmf(C, p, K):
    rng = np.random.default_rng(C * 1000 + p * 10 + K)
    alloc = rng.integers(0, K, (C, p)).astype(float)
    eng = make_engine(C)
    prev = rng.standard_normal(C)
    for rows in (1, p):
        prob = rng.dirichlet(np.ones(K), rows)
        row = np.arange(p) if rows > 1 else np.zeros(p, dtype=int)
        lp = np.log(prob[row[None, :], alloc.astype(int)])
        for acc in (False, True):
            out = eng.to_device(prev)
            eng.categorical_logpmf(eng.to_device(alloc), eng.to_device(prob), out, accumulate=acc)
            assert_close(host(out), lp.sum(axis=1) + (prev if acc else 0.0), np.abs(lp).sum(axis=1) + np.abs(prev))
    if K > 1:  # a zero probability where an element sits gives -inf, as stats.multinomial.logpmf does
        prob = np.full((1, K), 1.0 / (K - 1))
        prob[0, 0] = 0.0
        a0 = np.ones((C, p))
        a0[0, p - 1] = 0.0
        out = eng.empty(C)
        eng.categorical_logpmf(eng.to_device(a0), eng.to_device(prob), out)
        got = host(out)
        assert got[0] == -np.inf and stats.multinomial.logpmf(np.eye(K)[0], 1, prob[0]) == -np.inf
        assert np.all(np.isfinite(got[1:]))
    eng.check_status()
    bad = alloc.copy()
    bad[C - 1, p // 2] = K
    eng.categorical_logpmf(eng.to_device(bad), eng.to_device(np.full((1, K), 1.0 / K)), eng.empty(C))
    with pytest.raises(np.linalg.LinAlgError, match=f"chain {C - 1}\\)"):
        eng.check_status()
    eng.close()


# ---------------------------------------------------------------------------------------------------- B. draws
def host_uniforms(seed, draw, chain, p, block0=0):
    x, y, z, w = pm.rng_blocks(seed, draw, "uniform", chain, block0 + np.arange((p + 1) // 2))
    u = np.empty(2 * ((p + 1) // 2))
    u[0::2], u[1::2] = pm.u53(x, y), pm.u53(z, w)
    return u[:p]


def allocation_ref(y, prior, mean, prec, u):
    """np.sum(U > cumsum(prob / total)) with the densities in the kernel's order of operations."""
    sd = 1.0 / np.sqrt(prec)
    z = (y[..., None] - mean) / sd
    dens = prior * (np.exp(-(z * z) / 2.0) / 2.5066282746310002 / sd)
    with np.errstate(invalid="ignore", divide="ignore"):
        cum = np.cumsum(dens / dens.sum(axis=-1, keepdims=True), axis=-1)
    return np.sum(u[..., None] > cum, axis=-1).astype(float)


def allocation_ref_cum(y, prior, mean, prec):
    """prob / total of one element (the increments of the kernel's running sum)."""
    sd = 1.0 / np.sqrt(prec)
    z = (y - mean) / sd
    dens = prior * (np.exp(-(z * z) / 2.0) / 2.5066282746310002 / sd)
    return dens / dens.sum()


def test_uniform_and_allocation_draws_are_the_host_words():
    C, p, K, seed, off, draw, sub = 1100, 65, 17, 0xDEADBEEF12345, (1 << 32) - 3, (5 << 32) + 77, 3
    rng = np.random.default_rng(1)
    lower, rngw = rng.standard_normal(p), rng.uniform(0.5, 3.0, p)
    eng = make_engine(C, seed=seed, offset=off)
    got = host(eng.uniform_draw(eng.to_device(lower), eng.to_device(rngw), draw_index=draw, sub=sub))
    y = rng.standard_normal((C, p)) * 3
    prior = rng.dirichlet(np.ones(K), p)
    mean, prec = rng.standard_normal(K) * 2, rng.uniform(0.2, 3.0, K)
    alloc = host(eng.mixture_allocation(eng.to_device(y), eng.to_device(prior), eng.to_device(mean), eng.to_device(prec),
                                        draw_index=draw))
    for c in range(C):
        u = host_uniforms(seed, draw, off + c, p, block0=sub)
        assert np.array_equal(got[c], lower + rngw * u), c
        ua = host_uniforms(seed, draw, off + c, p)
        assert np.array_equal(alloc[c], allocation_ref(y[c], prior, mean, prec, ua)), c
    eng.check_status()
    eng.close()


def test_allocation_ties_and_underflow():
    """u exactly on a cumulative boundary stays below it, the next double above goes past it; u = 1 and the smallest u;
    densities that all underflow give 0/0 in the reference and allocation 0."""
    K = 4
    prior = np.array([[0.5, 0.25, 0.125, 0.125]])
    mean, prec = np.zeros((3, K)), np.ones((3, K))
    bounds = np.cumsum(allocation_ref_cum(0.0, prior[0], mean[0], prec[0]))
    us = np.concatenate([bounds, np.nextafter(bounds, 2.0)[:K - 1], np.nextafter(bounds, 0.0), [1.0, 2.0**-53]])
    C, p = 3, us.size
    y = np.zeros((C, p))
    y[2] = 1e3  # 1e3 standard deviations from every mean: every density is 0
    u = np.tile(us, (C, 1))
    eng = make_engine(C)
    alloc = host(eng.mixture_allocation(eng.to_device(y), eng.to_device(prior), eng.to_device(mean), eng.to_device(prec),
                                        u=eng.to_device(u)))
    expect = np.sum(us[:, None] > bounds[None, :], axis=1).astype(float)
    assert np.array_equal(alloc[0], expect) and np.array_equal(alloc[1], expect)
    assert np.array_equal(alloc[0], allocation_ref(y[0], prior[0], mean[0], prec[0], us))
    assert np.array_equal(alloc[2], np.zeros(p))
    assert np.array_equal(alloc[2], allocation_ref(y[2], prior[0], mean[0], prec[0], us))
    eng.close()


@pytest.mark.parametrize("C,p,K", [(1, 1, 1), (5, 65, 3), (3, 130, 17), (4, 1000, 255)])
def test_mixture_normal_gamma_statistics_with_injected_g(C, p, K):
    """out = g / (b0 + ss_k / 2): dyadic residuals make ss_k exact, so the result is exact; empty components keep b0."""
    rng = np.random.default_rng(C + p + K)
    alloc = rng.integers(0, min(K, 5) if K > 16 else K, (C, p)).astype(float)  # K > 16: most components empty
    resid = rng.integers(-40, 41, (C, p)) / 8.0
    a0, b0 = rng.uniform(0.5, 3.0, K), rng.uniform(0.5, 3.0, K)
    g = rng.gamma(2.0, 1.0, (C, K))
    eng = make_engine(C)
    out = host(eng.mixture_normal_gamma(eng.to_device(resid), eng.to_device(alloc), eng.to_device(a0), eng.to_device(b0),
                                        g=eng.to_device(g)))
    ss = np.stack([((alloc == k) * resid**2).sum(axis=1) for k in range(K)], axis=1)
    assert np.array_equal(out, g * (1.0 / (b0 + 0.5 * ss)))
    # residuals of any value: the sums within 1e-13 of their size
    resid = rng.standard_normal((C, p))
    out = host(eng.mixture_normal_gamma(eng.to_device(resid), eng.to_device(alloc), eng.to_device(a0), eng.to_device(b0),
                                        g=eng.to_device(g)))
    ss = np.stack([((alloc == k) * resid**2).sum(axis=1) for k in range(K)], axis=1)
    assert_close(out, g / (b0 + 0.5 * ss), g / (b0 + 0.5 * ss))
    eng.check_status()
    eng.close()


def _mixture_problem(C, p=40, K=4):
    rng = np.random.default_rng(12)
    alloc1 = np.repeat(np.arange(K - 1), p // (K - 1) + 1)[:p].astype(float)  # component K - 1 empty
    resid1 = rng.standard_normal(p)
    a0 = np.array([0.3, 2.0, 1.0, 0.5][:K])  # one component with a < 1 after its data: the boost path
    b0 = np.array([1.0, 0.5, 2.0, 1.5][:K])
    alloc1[:1] = 0.0
    return np.tile(alloc1, (C, 1)), np.tile(resid1, (C, 1)), a0, b0


def test_mixture_normal_gamma_draws_in_law():
    C, K = 20000, 4
    alloc, resid, a0, b0 = _mixture_problem(C, K=K)
    a0[0] = 1e-3  # n_0 >= 1: shape >= 0.5
    eng = make_engine(C, seed=321)
    out = host(eng.mixture_normal_gamma(eng.to_device(resid), eng.to_device(alloc), eng.to_device(a0), eng.to_device(b0),
                                        draw_index=9))
    eng.check_status()
    for k in range(K):
        sel = alloc[0] == k
        a, b = a0[k] + 0.5 * sel.sum(), b0[k] + 0.5 * np.sum(resid[0][sel] ** 2)
        assert stats.kstest(out[:, k], "gamma", args=(a, 0, 1 / b)).pvalue > 1e-3, k
    r = np.corrcoef(np.log(out).T)
    assert np.max(np.abs(r - np.eye(K))) < 4.5 / np.sqrt(C)  # components are independent streams
    eng.close()


def test_mixture_normal_gamma_streams_are_the_host_model():
    """Component k reads the gamma stream of its draw index from block (k + 1) << 24 on (the field map of omc_common.h)."""
    C, K, seed, off, draw = 6, 4, 77, (1 << 33) + 2, 5
    alloc, resid, a0, b0 = _mixture_problem(C, K=K)
    eng = make_engine(C, seed=seed, offset=off)
    out = host(eng.mixture_normal_gamma(eng.to_device(resid), eng.to_device(alloc), eng.to_device(a0), eng.to_device(b0),
                                        draw_index=draw))
    for c in range(C):
        for k in range(K):
            sel = alloc[c] == k
            a, b = a0[k] + 0.5 * sel.sum(), b0[k] + 0.5 * np.sum(resid[c][sel] ** 2)
            g = pm.standard_gamma(seed, draw, off + c, a, block0=pm.mixture_component_block0(k))
            assert abs(out[c, k] - g / b) <= 1e-12 * (g / b), (c, k)
    eng.close()


def test_mixture_components_do_not_share_streams_with_other_gamma_draws():
    """Component k at draw index d and a plain Gamma draw at d + k 2^40 (a prior draw: (1 << 40) + position) or at
    d + (k / 16) 2^44 (a `sub` stream) read different uniforms."""
    C, K, d = 512, 17, 3
    eng = make_engine(C, seed=5)
    alloc, resid = eng.zeros(C, 1), eng.zeros(C, 1)  # every component: Gamma(a0, rate b0) with no data but component 0
    a0, b0 = np.full(K, 2.5), np.ones(K)
    mix = host(eng.mixture_normal_gamma(resid, alloc, eng.to_device(a0), eng.to_device(b0), draw_index=d))
    for k, other in ((0, d), (1, d + (1 << 40)), (2, d + (2 << 40)), (16, d + (1 << 44))):
        a = a0[k] + (0.5 if k == 0 else 0.0)
        plain = eng.empty(C)
        eng.normal_gamma_update(a, 1.0, 0, eng.zeros(C), plain, draw_index=other)
        same = np.abs(mix[:, k] - host(plain)) <= 1e-12 * np.abs(host(plain))
        assert same.mean() < 0.01, (k, same.mean())
    eng.check_status()
    eng.close()


def test_mixture_normal_gamma_repeatable_and_shard_invariant():
    C, K = 10, 4
    alloc, resid, a0, b0 = _mixture_problem(C, K=K)
    rng = np.random.default_rng(3)
    resid = resid + 0.1 * rng.standard_normal(resid.shape)

    def run(n, offset, lo):
        eng = make_engine(n, seed=99, offset=offset)
        o = host(eng.mixture_normal_gamma(eng.to_device(resid[lo:lo + n]), eng.to_device(alloc[lo:lo + n]),
                                          eng.to_device(a0), eng.to_device(b0), draw_index=4))
        eng.check_status()
        eng.close()
        return o

    full = run(C, 0, 0)
    assert np.array_equal(full, run(C, 0, 0))
    assert np.array_equal(full, np.concatenate([run(4, 0, 0), run(6, 4, 4)]))


# ---------------------------------------------------------------------------------------------------- D. small matrices
@pytest.mark.parametrize("kmax", [1, 21, 22, 36])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 1023, 1024, 1025, 40000])
def test_design_gram_batched_and_select(kmax, n):
    C = 4 if n < 40000 else 3  # few chains: the rows split into up to 16 parts
    rng = np.random.default_rng(kmax * 100003 + n)
    B, B_alt = rng.standard_normal((C, kmax, n)), rng.standard_normal((C, kmax, n))
    w, rs, rc = rng.uniform(0.5, 2.0, n), rng.standard_normal(n), rng.standard_normal((C, n))
    cnt = np.array([0, kmax, max(kmax - 1, 0), 1][:C], dtype=float)
    cnt_alt = np.array([kmax, 0, 1, max(kmax - 1, 0)][:C], dtype=float)
    sel = np.array([0, 1, 1, 0][:C], dtype=np.int32)
    rtol = 1e-12

    def ref(Bm, k, r=None):
        live = (np.arange(kmax) < k)
        Bl = Bm * live[:, None]
        G = np.einsum("ai,i,bi->ab", Bl, w, Bl)
        Gs = np.einsum("ai,i,bi->ab", np.abs(Bl), w, np.abs(Bl))
        if r is None:
            return G, Gs
        return G, Gs, Bl @ (w * r), np.abs(Bl) @ (w * np.abs(r))

    eng = make_engine(C)
    Bd, Bad, Wd = eng.to_device(B), eng.to_device(B_alt), eng.to_device(w)
    gram, rhs = eng.design_gram_batched(Bd, w=Wd, resid_shared=eng.to_device(rs), resid_chain=eng.to_device(rc),
                                        count=eng.to_device(cnt))
    gram, rhs = host(gram), host(rhs)
    for c in range(C):
        G, Gs, g, gs = ref(B[c], cnt[c], rs - rc[c])
        assert_close(gram[c], G, Gs, rtol)
        assert_close(rhs[c], g, gs, rtol)
        k = int(cnt[c])
        assert np.all(gram[c][k:, :] == 0.0) and np.all(gram[c][:, k:] == 0.0) and np.all(rhs[c][k:] == 0.0)
    sel_d = torch.as_tensor(sel, device=eng.device)
    gram = host(eng.design_gram_select(Bd, eng.to_device(cnt), Bad, eng.to_device(cnt_alt), sel_d, w=Wd))
    for c in range(C):
        G, Gs = ref(B_alt[c], cnt_alt[c]) if sel[c] else ref(B[c], cnt[c])
        assert_close(gram[c], G, Gs, rtol)
    eng.check_status()
    eng.close()


@pytest.mark.parametrize("kmax", [1, 2, 7, 31, 63, 64])
def test_small_sample_canonical_against_cholesky(kmax):
    C = 5
    rng = np.random.default_rng(kmax)
    X = rng.standard_normal((C, kmax, 2 * kmax + 3))
    G = np.einsum("cin,cjn->cij", X, X)
    g = rng.standard_normal((C, kmax))
    prior_prec, prior_mean = rng.uniform(0.5, 2.0, (C, kmax)), rng.standard_normal((C, kmax))
    tau, z = rng.uniform(0.5, 2.0, C), rng.standard_normal((C, kmax))
    cnt = edge_counts(rng, C, kmax)
    eng = make_engine(C)
    mu_out = eng.empty(C, kmax)
    x = host(eng.small_sample_canonical(eng.to_device(G), eng.to_device(g), eng.to_device(prior_prec),
                                        lik_scale=eng.to_device(tau), prior_mean=eng.to_device(prior_mean),
                                        count=eng.to_device(cnt), z=eng.to_device(z), mean_out=mu_out))
    mu = host(mu_out)
    eng.check_status()
    for c in range(C):
        k = int(cnt[c])
        assert np.all(x[c, k:] == 0.0) and np.all(mu[c, k:] == 0.0)
        if k == 0:
            continue
        Q = tau[c] * G[c, :k, :k] + np.diag(prior_prec[c, :k])
        b = tau[c] * g[c, :k] + prior_prec[c, :k] * prior_mean[c, :k]
        L = np.linalg.cholesky(Q)
        m = np.linalg.solve(Q, b)
        v = np.linalg.solve(L.T, z[c, :k])
        cond = np.linalg.cond(Q)
        # a solve is exact to about k eps cond(Q) of the solution's size
        bar = max(4 * k * EPS * cond, 1e-13)
        assert_close(mu[c, :k], m, np.max(np.abs(m)), bar)
        assert_close(x[c, :k], m + v, np.max(np.abs(m)) + np.max(np.abs(v)), bar)
    eng.close()


def spd_with_condition(rng, C, k, cond):
    """A = Q diag(lam) Q' with log-spaced eigenvalues 1 .. cond: log det A = sum log lam exactly, up to the rounding of A."""
    A = np.empty((C, k, k))
    logdet = np.empty(C)
    for c in range(C):
        Q, _ = np.linalg.qr(rng.standard_normal((k, k)))
        lam = np.logspace(0.0, np.log10(cond), k) if k > 1 else np.array([cond])
        A[c] = (Q * lam) @ Q.T
        A[c] = 0.5 * (A[c] + A[c].T)
        logdet[c] = math.fsum(np.log(lam))
    return A, logdet


@pytest.mark.parametrize("k", [1, 2, 31, 63, 64, 65])
@pytest.mark.parametrize("cond", [10.0, 1e6, 1e12])
def test_small_spd_ops_and_the_switch_to_chain_spd_ops(k, cond):
    """k <= 64: omc_small_spd_ops; k = 65: Engine.chain_spd_ops (ManifoldMALA's switch), the same inputs and bars.
    log det from the construction; forming A rounds it by eps |A|, which moves log det by up to k eps cond(A)."""
    C = 5
    rng = np.random.default_rng(k + int(math.log10(cond)))
    A, logdet = spd_with_condition(rng, C, k, cond)
    v = rng.standard_normal((C, k))
    eng = make_engine(C)
    ops = eng.small_spd_ops if k <= 64 else eng.chain_spd_ops
    Ad, vd = eng.to_device(A), eng.to_device(v)
    Av, quad, ld = ops(Ad, vd, want_Av=True, want_quad=True, want_logdet=True)
    eng.check_status()
    ref_av = np.einsum("cij,cj->ci", A.astype(np.longdouble), v.astype(np.longdouble)).astype(float)
    av_scale = np.einsum("cij,cj->ci", np.abs(A), np.abs(v))
    assert_close(host(Av), ref_av, av_scale, 1e-13)
    ref_q = np.einsum("ci,ci->c", v.astype(np.longdouble), ref_av.astype(np.longdouble)).astype(float)
    assert_close(host(quad), ref_q, np.einsum("ci,ci->c", np.abs(v), av_scale), 1e-13)
    sign, ld_np = np.linalg.slogdet(A)
    assert np.all(sign == 1.0)
    bar = 8 * k * EPS * cond + 1e-13 * np.abs(logdet)
    assert np.all(np.abs(host(ld) - logdet) <= bar), (host(ld) - logdet, bar)
    assert np.all(np.abs(ld_np - logdet) <= bar)  # the bar holds for LAPACK too
    eng.close()


@pytest.mark.parametrize("k", [63, 64, 65])
def test_non_positive_definite_chain_is_reported(k):
    C = 4
    rng = np.random.default_rng(k)
    A, _ = spd_with_condition(rng, C, k, 10.0)
    A[2] -= 5.0 * np.eye(k)  # chain 2: indefinite (eigenvalues -4 .. 5)
    eng = make_engine(C)
    Ad, vd = eng.to_device(A), eng.to_device(rng.standard_normal((C, k)))
    if k <= 64:
        _, _, ld = eng.small_spd_ops(Ad, vd, want_logdet=True)
        with pytest.raises(np.linalg.LinAlgError, match=r"chain 2\)"):
            eng.check_status()
        got = host(ld)
        assert np.isnan(got[2]) and np.all(np.isfinite(np.delete(got, 2)))
    else:
        with pytest.raises(np.linalg.LinAlgError, match=r"chain 2\)"):
            eng.chain_spd_ops(Ad, vd, want_logdet=True)
    eng.check_status()
    eng.close()


def test_store_ragged_fill():
    C, width = 5, 130
    rng = np.random.default_rng(2)
    src = rng.standard_normal((C, width))
    cnt = edge_counts(rng, C, width)
    eng = make_engine(C)
    dst = eng.full((C, width + 3), 1.5)
    eng.store_ragged(eng.to_device(src), eng.to_device(cnt), dst)
    live = np.arange(width)[None, :] < cnt[:, None]
    got = host(dst)
    assert np.array_equal(got[:, :width], np.where(live, src, np.nan), equal_nan=True)
    assert np.all(got[:, width:] == 1.5)
    eng.close()
