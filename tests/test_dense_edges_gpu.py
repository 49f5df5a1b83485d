"""omc_dense_sample_canonical at its edges: every order next to a multiple of 64 (the kernels' block width), the blocked
factor forced onto small orders, both panel forms, the two-stream split of the chains, leading dimensions larger than p,
ill-conditioned and graded matrices, orders up to 8193, and non-positive pivots met in a late panel.

The yardstick is oracle.longdouble_ref.dense_draw (natural-order Cholesky and substitutions in 64-bit-mantissa
arithmetic on the exact combination of the fp64 inputs).  Per chain, for x, mean_out and logdet_out:

  forward error   relative in the max norm (log det: relative to max(1, |log det|)) at most
                  16 * max(e64, p * 2^-53), e64 being the error the reference project's own fp64 route
                  (oracle.gmrf_ref.draw_canonical: np.linalg.cholesky, cho_solve, np.linalg.solve) makes against the same
                  longdouble answer on the same inputs.  Both are backward-stable Cholesky solves of one matrix that differ
                  in the order of accumulation only (64-wide left-looking blocks, FMA, matrix-core panel rows against
                  LAPACK's blocking): that moves the forward error by a small factor, not by a power of the condition
                  number, and 16 leaves about a digit.  The floor is there because e64 can be exactly 0.
  backward error  of the mean, componentwise: |b - Q mu| <= gamma (|L| |L'| |mu|), gamma = (3p+1)u / (1 - (3p+1)u),
                  u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.4), evaluated in longdouble
                  with the reference's L.  Q is the exact combination of the terms (the roundings of the kernel's assembly
                  of Q are inside the measured ratio).  b is the right-hand side as the entry point forms it in fp64,
                  b = fma(s_k, rhs_k, ...fma(s_0, rhs_0, rhs_chain)) (k_dense_rhs), reproduced exactly on the host and
                  given to the reference, to NumPy's route and to the residual alike: the bound is about the system that
                  is solved, and where the terms of b cancel, the roundings of forming it are no solver's to answer for
                  (measured at p = 1, seed 1001, chain 2: |b| = 0.036 from terms of 0.18, 0.39 and 0.17; against the
                  exact sum even the exact solution of the assembled system sits at 1.33 of the bound, 4u |Q| |mu|,
                  and so did the kernel; against the assembled b the kernel is at 0.27).  Above order 1000, where the
                  longdouble factor is too slow, this is the check, with NumPy's fp64 factor for L, next to a comparison
                  with NumPy at 16 p u cond(Q).
  bit equality    where the code promises it: the same call twice, dense_overlap 0 against 1.  Not across batch sizes
                  (rocBLAS may pick another GEMM kernel for another batch count).

Every test prints its worst ratios ("dense-edges ..." lines, pytest -s); profiles/dense_edges_accuracy.txt keeps them.
"""

from fractions import Fraction

import numpy as np
import pytest

from oracle import gmrf_ref
from oracle.longdouble_ref import dense_draw

pytestmark = pytest.mark.gpu

U = 2.0**-53
MARGIN = 16.0
SENTINEL = -12345.678
PAD = 5
LD = np.longdouble


def make_engine(C, **kw):
    from openmcmc_amd.engine import Engine

    return Engine(C, **kw)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def spectrum_matrices(rng, p, cond, n_mat, graded=False):
    """n_mat symmetric matrices U diag(ev * w_k) U' with one orthogonal U (QR of a Gaussian matrix), ev log-spaced from 1
    down to 1 / cond and w_k in [0.5, 1.5] (w_0 = 1): any positive combination sum_k s_k M_k has the spectrum
    ev * sum_k s_k w_k, i.e. condition number within a factor 3 of `cond`.  graded: D M_k D with D a random permutation
    of 10^(-4 .. 4) -- eight more decades between the rows, mixed inside every 64-column panel."""
    Uq, _ = np.linalg.qr(rng.standard_normal((p, p)))
    ev = cond ** (-np.arange(p) / max(p - 1, 1))
    D = rng.permutation(10.0 ** np.linspace(-4.0, 4.0, p)) if graded else None
    mats = []
    for k in range(n_mat):
        w = np.ones(p) if k == 0 else 0.5 + rng.random(p)
        M = (Uq * (ev * w)) @ Uq.T
        M = 0.5 * (M + M.T)
        if graded:
            M = D[:, None] * M * D[None, :]
            M = 0.5 * (M + M.T)
        mats.append(M)
    return mats


def make_problem(seed, p, C, cond=1e2, graded=False, n_terms=2, shared_rhs=True, rhs_chain=True):
    """Host side of one call: n_terms matrices with per-chain scales (the chains differ), shared right-hand sides,
    a per-chain right-hand side, injected draws."""
    rng = np.random.default_rng(seed)
    prob = {"p": p, "C": C, "mats": spectrum_matrices(rng, p, cond, n_terms, graded),
            "scales": [0.5 + rng.random(C) for _ in range(n_terms)],
            "rhs": [rng.standard_normal(p) if shared_rhs else None for _ in range(n_terms)],
            "rhs_chain": rng.standard_normal((C, p)) if rhs_chain else None, "diag_chain": None,
            "z": rng.standard_normal((C, p))}
    return prob


def assembled_rhs(prob, c):
    """b_c as k_dense_rhs forms it: v = rhs_chain[c] (or 0), then v = fma(s_k[c], rhs_k, v) term by term, every fma
    rounded once (exact rational arithmetic, one rounding to fp64 per step)."""
    p = prob["p"]
    v = [0.0] * p if prob["rhs_chain"] is None else [float(t) for t in prob["rhs_chain"][c]]
    for s, r in zip(prob["scales"], prob["rhs"]):
        if r is not None:
            sc = Fraction(float(s[c]))
            v = [float(sc * Fraction(float(ri)) + Fraction(vi)) for ri, vi in zip(r, v)]
    return np.array(v, dtype=np.float64)


def assemble(prob, c, dtype):
    """Q_c = sum_k s_k[c] M_k (+ diag_chain[c]) in `dtype` arithmetic, and b_c = assembled_rhs (fp64 values)."""
    p = prob["p"]
    Q = np.zeros((p, p), dtype=dtype)
    for M, s in zip(prob["mats"], prob["scales"]):
        Q += dtype(s[c]) * (np.eye(p, dtype=dtype) if M is None else M.astype(dtype))
    if prob["diag_chain"] is not None:
        Q[np.diag_indices(p)] += prob["diag_chain"][c].astype(dtype)
    return Q, assembled_rhs(prob, c).astype(dtype)


# ---- the call -------------------------------------------------------------------------------------------------------
def device_terms(eng, prob):
    return [{"mat": None if M is None else eng.to_device(M), "rhs": None if r is None else eng.to_device(r),
             "scale": eng.to_device(s)} for M, s, r in zip(prob["mats"], prob["scales"], prob["rhs"])]


def padded(eng, C, p, fill=None):
    """A (C, p) view of a (C, p + PAD) allocation filled with SENTINEL (fill: host values for the view)."""
    import torch

    wide = torch.full((C, p + PAD), SENTINEL, dtype=torch.float64, device=eng.device)
    if fill is not None:
        wide[:, :p] = eng.to_device(fill)
    return wide, wide[:, :p]


def padding_untouched(wide, p):
    return bool((wide[:, p:] == SENTINEL).all().item())


def run_draw(eng, prob, terms=None, strided=False, z="inject", draw_index=0):
    """One omc_dense_sample_canonical call; (x, mean, logdet) as host arrays.  strided: x, mean, z and rhs_chain are
    [:, :p] views of wider allocations, whose padding must come back untouched."""
    p, C = prob["p"], prob["C"]
    terms = device_terms(eng, prob) if terms is None else terms
    zh = prob["z"] if z == "inject" else None
    logdet = eng.empty(C)
    wides = []
    if strided:
        (xw, x), (mw, mean) = padded(eng, C, p), padded(eng, C, p)
        wides = [xw, mw]
        dz = dr = None
        if zh is not None:
            zw, dz = padded(eng, C, p, zh)
            wides.append(zw)
        if prob["rhs_chain"] is not None:
            rw, dr = padded(eng, C, p, prob["rhs_chain"])
            wides.append(rw)
        assert x.stride(0) == p + PAD
    else:
        x, mean = eng.empty(C, p), eng.empty(C, p)
        dz = None if zh is None else eng.to_device(zh)
        dr = None if prob["rhs_chain"] is None else eng.to_device(prob["rhs_chain"])
    dd = None if prob["diag_chain"] is None else eng.to_device(prob["diag_chain"])
    eng.dense_sample_canonical(p, terms, x, z=dz, rhs_chain=dr, draw_index=draw_index, mean_out=mean, logdet_out=logdet,
                               diag_chain=dd)
    eng.synchronize()
    for w in wides:
        assert padding_untouched(w, p), "the call wrote (or the inputs changed) beyond column p of a strided tensor"
    return x.cpu().numpy().copy(), mean.cpu().numpy().copy(), logdet.cpu().numpy().copy()


# ---- the bars -------------------------------------------------------------------------------------------------------
def maxrel(a, ref):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - ref)) / max(np.max(np.abs(ref)), 1e-300))


def chain_ratios(prob, c, x, mean, logdet):
    """(forward ratios e_gpu / max(e64, p u) of x, mean, log det; backward-error ratio of the mean against Higham's
    bound; e64 of x) for chain c.  Forward ratios up to MARGIN and a backward ratio up to 1 pass."""
    p = prob["p"]
    Qx, bx = assemble(prob, c, LD)
    xr, mr, lr, L = dense_draw(Qx, bx, prob["z"][c])
    Q64, b64 = assemble(prob, c, np.float64)
    xo, mo, Lo = gmrf_ref.draw_canonical(b64.reshape(p, 1), Q64, prob["z"][c].reshape(p, 1))
    lo = 2.0 * np.sum(np.log(np.diag(Lo)))
    floor = p * U
    fwd, e64x = [], maxrel(xo.ravel(), xr)
    for got, ref64, ref in ((x[c], xo.ravel(), xr), (mean[c], mo.ravel(), mr)):
        if np.max(np.abs(ref)) == 0.0:  # no right-hand side: the caller asserts the exact zero
            fwd.append(0.0)
            continue
        fwd.append(maxrel(got, ref) / max(maxrel(ref64, ref), floor))
    ld_scale = max(1.0, abs(lr))
    fwd.append((abs(logdet[c] - lr) / ld_scale) / max(abs(lo - lr) / ld_scale, floor))
    mu = mean[c].astype(LD)
    gamma = LD((3 * p + 1) * U) / (1 - LD((3 * p + 1) * U))
    aL = np.abs(L)
    bound = gamma * (aL @ (aL.T @ np.abs(mu)))
    resid = np.abs(bx - Qx @ mu)
    with np.errstate(invalid="ignore", divide="ignore"):
        back = float(np.max(np.where(bound > 0, resid / bound, np.where(resid > 0, np.inf, 0.0))))
    return fwd, back, e64x


def hold_to_reference(tag, prob, x, mean, logdet, chains=None):
    """Assert the forward and backward bars on `chains` (default: all) and print the worst ratios."""
    chains = range(prob["C"]) if chains is None else chains
    assert np.all(np.isfinite(x[list(chains)])) and np.all(np.isfinite(mean[list(chains)])) and np.all(np.isfinite(logdet[list(chains)]))
    worst_b = e64 = 0.0
    per = np.zeros(3)
    for c in chains:
        f, b, e = chain_ratios(prob, c, x, mean, logdet)
        per, worst_b, e64 = np.maximum(per, f), max(worst_b, b), max(e64, e)
    worst_f = float(per.max())
    print(f"dense-edges {tag} p={prob['p']} C={prob['C']}: e64(x)={e64:.2e} worst e_gpu/max(e64,pu)={worst_f:.3f} "
          f"(x {per[0]:.3f}, mean {per[1]:.3f}, log det {per[2]:.3f}) worst backward ratio={worst_b:.4f}")
    assert worst_f <= MARGIN, f"{tag}: forward error {worst_f:.2f} x that of the fp64 reference route (bar {MARGIN})"
    assert worst_b <= 1.0, f"{tag}: componentwise backward error of the mean at {worst_b:.3f} of Higham's bound"


def split_chains(C):
    """First, last and the two chains either side of the two-stream split (C // 2, used from 64 chains on)."""
    return sorted({0, C - 1, max(C // 2 - 1, 0), min(C // 2, C - 1)})


# ---- 1-3: orders around every block edge, the blocked factor on small orders, both panel forms ----------------------------
# (the default hand-over to the own blocked factor, dense_blocked_min, is 144: by default 191 .. 255 take the own factor
# already, so the first list runs twice, at the default dispatch and with rocSOLVER's factor asked for)
ROCSOLVER_ORDERS = [33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255]
BLOCKED_ORDERS = [256, 257, 319, 321, 383, 385, 511, 512, 513, 577, 1000]
FORCED_ORDERS = [1, 2, 31, 63, 64, 65, 100, 129, 200]


def edge_case(p, tag, options):
    C = 3
    prob = make_problem(1000 + p, p, C, cond=1e4 if p == 1000 else 1e2)
    eng = make_engine(C)
    for name, value in options.items():
        eng.set_option(name, value)
    x, mean, logdet = run_draw(eng, prob)
    eng.check_status()
    again = run_draw(eng, prob)
    eng.check_status()
    eng.close()
    for a, b in zip((x, mean, logdet), again):
        assert np.array_equal(a, b), "the same call twice must give the same bits"
    hold_to_reference(tag, prob, x, mean, logdet)


@pytest.mark.parametrize("p", ROCSOLVER_ORDERS + BLOCKED_ORDERS)
def test_orders_around_block_edges_default_dispatch(p):
    """Set 1.  Below dense_blocked_min (144): rocSOLVER's factor and the own 64-column solves; from there: the own factor."""
    edge_case(p, "set1-default", {})


@pytest.mark.parametrize("p", ROCSOLVER_ORDERS)
def test_orders_around_block_edges_rocsolver_factor(p):
    """Set 1, dense_use_rocsolver = 1: rocSOLVER's factor under the own 64-column solves at every order up to 255."""
    edge_case(p, "set1-rocsolver", {"dense_use_rocsolver": 1})


@pytest.mark.parametrize("p", FORCED_ORDERS)
def test_blocked_factor_forced_on_small_orders(p):
    """Set 2.  dense_blocked_min = 1: a first panel that is itself partial (p < 64) and one with no rows below it."""
    edge_case(p, "set2-forced", {"dense_blocked_min": 1})


@pytest.mark.parametrize("p", BLOCKED_ORDERS + FORCED_ORDERS)
def test_old_panel_form(p):
    """Set 3.  dense_panel_old = 1 (k_chol_panel: one thread per row below the block) on its own bar."""
    edge_case(p, "set3-panel-old", {"dense_blocked_min": 1, "dense_panel_old": 1})


# ---- 4: chains around the two-stream split --------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 63, 64, 65, 129])
def test_chain_counts_around_the_two_stream_split(C):
    """Set 4, p = 321: one stream below 64 chains, two halves from there (uneven at 65 and 129).  First, last and the chains
    either side of the split against the reference; overlap 0 against 1 and a repeated call bit-identical in all chains."""
    p = 321
    prob = make_problem(4000 + C, p, C)
    eng = make_engine(C)
    terms = device_terms(eng, prob)
    out = {}
    for overlap in (0, 1, 1):
        eng.set_option("dense_overlap", overlap)
        res = run_draw(eng, prob, terms)
        eng.check_status()
        if overlap in out:
            for a, b in zip(out[overlap], res):
                assert np.array_equal(a, b), "the same call twice must give the same bits"
        out[overlap] = res
    eng.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b), "dense_overlap must not change a bit"
    hold_to_reference("set4-chains", prob, *out[1], chains=split_chains(C))


@pytest.mark.parametrize("C", [65, 129])
def test_overlap_bit_equality_with_in_kernel_draws(C):
    """dense_overlap 0 against 1 at p = 321 with the chains' own Philox draws (the existing test holds p = 320)."""
    p = 321
    prob = make_problem(4500 + C, p, C)
    eng = make_engine(C, seed=11)
    terms = device_terms(eng, prob)
    out = {}
    for overlap in (0, 1):
        eng.set_option("dense_overlap", overlap)
        out[overlap] = run_draw(eng, prob, terms, z=None, draw_index=5)
        eng.check_status()
    zz = eng.fill_normal(p, draw_index=5).cpu().numpy()
    eng.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b), "dense_overlap must not change a bit"
    prob["z"] = zz
    hold_to_reference("set4-philox", prob, *out[1], chains=split_chains(C))


# ---- 5: strides and term forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [65, 257])
@pytest.mark.parametrize("n_terms", [1, 2, 4])
def test_strided_tensors_and_term_counts(p, n_terms):
    """x, mean, z and rhs_chain as [:, :p] views of wider allocations (ld = p + 5), 1, 2 and 4 terms: the padding stays
    untouched, the values meet the bars and equal the contiguous call's bit for bit."""
    C = 3
    prob = make_problem(5000 + 10 * p + n_terms, p, C, n_terms=n_terms)
    eng = make_engine(C)
    terms = device_terms(eng, prob)
    res = run_draw(eng, prob, terms, strided=True)
    plain = run_draw(eng, prob, terms)
    eng.check_status()
    eng.close()
    for a, b in zip(res, plain):
        assert np.array_equal(a, b), "a leading dimension must not change a bit"
    hold_to_reference(f"set5-strided-{n_terms}terms", prob, *res)


@pytest.mark.parametrize("p", [65, 257])
def test_identity_term_alone_with_diag_chain(p):
    """mat = None alone with diag_chain: Q_c = s_c I + diag(d_c), a diagonal matrix through the whole factor route."""
    C = 3
    rng = np.random.default_rng(5100 + p)
    prob = make_problem(5100 + p, p, C, n_terms=1)
    prob["mats"] = [None]
    prob["diag_chain"] = 10.0 ** rng.uniform(-2.0, 2.0, (C, p))
    eng = make_engine(C)
    res = run_draw(eng, prob, strided=True)
    eng.check_status()
    eng.close()
    hold_to_reference("set5-identity+diag_chain", prob, *res)
    for c in range(C):  # and by hand: every component on its own
        d = prob["scales"][0][c] + prob["diag_chain"][c]
        b = prob["scales"][0][c] * prob["rhs"][0] + prob["rhs_chain"][c]
        size = (np.abs(prob["scales"][0][c] * prob["rhs"][0]) + np.abs(prob["rhs_chain"][c])) / d  # no cancellation in it
        assert np.all(np.abs(res[1][c] - b / d) <= 16 * U * size)
        assert np.all(np.abs(res[0][c] - (b / d + prob["z"][c] / np.sqrt(d))) <= 16 * U * (size + np.abs(prob["z"][c]) / np.sqrt(d)))


@pytest.mark.parametrize("p", [65, 257])
def test_no_right_hand_side_gives_an_exactly_zero_mean(p):
    """Neither shared nor per-chain right-hand sides: b = 0, the mean is exactly zero and x = L^-T z."""
    C = 3
    prob = make_problem(5200 + p, p, C, shared_rhs=False, rhs_chain=False)
    eng = make_engine(C)
    x, mean, logdet = run_draw(eng, prob, strided=True)
    eng.check_status()
    eng.close()
    assert np.array_equal(mean, np.zeros((C, p)))
    hold_to_reference("set5-no-rhs", prob, x, mean, logdet)


@pytest.mark.parametrize("p", [64, 65, 256, 257])
def test_in_kernel_draws_equal_fill_normal_injected(p):
    """z = None with draw_index d consumes the normals fill_normal(p, d) returns (k_add_draw: two per thread, the odd
    order's last pair half used): held to the reference computed from those normals, and to the injected call."""
    C = 3
    prob = make_problem(5300 + p, p, C)
    eng = make_engine(C, seed=3)
    terms = device_terms(eng, prob)
    zz = eng.fill_normal(p, draw_index=9)
    prob["z"] = zz.cpu().numpy()
    own = run_draw(eng, prob, terms, z=None, draw_index=9)
    inj = run_draw(eng, prob, terms)
    other = run_draw(eng, prob, terms, z=None, draw_index=10)
    eng.check_status()
    eng.close()
    hold_to_reference("set5-philox", prob, *own)
    print(f"dense-edges set5-philox p={p}: in-kernel draw bit-identical to the injected one: {np.array_equal(own[0], inj[0])}")
    assert maxrel(own[0], inj[0]) <= 1e-12, "the in-kernel normals are not fill_normal's"  # the bar of tests/test_dense_gpu.py
    assert np.array_equal(own[1], inj[1]) and np.array_equal(own[2], inj[2])
    assert not np.array_equal(own[0], other[0]) and np.array_equal(own[1], other[1])


# ---- 6: conditioning -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [129, 321, 577])
@pytest.mark.parametrize("family", ["cond1e2", "cond1e8", "cond1e12", "graded"])
def test_conditioning(p, family):
    """Set 6: prescribed condition numbers 1e2, 1e8, 1e12 and the graded family D Q D (D over eight decades, base 1e2)."""
    C = 3
    cond = {"cond1e2": 1e2, "cond1e8": 1e8, "cond1e12": 1e12, "graded": 1e2}[family]
    prob = make_problem(6000 + p, p, C, cond=cond, graded=family == "graded")
    eng = make_engine(C)
    res = run_draw(eng, prob)
    eng.check_status()
    eng.close()
    hold_to_reference(f"set6-{family}", prob, *res)


@pytest.mark.parametrize("family", ["cond1e8", "graded"])
def test_conditioning_old_panel_form_and_alone(family):
    """The hard families through the old panel form, and a chain run alone (C = 1) next to the same chain inside a batch:
    each is held to the reference, not to the other (nothing is promised across batch sizes)."""
    p, C = 321, 3
    cond = 1e8 if family == "cond1e8" else 1e2
    prob = make_problem(6500, p, C, cond=cond, graded=family == "graded")
    eng = make_engine(C)
    eng.set_option("dense_panel_old", 1)
    res = run_draw(eng, prob)
    eng.check_status()
    eng.close()
    hold_to_reference(f"set6-{family}-panel-old", prob, *res)
    alone = dict(prob, C=1, scales=[s[1:2] for s in prob["scales"]], rhs_chain=prob["rhs_chain"][1:2], z=prob["z"][1:2])
    eng = make_engine(1)
    res = run_draw(eng, alone)
    eng.check_status()
    eng.close()
    hold_to_reference(f"set6-{family}-alone", alone, *res)


# ---- 7: large orders ---------------------------------------------------------------------------------------------------
def large_order_case(p, C):
    """Q_c = s_c (A A' + p I): backward error of the mean against Higham's bound with NumPy's fp64 factor for L (residual
    in longdouble, by row blocks), and x, mean, log det against NumPy's fp64 route at 16 p u cond(Q)."""
    rng = np.random.default_rng(p)
    A = rng.standard_normal((p, p))
    M = A @ A.T + p * np.eye(p)
    del A
    M = 0.5 * (M + M.T)
    ev = np.linalg.eigvalsh(M)
    cond = float(ev[-1] / ev[0])
    prob = {"p": p, "C": C, "mats": [M], "scales": [np.array([1.0, 1.5])[:C]], "rhs": [rng.standard_normal(p)],
            "rhs_chain": rng.standard_normal((C, p)), "diag_chain": None, "z": rng.standard_normal((C, p))}
    eng = make_engine(C)
    x, mean, logdet = run_draw(eng, prob)  # a launch the device refuses comes back as an error return: RuntimeError here
    eng.check_status()
    eng.close()
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(mean)) and np.all(np.isfinite(logdet))
    bar = MARGIN * p * U * cond
    gamma = (3 * p + 1) * U / (1 - (3 * p + 1) * U)
    for c in range(C):
        s = prob["scales"][0][c]
        Q64 = s * M
        b64 = s * prob["rhs"][0] + prob["rhs_chain"][c]
        xo, mo, Lo = gmrf_ref.draw_canonical(b64.reshape(p, 1), Q64, prob["z"][c].reshape(p, 1))
        lo = 2.0 * np.sum(np.log(np.diag(Lo)))
        fwd = max(maxrel(x[c], xo.ravel()), maxrel(mean[c], mo.ravel()), abs(logdet[c] - lo) / max(1.0, abs(lo)))
        aL = np.abs(Lo)
        bound = gamma * (aL @ (aL.T @ np.abs(mean[c])))
        del aL, Lo
        mu, bx = mean[c].astype(LD), LD(s) * prob["rhs"][0].astype(LD) + prob["rhs_chain"][c].astype(LD)
        resid = np.empty(p, dtype=LD)
        for r0 in range(0, p, 512):
            resid[r0:r0 + 512] = bx[r0:r0 + 512] - LD(s) * (M[r0:r0 + 512].astype(LD) @ mu)
        back = float(np.max(np.abs(resid) / bound))
        print(f"dense-edges set7-large p={p} C={C} chain {c}: cond={cond:.2f} forward vs numpy={fwd:.2e} (bar {bar:.2e}) "
              f"backward ratio={back:.4f}")
        assert fwd <= bar
        assert back <= 1.0


def test_large_order_4032():
    """8 * 4032 + 33280 = 65536 bytes of dynamic LDS in the triangular solves: the last order inside 64 KiB."""
    large_order_case(4032, 2)


def test_large_order_4033():
    """The first order whose triangular solves ask for more than 64 KiB of dynamic LDS."""
    large_order_case(4033, 2)


def test_large_order_8192():
    """The last order of the own triangular solves (96.5 KiB of dynamic LDS)."""
    large_order_case(8192, 2)


def test_large_order_8193():
    """The first order whose solves go through rocblas_dtrsv_strided_batched."""
    large_order_case(8193, 1)


# ---- failures found in a late panel ------------------------------------------------------------------------------------
def failure_problem(seed, p, C, bad):
    """One shared healthy Q = L0 L0'; `bad` maps chain -> k: that chain's diag_chain takes 2 L0[k,k]^2 off Q[k,k], so its
    leading k x k block stays positive definite and pivot k (about -L0[k,k]^2) is the first to fail.  The other chains'
    diag_chain is zero: they share the healthy matrix."""
    rng = np.random.default_rng(seed)
    L0 = 0.5 * np.tril(rng.standard_normal((p, p)), -1) / np.sqrt(p)
    L0[np.diag_indices(p)] = 1.0 + rng.random(p)
    Q = L0 @ L0.T
    Q = 0.5 * (Q + Q.T)
    diag = np.zeros((C, p))
    for c, k in bad.items():
        diag[c, k] = -2.0 * L0[k, k] ** 2
    prob = {"p": p, "C": C, "mats": [Q], "scales": [np.ones(C)], "rhs": [rng.standard_normal(p)],
            "rhs_chain": rng.standard_normal((C, p)), "diag_chain": diag, "z": rng.standard_normal((C, p))}
    for c, k in bad.items():  # the construction does what it says (the reference reports k)
        with pytest.raises(np.linalg.LinAlgError) as info:
            dense_draw(*assemble(prob, c, LD), prob["z"][c])
        assert info.value.pivot == k
    return prob


def failure_case(tag, p, C, bad, options, check=None):
    prob = failure_problem(7000 + p + 7 * C + sum(bad.values()), p, C, bad)
    eng = make_engine(C)
    for name, value in options.items():
        eng.set_option(name, value)
    terms = device_terms(eng, prob)
    x, mean, logdet = run_draw(eng, prob, terms, strided=True)  # asserts every chain's padding untouched, the failed one's too
    with pytest.raises(np.linalg.LinAlgError, match=f"chain {min(bad)}\\)"):
        eng.check_status()
    # the latch is cleared by the status call that reported it (include/omcmc_hip.h): a healthy call on the same engine is clean
    healthy = dict(prob, diag_chain=np.zeros((C, p)))
    hx, hmean, hlogdet = run_draw(eng, healthy, terms, strided=True)
    eng.check_status()
    eng.close()
    good = [c for c in (range(C) if check is None else check) if c not in bad]
    hold_to_reference(tag, prob, x, mean, logdet, chains=good)
    hold_to_reference(tag + "-healthy-after", healthy, hx, hmean, hlogdet, chains=sorted(bad))
    for c in good:  # a healthy chain is the same chain whether or not a neighbour fails
        assert np.array_equal(x[c], hx[c]) and np.array_equal(mean[c], hmean[c]) and logdet[c] == hlogdet[c]


@pytest.mark.parametrize("panel_old", [0, 1])
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 127, 128, 200, 299])
def test_late_failure_own_factor(k, panel_old):
    """p = 300, the own blocked factor in both panel forms: chain 3 of 5 fails first at pivot k."""
    failure_case(f"fail-own-k{k}-old{panel_old}", 300, 5, {3: k}, {"dense_panel_old": panel_old})


@pytest.mark.parametrize("rocsolver", [1, 0])
@pytest.mark.parametrize("k", [0, 70, 149])
def test_late_failure_order_150(k, rocsolver):
    """p = 150, chain 3 of 5 fails first at pivot k: through rocSOLVER's factor (its info array, latched by
    k_dense_post_factor) and at the default dispatch (150 >= dense_blocked_min: the own factor, last panel 22 wide)."""
    failure_case(f"fail-p150-k{k}-rocsolver{rocsolver}", 150, 5, {3: k}, {"dense_use_rocsolver": rocsolver})


@pytest.mark.parametrize("p,panel_old,rocsolver", [(300, 0, 0), (300, 1, 0), (150, 0, 1)])
def test_two_failed_chains_report_the_lower_index(p, panel_old, rocsolver):
    """The later pivot in the lower-numbered chain: chain 1 (pivot p - 2) is named, not chain 3 (pivot 5)."""
    failure_case(f"fail-two-p{p}-old{panel_old}-rocsolver{rocsolver}", p, 5, {1: p - 2, 3: 5},
                 {"dense_panel_old": panel_old, "dense_use_rocsolver": rocsolver})


@pytest.mark.parametrize("panel_old", [0, 1])
@pytest.mark.parametrize("C", [65, 129])
def test_late_failure_in_the_second_half_of_the_chains(C, panel_old):
    """From 64 chains on the second half runs on the side stream with local chain numbers: a chain failing at pivot 200
    there is named under its global index; first, last and the split's neighbours are healthy and meet the bars."""
    bad = C // 2 + 3
    failure_case(f"fail-second-half-C{C}-old{panel_old}", 300, C, {bad: 200}, {"dense_panel_old": panel_old},
                 check=split_chains(C) + [bad - 1, bad + 1])
