"""The small kernels of the reversible-jump sweep (omc_rj.hip) at their edges, each through its Engine method against a
plain host restatement of the same operation in numpy longdouble (x87 extended: 64-bit mantissa) or the pinned oracles
(oracle/rj_sweep_ref.py, oracle/truncnorm_ref.py, tests/philox_model.py).  Draws are injected unless the draw is under test.

Every tolerance is either a constant of tests/test_rj_primitives_gpu.py / tests/test_rng_gpu.py or a bar derived in the
test's docstring from the number of roundings (EPS = 2**-53 per rounding, first order); none is fitted to the kernels."""

import numpy as np
import pytest

import philox_model as pm
from test_rj_primitives_gpu import RTOL, rel_err

pytestmark = pytest.mark.gpu

EPS = 2.0**-53
LD = np.longdouble
SENTINEL = -7.25  # what a kernel must leave alone (an exact binary fraction no kernel here produces)


def make_engine(C, **kw):
    from openmcmc_amd.engine import Engine

    return Engine(C, **kw)


def i32(eng, a):
    import torch

    return torch.as_tensor(np.asarray(a, dtype=np.int32), device=eng.device)


def i64(eng, a):
    import torch

    return torch.as_tensor(np.asarray(a, dtype=np.int64), device=eng.device)


def offset_view(eng, shape):
    """A contiguous tensor of `shape` that starts one double into its buffer: 8-byte but not 16-byte aligned."""
    buf = eng.full((int(np.prod(shape)) + 1,), SENTINEL)
    view = buf[1:].view(*shape)
    assert view.data_ptr() % 16 == 8
    return view


# ------------------------------------------------------------------------------------------------ Gaussian basis
def basis_exact(X, knots, scales):
    """phi((x - theta) / s) / s in longdouble: (values (C, kmax, n), t (C, kmax, n))."""
    t = (X.astype(LD)[None, None, :] - knots.astype(LD)[:, :, None]) / scales.astype(LD)[:, :, None]
    return np.exp(-(t * t) / 2) / np.sqrt(2 * LD(np.pi)) / scales.astype(LD)[:, :, None], t


def basis_numpy(X, knots, scales):
    """The float64 restatement (the line in test_knot_loop_gpu.knot_loop_numpy)."""
    s = scales[:, :, None]
    return np.exp(-(((X[None, None, :] - knots[:, :, None]) / s) ** 2) / 2.0) / np.sqrt(2 * np.pi) / s


def basis_inputs(n, kmax):
    """Locations and knots in [-5, 5], per-knot scales in [0.3, 2]: |t| <= 34, so no value is subnormal."""
    rng = np.random.default_rng(1000 * kmax + n)
    X = np.linspace(-5, 5, n) if n > 1 else np.array([-5.0])
    return X, rng.uniform(-5, 5, size=(3, kmax)), rng.uniform(0.3, 2.0, size=(3, kmax))


_BASIS_K = []


def basis_K():
    """Rounding t = (x - theta) / s (two roundings) and t * t (one more) puts a relative error of up to 5 EPS on the
    exponent's argument, which exp turns into a relative error of that many EPS times t^2 / 2 on the value; the exp itself
    and the two divisions add a few EPS more.  So the error of the float64 numpy restatement is measured in units of
    (1 + t^2 / 2) EPS against the longdouble reference: K is the worst such ratio over the largest inputs of the test below
    (n = 8193, kmax = 20; shared scales 1.0 and 0.37 and per-knot scales).  Measured: K = 4.52."""
    if not _BASIS_K:
        X, knots, per_knot = basis_inputs(8193, 20)
        K = 0.0
        for scales in (np.full(knots.shape, 1.0), np.full(knots.shape, 0.37), per_knot):
            exact, t = basis_exact(X, knots, scales)
            K = max(K, float(np.max(np.abs(basis_numpy(X, knots, scales).astype(LD) - exact) / exact / ((1 + t * t / 2) * EPS))))
        assert 1.0 < K < 6.0, K  # what the count of roundings above allows
        _BASIS_K.append(K)
    return _BASIS_K[0]


def basis_bar(X, knots, scales):
    """(exact values, relative bar per value): four times the restatement's measured error, 4 K (1 + t^2 / 2) EPS, plus 2 EPS
    for the device's exp."""
    exact, t = basis_exact(X, knots, scales)
    return exact, ((4 * basis_K() * (1 + t * t / 2) + 2) * EPS).astype(np.float64)


@pytest.mark.parametrize("kmax", [1, 7, 20])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 8192, 8193])
def test_gaussian_basis_against_longdouble(n, kmax):
    """omc_gaussian_basis at C = 3 with counts {0, 1, kmax}.  n = 1: one live thread; 255 / 256 / 257: one workgroup of 256
    rows short by one, full, and one row into a second; 8192: the 32 workgroups the grid is capped at, one row each per
    thread; 8193: the first n whose rows need the strided loop.  kmax = 1, 7 and 20 (the benchmark's).  Forms: shared scale
    1.0 and 0.37, per-knot scales, count=None (all kmax columns live), one column only, and prev_count.

    Tolerance (basis_K, basis_bar): the float64 numpy restatement is within K (1 + t^2 / 2) EPS of the longdouble reference,
    measured K = 4.52 (its worst relative error is 1.5e-13, at t^2 / 2 = 375); the kernel's bar is four times that plus
    2 EPS for the device's exp, (18.1 (1 + t^2 / 2) + 2) EPS: 20 EPS at the knot, 7.8e-13 at the largest t^2 / 2 = 387."""
    C = 3
    X, knots, scales = basis_inputs(n, kmax)
    count = np.array([0, 1, kmax], dtype=float)
    live = (np.arange(kmax)[None, :] < count[:, None])[:, :, None]
    eng = make_engine(C)
    dX, dk, dc = eng.to_device(X), eng.to_device(knots), eng.to_device(count)

    def check(got, scales, alive):
        exact, bar = basis_bar(X, knots, scales)
        got = got.cpu().numpy()
        err = np.abs(got.astype(LD) - exact) / exact
        assert np.all(np.where(alive, err <= bar, True)), float(np.max(np.where(alive, err / bar, 0)))
        assert np.array_equal(got == 0.0, np.broadcast_to(~alive, got.shape))  # dead columns are exactly 0.0

    for scale in (1.0, 0.37):
        got = eng.gaussian_basis(dX, dk, eng.full((C, kmax, n), np.nan), count=dc, scale=scale)
        check(got, np.full((C, kmax), scale), live)
    ds = eng.to_device(scales)
    check(eng.gaussian_basis(dX, dk, eng.full((C, kmax, n), np.nan), count=dc, scales=ds), scales, live)
    check(eng.gaussian_basis(dX, dk, eng.full((C, kmax, n), np.nan), count=None, scales=ds), scales, np.ones_like(live))
    full = eng.gaussian_basis(dX, dk, eng.full((C, kmax, n), np.nan), count=dc, scales=ds).cpu().numpy()

    # one column: the others keep every bit; the column of a chain with count <= j becomes zero
    for j in sorted({0, kmax // 2, kmax - 1}):
        out = eng.full((C, kmax, n), SENTINEL)
        got = eng.gaussian_basis(dX, dk, out, count=dc, scales=ds, column=j).cpu().numpy()
        want = np.full((C, kmax, n), SENTINEL)
        want[:, j] = full[:, j]
        assert np.array_equal(got, want), j
        assert not got[0, j].any() and (j == 0 or not got[1, j].any())

    # prev_count: columns [count, prev_count) are zeroed, columns >= max(count, prev_count) are not touched
    prev = np.array([min(2, kmax), 0, kmax - 1], dtype=float)
    out = eng.full((C, kmax, n), SENTINEL)
    got = eng.gaussian_basis(dX, dk, out, count=dc, scales=ds, prev_count=eng.to_device(prev)).cpu().numpy()
    want = np.full((C, kmax, n), SENTINEL)
    for c in range(C):
        hi = int(max(count[c], prev[c]))
        want[c, :hi] = full[c, :hi]
    assert np.array_equal(got, want)
    eng.check_status()
    eng.close()


# ------------------------------------------------------------------------------------------------ fitted values
def design_problem(C, n, kmax, seed):
    """B (C, kmax, n), coefficients with exact zeros BETWEEN live ones (every third column), offsets, weights."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((C, kmax, n))
    coef = rng.standard_normal((C, kmax))
    coef[:, 1::3] = 0.0
    if kmax > 4:
        coef[0, 3:5] = 0.0  # two neighbours
    return rng, B, coef, rng.standard_normal((C, n)), rng.standard_normal(n)


@pytest.mark.parametrize("n,kmax", [(1, 1), (2, 8), (3, 9), (511, 17), (512, 36), (513, 8), (16385, 9), (32770, 17)])
def test_design_predict_batched_against_longdouble(n, kmax):
    """omc_design_predict_batched at C = 2.  n = 1, 3: odd, one node per thread (W = 1); n = 2: the smallest two-node (W = 2)
    launch; 511 / 512 / 513: one workgroup's 256 thread-slots at W = 2 short, full, and (odd) W = 1 with three workgroups;
    16385: odd, one more node than the 64 x 256 thread-slots the grid is capped at, so the row loop strides at W = 1;
    32770: the same at W = 2.  kmax = 1, 8 (one full group of eight columns), 9 (one column into the second group), 17, 36:
    the column loop's remainder.  Zero coefficients stand between live ones (their loads are skipped).

    For even n the same data runs twice: with every tensor as allocated (16-byte aligned: the W = 2 route) and with `out`,
    and then `add_chain`, a view one double into a larger buffer (the W = 1 fall-back).  Both apply the same fused
    multiply-adds in column order, so they agree bit for bit.

    Bar per node: kmax fused multiply-adds, two additions and the scaling by chain_scale are kmax + 3 roundings (alpha is
    +-1: exact), each of a partial result no larger than S = |chain_scale| (sum_j |B_j coef_j| + |add_chain| + |add_shared|):
    |out - exact| <= (kmax + 3) EPS S."""
    C = 2
    rng, B, coef, addc, adds = design_problem(C, n, kmax, 7 * n + kmax)
    cs = np.array([0.7, -1.9])
    eng = make_engine(C)
    dB, dcoef, daddc, dadds, dcs = (eng.to_device(v) for v in (B, coef, addc, adds, cs))
    terms = np.abs(B.astype(LD) * coef.astype(LD)[:, :, None]).sum(axis=1)
    fit = (B.astype(LD) * coef.astype(LD)[:, :, None]).sum(axis=1)
    for full in (True, False):
        if full:
            exact = cs.astype(LD)[:, None] * (-fit + addc + adds[None, :])
            S = np.abs(cs)[:, None] * (terms + np.abs(addc) + np.abs(adds)[None, :])
            kw = dict(add_chain=daddc, add_shared=dadds, alpha=-1.0, chain_scale=dcs)
        else:
            exact, S, kw = fit, terms, {}
        got = eng.design_predict_batched(dB, dcoef, out=eng.full((C, n), np.nan), **kw).cpu().numpy()
        bar = ((kmax + 3) * EPS * S).astype(np.float64)
        err = np.abs(got.astype(LD) - exact).astype(np.float64)
        assert np.all(err <= bar), float(np.max(err / bar))
        if n % 2 == 0:
            out = offset_view(eng, (C, n))
            eng.design_predict_batched(dB, dcoef, out=out, **kw)
            assert np.array_equal(out.cpu().numpy(), got)
            if full:
                shifted = offset_view(eng, (C, n))
                shifted.copy_(daddc)
                got2 = eng.design_predict_batched(dB, dcoef, out=eng.full((C, n), np.nan), **dict(kw, add_chain=shifted))
                assert np.array_equal(got2.cpu().numpy(), got)
    eng.check_status()
    eng.close()


def resid_sq_check(C, n, kmax, seed):
    """Bar of omc_design_resid_sq_batched against longdouble.  Row i: the fitted value is kmax fused multiply-adds and two
    additions, the residual one subtraction: |dr_i| <= (kmax + 3) EPS S_i with S_i = sum_j |B_ij coef_j| + |add_chain_i| +
    |add_shared_i| + |y_i|.  w r r is two more roundings, and a term passes through at most A additions on its way into the
    chain's sum: ceil(n / 256) in its thread, 8 levels of the workgroup's tree and ceil(n / 1024) - 1 partial sums of the
    second launch.  To first order
        |out - exact| <= EPS (sum_i 2 w_i |r_i| (kmax + 3) S_i + (2 + A) sum_i w_i r_i^2)."""
    rng, B, coef, addc, adds = design_problem(C, n, kmax, seed)
    y, w = rng.standard_normal(n), 0.5 + rng.random(n)
    eng = make_engine(C)
    dB, dcoef, daddc, dadds, dy, dw = (eng.to_device(v) for v in (B, coef, addc, adds, y, w))
    fit = (B.astype(LD) * coef.astype(LD)[:, :, None]).sum(axis=1)
    terms = np.abs(B.astype(LD) * coef.astype(LD)[:, :, None]).sum(axis=1)
    A = -(-n // 256) + 8 + -(-n // 1024) - 1
    for with_chain, with_shared, with_w in ((True, True, True), (False, False, False), (True, False, True), (False, True, False)):
        f = fit + (addc if with_chain else 0) + (adds[None, :] if with_shared else 0)
        S = terms + (np.abs(addc) if with_chain else 0) + (np.abs(adds)[None, :] if with_shared else 0) + np.abs(y)[None, :]
        ww = w.astype(LD) if with_w else np.ones(n, dtype=LD)
        r = y.astype(LD)[None, :] - f
        exact = (ww[None, :] * r * r).sum(axis=1)
        bar = EPS * ((2 * ww[None, :] * np.abs(r) * (kmax + 3) * S).sum(axis=1) + (2 + A) * exact)
        got = eng.design_resid_sq_batched(dB, dcoef, dy, add_chain=daddc if with_chain else None,
                                          add_shared=dadds if with_shared else None, w=dw if with_w else None,
                                          out=eng.full((C,), np.nan)).cpu().numpy()
        err = np.abs(got.astype(LD) - exact)
        assert np.all(err <= bar), float(np.max(err / bar))
    eng.check_status()
    eng.close()


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_design_resid_sq_row_blocks(n):
    """C = 3, kmax = 5 (one column into the second group of four).  A workgroup owns 1024 rows: n = 1 (one live thread),
    1023 and 1024 (one row block, short by a row and full: the single launch), 1025 (a second block with ONE row: two
    partial sums and the ordered sum of the second launch), 2049 (three blocks)."""
    resid_sq_check(3, n, 5, 900 + n)


def test_design_resid_sq_many_chains_walk_their_row_blocks():
    """C = 512 sends one workgroup per chain that walks ALL row blocks itself (gridDim.x == 1); n = 1025 gives it a second
    block, of one row.  Compared with longdouble, not with the other route: the two sum in different orders."""
    resid_sq_check(512, 1025, 2, 77)


# ------------------------------------------------------------------------------------------------ ragged resize, select
@pytest.mark.parametrize("rows", [1, 5, 5000])
@pytest.mark.parametrize("kmax", [1, 2, 20, 64])
def test_ragged_resize_edges(kmax, rows):
    """np.concatenate / np.delete on the ragged axis, array_equal throughout.  The chains: deaths of index 0 and of index k - 1
    at k = kmax and at k = max(1, kmax // 2), a death at k = 1 (leaves zeros: at kmax = 1 the whole row), births from
    kmax - 1 (into the LAST column; from 0 at kmax = 1), from 1 and from 0.  rows = 1 and 5 fit one launch's threads many
    times over; rows = 5000 with kmax = 64 is 320000 elements for 64 x 256 threads: the strided loop (and the basis of the
    benchmark's n = 5000).  Layouts: columns ragged (theta, axis = 1), the same matrix column-major per chain (the basis),
    rows ragged (beta, axis = 0), and a birth without new values (zeros)."""
    half = max(1, kmax // 2)
    moves = [(kmax, False, 0), (kmax, False, kmax - 1), (half, False, 0), (half, False, half - 1), (1, False, 0),
             (kmax - 1, True, -1), (min(1, kmax - 1), True, -1), (0, True, -1)]
    C = len(moves)
    count = np.array([m[0] for m in moves])
    birth = np.array([m[1] for m in moves])
    dele = np.array([m[2] for m in moves], dtype=np.int64)
    rng = np.random.default_rng(31 * kmax + rows)
    val = rng.standard_normal((C, rows, kmax))
    for c in range(C):
        val[c][:, count[c]:] = 0.0
    new = rng.standard_normal((C, rows))

    def expect(new_vals):
        out = np.zeros_like(val)
        for c in range(C):
            live = val[c][:, :count[c]]
            res = np.concatenate((live, new_vals[c].reshape(-1, 1)), axis=1) if birth[c] else np.delete(live, dele[c], axis=1)
            out[c][:, :res.shape[1]] = res
        return out

    exp = expect(new)
    eng = make_engine(C)
    cd, bd, dd = eng.to_device(count.astype(float)), i32(eng, birth), i64(eng, dele)
    got = eng.ragged_resize(eng.to_device(val), cd, bd, dd, axis=1, new_vals=eng.to_device(new))
    assert np.array_equal(got.cpu().numpy(), exp)
    got = eng.ragged_resize(eng.to_device(val), cd, bd, dd, axis=1)
    assert np.array_equal(got.cpu().numpy(), expect(np.zeros((C, rows))))
    phys = eng.to_device(np.ascontiguousarray(val.transpose(0, 2, 1)))  # (C, kmax, rows): column j of a chain contiguous
    got = eng.ragged_resize(phys.transpose(1, 2), cd, bd, dd, axis=1, new_vals=eng.to_device(new))
    assert got.transpose(1, 2).is_contiguous() and np.array_equal(got.cpu().numpy(), exp)
    got = eng.ragged_resize(phys, cd, bd, dd, axis=0, new_vals=eng.to_device(new))  # rows ragged, `rows` replicates
    assert np.array_equal(got.cpu().numpy(), exp.transpose(0, 2, 1))
    vec = np.ascontiguousarray(val[:, :1, :].transpose(0, 2, 1))  # beta (kmax, 1)
    got = eng.ragged_resize(eng.to_device(vec), cd, bd, dd, axis=0, new_vals=eng.to_device(new[:, :1].copy()))
    assert np.array_equal(got.cpu().numpy()[:, :, 0], exp[:, 0, :])
    eng.check_status()
    eng.close()


def test_chain_select_many_takes_two_launches():
    """OMC_SELECT_MAX + 3 pairs in one call: a full launch and one of three entries.  Widths 1, 7, 257 (one element into a
    second 256-thread row) and 5000 x 3 (15000: four workgroups of 16 elements per thread) alternate, so both launches mix
    them.  Accepted chains are copied; rejected chains, one of them between two accepted ones, keep every bit."""
    from openmcmc_amd import _abi

    C = 5
    accept = np.array([1, 0, 1, 1, 0], dtype=np.int32)
    shapes = [(1,), (7,), (257,), (5000, 3)]
    rng = np.random.default_rng(4)
    eng = make_engine(C)
    m = _abi.OMC_SELECT_MAX + 3
    src = [rng.standard_normal((C,) + shapes[e % 4]) for e in range(m)]
    dst = [rng.standard_normal((C,) + shapes[e % 4]) for e in range(m)]
    dsrc, ddst = [eng.to_device(s) for s in src], [eng.to_device(t) for t in dst]
    eng.chain_select_many(i32(eng, accept), list(zip(dsrc, ddst)))
    eng.check_status()
    for e in range(m):
        want = np.where(accept.astype(bool).reshape((C,) + (1,) * len(shapes[e % 4])), src[e], dst[e])
        assert np.array_equal(ddst[e].cpu().numpy(), want), e
        assert np.array_equal(dsrc[e].cpu().numpy(), src[e]), e
    eng.close()


# ------------------------------------------------------------------------------------------------ matched transitions
MATCH_SCALE = 1.3


def matched_problem(kmax, limits, seed, draw=None):
    """Six chains on standard-normal design columns (n = 200): birth from kmax - 1, birth from 1, death of column 0 and of
    column k - 1 at k = kmax, death at k = 2, and a birth at k = kmax (which the kernel answers with NaN)."""
    from oracle import rj_sweep_ref

    n = 200
    rng = np.random.default_rng(seed)
    moves = [(kmax - 1, True, -1), (1, True, -1), (kmax, False, 0), (kmax, False, kmax - 1), (2, False, 1), (kmax, True, -1)]
    C = len(moves)
    count = np.array([m[0] for m in moves])
    birth = np.array([m[1] for m in moves])
    dele = np.array([m[2] for m in moves], dtype=np.int64)
    cols = rng.standard_normal((C, kmax + 1, n))
    beta = rng.standard_normal((C, kmax)) * 2
    if draw is None:
        draw = rng.random(C) if limits is not None else rng.standard_normal(C)
    Bc, Bp = np.zeros((C, kmax, n)), np.zeros((C, kmax, n))
    exp_beta, exp_f, exp_r = np.zeros((C, kmax)), np.zeros(C), np.zeros(C)
    for c in range(C):
        k = count[c]
        cur = cols[c, :k].T
        Bc[c, :k] = cur.T
        beta[c, k:] = 0.0
        if birth[c] and k == kmax:
            exp_beta[c], exp_f[c], exp_r[c] = np.nan, np.nan, np.nan
            continue
        big = cols[c, :k + 1].T if birth[c] else cur
        # the condition on the inputs: the system the transition solves is well conditioned
        assert np.linalg.cond(big.T @ big + 1e-10 * np.eye(big.shape[1])) < 1e3
        if birth[c]:
            prop = big
            out, f, r = rj_sweep_ref.matched_birth(cur, prop, beta[c, :k].reshape(k, 1), MATCH_SCALE, limits, draw[c])
        else:
            prop = np.delete(cur, dele[c], axis=1)
            out, f, r = rj_sweep_ref.matched_death(cur, prop, beta[c, :k].reshape(k, 1), MATCH_SCALE, limits, int(dele[c]))
        Bp[c, :prop.shape[1]] = prop.T
        exp_beta[c, :out.size], exp_f[c], exp_r[c] = out.ravel(), f, r
    return dict(C=C, kmax=kmax, count=count, birth=birth, dele=dele, beta=beta, draw=draw, Bc=Bc, Bp=Bp, exp_beta=exp_beta,
                exp_f=exp_f, exp_r=exp_r)


def matched_device(eng, P, limits, inject, **kw):
    """(coef_prop, lq_fwd, lq_rev) with 0.25 and -0.5 already in the two sums.  Gram matrices from omc_design_gram_batched up to
    its kmax of 36, from the host above."""
    if P["kmax"] <= 36:
        gc, _ = eng.design_gram_batched(eng.to_device(P["Bc"]))
        gp, _ = eng.design_gram_batched(eng.to_device(P["Bp"]))
    else:
        gc = eng.to_device(np.einsum("cin,cjn->cij", P["Bc"], P["Bc"]))
        gp = eng.to_device(np.einsum("cin,cjn->cij", P["Bp"], P["Bp"]))
    lqf, lqr = eng.full((P["C"],), 0.25), eng.full((P["C"],), -0.5)
    got = eng.rj_matched_transition(gc, gp, eng.to_device(P["count"].astype(float)), i32(eng, P["birth"]), i64(eng, P["dele"]),
                                    eng.to_device(P["beta"]), MATCH_SCALE, limits, lqf, lqr,
                                    inject=None if inject is None else eng.to_device(inject), **kw)
    eng.check_status()
    return got.cpu().numpy(), lqf.cpu().numpy(), lqr.cpu().numpy()


def matched_compare(P, got):
    gb, gf, gr = got
    bad = np.isnan(P["exp_f"])
    assert np.isnan(gb[bad]).all() and np.isnan(gf[bad]).all() and np.isnan(gr[bad]).all()
    ok = ~bad
    assert np.isfinite(gb[ok]).all()
    assert rel_err(gb[ok], P["exp_beta"][ok]) < RTOL
    assert rel_err(gf[ok] - 0.25, P["exp_f"][ok]) < RTOL and rel_err(gr[ok] + 0.5, P["exp_r"][ok]) < RTOL


@pytest.mark.parametrize("limits", [(-10.0, 10.0), None])
@pytest.mark.parametrize("kmax", [2, 20, 36, 64])
def test_matched_transitions_at_full_width(kmax, limits):
    """omc_rj_matched_transition against the oracle at kmax = 2 (the smallest with a death), 20 (the benchmark's), 36 (the
    largest the Gram kernel serves) and 64 (every lane of the wave owns a row; LDS grows with kmax^2), on the moves of
    matched_problem.  Bar: RTOL of test_rj_primitives_gpu; the designs are well conditioned (asserted on the host), so
    there is no allowance for the condition number.  What lq_fwd / lq_rev held before is added to."""
    P = matched_problem(kmax, limits, 300 + kmax)
    eng = make_engine(P["C"])
    matched_compare(P, matched_device(eng, P, limits, P["draw"]))
    eng.close()


@pytest.mark.parametrize("limits", [(-10.0, 10.0), None])
def test_matched_transition_draws_in_the_kernel(limits):
    """inject=None: the new coefficient's draw is block `sub` of the chain's stream: u53 of words 0 and 1 of its uniform
    stream with limits (bit for bit against the injected run), the first normal of the block's pair without (the host
    model's sin / cos / log differ from the device's in the last bits: 1e-12 on the normal as in test_rng_gpu, which RTOL
    on the outputs covers)."""
    seed, draw_index, sub, offset, kmax = 99, (2 << 32) | 5, 6, (1 << 32) + 11, 20
    C = 6
    draw = np.empty(C)
    for c in range(C):
        w = pm.rng_blocks(seed, draw_index, "uniform" if limits is not None else "normal", offset + c, [sub])
        draw[c] = pm.u53(w[0], w[1])[0] if limits is not None else pm.normal_pairs(*w)[0][0]
    P = matched_problem(kmax, limits, 17, draw=draw)
    eng = make_engine(C, seed=seed, chain_id_offset=offset)
    drawn = matched_device(eng, P, limits, None, draw_index=draw_index, sub=sub)
    matched_compare(P, drawn)
    if limits is not None:
        injected = matched_device(eng, P, limits, draw)
        for a, b in zip(drawn, injected):
            assert np.array_equal(a, b, equal_nan=True)
    other = matched_device(eng, P, limits, None, draw_index=draw_index, sub=sub + 1)
    assert other[0][0, kmax - 1] != drawn[0][0, kmax - 1]
    eng.close()


# ------------------------------------------------------------------------------------------------ diagonal manifold MALA
MALA_STEP = 0.7


def mala_problem(C, kmax, seed):
    rng = np.random.default_rng(seed)
    count = rng.integers(0, kmax + 1, size=C)
    count[0] = kmax
    count[-1] = 0 if C > 1 else kmax
    if C > 2:
        count[1] = 0
    return dict(C=C, kmax=kmax, count=count, x=rng.standard_normal((C, kmax)), grad=rng.standard_normal((C, kmax)) * 3,
                h=rng.uniform(0.2, 5.0, size=(C, kmax)), z=rng.standard_normal((C, kmax)))


def mala_exact(P, z, x_prop=None):
    """The kernel's comment in longdouble: precision h / step^2, L = sqrt(precision), m = x + grad / (2 precision),
    x' = m + z / L, log q = sum log L - |L (x' - m)|^2 / 2 over the live entries.  Returns (x', log q at x_prop or x', bars)."""
    live = np.arange(P["kmax"])[None, :] < P["count"][:, None]
    x, g, h = (P[k].astype(LD) for k in ("x", "grad", "h"))
    prec = h / (LD(MALA_STEP) * LD(MALA_STEP))
    L = np.sqrt(prec)
    shift = g / (2 * prec)
    m = x + shift
    prop = np.where(live, m + z.astype(LD) / L, 0)
    at = prop if x_prop is None else x_prop.astype(LD)
    w = np.where(live, L * (at - m), 0)
    logL = np.where(live, np.log(L), 0)
    lq = logL.sum(axis=1) - (w * w).sum(axis=1) / 2
    # roundings, first order.  precision: 2 (step * step, the division); L: the square root halves those and adds its own: 2;
    # grad / precision: 3; m: that and its own addition: dm = EPS (3 |shift| + |m|); z / L: 3; x': dm + EPS (3 |z / L| + |x'|)
    dm = EPS * (3 * np.abs(shift) + np.abs(m))
    bar_x = dm + EPS * (3 * np.abs(z.astype(LD) / L) + np.abs(prop))
    # w = L (x' - m): L's 2, the subtraction, the product, and m's error scaled by L: dw = L dm + 4 EPS |w|;
    # sum of w^2 by k fused multiply-adds: sum 2 |w| dw + (k + 1) EPS sum w^2 (halved exactly);
    # log L: 2 EPS from L and 1 EPS |log L| of its own, k additions of partial sums below sum |log L|; the last subtraction.
    # Twice that, for a device sqrt and log that may be an ulp or two off where the count above assumes half an ulp.
    k = P["count"][:, None].astype(LD)
    dw = L * dm + 4 * EPS * np.abs(w)
    bar_q = (np.where(live, 2 * np.abs(w) * dw, 0).sum(axis=1) / 2 + (k[:, 0] + 1) * EPS * (w * w).sum(axis=1) / 2
             + EPS * np.where(live, 2 + (k + 1) * np.abs(logL), 0).sum(axis=1) + EPS * np.abs(lq))
    return prop, lq, (2 * np.where(live, bar_x, 0)).astype(np.float64), (2 * bar_q).astype(np.float64)


@pytest.mark.parametrize("C", [1, 65, 257])
@pytest.mark.parametrize("kmax", [1, 7, 20, 64])
def test_mala_diag_against_longdouble(kmax, C):
    """omc_mala_diag (one thread per chain, 64 per workgroup) at C = 1, 65 (one chain into a second workgroup) and 257, kmax =
    1, 7, 20 and 64, ragged counts that include 0 (log q = 0, no entry written but zeros) and kmax.  Propose with injected
    normals: proposal and log q within the bars derived in mala_exact from the roundings (the density is compared at the
    proposal the kernel returned: that is the point it is the density OF); dead entries exactly 0.  The reverse-move form with
    x_other = that proposal and the same x, grad and h is the same arithmetic: the same log q bit for bit."""
    P = mala_problem(C, kmax, 50 * kmax + C)
    eng = make_engine(C)
    d = eng.to_device
    dx, dg, dh, dc = d(P["x"]), d(P["grad"]), d(P["h"]), d(P["count"].astype(float))
    prop, lq = eng.mala_diag(dx, dg, dh, MALA_STEP, count=dc, z=d(P["z"]))
    eng.check_status()
    gp, gq = prop.cpu().numpy(), lq.cpu().numpy()
    exact_x, _, bar_x, _ = mala_exact(P, P["z"])
    _, exact_q, _, bar_q = mala_exact(P, P["z"], x_prop=gp)
    live = np.arange(kmax)[None, :] < P["count"][:, None]
    assert np.all(gp[~live] == 0.0)
    err = np.abs(gp.astype(LD) - exact_x).astype(np.float64)
    assert np.all(err[live] <= bar_x[live]), float(np.max(err[live] / bar_x[live]))
    errq = np.abs(gq.astype(LD) - exact_q).astype(np.float64)
    assert np.all(errq <= bar_q), float(np.max(errq / np.maximum(bar_q, 1e-300)))
    assert np.all(gq[P["count"] == 0] == 0.0)
    rev = eng.mala_diag(dx, dg, dh, MALA_STEP, count=dc, x_other=prop)
    eng.check_status()
    assert np.array_equal(rev.cpu().numpy(), gq)
    assert np.array_equal(prop.cpu().numpy(), gp)  # the reverse form reads x_other
    if C == 1:  # count=None: every entry is live
        P["count"][:] = kmax
        prop, lq = eng.mala_diag(dx, dg, dh, MALA_STEP, z=d(P["z"]))
        gp = prop.cpu().numpy()
        exact_x, _, bar_x, _ = mala_exact(P, P["z"])
        _, exact_q, _, bar_q = mala_exact(P, P["z"], x_prop=gp)
        assert np.all(np.abs(gp.astype(LD) - exact_x) <= bar_x) and np.all(np.abs(lq.cpu().numpy().astype(LD) - exact_q) <= bar_q)
    eng.close()


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan")])
def test_mala_diag_latches_a_bad_curvature_in_a_live_entry_only(bad):
    """h <= 0 or NaN in a LIVE entry makes check_status raise and name the lowest such chain; the same value in a dead
    entry does not."""
    C, kmax = 65, 7
    P = mala_problem(C, kmax, 3)
    P["count"][[9, 40, 64]] = [3, 5, 2]
    h = P["h"].copy()
    h[9, 4], h[40, 6], h[64, 2], h[1, 0] = bad, bad, bad, bad  # all dead (count[1] == 0)
    eng = make_engine(C)
    d = eng.to_device
    args = (d(P["x"]), d(P["grad"]))
    _, lq = eng.mala_diag(*args, d(h), MALA_STEP, count=d(P["count"].astype(float)), z=d(P["z"]))
    eng.check_status()
    assert np.isfinite(lq.cpu().numpy()).all()
    h[40, 4], h[64, 1], h[9, 3] = bad, bad, bad  # live in chains 40 and 64, still dead in chain 9
    eng.mala_diag(*args, d(h), MALA_STEP, count=d(P["count"].astype(float)), z=d(P["z"]))
    with pytest.raises(np.linalg.LinAlgError, match=r"chain 40\)"):
        eng.check_status()
    eng.close()


def test_mala_diag_normals_drawn_in_the_kernel():
    """z=None: entry j of global chain g is normal 2 sub + j of g's normal stream at the draw index (half j & 1 of block
    sub + j // 2).  Against the run with philox_model.normals injected; the host model's normals are within 1e-12 of the
    device's (the constant of test_rng_gpu), and x' = m + z / L carries that as 1e-12 / L, plus the rounding of x'."""
    C, kmax, seed, draw_index, sub, offset = 5, 7, 2024, (1 << 32) | 9, 3, (1 << 33) + 2
    P = mala_problem(C, kmax, 8)
    z = np.stack([pm.normals(seed, draw_index, offset + c, 2 * sub + kmax)[2 * sub:] for c in range(C)])
    eng = make_engine(C, seed=seed, chain_id_offset=offset)
    d = eng.to_device
    args = (d(P["x"]), d(P["grad"]), d(P["h"]), MALA_STEP)
    dc = d(P["count"].astype(float))
    drawn, lq_drawn = eng.mala_diag(*args, count=dc, draw_index=draw_index, sub=sub)
    injected, lq_inj = eng.mala_diag(*args, count=dc, z=d(z))
    eng.check_status()
    a, b = drawn.cpu().numpy(), injected.cpu().numpy()
    L = np.sqrt(P["h"]) / MALA_STEP
    live = np.arange(kmax)[None, :] < P["count"][:, None]
    assert np.all(np.abs(a - b)[live] <= (1e-12 / L + 2 * EPS * np.abs(b))[live])
    assert np.all(a[~live] == 0.0)
    # log q = sum log L - sum z^2 / 2 in these terms: 1e-12 on each z
    assert np.all(np.abs(lq_drawn.cpu().numpy() - lq_inj.cpu().numpy()) <= 1e-12 * (np.abs(z) * live).sum(axis=1) + 1e-13)
    other, _ = eng.mala_diag(*args, count=dc, draw_index=draw_index, sub=sub + 1)
    assert not np.array_equal(other.cpu().numpy(), a)  # another sub-stream: other normals
    eng.close()


# ------------------------------------------------------------------------------------------------ truncated proposals, p > 1
@pytest.mark.parametrize("p", [2, 3, 5])
def test_truncated_proposal_of_several_elements_drawn_in_the_kernel(p):
    """omc_rw_propose with limits, p elements, per-element step, lower and upper, uniforms drawn in the kernel: element e reads
    block sub + e // 2 of the chain's uniform stream, words 0-1 when e is even and words 2-3 when it is odd (p = 2: both
    halves of one block; 3: into a second block; 5: a third).  The uniforms rebuilt from philox_model and injected give the
    same proposal and densities bit for bit; the densities are the sums over the elements of oracle/truncnorm_ref's."""
    from oracle import truncnorm_ref

    C, seed, draw_index, sub, offset = 9, 4242, (5 << 32) | 3, 2, (1 << 32) + 7
    rng = np.random.default_rng(p)
    step = rng.uniform(0.2, 1.5, size=p)
    lower, upper = -1.0 - rng.random(p), 1.0 + rng.random(p)
    x = rng.uniform(-1, 1, size=(C, p, 1))
    u = np.empty((C, p))
    for c in range(C):
        w = pm.rng_blocks(seed, draw_index, "uniform", offset + c, sub + np.arange((p + 1) // 2))
        both = np.stack([pm.u53(w[0], w[1]), pm.u53(w[2], w[3])], axis=1).reshape(-1)
        u[c] = both[:p]
    eng = make_engine(C, seed=seed, chain_id_offset=offset)
    d = eng.to_device
    dx, dstep, dlo, dhi = d(x), d(step), d(lower), d(upper)
    z1, z2 = eng.full((C, p, 1), np.nan), eng.full((C, p, 1), np.nan)
    f1, r1 = eng.rw_propose(dx, z1, dstep, dlo, dhi, draw_index=draw_index, sub=sub)
    f2, r2 = eng.rw_propose(dx, z2, dstep, dlo, dhi, inject=d(u))
    eng.check_status()
    assert np.array_equal(z1.cpu().numpy(), z2.cpu().numpy())
    assert np.array_equal(f1.cpu().numpy(), f2.cpu().numpy()) and np.array_equal(r1.cpu().numpy(), r2.cpu().numpy())
    z = z1.cpu().numpy()[:, :, 0]
    assert np.all((z >= lower[None, :]) & (z <= upper[None, :]))
    exp_z, exp_f, exp_r = np.empty((C, p)), np.zeros(C), np.zeros(C)
    for e in range(p):
        exp_z[:, e] = truncnorm_ref.truncated_normal_rv(x[:, e, 0], step[e], lower[e], upper[e], u[:, e])
        exp_f += truncnorm_ref.truncated_normal_log_pdf(exp_z[:, e], x[:, e, 0], step[e], lower[e], upper[e])
        exp_r += truncnorm_ref.truncated_normal_log_pdf(x[:, e, 0], exp_z[:, e], step[e], lower[e], upper[e])
    assert rel_err(z, exp_z) < RTOL
    assert rel_err(f1.cpu().numpy(), exp_f) < RTOL and rel_err(r1.cpu().numpy(), exp_r) < RTOL
    eng.close()
