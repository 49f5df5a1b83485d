"""The truncated normal of omc_truncnorm.h against an exact table, through every kernel that draws from it, and the two
domain checks of the engine.

tests/golden/truncnorm_mp.npz (written by tests/golden/make_golden_truncnorm_mp.py with mpmath at 80 digits, checked on
the CPU by tests/test_truncnorm_exact_host.py) holds the exact quantile for 34 standardised windows x 15 uniforms: the
+-13 and 1e-15 switches of the far-limits shortcut from both sides, windows wholly in one tail out to 1000 sigma (the
erfcx and asymptote branches), narrow windows, u = 0 and u = 1, limits at 0.  The kernels get the windows exactly: mean
0, scale 1, identity precision with zero off-diagonals, x0 = 0, right-hand side 0, so the conditional mean, variance and
standard deviation are exactly 0, 1, 1 and no bar needs a term for input rounding.  Bars: oracle/truncnorm_exact.py
(32 ulp of max(1, |exact|) for a draw; the same for a density, plus the forward bound of the log-tail subtraction for a
window in one tail).  Independently of the bars every draw lies in [a, b] and the draws for u = 0 and u = 1 ARE the limits.

rw_propose sums its densities over the elements of a chain, so the table goes through it twice: once in a single launch
(p = windows, C = uniforms) for the draws, and window by window (p = 1) for the two densities of every row.

Worst errors on an MI355X, in ulps of max(1, |exact|) (each test prints its own):

    rw_propose draws                        1.58   (window (-1e-3, 1e-3), u = 1 - 1e-9)
    rw_propose forward / reverse density    1.87 / 1.63 of the bar's 32
    tridiag_gibbs_truncated                 1.58
    band_gibbs_truncated                    1.58
    dense_gibbs_truncated, plain and diag   1.58 / 1.58
    small_gibbs_truncated                   1.58

What the table caught: the quantile of u = 1 (and of u = 0) came back one ulp inside a finite limit (6.999999999999999 for
the window (-7, 7)), through every entry point; omc_truncnorm_ppf now returns the limit itself.  Three faults put in on
purpose are each seen: the scan's +-13 lowered to +-6 (the draw for (-6.5, 30), u = 1e-15 leaves its window), one Newton
step instead of four below y = -600 (7000 ulp at the window (34, inf), every entry point), the last digits of one tail
coefficient of the four-wide AS 241 zeroed (171 ulp at u = 1e-3, the tridiagonal scan only: its sole caller).
"""

import numpy as np
import pytest

from oracle import truncnorm_exact as tx

pytestmark = pytest.mark.gpu

N_SITES, N_CHAINS = 130, 65  # the scans: over a 64-site block and the 16-site rounds, over a 64-chain wave


def make_engine(C, **kw):
    from openmcmc_amd.engine import Engine

    return Engine(C, **kw)


@pytest.fixture(scope="module")
def table():
    return tx.load_table()


def uniforms_for(T, w_idx, k_idx):
    """(u, t_exact) for the (window, uniform) index arrays (broadcast against each other); a row the table leaves out
    (u = 0 or 1 against an infinite limit: the draw would be infinite) gets u = 1/2 instead."""
    w_idx, k_idx = np.broadcast_arrays(w_idx, k_idx)
    half = int(np.flatnonzero(T["u"] == 0.5)[0])
    k_idx = np.where(np.isnan(T["t"][w_idx, k_idx]), half, k_idx)
    return T["u"][k_idx], T["t"][w_idx, k_idx], k_idx


def check_draws(name, got, t, a, b, u):
    """Bars and clamps for arrays of one shape; prints the worst error in ulp; returns it."""
    err = np.abs(got - t)
    ulps = tx.ulps_of(err, t)
    i = np.unravel_index(int(np.argmax(ulps)), ulps.shape)
    print(f"{name}: worst draw error {ulps[i]:.2f} ulp at window ({a[i]!r}, {b[i]!r}), u = {u[i]!r}")
    bad = ~(err <= tx.draw_bar(t))
    assert not bad.any(), [(a[j], b[j], u[j], got[j], t[j], float(ulps[j])) for j in zip(*np.nonzero(bad))][:12]
    out = ~((got >= a) & (got <= b))
    assert not out.any(), [(a[j], b[j], u[j], got[j]) for j in zip(*np.nonzero(out))][:12]
    lo, hi = (u == 0.0) & (got != a), (u == 1.0) & (got != b)
    assert not (lo | hi).any(), [(a[j], b[j], u[j], got[j]) for j in zip(*np.nonzero(lo | hi))][:12]
    return float(ulps[i])


def scan_layout(T):
    """Sites across the window table (shifted by one every pass, so that a window meets both sites of a producing wave's
    pair), chains across the uniforms."""
    nw, nu = len(T["a"]), len(T["u"])
    i = np.arange(N_SITES)
    w_idx = (i + i // nw) % nw
    k_idx = np.arange(N_CHAINS) % nu
    u, t, _ = uniforms_for(T, w_idx[None, :], k_idx[:, None])
    a = np.broadcast_to(T["a"][w_idx][None, :], u.shape)
    b = np.broadcast_to(T["b"][w_idx][None, :], u.shape)
    return a, b, u, t


def test_rw_propose_draws_in_one_launch(table):
    """p = 34 windows (limits are per element), C = 15 uniforms, injected."""
    T = table
    nw, nu = len(T["a"]), len(T["u"])
    u, t, _ = uniforms_for(T, np.arange(nw)[None, :], np.arange(nu)[:, None])  # (C, p)
    eng = make_engine(nu)
    z = eng.empty(nu, nw, 1)
    eng.rw_propose(eng.zeros(nu, nw, 1), z, eng.full((nw,), 1.0), eng.to_device(T["a"]), eng.to_device(T["b"]),
                   inject=eng.to_device(u))
    eng.check_status()
    a, b = np.broadcast_to(T["a"][None, :], u.shape), np.broadcast_to(T["b"][None, :], u.shape)
    check_draws("rw_propose", z.cpu().numpy()[:, :, 0], t, a, b, u)
    eng.close()


def test_rw_propose_densities_window_by_window(table):
    """One launch per window (p = 1, C = 15 uniforms): the forward density of the draw and the reverse density of 0 under
    the proposal centred on the draw, for every row; finite on a draw that IS a limit (u = 0, u = 1), -inf for the reverse
    move of a window that does not hold 0."""
    T = table
    nw, nu = len(T["a"]), len(T["u"])
    eng = make_engine(nu)
    worst = {"draw": 0.0, "fwd": 0.0, "rev": 0.0}
    x0, step = eng.zeros(nu, 1, 1), eng.full((1,), 1.0)
    for w in range(nw):
        a, b = T["a"][w], T["b"][w]
        u, t, k_idx = uniforms_for(T, np.full(nu, w), np.arange(nu))
        z = eng.empty(nu, 1, 1)
        lqf, lqr = eng.rw_propose(x0, z, step, eng.full((1,), a), eng.full((1,), b), inject=eng.to_device(u.reshape(nu, 1)))
        eng.check_status()
        got, f, r = z.cpu().numpy().ravel(), lqf.cpu().numpy(), lqr.cpu().numpy()
        err = np.abs(got - t)
        assert np.all(err <= tx.draw_bar(t)) and np.all((got >= a) & (got <= b)), (a, b, got, t)
        worst["draw"] = max(worst["draw"], float(tx.ulps_of(err, t).max()))
        big, small = tx.window_tails(T, w)
        ref = tx.expected_forward(T, w, got)
        bar = tx.density_bar(ref, big, small)
        assert np.all(np.isfinite(f)), (a, b, u, f)
        assert np.all(np.abs(f - ref) <= bar), (a, b, u, f, ref, bar)
        worst["fwd"] = max(worst["fwd"], float((np.abs(f - ref) / bar).max()))
        for c in range(nu):
            ref_r, big_r, small_r = tx.expected_reverse(T, w, int(k_idx[c]), got[c])
            if np.isneginf(ref_r):
                assert np.isneginf(r[c]), (a, b, u[c], r[c])
                continue
            bar_r = float(tx.density_bar(ref_r, big_r, small_r))
            assert np.isfinite(r[c]) and abs(r[c] - ref_r) <= bar_r, (a, b, u[c], got[c], r[c], ref_r, bar_r)
            worst["rev"] = max(worst["rev"], abs(r[c] - ref_r) / bar_r)
    print(f"rw_propose window by window: draws worst {worst['draw']:.2f} ulp; densities worst share of the bar "
          f"forward {32 * worst['fwd']:.2f} / 32, reverse {32 * worst['rev']:.2f} / 32")
    eng.close()


@pytest.mark.parametrize("side", ["below", "above", "on_lower", "on_upper"])
def test_reverse_density_of_a_current_value_outside_the_window(side):
    """The current value one ulp outside [1, 3]: the proposal is still drawn inside and its density is finite, the reverse
    density (of the current value under the proposal centred on the draw) is -inf.  On the limit both are finite.  The
    uniforms keep every subtraction of the kernel exact, so that the one ulp is not rounded away before the comparison (the
    reference compares the same rounded differences): the draws 1 and 3 of u = 0 and u = 1 are representable and the draws
    of the others share a binade with the limit next to the current value.  From below, u = 1 would need 1 - 2^-53 - 3,
    which is not a double; 1/4 stands in for it there."""
    lo, hi = 1.0, 3.0
    mu = {"below": np.nextafter(lo, -np.inf), "above": np.nextafter(hi, np.inf), "on_lower": lo, "on_upper": hi}[side]
    u = np.array([0.0, 0.5, 0.25 if side == "below" else 1.0])
    eng = make_engine(3)
    z = eng.empty(3, 1, 1)
    lqf, lqr = eng.rw_propose(eng.full((3, 1, 1), mu), z, eng.full((1,), 1.0), eng.full((1,), lo), eng.full((1,), hi),
                              inject=eng.to_device(u.reshape(3, 1)))
    eng.check_status()
    got, f, r = z.cpu().numpy().ravel(), lqf.cpu().numpy(), lqr.cpu().numpy()
    assert got[0] == lo and lo < got[1] < hi and (got[2] == hi if u[2] == 1.0 else lo < got[2] < 2.0), got
    assert np.all(np.isfinite(f)), f
    for c in range(3):
        ref_f = tx.truncated_normal_log_pdf(float(got[c]), float(mu), 1.0, lo, hi)
        assert abs(f[c] - ref_f) <= 1e-13 * max(1.0, abs(ref_f)), (c, f[c], ref_f)  # (the exact tests are above: a sanity bar)
    if side in ("below", "above"):
        assert np.all(np.isneginf(r)), r
    else:
        assert np.all(np.isfinite(r)), r
    eng.close()


def test_tridiagonal_scan(table):
    """k_tridiag_gibbs_truncated, n = 130, C = 65: the only caller of the four-wide AS 241 and of the second copy of the
    far-limits test (as < -13, bs > 13, 1e-15 < u < 1 - 1e-15: the table holds both sides of each, as == -13 and bs == 13
    exactly included)."""
    T = table
    a, b, u, t = scan_layout(T)
    assert np.any((a == -13.0) & (b > 13.0)) and np.any((a < -13.0) & (b == 13.0)) and np.any((a < -13.0) & (b > 13.0) & (u == 1e-15))
    eng = make_engine(N_CHAINS)
    n = N_SITES
    x = eng.zeros(N_CHAINS, n)
    eng.tridiag_gibbs_truncated(n, [{"diag": eng.full((n,), 1.0), "off": eng.zeros(n - 1)}], x, lower=eng.to_device(a[0]),
                                upper=eng.to_device(b[0]), u=eng.to_device(u))
    eng.check_status()
    check_draws("tridiag_gibbs_truncated", x.cpu().numpy(), t, a, b, u)
    eng.close()


def test_band_scan(table):
    """k_band_gibbs_truncated with a stored (zero) first sub-diagonal: the scalar omc_truncated_normal_rv, one lane per chain."""
    T = table
    a, b, u, t = scan_layout(T)
    eng = make_engine(N_CHAINS)
    n = N_SITES
    band = np.zeros((2, n))
    band[0] = 1.0
    x = eng.zeros(N_CHAINS, n)
    eng.band_gibbs_truncated(n, [{"band": eng.to_device(band)}], x, lower=eng.to_device(a[0]), upper=eng.to_device(b[0]),
                             u=eng.to_device(u))
    eng.check_status()
    check_draws("band_gibbs_truncated", x.cpu().numpy(), t, a, b, u)
    eng.close()


@pytest.mark.parametrize("diag_chain", [False, True])
def test_dense_scan(table, diag_chain):
    """k_dense_gibbs_truncated (Q = I) and k_dense_gibbs_truncated_diag (Q = I/2 + a per-chain diagonal of 1/2: Q_ii = 1
    exactly either way)."""
    T = table
    a, b, u, t = scan_layout(T)
    eng = make_engine(N_CHAINS)
    n = N_SITES
    x = eng.zeros(N_CHAINS, n)
    mat = np.eye(n) * (0.5 if diag_chain else 1.0)
    eng.dense_gibbs_truncated(n, [{"mat": eng.to_device(mat)}], x, lower=eng.to_device(a[0]), upper=eng.to_device(b[0]),
                              u=eng.to_device(u), diag_chain=eng.full((N_CHAINS, n), 0.5) if diag_chain else None)
    eng.check_status()
    check_draws("dense_gibbs_truncated" + (" (diag_chain)" if diag_chain else ""), x.cpu().numpy(), t, a, b, u)
    eng.close()


def test_small_scan_window_by_window(table):
    """k_small_gibbs_truncated takes scalar limits: one launch per window, the 15 uniforms as 5 chains x 3 sites (Q = the
    prior precision 1, no likelihood).  The draw is inlined there by a statement attribute."""
    T = table
    nw, nu = len(T["a"]), len(T["u"])
    C, kmax = 5, 3
    assert C * kmax == nu
    eng = make_engine(C)
    gram, rhs, prec = eng.zeros(C, kmax, kmax), eng.zeros(C, kmax), eng.full((C, kmax), 1.0)
    worst = 0.0
    for w in range(nw):
        a, b = float(T["a"][w]), float(T["b"][w])
        u, t, _ = uniforms_for(T, np.full(nu, w), np.arange(nu))
        x = eng.zeros(C, kmax)
        eng.small_gibbs_truncated(gram, rhs, prec, x, lower=a, upper=b, u=eng.to_device(u.reshape(C, kmax)))
        eng.check_status()
        got = x.cpu().numpy().ravel()
        err = np.abs(got - t)
        worst = max(worst, float(tx.ulps_of(err, t).max()))
        assert np.all(err <= tx.draw_bar(t)), (a, b, u, got, t)
        assert np.all((got >= a) & (got <= b)), (a, b, u, got)
        assert np.all(got[u == 0.0] == a) and np.all(got[u == 1.0] == b), (a, b, got)
    print(f"small_gibbs_truncated: worst draw error {worst:.2f} ulp")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the domain rule: a chain is outside when any (live) element is < lower or > upper (location_scale.py's
# check_domain_response: two strict comparisons, so a value on a limit is inside and so is a NaN)
SIZES = [1, 63, 64, 65, 130, 257, 1000]
CHAIN_COUNTS = [1, 4, 5]
KINDS = ["inside", "on_limits", "below", "above_last", "nan"]


def outside_rule(x, lower, upper, count=None):
    out = np.zeros(x.shape[0], dtype=bool)
    for c in range(x.shape[0]):
        live = x[c, : x.shape[1] if count is None else int(count[c])]
        lo = lower if lower is None or np.ndim(lower) == 0 else lower[: live.size]
        hi = upper if upper is None or np.ndim(upper) == 0 else upper[: live.size]
        with np.errstate(invalid="ignore"):
            out[c] = (lo is not None and bool(np.any(live < lo))) or (hi is not None and bool(np.any(live > hi)))
    return out


def fill_chain(row, kind, lower, upper, rng, live, pos, far):
    """One chain's row: strictly inside its limits (at -far / far where a side is open: an open side admits anything), then
    the edge of `kind` at a live position whose limit on that side is finite."""
    n = row.size
    lower, upper = np.broadcast_to(lower, (n,)), np.broadcast_to(upper, (n,))
    lo_f, hi_f = np.where(np.isfinite(lower), lower, -50.0), np.where(np.isfinite(upper), upper, 50.0)
    row[:] = lo_f + (hi_f - lo_f) * (0.1 + 0.8 * rng.random(n))
    row[np.isposinf(upper)] = far
    row[np.isneginf(lower)] = -far
    fin_lo, fin_hi = np.flatnonzero(np.isfinite(lower[:live])), np.flatnonzero(np.isfinite(upper[:live]))
    if kind == "on_limits":
        if fin_lo.size:
            row[fin_lo[pos % fin_lo.size]] = lower[fin_lo[pos % fin_lo.size]]
        if fin_hi.size:
            row[fin_hi[-1]] = upper[fin_hi[-1]]
    elif kind == "below" and fin_lo.size:
        row[fin_lo[pos % fin_lo.size]] = np.nextafter(lower[fin_lo[pos % fin_lo.size]], -np.inf)
    elif kind == "above_last" and fin_hi.size:
        row[fin_hi[-1]] = np.nextafter(upper[fin_hi[-1]], np.inf)
    elif kind == "nan" and live:
        row[pos % live] = np.nan


@pytest.mark.parametrize("C", CHAIN_COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_domain_penalty(n, C):
    """Per-element limits, some infinite on either side, rows wider than n (the columns beyond hold 1e9 and must not be
    read), either limit vector or both absent: -inf for the chains outside, the others bit for bit as they were."""
    rng = np.random.default_rng(1000 * n + C)
    lower = -1.0 - rng.random(n)
    upper = 2.0 + rng.random(n)
    lower[np.arange(n) % 5 == 2] = -np.inf
    upper[np.arange(n) % 7 == 3] = np.inf
    eng = make_engine(C)
    lo_d, hi_d = eng.to_device(lower), eng.to_device(upper)
    seen = set()
    for shift in range(len(KINDS)):
        wide = np.full((C, n + 3), 1e9)
        for c in range(C):
            fill_chain(wide[c, :n], KINDS[(c + shift) % len(KINDS)], lower, upper, rng, n, 7 * c + 13 * shift, 1e308)
        x = eng.to_device(wide)[:, :n]
        assert x.stride(0) == n + 3
        out0 = rng.standard_normal(C)
        for lo, hi, lo_h, hi_h in ((lo_d, hi_d, lower, upper), (None, hi_d, None, upper), (lo_d, None, lower, None),
                                   (None, None, None, None)):
            out = eng.to_device(out0)
            eng.domain_penalty(x, out, lower=lo, upper=hi)
            eng.check_status()
            outside = outside_rule(wide[:, :n], lo_h, hi_h)
            want = np.where(outside, -np.inf, out0)
            assert np.array_equal(out.cpu().numpy().view(np.int64), want.view(np.int64)), (shift, lo is None, hi is None)
            seen.update(outside.tolist())
    assert seen == {True, False}
    eng.close()


@pytest.mark.parametrize("C", CHAIN_COUNTS)
@pytest.mark.parametrize("kmax", SIZES)
def test_diag_gauss_logpdf_limits(kmax, C):
    """Scalar limits (finite, or infinite on either side), ragged counts (0 and kmax among them) whose dead entries lie
    outside, accumulate on and off: -inf for a chain with a live element outside, and for every other chain the value of
    diag_gauss_logpdf bit for bit (a live NaN is not outside: the value is the NaN of the plain density), which is also
    held to the sums in extended precision."""
    rng = np.random.default_rng(77 * kmax + C)
    eng = make_engine(C)
    prec_h = 0.5 + rng.random((C, kmax))
    mean_h = rng.standard_normal((C, kmax))
    prec, mean = eng.to_device(prec_h), eng.to_device(mean_h)
    counts = [None, np.array([(0, kmax, kmax // 2, max(kmax - 1, 0), 1)[c % 5] for c in range(C)], dtype=np.float64)]
    seen = set()
    for shift in range(len(KINDS)):
        for lower, upper in ((-1.0, 2.0), (-np.inf, 2.0), (-1.0, np.inf), (-np.inf, np.inf)):
            for count in counts:
                x_h = np.empty((C, kmax))
                for c in range(C):
                    live = kmax if count is None else int(count[c])
                    fill_chain(x_h[c], KINDS[(c + shift) % len(KINDS)], lower, upper, rng, live, 7 * c + 13 * shift, 1e6)
                    x_h[c, live:] = 1e9 if c % 2 else -1e9  # dead entries, outside
                x = eng.to_device(x_h)
                cnt = None if count is None else eng.to_device(count)
                outside = outside_rule(x_h, lower, upper, count)
                seen.update(outside.tolist())
                for accumulate in (False, True):
                    out0 = rng.standard_normal(C)
                    out, plain = eng.to_device(out0), eng.to_device(out0)
                    eng.diag_gauss_logpdf_limits(x, prec, out, lower=lower, upper=upper, mean=mean, count=cnt, accumulate=accumulate)
                    eng.diag_gauss_logpdf(x, prec, plain, mean=mean, count=cnt, accumulate=accumulate)
                    eng.check_status()
                    got, base = out.cpu().numpy(), plain.cpu().numpy()
                    assert np.all(np.isneginf(got[outside])), (shift, lower, upper, count is None, accumulate, got)
                    ins = ~outside
                    assert np.array_equal(got[ins].view(np.int64), base[ins].view(np.int64)), (shift, lower, upper, accumulate)
                    for c in np.flatnonzero(ins):
                        live = kmax if count is None else int(count[c])
                        xs, d, m = (v[c, :live].astype(np.longdouble) for v in (x_h, prec_h, mean_h))
                        if np.isnan(x_h[c, :live]).any():
                            assert np.isnan(got[c])
                            continue
                        terms = np.concatenate([np.log(d), -d * (xs - m) ** 2, [-live * np.log(2 * np.longdouble(np.pi))]])
                        ref = 0.5 * terms.sum() + (out0[c] if accumulate else 0.0)
                        # a sum of 2 live + 1 terms in any order: at most (2 live + 4) roundings of the sum of magnitudes
                        bar = (2 * live + 4) * tx.EPS * float(0.5 * np.abs(terms).sum() + abs(out0[c]))
                        assert abs(got[c] - float(ref)) <= bar, (c, got[c], float(ref), bar)
    assert seen == {True, False}
    eng.close()
