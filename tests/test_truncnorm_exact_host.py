"""The exact truncated-normal table (tests/golden/truncnorm_mp.npz) checks itself, and the formulas of omc_truncnorm.h,
restated in NumPy (oracle/truncnorm_exact.py), stay inside the bars the GPU tests use.  No GPU.

Measured with the restatement (SciPy 1.15 special functions) over the whole table, in ulps of max(1, |exact|):
draws worst 2.3 (median 0: most rows come out correctly rounded); densities 1.3 (forward) and 1.0 (reverse) of their bar's 32.
"""

import importlib.util
import os

import numpy as np
import pytest

from oracle import truncnorm_exact as tx

mpmath = pytest.importorskip("mpmath")

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_golden_truncnorm_mp", os.path.join(HERE, "golden", "make_golden_truncnorm_mp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table():
    return tx.load_table()


def kept_rows(T):
    return [(w, k) for w in range(len(T["a"])) for k in range(len(T["u"])) if not np.isnan(T["t"][w, k])]


def test_table_covers_the_listed_windows_and_uniforms(table, maker):
    assert np.array_equal(table["a"], [w[0] for w in maker.WINDOWS]) and np.array_equal(table["b"], [w[1] for w in maker.WINDOWS])
    assert np.array_equal(table["u"], maker.UNIFORMS)
    a, b, u = table["a"], table["b"], table["u"]
    # only u = 0 against an open lower side and u = 1 against an open upper side are left out
    gone = np.isnan(table["t"])
    want = (np.isneginf(a)[:, None] & (u == 0.0)[None, :]) | (np.isposinf(b)[:, None] & (u == 1.0)[None, :])
    assert np.array_equal(gone, want)
    assert os.path.getsize(tx.GOLDEN) < 200 * 1024


def test_script_reproduces_the_committed_file_bit_for_bit(maker, tmp_path):
    path = tmp_path / "again.npz"
    maker.write_npz(str(path), maker.build())
    with open(tx.GOLDEN, "rb") as f:
        assert path.read_bytes() == f.read()


def test_rows_recomputed_and_round_trip(table, maker):
    """Every 9th row (some 55, every window and every uniform among them): the quantile solved again equals the stored double;
    the truncated CDF at the unrounded solution gives u back to 1e-40; and, without any solver, the stored double is the
    correctly rounded one: the CDF at the midpoints to its two neighbouring doubles brackets u."""
    mp, mpf = mpmath.mp, mpmath.mpf
    rows = kept_rows(table)[::9]
    assert len(rows) >= 36
    assert {w for w, _ in rows} == set(range(len(table["a"]))) and {k for _, k in rows} == set(range(len(table["u"])))
    for w, k in rows:
        a, b, u, t = float(table["a"][w]), float(table["b"][w]), float(table["u"][k]), float(table["t"][w, k])
        t_mp = maker.quantile(a, b, u)
        assert float(t_mp) == t, (a, b, u)
        assert abs(maker.truncated_cdf(t_mp, a, b) - mpf(u)) < mpf(10) ** -40, (a, b, u)
        assert a <= t <= b
        if a < t < b and t != 0.0:  # (0 is exact by symmetry; its neighbours are beyond 80 digits)
            below = (mpf(t) + mpf(float(np.nextafter(t, -np.inf)))) / 2
            above = (mpf(t) + mpf(float(np.nextafter(t, np.inf)))) / 2
            assert maker.truncated_cdf(below, a, b) <= mpf(u) <= maker.truncated_cdf(above, a, b), (a, b, u)
    assert mp.dps >= 60


def test_masses_recomputed(table, maker):
    mpf = mpmath.mpf
    for w in range(len(table["a"])):
        a, b = float(table["a"][w]), float(table["b"][w])
        assert table["logmass"][w] == float(maker.log_mass(a, b))
        # another form of the same number: from the two log-tails of the table (doubles: their rounding is what the
        # one-tail bar allows for), or the kernel's erf sum
        if b <= 0:
            alt = mpf(table["logphi_b"][w]) + mpmath.log1p(-mpmath.exp(mpf(table["logphi_a"][w]) - mpf(table["logphi_b"][w])))
        elif a >= 0:
            alt = mpf(table["logphi_ma"][w]) + mpmath.log1p(-mpmath.exp(mpf(table["logphi_mb"][w]) - mpf(table["logphi_ma"][w])))
        else:  # a < 0 < b: the sum of two positive erf terms
            alt = mpmath.log((mpmath.erf(mpf(b) / mpmath.sqrt(2)) + mpmath.erf(-mpf(a) / mpmath.sqrt(2))) / 2)
        big, small = tx.window_tails(table, w)
        assert abs(float(alt) - table["logmass"][w]) <= tx.density_bar(table["logmass"][w], big, small), (a, b)


def test_restated_formulas_stay_inside_the_bars(table):
    """omc_truncnorm.h's branches in IEEE double with SciPy's special functions: the bars of the GPU tests are not met by
    luck of one library.  Prints the worst draw error; the clamps hold exactly."""
    T = table
    worst, errs = 0.0, []
    worst_f = worst_r = 0.0
    for w, k in kept_rows(T):
        a, b, u, t = float(T["a"][w]), float(T["b"][w]), float(T["u"][k]), float(T["t"][w, k])
        got = tx.truncnorm_ppf(u, a, b)
        assert a <= got <= b
        if u == 0.0:
            assert got == a
        if u == 1.0:
            assert got == b
        err = abs(got - t)
        assert err <= tx.draw_bar(t), (a, b, u, got, t)
        errs.append(float(tx.ulps_of(err, t)))
        big, small = tx.window_tails(T, w)
        ref = tx.expected_forward(T, w, got)
        f = tx.truncated_normal_log_pdf(got, 0.0, 1.0, a, b)
        bar = tx.density_bar(ref, big, small)
        assert np.isfinite(f) and abs(f - ref) <= bar, (a, b, u, f, ref)
        worst_f = max(worst_f, abs(f - ref) / bar)
        ref, big, small = tx.expected_reverse(T, w, k, got)
        r = tx.truncated_normal_log_pdf(0.0, got, 1.0, a, b)
        if np.isneginf(ref):
            assert np.isneginf(r), (a, b, u)
        else:
            bar = tx.density_bar(ref, big, small)
            assert abs(r - ref) <= bar, (a, b, u, r, ref)
            worst_r = max(worst_r, abs(r - ref) / bar)
    worst = max(errs)
    print(f"restatement: draws worst {worst:.2f} ulp, median {np.median(errs):.2f} ulp; "
          f"densities forward {32 * worst_f:.2f} / reverse {32 * worst_r:.2f} of 32")
    assert worst < 8.0  # SciPy's functions are good to an ulp or two each; far beyond that the restatement itself is off


def test_far_inversion_needs_its_newton_steps(table):
    """The rows below y = -600 (windows at 35 sigma and beyond) tell a tail inversion that stops after one Newton step from
    one that takes its four: the table can see that fault."""
    T = table
    seen = 0
    for w, k in kept_rows(T):
        a, b, u, t = float(T["a"][w]), float(T["b"][w]), float(T["u"][k]), float(T["t"][w, k])
        if not (a >= 35.0 or b <= -35.0) or not 0.0 < u < 1.0:
            continue
        lo, hi = (-a, -b) if a > 0.0 else (a, b)  # the tail that is inverted
        y = tx.logaddexp(np.log1p(-u) + tx.log_ndtr(lo), np.log(u) + tx.log_ndtr(hi))
        assert y < -600.0
        exact = -abs(t)
        assert abs(tx.ndtri_exp_lower(y) - exact) <= tx.draw_bar(exact)
        seen += abs(tx.ndtri_exp_lower(y, far_iters=1) - exact) > tx.draw_bar(exact)
    assert seen > 0
