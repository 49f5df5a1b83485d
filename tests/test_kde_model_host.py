"""The numpy restatement of the binned kernel density estimate (tests/kde_model.py; no GPU) against what it restates: scipy's
gaussian_kde where binning loses nothing (draws on the bin centres, a given bandwidth, no bounds), the size of the improved
Sheather-Jones bandwidth on samples whose answer is known (a normal sample: close to the normal-reference rule; a well separated
mixture: far below it), and itself at fp64 against np.longdouble on the cases the GPU test uses -- bandwidth, density, flags, the
bracket of the ISJ root and the bin of the mode."""

import numpy as np
import pytest
from kde_cases import cases, reference
from kde_model import kde_column, kde_model


def test_equals_scipy_when_the_draws_lie_on_the_bin_centres():
    from scipy.stats import gaussian_kde

    rng = np.random.default_rng(0)
    for G, lo, hi, h in ((8, -1.0, 3.0, 0.7), (100, -3.1, 4.3, 0.21), (512, 0.5, 9.0, 0.05)):
        counts = rng.integers(0, 6, G)
        centres = lo + (np.arange(G) + 0.5) * (hi - lo) / G
        x = np.repeat(centres, counts)
        want = gaussian_kde(x, bw_method=h / np.std(x, ddof=1))(centres)
        got = kde_column(counts, lo, hi, "given", bw=h)
        assert got["flag"] == 0 and float(got["bw"]) == h and got["n"] == counts.sum()
        assert np.max(np.abs(got["density"].astype(np.float64) - want) / want) < 1e-12
        assert float(got["mode"]) == pytest.approx(centres[np.argmax(want)], rel=1e-14)


@pytest.mark.parametrize("n", (1000, 20_000, 131_072))
def test_isj_of_a_normal_sample_is_close_to_the_normal_reference_rule(n):
    x = np.random.default_rng(n).standard_normal(n)
    lo, hi = x.min() - 0.1 * np.ptp(x), x.max() + 0.1 * np.ptp(x)
    r = kde_column(np.histogram(x, 512, (lo, hi))[0], lo, hi, "isj")
    want = 1.06 * np.std(x, ddof=1) * n ** -0.2
    assert r["flag"] == 0 and abs(float(r["bw"]) / want - 1) < 0.10, (float(r["bw"]), want)


def test_isj_of_a_separated_mixture_is_far_below_scott():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.normal(-4, 0.5, 10_000), rng.normal(4, 0.5, 10_000)])
    lo, hi = x.min() - 0.1 * np.ptp(x), x.max() + 0.1 * np.ptp(x)
    c = np.histogram(x, 512, (lo, hi))[0]
    isj, scott = kde_column(c, lo, hi, "isj"), kde_column(c, lo, hi, "scott")
    assert isj["flag"] == 0 and scott["flag"] == 0 and float(isj["bw"]) < 0.25 * float(scott["bw"])
    # ... and the experimental rule is the mean of Silverman's and ISJ's
    silver, both = kde_column(c, lo, hi, "silverman"), kde_column(c, lo, hi, "experimental")
    assert float(both["bw"]) == pytest.approx(0.5 * (float(silver["bw"]) + float(isj["bw"])), rel=1e-15)


def test_rules_from_the_binned_moments_and_quantiles():
    # counts whose moments and quartiles are read off by hand: bins of width 1 on [0, 8], 4 draws in bin 1, 8 in bin 3, 4 in bin 6
    c = np.array([0, 4, 0, 8, 0, 0, 4, 0])
    g = np.arange(8) + 0.5
    N, m = 16, (4 * 1.5 + 8 * 3.5 + 4 * 6.5) / 16
    sd = np.sqrt((4 * (1.5 - m) ** 2 + 8 * (3.5 - m) ** 2 + 4 * (6.5 - m) ** 2) / 15)
    q1, q3 = 1 + 4 / 4, 3 + (12 - 4) / 8  # u N = 4 falls at the end of bin 1, u N = 12 at the end of bin 3
    r = kde_model(np.stack([c, c]), 0.0, 8.0, "scott", bw_fct=2.0)
    assert np.allclose(r["bw"].astype(np.float64), 2.0 * 1.06 * sd * N ** -0.2, rtol=1e-15)
    r = kde_column(c, 0.0, 8.0, "silverman")
    assert float(r["bw"]) == pytest.approx(0.9 * min(sd, (q3 - q1) / 1.34) * N ** -0.2, rel=1e-15)
    assert float(r["mode"]) == g[3]
    # both quartiles inside one crowded bin: the binned quantile interpolates within it, (23 - 7) / 30 of its width apart
    c0 = np.array([1, 0, 0, 30, 0, 0, 0, 1])
    assert float(kde_column(c0, 0.0, 8.0, "silverman")["bw"]) == pytest.approx(0.9 * (16 / 30 / 1.34) * 32 ** -0.2, rel=1e-14)


def test_reflection_keeps_the_mass_inside():
    rng = np.random.default_rng(3)
    x = rng.exponential(1.0, 5000)
    c = np.histogram(x, 200, (0.0, 12.0))[0]
    plain = kde_column(c, 0.0, 12.0, "given", bw=0.3)
    mirrored = kde_column(c, 0.0, 12.0, "given", bw=0.3, reflect=(True, False))
    delta = 12.0 / 200
    assert float(plain["density"].sum() * delta) < 0.97  # the mass a kernel puts below zero is lost ...
    assert abs(float(mirrored["density"].sum() * delta) - 1) < 1e-3  # ... and comes back with the reflection
    both = kde_column(c[::-1], 0.0, 12.0, "given", bw=0.3, reflect=(False, True))  # the mirror image at the upper bound
    assert np.max(np.abs(both["density"][::-1] - mirrored["density"])) < 1e-15


def test_fp64_agrees_with_longdouble_on_the_gpu_cases():
    for i, c in enumerate(cases()):
        ld, f64 = reference(i), reference(i, np.float64)
        assert np.array_equal(ld["flag"], f64["flag"]) and np.array_equal(ld["n"], f64["n"]), c["name"]
        assert np.array_equal(ld["bracket"], f64["bracket"]), c["name"]
        good = ld["flag"] != 2
        assert np.isnan(f64["bw"][~good]).all() and np.isnan(f64["density"][~good]).all() and np.isnan(f64["mode"][~good]).all()
        assert np.max(np.abs(f64["bw"][good] / ld["bw"][good] - 1)) < 1e-12, c["name"]
        err = np.abs(f64["density"][good] - ld["density"][good]) / np.maximum(np.abs(ld["density"][good]), np.longdouble(1e-300))
        assert np.max(err) < 1e-12, c["name"]
        assert np.array_equal(np.argmax(ld["density"][good], axis=-1), np.argmax(f64["density"][good], axis=-1)), c["name"]
        assert np.max(np.abs(f64["mode"][good] / ld["mode"][good] - 1)) < 1e-12, c["name"]
