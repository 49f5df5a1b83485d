"""The exact truncated-normal table (tests/golden/truncnorm_mp.npz, written by tests/golden/make_golden_truncnorm_mp.py
with mpmath), the bars its tests hold results to, and a NumPy restatement of the device formulas of
openmcmc_amd/csrc/omc_truncnorm.h that shows on the CPU what those formulas reach in IEEE double.
TEST INFRASTRUCTURE ONLY.

Bars (EPS = 2^-52, one ulp of 1):

  draw      |t_got - t_exact| <= 32 EPS max(1, |t_exact|).  The formulas, evaluated with SciPy's erfc / erfcx / ndtri, stay
            within 2.3 ulp of the exact quantile over the whole table (tests/test_truncnorm_exact_host.py measures it); some
            14 times that leaves room for the device library's erfc, erfcx, log and normcdfinv (a few ulp each) and the 1e-16
            of the AS 241 rational approximations.
  density   window with a < 0 < b (a sum of two positive erf terms): 32 EPS max(1, |ref|).
            window in one tail: log mass = L + log(1 - exp(-(L - S))) with L >= S the two log-tails.  A relative error e
            in each of them moves the result by at most (e |L| + e |S|) / (1 - exp(-(L - S))) (the partial derivatives
            are 1 / (1 - exp(-d)) and -exp(-d) / (1 - exp(-d)), d = L - S), so 32 EPS (|L| + |S|) / (1 - exp(-d)) is
            added.  An infinite limit has S = -inf: its derivative is exactly 0 and so is its share of the bound.
"""

import math
import os

import numpy as np
from scipy import special

EPS = 2.0 ** -52
ULPS = 32.0
LOG_SQRT_2PI = 0.91893853320467274178
_RSQRT2 = 0.70710678118654752440

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "truncnorm_mp.npz")


def load_table():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def draw_bar(t_exact):
    return ULPS * EPS * np.maximum(1.0, np.abs(t_exact))


def density_bar(ref, tail_big=np.nan, tail_small=np.nan):
    """tail_big / tail_small: the two log-tails of a one-tail window (NaN for a window with a < 0 < b)."""
    ref, big, small = np.broadcast_arrays(np.asarray(ref, float), np.asarray(tail_big, float), np.asarray(tail_small, float))
    bar = ULPS * EPS * np.maximum(1.0, np.abs(ref))
    one = ~np.isnan(big)
    with np.errstate(invalid="ignore", over="ignore"):
        share_small = np.where(np.isfinite(small), np.abs(small), 0.0)
        extra = ULPS * EPS * (np.abs(big) + share_small) / -np.expm1(-(big - small))
    return bar + np.where(one, extra, 0.0)


def window_tails(T, w):
    """(big, small) log-tails that omc_log_gauss_mass subtracts for window w of the table, NaNs if a < 0 < b."""
    a, b = T["a"][w], T["b"][w]
    if b <= 0.0:
        return T["logphi_b"][w], T["logphi_a"][w]
    if a >= 0.0:
        return T["logphi_ma"][w], T["logphi_mb"][w]
    return np.nan, np.nan


def ulps_of(err, scale):
    """err in ulps of max(1, |scale|)."""
    return np.abs(err) / (EPS * np.maximum(1.0, np.abs(scale)))


# ---------------------------------------------------------------------------------------------------------------------
# omc_truncnorm.h restated: the same branches and thresholds in IEEE double, SciPy's special functions for the device
# library's (erfc, erfcx, normcdfinv -> ndtri; the far-limits shortcut's AS 241 -> ndtri as well)
def log_ndtr(t):
    if t > 0.0:
        return math.log1p(-0.5 * special.erfc(t * _RSQRT2))
    if t > -20.0:
        return math.log(0.5 * special.erfc(-t * _RSQRT2))
    if t == -math.inf:
        return -math.inf
    return math.log(0.5 * special.erfcx(-t * _RSQRT2)) - 0.5 * t * t


def logaddexp(p, q):
    m, lo = max(p, q), min(p, q)
    if m == -math.inf:
        return -math.inf
    return m + math.log1p(math.exp(lo - m))


def ndtri_exp_lower(y, far_iters=4):
    if y == -math.inf:
        return -math.inf
    if y > -600.0:
        x, iters = float(special.ndtri(math.exp(y))), 1
    else:
        r = -2.0 * y - 1.8378770664093453
        x, iters = -math.sqrt(r - math.log(r)), far_iters
    for _ in range(iters):
        mills = 1.2533141373155003 * special.erfcx(-x * _RSQRT2)
        x -= (log_ndtr(x) - y) * mills
    return x


def truncnorm_ppf(u, a, b):
    if a < -13.0 and b > 13.0 and 1e-15 < u < 1.0 - 1e-15:
        return float(special.ndtri(u))
    if u <= 0.0:
        return a
    if u >= 1.0:
        return b
    l1, l0 = math.log1p(-u), math.log(u)
    yp = logaddexp(l1 + log_ndtr(a), l0 + log_ndtr(b))
    if yp <= -0.69314718055994530942:
        x = ndtri_exp_lower(yp)
    else:
        x = -ndtri_exp_lower(logaddexp(l1 + log_ndtr(-a), l0 + log_ndtr(-b)))
    return min(max(x, a), b)


def log_gauss_mass(a, b):
    if b <= 0.0:
        lb = log_ndtr(b)
        return lb + math.log(-math.expm1(log_ndtr(a) - lb))
    if a >= 0.0:
        la = log_ndtr(-a)
        return la + math.log(-math.expm1(log_ndtr(-b) - la))
    return math.log(0.5 * (special.erf(b * _RSQRT2) + special.erf(-a * _RSQRT2)))


def truncated_normal_log_pdf(x, mean, scale, lower, upper):
    a, b, t = (lower - mean) / scale, (upper - mean) / scale, (x - mean) / scale
    if not (a <= t <= b):
        return -math.inf
    return -0.5 * t * t - LOG_SQRT_2PI - log_gauss_mass(a, b) - math.log(scale)


# ---------------------------------------------------------------------------------------------------------------------
# what the tests expect of a density, from the table and the draw the kernel returned
def expected_forward(T, w, t_got):
    """log density of the draw t_got under N(0, 1) truncated to window w."""
    return -0.5 * t_got * t_got - LOG_SQRT_2PI - T["logmass"][w]


def expected_reverse(T, w, k, t_got):
    """log density of 0 under the proposal centred on the draw, (value, tail_big, tail_small); -inf if 0 is outside the
    window.  The table's mass is that of the window the exact draw gives; a draw that differs from it in its last bits
    moves the log-mass by rev_dlogmass * (t_got - t) to first order (the second order is below 1e-28).  The kernel rounds
    a - t_got and b - t_got once each: half an ulp of a limit moves the log-mass by at most |a'| phi(a') / mass / 2^53 <= 1
    ulp of 1 for a window with a' <= 0 <= b', which the 32 ulp hold."""
    a, b = T["a"][w], T["b"][w]
    if not (a <= 0.0 <= b):
        return -np.inf, np.nan, np.nan
    logmass = T["rev_logmass"][w, k] + T["rev_dlogmass"][w, k] * (t_got - T["t"][w, k])
    big, small = T["rev_tail_big"][w, k], T["rev_tail_small"][w, k]
    if t_got != T["t"][w, k]:
        # the case the kernel takes follows ITS window: a draw clamped onto a limit (b - t_got = 0) goes the one-tail way
        # where the exact draw, an ulp inside, does not.  The two log-tails only size the bar: the restated ones will do
        ra, rb = float(a - t_got), float(b - t_got)
        big, small = (log_ndtr(rb), log_ndtr(ra)) if rb <= 0.0 else (log_ndtr(-ra), log_ndtr(-rb)) if ra >= 0.0 else (np.nan, np.nan)
    return -0.5 * t_got * t_got - LOG_SQRT_2PI - logmass, big, small
