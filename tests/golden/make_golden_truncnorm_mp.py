"""Exact truncated-normal quantiles and log-masses for tests/test_truncnorm_exact_gpu.py and
tests/test_truncnorm_exact_host.py, worked out with mpmath at 80 digits and rounded to double last.

    python tests/golden/make_golden_truncnorm_mp.py          # writes tests/golden/truncnorm_mp.npz

For every standardised window (a, b) of WINDOWS and every uniform u of UNIFORMS (all of them the exact doubles the tests
pass to the kernels) the file holds

    t[w, k]        the truncated quantile: Phi(t) = (1 - u) Phi(a) + u Phi(b), solved on the log of the SMALLER of the two
                   tails ((1 - u) Q(a) + u Q(b) with Q = 1 - Phi for the upper one), clamped to [a, b], rounded to double;
                   NaN where the row is left out (u = 0 / u = 1 against an infinite limit on that side)
    logmass[w]     log(Phi(b) - Phi(a))
    logphi_a/b[w]  log Phi(a), log Phi(b);  logphi_ma/mb[w]: log Phi(-a), log Phi(-b) (what an upper-tail window uses)

and, for the rows whose window holds 0 (the reverse move of a proposal made from 0 back to 0 exists), the window of the
reverse density: a proposal centred on the draw t has the standardised limits ra = fl(a - t), rb = fl(b - t) (one
subtraction in double, as the kernel forms them)

    rev_a, rev_b[w, k]        those two doubles
    rev_logmass[w, k]         log(Phi(rb) - Phi(ra)) for exactly those doubles
    rev_dlogmass[w, k]        d/dt log(Phi(b - t) - Phi(a - t)) = (phi(ra) - phi(rb)) / mass: first-order correction for a
                              draw that differs from t in its last bits
    rev_tail_big/small[w, k]  the two log-tails the one-tail formula subtracts when rb <= 0 or ra >= 0 (NaN otherwise)

The .npz is written with fixed zip time stamps and no compression: the script reproduces the committed file bit for bit.
Nothing here comes from another project; the only inputs are the definitions of Phi and of the truncated quantile.
"""

import io
import os
import zipfile

import numpy as np
from mpmath import mp, mpf

mp.dps = 80

INF = float("inf")
C15 = 1.0 - 1e-15  # the double the kernels compare a uniform with

WINDOWS = [
    (-INF, INF), (-13.0, 13.0), (float(np.nextafter(-13.0, -INF)), float(np.nextafter(13.0, INF))), (-13.5, 13.5),
    (-12.5, 40.0), (-40.0, 12.5), (-INF, -8.0), (8.0, INF), (5.0, INF), (-2.0, INF), (-INF, 1.0), (-0.5, 1.0), (-30.0, 0.4),
    (19.9, INF), (20.1, INF), (20.0, 21.0), (-21.0, -20.0), (34.0, INF), (35.0, INF), (40.0, INF), (-INF, -40.0),
    (100.0, 101.0), (1000.0, INF), (-1e-3, 1e-3), (1e-8, 2e-8), (3.0, 3.0000001), (5.0, 5.01),
    # one limit on the far side of +-13 and the other exactly on it: each half of the scan's far-limits test alone
    (-13.5, 13.0), (-13.0, 13.5),
    # limits inside +-13 where the window still moves the quantile of a small uniform (Phi(-7) = 1.3e-12): a far-limits
    # threshold set too low returns Phi^-1(u), outside the window
    (-7.0, 7.0), (-6.5, 30.0), (-30.0, 6.5),
    # a limit at 0: the positivity constraint seen from a site whose conditional mean sits on it
    (0.0, INF), (-3.0, 0.0),
]

UNIFORMS = [
    0.0, 1.0, 2.0 ** -53, 1e-15, float(np.nextafter(1e-15, 1.0)), 1e-12, 1e-3, 0.25, 0.5, 0.9, 1.0 - 1e-9,
    float(np.nextafter(C15, 0.0)), C15, float(np.nextafter(C15, 2.0)), 1.0 - 2.0 ** -53,
]

SQRT2 = mp.sqrt(2)


def M(x):
    """The exact value of a double (or +-inf) as an mpf."""
    return mpf(x)


def Phi(x):
    return mp.erfc(-x / SQRT2) / 2


def Q(x):
    return mp.erfc(x / SQRT2) / 2


def phi(x):
    return mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi) if mp.isfinite(x) else mpf(0)


def log_Phi(x):
    if x == -mp.inf:
        return -mp.inf
    return mp.log(Phi(x))


def solve_log_lower(y):
    """x with log Phi(x) = y, for y <= ~log(1/2): Newton on the concave log Phi (monotone from the left)."""
    if y < -10:
        r = -2 * y - mp.log(2 * mp.pi)
        x = -mp.sqrt(r - mp.log(r))
    else:
        x = mpf(-1)
    for _ in range(400):
        dx = (log_Phi(x) - y) * Phi(x) / phi(x)
        x -= dx
        if abs(dx) <= mpf(10) ** -70 * max(1, abs(x)):
            return x
    raise RuntimeError("no convergence")


def quantile(a, b, u):
    """The truncated quantile as an mpf (not yet rounded), a, b, u doubles."""
    a, b, u = M(a), M(b), M(u)
    if a == -b and u == mpf(1) / 2:
        return mpf(0)  # by symmetry, exactly (the iteration would stop 1e-80 away from it)
    lower = (1 - u) * Phi(a) + u * Phi(b)
    upper = (1 - u) * Q(a) + u * Q(b)
    t = solve_log_lower(mp.log(lower)) if lower <= upper else -solve_log_lower(mp.log(upper))
    return min(max(t, a), b)


def truncated_cdf(x, a, b):
    """(Phi(x) - Phi(a)) / (Phi(b) - Phi(a)) with upper tails for a window right of 0 (no cancellation against 1)."""
    a, b = M(a), M(b)
    if a >= 0:
        return (Q(a) - Q(x)) / (Q(a) - Q(b))
    return (Phi(x) - Phi(a)) / (Phi(b) - Phi(a))


def log_mass(a, b):
    a, b = M(a), M(b)
    if a >= 0:
        return mp.log(Q(a) - Q(b))
    return mp.log(Phi(b) - Phi(a))


def row_is_kept(a, b, u):
    return not ((u == 0.0 and a == -INF) or (u == 1.0 and b == INF))


def build():
    nw, nu = len(WINDOWS), len(UNIFORMS)
    nan = np.full((nw, nu), np.nan)
    out = {
        "a": np.array([w[0] for w in WINDOWS]), "b": np.array([w[1] for w in WINDOWS]), "u": np.array(UNIFORMS),
        "t": nan.copy(), "rev_a": nan.copy(), "rev_b": nan.copy(), "rev_logmass": nan.copy(), "rev_dlogmass": nan.copy(),
        "rev_tail_big": nan.copy(), "rev_tail_small": nan.copy(),
    }
    for name, f in (("logmass", lambda a, b: log_mass(a, b)), ("logphi_a", lambda a, b: log_Phi(M(a))),
                    ("logphi_b", lambda a, b: log_Phi(M(b))), ("logphi_ma", lambda a, b: log_Phi(-M(a))),
                    ("logphi_mb", lambda a, b: log_Phi(-M(b)))):
        out[name] = np.array([float(f(a, b)) for a, b in WINDOWS])
    for w, (a, b) in enumerate(WINDOWS):
        for k, u in enumerate(UNIFORMS):
            if not row_is_kept(a, b, u):
                continue
            t_mp = quantile(a, b, u)
            assert abs(truncated_cdf(t_mp, a, b) - M(u)) < mpf(10) ** -40, (a, b, u)
            t = float(t_mp)
            out["t"][w, k] = t
            if not (a <= 0.0 <= b):
                continue
            ra, rb = float(np.float64(a) - np.float64(t)), float(np.float64(b) - np.float64(t))
            out["rev_a"][w, k], out["rev_b"][w, k] = ra, rb
            out["rev_logmass"][w, k] = float(log_mass(ra, rb))
            mass = Phi(M(rb)) - Phi(M(ra))
            out["rev_dlogmass"][w, k] = float((phi(M(ra)) - phi(M(rb))) / mass)
            if rb <= 0.0:    # the order of the kernel's cases
                out["rev_tail_big"][w, k], out["rev_tail_small"][w, k] = float(log_Phi(M(rb))), float(log_Phi(M(ra)))
            elif ra >= 0.0:
                out["rev_tail_big"][w, k], out["rev_tail_small"][w, k] = float(log_Phi(-M(ra))), float(log_Phi(-M(rb)))
    return out


def write_npz(path, arrays):
    """np.savez without the clock: fixed time stamps, stored (not deflated), keys in the order given."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for key, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr, dtype=np.float64), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    write_npz(os.path.join(here, "truncnorm_mp.npz"), build())
