"""Inputs for the spectral dense draw (csrc/omc_spectral.hip) and a plain host evaluation of it, chain by chain.

The draw, as the header comment of omc_spectral.hip states it: with M = V diag(ev) V' shared by all chains and
Q_c = a_c I + b_c M,

    b    = sum_k s_k rhs_k + rhs_chain          (an absent scale is 1, an absent rhs is 0)
    d    = sum_{k != k_mat} s_k + s_{k_mat} ev
    m    = V'b / d                              (the mean in the eigenbasis)
    x    = V (m + z / sqrt(d)),   mean = V m,   logdet = sum log d.

Two builders.  exact_case: data on which every intermediate of that route is exactly representable in float64 -- V a signed
permutation (every dot product has one non-zero term), every d a power of 4 (so 1 / d and sqrt(1 / d) are powers of 2), all
other numbers small dyadic rationals -- so the answer does not depend on the order of any summation and a kernel can be held to
np.array_equal however it tiles or splits its products.  Only the log-determinant (a logarithm) is rounded.  random_case: a
random orthogonal V and well-conditioned scales, for a comparison to rounding with the np.longdouble evaluation.

Host only: nothing here needs a GPU, and torch is never imported.  The library keeps V with eigenvector j in memory row j
(what omc_dense_spectral_prepare leaves: the column-major V); Case.V is that array, so V'b reads V @ b and V y reads V.T @ y.
"""

from fractions import Fraction

import numpy as np

EV_EXACT = (0.0, 3.0, 15.0, 63.0)  # 1 + ev is a power of 4
# the terms of the default layout, in order: identity with a rhs, the matrix term with a rhs (k_mat = 1), identity without
# (kind, has a rhs, scale): the scale is a multiple of 4^j_c (identity terms of an exact case sum to 4^j_c, the matrix term's
# is 4^j_c); None is an absent scale (the library reads 1); "vary" a per-chain pick of {1/4, 1/2, 3/4} 4^j_c; "fill" whatever
# brings the identity terms to 4^j_c in sum
DEFAULT_LAYOUT = (("I", True, 0.75), ("M", True, 1.0), ("I", False, 0.25))
# the shapes (p, C) tests/test_spectral_gpu.py runs, so that tests/test_spectral_problem_host.py guards exactly those
GPU_SHAPES = [(1, 1), (2, 5), (3, 17), (31, 5), (32, 16), (33, 17), (63, 5), (64, 65), (65, 17), (130, 5), (513, 3), (514, 3)]
FRACTION_P = (1, 2, 3, 31, 33, 65, 130)  # orders at which the exact construction is checked in rationals


class Case:
    """One call of omc_dense_spectral_sample.  V (p, p) eigenvector j in row j, ev (p,), terms a list of
    {"kind": "I" | "M", "rhs": (p,) or None, "scale": (C,) or None}, k_mat, rhs_chain (C, p) or None, z (C, p).  Never modified."""

    def __init__(self, V, ev, terms, k_mat, rhs_chain, z):
        self.V, self.ev, self.terms, self.k_mat, self.rhs_chain, self.z = V, ev, terms, k_mat, rhs_chain, z
        self.C, self.p = z.shape
        assert terms[k_mat]["kind"] == "M" and sum(t["kind"] == "M" for t in terms) == 1

    def replace(self, **kw):
        f = dict(V=self.V, ev=self.ev, terms=self.terms, k_mat=self.k_mat, rhs_chain=self.rhs_chain, z=self.z)
        f.update(kw)
        return Case(**f)


def signed_cycle(p, rng):
    """V (eigenvectors in columns): column i is sign_i e_{perm(i)}, perm one p-cycle (for p <= 2 the reversal).  For p >= 3 it
    is not its own inverse: V handed where V' is wanted gives another vector."""
    perm = np.roll(np.arange(p), 1) if p > 2 else np.arange(p)[::-1]
    V = np.zeros((p, p))
    V[perm, np.arange(p)] = rng.choice([-1.0, 1.0], size=p)
    return V


def _exact_scales(layout, C, rng, j_values):
    j = rng.choice(np.asarray(j_values), size=C)
    unit = 4.0 ** j
    scales, ident_sum, fill_at = [], np.zeros(C), None
    for k, (kind, _, coef) in enumerate(layout):
        if coef is None:
            s, contrib = None, np.ones(C)
        elif coef == "vary":
            s = rng.choice([0.25, 0.5, 0.75], size=C) * unit
            contrib = s
        elif coef == "fill":
            assert kind == "I" and fill_at is None
            s, contrib, fill_at = None, np.zeros(C), k
        else:
            s = coef * unit
            contrib = s
        scales.append(s)
        if kind == "I":
            ident_sum = ident_sum + contrib
    if fill_at is not None:
        scales[fill_at] = unit - ident_sum
        assert np.all(scales[fill_at] > 0)
    return scales


def exact_case(p, C, seed, layout=DEFAULT_LAYOUT, j_values=(-2, -1, 0, 1, 2), with_rhs_chain=True):
    """ev in {0, 3, 15, 63}; per chain j_c in j_values, the matrix term's scale 4^j_c and the identity terms' scales summing to
    4^j_c, so d = 4^j_c (1 + ev) is a power of 4; shared right-hand sides multiples of 1/4 and of 1/8 (alternating by term) in
    [-2, 2], rhs_chain multiples of 1/16 in [-1, 1], z multiples of 1/16 in [-2, 2]."""
    for attempt in range(64):
        case = _exact_case(p, C, seed, attempt, layout, j_values, with_rhs_chain)
        if logdet_is_well_conditioned(case):
            return case
    raise AssertionError(f"no attempt below 64 gives a log-determinant free of cancellation for {(p, C, seed)}")


def logdet_is_well_conditioned(case):
    """sum log d of every chain is at least a quarter of sum |log d| (all d = 1 included: both are 0 then, exactly).  The exact
    data has d on both sides of 1; where the logarithms cancel, a bar relative to their sum would measure the cancellation and
    not the kernel.  exact_case takes the first attempt that passes: a look at the inputs alone."""
    for c in range(case.C):
        a = sum(1.0 if t["scale"] is None else t["scale"][c] for k, t in enumerate(case.terms) if k != case.k_mat)
        s = case.terms[case.k_mat]["scale"]
        logs = np.log(a + (1.0 if s is None else s[c]) * case.ev)
        if abs(logs.sum()) < 0.25 * np.abs(logs).sum():
            return False
    return True


def _exact_case(p, C, seed, attempt, layout, j_values, with_rhs_chain):
    rng = np.random.default_rng([int(p), int(C), int(seed), int(attempt), 20241020])
    V = signed_cycle(p, rng)
    ev = rng.choice(np.asarray(EV_EXACT), size=p)
    scales = _exact_scales(layout, C, rng, j_values)
    terms, n_rhs = [], 0
    for (kind, has_rhs, _), s in zip(layout, scales):
        rhs = None
        if has_rhs:
            grain = 4 if n_rhs % 2 == 0 else 8
            rhs = rng.integers(-2 * grain, 2 * grain + 1, size=p) / float(grain)
            n_rhs += 1
        terms.append({"kind": kind, "rhs": rhs, "scale": s})
    k_mat = [t["kind"] for t in terms].index("M")
    rhs_chain = rng.integers(-16, 17, size=(C, p)) / 16.0 if with_rhs_chain else None
    z = rng.integers(-32, 33, size=(C, p)) / 16.0
    return Case(np.ascontiguousarray(V.T), ev, terms, k_mat, rhs_chain, z)


def random_case(p, C, seed):
    """V from the QR factorisation of a Gaussian matrix, ev uniform in [0.1, 10], scales in [0.5, 2.5], Gaussian right-hand
    sides and z; the terms of the default layout."""
    rng = np.random.default_rng([int(p), int(C), int(seed), 20241021])
    V, _ = np.linalg.qr(rng.standard_normal((p, p)))
    ev = rng.uniform(0.1, 10.0, size=p)
    terms = [{"kind": kind, "rhs": rng.standard_normal(p) if has_rhs else None, "scale": rng.uniform(0.5, 2.5, size=C)}
             for kind, has_rhs, _ in DEFAULT_LAYOUT]
    return Case(np.ascontiguousarray(V.T), ev, terms, 1, rng.standard_normal((C, p)), rng.standard_normal((C, p)))


def reference(case, c, dtype=np.longdouble):
    """(x, mean, logdet) of chain c, every operation in `dtype`."""
    f = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    V, ev, z = f(case.V), f(case.ev), f(case.z[c])
    b = f(case.rhs_chain[c]) if case.rhs_chain is not None else np.zeros(case.p, dtype=dtype)
    a, bm = dtype(0), dtype(0)
    for k, t in enumerate(case.terms):
        s = dtype(1) if t["scale"] is None else dtype(t["scale"][c])
        if t["rhs"] is not None:
            b = b + s * f(t["rhs"])
        if k == case.k_mat:
            bm = s
        else:
            a = a + s
    d = a + bm * ev
    m = (V @ b) / d
    y = m + z / np.sqrt(d)
    return V.T @ y, V.T @ m, np.sum(np.log(d))


def reference_all(case, dtype=np.longdouble):
    """(x (C, p), mean (C, p), logdet (C,)) of all chains."""
    out = [reference(case, c, dtype) for c in range(case.C)]
    return tuple(np.array([o[i] for o in out]) for i in range(3))


# ---- the guard that makes array_equal legitimate ---------------------------------------------------------------------------

def fraction_reference(case, c):
    """(x, mean, d, sqrt d) of chain c in exact rationals.  sqrt d is the float64 square root read as a rational; that it squares
    back to d is asserted here, so x is the exact value of the formula."""
    F = lambda v: Fraction(float(v))  # noqa: E731
    p = case.p
    b = [F(v) for v in case.rhs_chain[c]] if case.rhs_chain is not None else [Fraction(0)] * p
    a, bm = Fraction(0), Fraction(0)
    for k, t in enumerate(case.terms):
        s = Fraction(1) if t["scale"] is None else F(t["scale"][c])
        if t["rhs"] is not None:
            b = [bi + s * F(r) for bi, r in zip(b, t["rhs"])]
        if k == case.k_mat:
            bm = s
        else:
            a += s
    d = [a + bm * F(e) for e in case.ev]
    rt = [F(np.sqrt(float(di))) for di in d]
    assert all(r * r == di for r, di in zip(rt, d)), "sqrt(d) is not exact"
    rows = [[(i, F(case.V[j, i])) for i in np.flatnonzero(case.V[j])] for j in range(p)]  # V'b: row j of the stored array
    m = [sum(v * b[i] for i, v in rows[j]) / d[j] for j in range(p)]
    y = [m[j] + F(case.z[c, j]) / rt[j] for j in range(p)]
    x, mean = [Fraction(0)] * p, [Fraction(0)] * p
    for j in range(p):
        for i, v in rows[j]:
            x[i] += v * y[j]
            mean[i] += v * m[j]
    return x, mean, d, rt


def assert_exact(case, fractions=False):
    """The float64 evaluation of every chain equals the np.longdouble one bit for bit, with the contractions walked the other
    way round (V and the vectors reversed), and -- where asked -- the one in rationals: no operation of the route rounds."""
    for c in range(case.C):
        x64, m64, _ = reference(case, c, np.float64)
        rev = case.replace(V=np.ascontiguousarray(case.V[::-1, ::-1]), ev=case.ev[::-1],
                           terms=[dict(t, rhs=None if t["rhs"] is None else t["rhs"][::-1]) for t in case.terms],
                           rhs_chain=None if case.rhs_chain is None else case.rhs_chain[:, ::-1], z=case.z[:, ::-1])
        xl, ml, _ = reference(rev, c, np.longdouble)
        assert np.array_equal(xl[::-1], x64.astype(np.longdouble)) and np.array_equal(ml[::-1], m64.astype(np.longdouble)), c
        if fractions:
            xf, mf, d, _ = fraction_reference(case, c)
            assert all(Fraction(float(g)) == w for g, w in zip(x64, xf)), c
            assert all(Fraction(float(g)) == w for g, w in zip(m64, mf)), c
            assert all(di > 0 and np.log2(float(di)) % 2 == 0 for di in d), c  # powers of 4


# ---- the layouts of terms tests/test_spectral_gpu.py runs at p = 33, C = 5 (exact data) ------------------------------------
LAYOUTS = {
    "k_mat=0": dict(layout=(("M", True, 1.0), ("I", True, 0.5), ("I", False, 0.25), ("I", True, 0.25))),
    "k_mat=1": dict(layout=(("I", True, 0.5), ("M", True, 1.0), ("I", False, 0.25), ("I", True, 0.25))),
    "k_mat=2": dict(layout=(("I", True, 0.5), ("I", False, 0.25), ("M", True, 1.0), ("I", True, 0.25))),
    "k_mat=3": dict(layout=(("I", True, 0.5), ("I", False, 0.25), ("I", True, 0.25), ("M", False, 1.0))),
    "one-identity": dict(layout=(("M", True, 1.0), ("I", True, 1.0))),
    "one-identity-no-rhs": dict(layout=(("I", False, 1.0), ("M", True, 1.0))),
    "two-identities": dict(layout=(("I", True, "vary"), ("M", False, 1.0), ("I", True, "fill"))),
    # absent scales: an identity that counts 1 (the other one 4^j - 1, j >= 1), and a matrix term that counts 1 (the identity
    # terms then sum to 1, split differently from chain to chain)
    "identity-scale-absent": dict(layout=(("I", True, None), ("M", True, 1.0), ("I", True, "fill")), j_values=(1, 2)),
    "matrix-scale-absent": dict(layout=(("I", True, "vary"), ("M", True, None), ("I", False, "fill")), j_values=(0,)),
    "rhs_chain-absent": dict(layout=DEFAULT_LAYOUT, with_rhs_chain=False),
    "no-rhs-at-all": dict(layout=(("I", False, 0.75), ("M", False, 1.0), ("I", False, 0.25)), with_rhs_chain=False),
}
LAYOUT_SHAPE = (33, 5)


_CASES = {}


def get_exact(p, C, seed=0, name=None):
    """The exact case of these parameters (name: a key of LAYOUTS, None the default layout), built once per process."""
    key = ("exact", p, C, seed, name)
    if key not in _CASES:
        _CASES[key] = exact_case(p, C, seed, **(LAYOUTS[name] if name else {}))
    return _CASES[key]


def get_random(p, C, seed=0):
    key = ("random", p, C, seed)
    if key not in _CASES:
        _CASES[key] = random_case(p, C, seed)
    return _CASES[key]
