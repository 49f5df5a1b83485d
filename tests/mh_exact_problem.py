"""Problems on which a whole Metropolis-Hastings step is exact in float64, and plain NumPy restatements of the five fused steps.

Every number of such a problem is a small dyadic rational, so every product and every sum a step forms is exactly representable:
the answer does not depend on the order of summation, and a kernel can be held to np.array_equal however it tiles, splits or
vectorises its contraction.  Only the log densities (logarithms, log 2 pi) are rounded; they enter the decision alone, which is
kept a margin away from the uniform it is tested against.

Host only: nothing here needs a GPU, and torch is never imported.  The formulas follow the header comments of
csrc/omc_mala.hip (a = L'(x - mu), a' = kappa a + z, rv = a - kappa a', ss = a squared norm, lp and lq of MhTarget).
State matrices are (C, d), one chain per row, so L'v of a chain reads v @ L and L^-T v reads v @ Linv.
"""

from fractions import Fraction

import numpy as np

LOG_2PI = 1.8378770664093453  # the constant of MhTarget::lp
MARGIN = 1e-6  # least |log u - log_alpha| of a decision (tests/test_rj_sweep_kernels_gpu.py uses the same)
LOG_U_MIN = -700.0  # log of the smallest uniform the builder injects (exp(-745) is the smallest positive double)


class Problem:
    """L (d, d) lower triangular, its inverse, sum log diag L and the target's mean, all in one dtype."""

    def __init__(self, L, Linv, sumlogL, mu):
        self.L, self.Linv, self.sumlogL, self.mu = L, Linv, sumlogL, mu
        self.d = L.shape[0]
        self.dtype = L.dtype
        self._memo = {}

    @property
    def LinvT(self):
        return self.Linv.T

    def without_mean(self):
        return Problem(self.L, self.Linv, self.sumlogL, np.zeros_like(self.mu))

    def Q(self, step):
        """The precision whose scaled factor L is: Q = step^2 L L'."""
        key = ("Q", float(step))
        if key not in self._memo:
            self._memo[key] = (step * step) * (self.L @ self.L.T)
        return self._memo[key]

    def drift(self, Q):
        """A1 = -(L L')^-1 Q through the explicit inverse."""
        key = ("A1", id(Q))
        if key not in self._memo:
            self._memo[key] = (Q, -(self.Linv.T @ (self.Linv @ Q)))  # (Q kept alive: its id is the key)
        return self._memo[key][1]


def _unit_bidiagonal_inverse(n):
    """inv(I + N) for N strictly lower bidiagonal with entries n in {-1, +1}: entry (i, j) = prod_{j <= k < i} (-n[k]) = P[i] P[j]."""
    P = np.concatenate(([1.0], np.cumprod(-n)))
    return np.tril(np.outer(P, P))


def build(d, seed):
    """L = inv(I + N1) (I + N2) diag(2^e): dense lower triangular, entries in {0, +-1, +-2} 2^e, about half fill, with an equally
    dense dyadic inverse (|entries| <= 4).  Returns a Problem; .L, .sumlogL, .mu, .LinvT are what the steps take."""
    rng = np.random.default_rng([int(d), int(seed), 20240917])
    n1 = rng.choice([-1.0, 1.0], size=d - 1)
    n2 = rng.choice([-1.0, 1.0], size=d - 1)
    e = rng.integers(-1, 2, size=d)
    eye = np.eye(d)
    L = _unit_bidiagonal_inverse(n1) @ (eye + np.diag(n2, -1)) * (2.0 ** e)[None, :]
    Linv = (2.0 ** -e)[:, None] * (_unit_bidiagonal_inverse(n2) @ (eye + np.diag(n1, -1)))
    assert np.array_equal(L @ Linv, eye) and np.array_equal(Linv @ L, eye)
    assert np.array_equal(L, np.tril(L)) and np.abs(Linv).max() <= 4.0 and np.abs(L).max() <= 4.0
    mu = rng.integers(-8, 9, size=d) / 4.0
    return Problem(L, Linv, float(e.sum()) * np.log(2.0), mu)


# ---- one step of each route ------------------------------------------------------------------------------------------------

def _sq(v):
    return np.sum(v * v, axis=1)


def _target(prob, d, log_step_term, lp_scale):
    logdetQ = 2.0 * (prob.sumlogL + log_step_term)
    c = prob.dtype.type
    lp = lambda ss: c(0.5) * (logdetQ - c(d) * c(LOG_2PI) - lp_scale * ss)  # noqa: E731
    lq = lambda ss: prob.sumlogL - c(0.5) * ss  # noqa: E731
    return lp, lq, logdetQ


def decide(rec, x, u):
    """Completes the record of a step with the test log u < log_alpha: accept flags, the new state (rejected chains keep theirs),
    the log target and the squared norm of the state left behind."""
    ok = np.log(np.asarray(u, dtype=rec["log_alpha"].dtype)) < rec["log_alpha"]
    rec["accept"] = ok
    rec["x"] = np.where(ok[:, None], rec["x_prop"], x)
    rec["logp"] = np.where(ok, rec["lp_prop"], rec["lp_cur"])
    rec["ss"] = np.where(ok, rec["ss_prop"], rec["ss_cur"])
    return rec


def _decide(x, x_prop, lp_cur, lp_prop, log_alpha, u, extra):
    out = {"log_alpha": log_alpha, "lp_cur": lp_cur, "lp_prop": lp_prop, "x_prop": x_prop}
    out.update(extra)
    return out if u is None else decide(out, x, u)  # (u None: the odds alone, for a builder that picks its uniforms from them)


def reference_mala_white(prob, step, x, z, u=None):
    """omc_mala_step_white / one step of omc_mala_run_white."""
    c = prob.dtype.type
    step = c(step)
    d = prob.d
    kappa = c(1.0) - c(0.5) * step * step
    a = (x - prob.mu) @ prob.L
    ap = kappa * a + z
    rv = a - kappa * ap
    s0, s1, s2, s3 = _sq(a), _sq(ap), _sq(rv), _sq(z)
    lp, lq, logdetQ = _target(prob, d, c(d) * np.log(step), step * step)
    lp_cur, lp_prop = lp(s0), lp(s1)
    log_alpha = lp_prop + lq(s2) - (lp_cur + lq(s3))
    x_prop = prob.mu + ap @ prob.Linv
    return _decide(x, x_prop, lp_cur, lp_prop, log_alpha, u,
                   {"a": a, "a_prop": ap, "rv": rv, "ss_cur": s0, "ss_prop": s1, "ss_rev": s2, "ss_fwd": s3, "logdetQ": logdetQ,
                    "lp_scale": step * step})


def reference_mala(prob, step, x, z, u=None, Q=None, A1=None):
    """omc_mala_step: the products route, with Q = step^2 L L' unless another Q (whose factor L is) is given."""
    c = prob.dtype.type
    step = c(step)
    d = prob.d
    Q = prob.Q(step) if Q is None else Q
    A1 = prob.drift(Q) if A1 is None else A1
    A1p = np.eye(d, dtype=prob.dtype) + c(0.5) * A1
    c0 = c(-0.5) * (A1 @ prob.mu)
    xp = x @ A1p.T + z @ prob.Linv + c0
    mp = xp @ A1p.T + c0
    t_cur, t_prop, t_rev = x - prob.mu, xp - prob.mu, x - mp
    n_cur, n_prop, n_rev = t_cur @ prob.L, t_prop @ prob.L, t_rev @ prob.L
    s0, s1, s2, s3 = _sq(n_cur), _sq(n_prop), _sq(n_rev), _sq(z)
    lp, lq, logdetQ = _target(prob, d, c(d) * np.log(step), step * step)
    lp_cur, lp_prop = lp(s0), lp(s1)
    log_alpha = lp_prop + lq(s2) - (lp_cur + lq(s3))
    return _decide(x, xp, lp_cur, lp_prop, log_alpha, u,
                   {"Q": Q, "A1": A1, "A1p": A1p, "c0": c0, "m_prop": mp, "n_cur": n_cur, "n_prop": n_prop, "n_rev": n_rev,
                    "ss_cur": s0, "ss_prop": s1, "ss_rev": s2, "ss_fwd": s3, "logdetQ": logdetQ, "lp_scale": step * step})


def _rw_move(x, z, step):
    prod = z * step  # two roundings, like mh_rw_move
    return x + prod


def reference_rw(prob, step, x, z, u=None):
    """omc_rw_step with LQ = L (the factor of Q = L L' itself)."""
    c = prob.dtype.type
    step = c(step)
    xp = _rw_move(x, z, step)
    n_cur, n_prop = (x - prob.mu) @ prob.L, (xp - prob.mu) @ prob.L
    s0, s1 = _sq(n_cur), _sq(n_prop)
    lp, _, logdetQ = _target(prob, prob.d, c(0.0), c(1.0))
    lp_cur, lp_prop = lp(s0), lp(s1)
    return _decide(x, xp, lp_cur, lp_prop, lp_prop - lp_cur, u,
                   {"n_cur": n_cur, "n_prop": n_prop, "ss_cur": s0, "ss_prop": s1, "logdetQ": logdetQ, "lp_scale": c(1.0)})


def reference_rw_white(prob, step, x, z, u=None):
    """omc_rw_step_white: a = L'(x - mu), a' = a + step L'z."""
    c = prob.dtype.type
    step = c(step)
    xp = _rw_move(x, z, step)
    a = (x - prob.mu) @ prob.L
    wz = z @ prob.L
    ap = a + step * wz
    s0, s1 = _sq(a), _sq(ap)
    lp, _, logdetQ = _target(prob, prob.d, c(0.0), c(1.0))
    lp_cur, lp_prop = lp(s0), lp(s1)
    return _decide(x, xp, lp_cur, lp_prop, lp_prop - lp_cur, u,
                   {"a": a, "wz": wz, "a_prop": ap, "ss_cur": s0, "ss_prop": s1, "logdetQ": logdetQ, "lp_scale": c(1.0)})


REFERENCES = {"mala_white": reference_mala_white, "mala": reference_mala, "rw": reference_rw, "rw_white": reference_rw_white}


# ---- the decision: uniforms that make both outcomes occur, a margin away from the odds -------------------------------------

def pick_uniforms(log_alpha, want_accept):
    """u per chain such that log u < log_alpha where an acceptance is wanted and possible, log u > log_alpha where a rejection
    is wanted and possible, the other outcome where it is not; |log u - log_alpha| is far above MARGIN either way."""
    log_alpha = np.asarray(log_alpha, dtype=np.float64)
    can_accept = log_alpha > LOG_U_MIN + 2.0
    can_reject = log_alpha < -1e-3
    accept = np.where(want_accept, can_accept | ~can_reject, ~can_reject & can_accept)
    if not np.all(can_accept | can_reject):
        raise AssertionError("a chain's odds allow neither outcome")
    log_u_acc = np.minimum(log_alpha, 0.0) - 1.0
    log_u_rej = np.maximum(0.5 * log_alpha, LOG_U_MIN)
    log_u = np.where(accept, log_u_acc, log_u_rej)
    u = np.exp(log_u)
    assert np.all((u > 0.0) & (u < 1.0))
    return u


class Case:
    """One trajectory: x0 (C, d), z (steps, C, d), u (steps, C) and the reference's record of every step."""

    def __init__(self, kind, prob, step, x0, z, u, trace):
        self.kind, self.prob, self.step, self.x0, self.z, self.u, self.trace = kind, prob, step, x0, z, u, trace
        self.steps, self.C, self.d = z.shape

    @property
    def accepts(self):
        return np.array([t["accept"] for t in self.trace])

    def check_decisions(self):
        """Both outcomes occur, the first proposal is accepted by one chain and rejected by another (one chain alone cannot do
        both: there the two outcomes fall on different steps), and no decision is within MARGIN of its uniform."""
        acc = self.accepts
        assert acc.any() and not acc.all(), "both outcomes must occur"
        if self.C >= 2:
            assert acc[0].any() and not acc[0].all(), "first proposal: one acceptance and one rejection"
        for t, rec in enumerate(self.trace):
            gap = np.abs(np.log(self.u[t]) - rec["log_alpha"])
            assert gap.min() >= MARGIN, (t, gap.min())


def _make_case(kind, d, C, step, steps, seed, with_mu, z_scale):
    prob = build(d, seed)
    if not with_mu:
        prob = prob.without_mean()
    rng = np.random.default_rng([int(d), int(C), int(steps), int(seed), 77])
    x0 = prob.mu + rng.integers(-8, 9, size=(C, d)) / 4.0
    if kind == "mala_white" and step != 2.0:
        # kappa != -1: far from the mode every proposal towards it is accepted whatever u; every other chain starts next to
        # the mode (one element a quarter off), where both outcomes can be forced
        x0[::2] = prob.mu
        x0[::2, 0] += 0.25
    z = rng.integers(-8, 9, size=(steps, C, d)) / 16.0 * z_scale
    ref = REFERENCES[kind]
    x = x0
    u = np.empty((steps, C))
    trace = []
    for t in range(steps):
        rec = ref(prob, step, x, z[t])
        la = rec["log_alpha"]
        want = (np.arange(C) + t) % 2 == 1
        if t == 0 and C >= 2:  # the first proposal: the chain with the best odds accepts, the one with the worst rejects
            want[np.argmax(la)], want[np.argmin(la)] = True, False
        u[t] = pick_uniforms(la, want)
        trace.append(decide(rec, x, u[t]))
        x = rec["x"]
    return Case(kind, prob, step, x0, z, u, trace)


def make_case(kind, d, C, step, steps, with_mu=True):
    """x0 - mu multiples of 2^-2 in [-2, 2], z multiples of 2^-4 in [-0.5, 0.5] (of 2^-6 in [-1/8, 1/8] from d = 1025 on, where
    the wider grid puts half the odds below what any log u > -745 can accept), u chosen per chain and step so that chain c is
    asked to accept step t when c + t is odd.  The first seed whose trajectory holds both outcomes (check_decisions) is taken:
    that looks at the reference alone."""
    z_scale = 0.25 if d >= 1025 else 1.0
    last = None
    for seed in range(32):
        try:
            case = _make_case(kind, d, C, step, steps, seed, with_mu, z_scale)
            case.check_decisions()
            case.seed = seed
            return case
        except AssertionError as e:
            last = e
    raise AssertionError(f"no seed below 32 gives both outcomes for {(kind, d, C, step, steps)}: {last}")


# ---- the guard that makes array_equal legitimate ---------------------------------------------------------------------------

def _ld_matmul_reversed(A, B):
    """A @ B in np.longdouble with the contraction walked from its far end."""
    return A[:, ::-1].astype(np.longdouble) @ B[::-1].astype(np.longdouble)


def _frac_matmul(A, B):
    FA = [[Fraction(float(v)) for v in row] for row in A]
    FB = [[Fraction(float(v)) for v in row] for row in B]
    return [[sum(FA[i][k] * FB[k][j] for k in range(len(FB))) for j in range(len(FB[0]))] for i in range(len(FA))]


def _grain(A):
    """The least p with every entry of A a multiple of 2^-p."""
    for p in range(0, 64):
        s = A * 2.0 ** p
        if np.array_equal(s, np.rint(s)):
            return p
    raise AssertionError("entries finer than 2^-63")


LD_MACS = 2e6  # multiply-adds of one product redone in np.longdouble (~2e8 per second); above that, a rotating subset of rows
_rot = [0]


def _same_product(A, B, got, what):
    """got == A @ B exactly, shown two ways.  (1) The bit budget: with A in units of 2^-p and B of 2^-q, every partial sum of
    every entry, in whatever order, is an integer of magnitude at most (|A| |B|) 2^(p+q); below 2^52 all of them are floats.
    (2) The recomputation in np.longdouble, contraction reversed: of every row, or -- where that would take seconds -- of
    every stride-th row, the offset rotating from product to product."""
    units = 2.0 ** (_grain(A) + _grain(B))
    assert (np.abs(A) @ np.abs(B)).max() * units < 2.0 ** 52, what
    macs = A.shape[0] * A.shape[1] * B.shape[1]
    stride = max(1, int(np.ceil(macs / LD_MACS)))
    _rot[0] += 1
    rows = slice(_rot[0] % stride, None, stride)
    want = _ld_matmul_reversed(A[rows], B)
    assert np.array_equal(want, got[rows].astype(np.longdouble)), what
    if A.shape[1] <= 4 and A.shape[0] * B.shape[1] <= 256:
        fr = _frac_matmul(A, B)
        assert all(fr[i][j] == Fraction(float(got[i, j])) for i in range(got.shape[0]) for j in range(got.shape[1])), what


def _same_sumsq(v, got, what):
    assert got.max() * 4.0 ** _grain(v) < 2.0 ** 52, what
    w = v[:, ::-1].astype(np.longdouble)
    want = np.zeros(v.shape[0], dtype=np.longdouble)
    for k in range(w.shape[1]):  # one element at a time: no pairwise tree, the reverse of the kernel's order
        want += w[:, k] * w[:, k]
    assert np.array_equal(want, got.astype(np.longdouble)), what
    if v.shape[1] <= 4 and v.shape[0] <= 64:
        for c in range(v.shape[0]):
            assert sum(Fraction(float(e)) ** 2 for e in v[c]) == Fraction(float(got[c])), what


def assert_exact(case):
    """Every matrix product and every sum of squares of the case, recomputed in np.longdouble (64-bit significand) with the
    contraction reversed -- and in exact rationals where d <= 4 -- equals the float64 result bit for bit, and fits the bit
    budget that makes it independent of the order of summation (_same_product)."""
    prob, step = case.prob, np.float64(case.step)
    L, Linv, mu = prob.L, prob.Linv, prob.mu
    x = case.x0
    if case.kind == "mala":
        rec = case.trace[0]
        _same_product(L, L.T, rec["Q"] / (step * step), "L L'")
        _same_product(Linv.T, Linv @ rec["Q"], -rec["A1"], "(L L')^-1 Q")
        _same_product(Linv, rec["Q"], Linv @ rec["Q"], "L^-1 Q")
        assert np.array_equal(rec["A1"], -(step * step) * np.eye(prob.d)), "the drift matrix is -step^2 I"
        _same_product(rec["A1"], mu[:, None], -2.0 * rec["c0"][:, None], "A1 mu")
    for t, rec in enumerate(case.trace):
        z = case.z[t]
        tag = (case.kind, case.d, case.C, t)
        if case.kind in ("mala_white", "rw_white"):
            _same_product(x - mu, L, rec["a"], tag + ("a",))
            # the library forms a = L'x + (-L'mu): both halves exact as well
            _same_product(x, L, rec["a"] + mu @ L, tag + ("L'x",))
            _same_product(mu[None, :], L, (mu @ L)[None, :], tag + ("L'mu",))
        if case.kind == "mala_white":
            kappa = 1.0 - 0.5 * step * step
            assert np.array_equal(rec["a_prop"].astype(np.longdouble), np.longdouble(kappa) * rec["a"].astype(np.longdouble) + z)
            assert np.array_equal(rec["rv"].astype(np.longdouble),
                                  rec["a"].astype(np.longdouble) - np.longdouble(kappa) * rec["a_prop"].astype(np.longdouble))
            _same_product(rec["a_prop"], Linv, rec["x_prop"] - mu, tag + ("L^-T a'",))
            assert np.array_equal((rec["x_prop"] - mu) + mu, rec["x_prop"])
            # before a first acceptance the stored state is mu + L^-T L'(x - mu) = x
            _same_product(rec["a"], Linv, x - mu, tag + ("L^-T a",))
            for k, v in (("ss_cur", rec["a"]), ("ss_prop", rec["a_prop"]), ("ss_rev", rec["rv"]), ("ss_fwd", z)):
                _same_sumsq(v, rec[k], tag + (k,))
        elif case.kind == "mala":
            xp = rec["x_prop"]
            ld = np.longdouble
            _same_product(x, rec["A1p"].T, x @ rec["A1p"].T, tag + ("A1p x",))
            _same_product(z, Linv, z @ Linv, tag + ("L^-T z",))
            # the library accumulates both products in one sum and adds c0 behind it
            both = _ld_matmul_reversed(np.hstack([x, z]), np.vstack([rec["A1p"].T, Linv]))
            assert np.array_equal(both + rec["c0"].astype(ld), xp.astype(ld)), tag + ("x'",)
            _same_product(xp, rec["A1p"].T, rec["m_prop"] - rec["c0"], tag + ("A1p x'",))
            for k, tm in (("n_cur", x - mu), ("n_prop", xp - mu), ("n_rev", x - rec["m_prop"])):
                _same_product(tm, L, rec[k], tag + (k,))
            assert np.array_equal(x.astype(ld) - rec["m_prop"].astype(ld), (x - rec["m_prop"]).astype(ld))
            for k, v in (("ss_cur", rec["n_cur"]), ("ss_prop", rec["n_prop"]), ("ss_rev", rec["n_rev"]), ("ss_fwd", z)):
                _same_sumsq(v, rec[k], tag + (k,))
        elif case.kind == "rw":
            xp = rec["x_prop"]
            assert np.array_equal(x.astype(np.longdouble) + z.astype(np.longdouble) * np.longdouble(step), xp.astype(np.longdouble))
            _same_product(x - mu, L, rec["n_cur"], tag + ("n_cur",))
            _same_product(xp - mu, L, rec["n_prop"], tag + ("n_prop",))
            _same_sumsq(rec["n_cur"], rec["ss_cur"], tag + ("ss_cur",))
            _same_sumsq(rec["n_prop"], rec["ss_prop"], tag + ("ss_prop",))
        else:
            assert np.array_equal(x.astype(np.longdouble) + z.astype(np.longdouble) * np.longdouble(step),
                                  rec["x_prop"].astype(np.longdouble))
            _same_product(z, L, rec["wz"], tag + ("L'z",))
            assert np.array_equal(rec["a"].astype(np.longdouble) + np.longdouble(step) * rec["wz"].astype(np.longdouble),
                                  rec["a_prop"].astype(np.longdouble))
            _same_sumsq(rec["a"], rec["ss_cur"], tag + ("ss_cur",))
            _same_sumsq(rec["a_prop"], rec["ss_prop"], tag + ("ss_prop",))
        x = rec["x"]


# ---- what the GPU file runs: one list, so that the host file guards exactly those cases ------------------------------------

SHAPES = [(1, 1), (2, 17), (31, 16), (32, 15), (33, 33), (63, 1), (64, 16), (65, 17), (66, 33), (127, 15), (128, 16), (129, 17),
          (130, 33), (257, 5), (513, 3), (1025, 2)]
HALF_STEP_SHAPES = [(2, 17), (33, 33), (64, 16), (65, 17), (130, 33), (513, 3)]  # step = 1: kappa = 1/2, a bit more per acceptance
RUN_SMALL_SHAPES = [(1, 1), (33, 33), (64, 16), (130, 33), (513, 3), (1025, 2)]
RUN_SMALL_STEPS, RUN_DRAW_STRIDE = 7, 3
RUN_WIDE_CASES = [(65, 131, 33), (130, 131, 33), (64, 128, 32), (257, 130, 34), (513, 128, 32)]


def step_cases():
    """(kind, d, C, step, steps, with_mu) of every single-step case."""
    out = []
    for d, C in SHAPES:
        for with_mu in (True, False):
            out.append(("mala_white", d, C, 2.0, 4, with_mu))
            out.append(("rw_white", d, C, 0.5, 4, with_mu))
        out.append(("mala", d, C, 2.0, 4, True))
        out.append(("rw", d, C, 0.5, 4, True))
    for d, C in HALF_STEP_SHAPES:
        out.append(("mala_white", d, C, 1.0, 3, True))
    return out


def run_cases():
    """(kind, d, C, step, steps, with_mu) of every omc_mala_run_white case."""
    return ([("mala_white", d, C, 2.0, RUN_SMALL_STEPS, True) for d, C in RUN_SMALL_SHAPES]
            + [("mala_white", d, C, 2.0, steps, True) for d, C, steps in RUN_WIDE_CASES])


_CASES = {}


def get_case(kind, d, C, step, steps, with_mu=True):
    """The case of these parameters, built once per process and never modified."""
    key = (kind, d, C, float(step), steps, with_mu)
    if key not in _CASES:
        _CASES[key] = make_case(kind, d, C, step, steps, with_mu=with_mu)
    return _CASES[key]


# ---- float data: the same restatements in np.longdouble against float64 -----------------------------------------------------

def _ld_lower_inverse(L):
    """inv(L) of a lower triangular float64 matrix by forward substitution in np.longdouble."""
    d = L.shape[0]
    Ll = L.astype(np.longdouble)
    X = np.zeros((d, d), dtype=np.longdouble)
    for i in range(d):
        X[i] = -(Ll[i, :i] @ X[:i])
        X[i, i] += 1
        X[i] /= Ll[i, i]
    return X


class FloatCase:
    """A random SPD target (as tests/test_mh_gpu.py::test_own_gemm_route_matches_rocblas_route draws it), L formed on the host,
    and two trajectories of one route under the same injected z and u: np.longdouble (the reference) and float64."""

    def __init__(self, kind, d, C, steps):
        from scipy.linalg import cho_solve, solve_triangular

        ld = np.longdouble
        rng = np.random.default_rng(d + C)
        A = rng.standard_normal((d, 2 * d))
        Qh = np.linalg.inv(A @ A.T / (2 * d))
        Qh = (Qh + Qh.T) / 2
        mu = rng.standard_normal(d)
        x0 = mu + np.linalg.solve(np.linalg.cholesky(Qh).T, rng.standard_normal((d, C))).T
        mala = kind in ("mala", "mala_white")
        step = 0.5 if mala else 0.05
        L = np.linalg.cholesky(Qh / step**2) if mala else np.linalg.cholesky(Qh)
        z = rng.standard_normal((steps, C, d))
        p64 = Problem(L, solve_triangular(L, np.eye(d), lower=True), float(np.log(np.diag(L)).sum()), mu)
        pld = Problem(L.astype(ld), _ld_lower_inverse(L), np.log(np.diag(L).astype(ld)).sum(), mu.astype(ld))
        kw64, kwld = {}, {}
        if kind == "mala":
            kw64 = {"Q": Qh, "A1": cho_solve((L, True), -Qh)}
            kwld = {"Q": Qh.astype(ld)}
        ref = REFERENCES[kind]
        self.kind, self.d, self.C, self.steps, self.step = kind, d, C, steps, step
        self.Q, self.L, self.sumlogL, self.mu, self.x0, self.z = Qh, L, p64.sumlogL, mu, x0, z
        self.u = np.empty((steps, C))
        self.trace_ld, self.trace_64 = [], []
        xl, x64 = x0.astype(ld), x0
        for t in range(steps):
            rec = ref(pld, step, xl, z[t].astype(ld), **kwld)
            want = (np.arange(C) + t) % 2 == 1
            self.u[t] = pick_uniforms(rec["log_alpha"].astype(np.float64), want)
            self.trace_ld.append(decide(rec, xl, self.u[t]))
            self.trace_64.append(ref(p64, step, x64, z[t], self.u[t], **kw64))
            xl, x64 = self.trace_ld[-1]["x"], self.trace_64[-1]["x"]

    def check_decisions(self):
        for t in range(self.steps):
            acc = self.trace_ld[t]["accept"]
            assert acc.any() and not acc.all()
            assert np.array_equal(acc, self.trace_64[t]["accept"])
            gap = np.abs(np.log(self.u[t]) - self.trace_ld[t]["log_alpha"].astype(np.float64))
            assert gap.min() >= MARGIN, (t, gap.min())


_FLOAT_CASES = {}


def get_float_case(kind, d, C=33, steps=3):
    key = (kind, d, C, steps)
    if key not in _FLOAT_CASES:
        _FLOAT_CASES[key] = FloatCase(kind, d, C, steps)
    return _FLOAT_CASES[key]
