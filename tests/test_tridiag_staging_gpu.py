"""First loads and exact rescaling of the segmented tridiagonal kernel (k_tridiag_seg), with injected draws.

Staging: the three shared vectors of the smoother (off-diagonal, diagonal, right-hand side) go from global memory through
registers into the wave's LDS tile.  Whatever path a wave takes for that -- full wave or the chain's partly empty last one,
vectors that are 16-byte aligned (the LDS-DMA parking of the quadratic forms' slices is then on) or only 8-byte aligned --
the tile image, and with it every x, must be the same bit for bit; x is held against the serial kernel and the fp64 oracle.

Scaling: the Moebius scans rescale by exact powers of two (mob_rescale, omc_tridiag_scan.h).  Precision scales from 1e-8 to
1e9 on chains of twelve and sixteen waves, and a chain that falls apart in the middle, against the 80-bit recurrence of
oracle/longdouble_ref.py at the bound of tests/test_tridiag_joins_gpu.py; the start values must be accepted as they come
(no sequential join sweep).

Segment width 10 throughout (a wave covers 640 nodes): n = 640 is the sub-wave form, 641 ... 1281 the generic
workgroup form on two and three waves, 7680 and 10 000 the structure-specialised forms."""

import numpy as np
import pytest
from scipy import sparse

from oracle import gmrf_ref, longdouble_ref

pytestmark = pytest.mark.gpu

TOL = 1e-10  # tests/test_tridiag_gpu.py: Gaussian quantities against the oracle, serial against segmented kernel

FORMS = ["smoother_p_first", "smoother_i_first", "shifted_shared_centre", "shifted_no_centre", "generic"]


def make_engine(C, **kw):
    from openmcmc_amd.engine import Engine

    return Engine(C, **kw)


def relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


class Problem:
    """Q_c = lam_c P + tau_c I,  rhs_c = tau_c y (if the identity term has a centre) + lam_c P m_c (if the prior has one)."""

    def __init__(self, n, C, form):
        rng = np.random.default_rng(1000 * n + C + 7 * FORMS.index(form))
        self.n, self.C, self.form = n, C, form
        pd = np.full(n, 2.0)
        pd[0] = pd[-1] = 1.0
        pd[0] += 1e-3
        self.pd = pd * (1 + 0.1 * rng.random(n))
        self.po = -np.ones(n - 1)
        self.y = rng.standard_normal(n) + 2
        self.lam, self.tau = 50 + 100 * rng.random(C), 0.5 + rng.random(C)
        self.z = rng.standard_normal((C, n))
        self.shifted = form.startswith("shifted")
        self.with_y = form != "shifted_no_centre"
        self.m = 0.3 * rng.standard_normal((C, n)) + 1.0 if self.shifted else None
        self.P = sparse.diags((self.po, self.pd, self.po), offsets=[-1, 0, 1], format="csc")

    def prior_pull(self):  # lam_c P m_c, the prior centre's part of the right-hand side
        return np.stack([self.lam[c] * (self.P @ self.m[c]) for c in range(self.C)])

    def oracle(self, c):
        n = self.n
        Q = (self.lam[c] * self.P + self.tau[c] * sparse.identity(n, format="csc")).tocsc()
        b = np.zeros(n)
        if self.with_y:
            b += self.tau[c] * self.y
        if self.shifted:
            b += self.lam[c] * (self.P @ self.m[c])
        x, _, _ = gmrf_ref.draw_canonical(b.reshape(n, 1), Q, self.z[c])
        return np.asarray(x).ravel()

    def draw(self, algo, misaligned=False):
        """x of every chain: algo 2 = segmented kernel in the form under test, 1 = serial kernel (per-chain centres go in
        as a right-hand side there: no kernel but the segmented one takes them)."""
        n, C = self.n, self.C
        eng = make_engine(C)
        eng.set_option("tridiag_algo", algo)
        eng.set_option("tridiag_seg", 10 if algo == 2 else 0)
        if self.form == "generic":
            eng.set_option("tridiag_generic", 1)

        def dev(v):
            if not misaligned:
                return eng.to_device(v)
            return eng.to_device(np.concatenate([[0.0], v]))[1:]  # data pointer = base + 8 bytes

        t_prior = {"diag": dev(self.pd), "off": dev(self.po), "scale": eng.to_device(self.lam)}
        t_lik = {"scale": eng.to_device(self.tau)}
        if self.with_y:
            d_y = dev(self.y)
            t_lik.update(rhs=d_y, center=d_y)
        rhs_chain = None
        if self.shifted and algo == 2:
            t_prior["center_chain"] = eng.to_device(self.m)
        elif self.shifted:
            rhs_chain = eng.to_device(self.prior_pull())
        terms = [t_lik, t_prior] if self.form == "smoother_i_first" else [t_prior, t_lik]
        x = eng.empty(C, n)
        eng.tridiag_sample_canonical(n, terms, x, z=eng.to_device(self.z), rhs_chain=rhs_chain, quad_out=eng.empty(2, C))
        eng.check_status()
        out = x.cpu().numpy().copy()
        eng.close()
        return out


# (n = 640 is 64 segments, the sub-wave form: per-chain centres exist from the workgroup form on, so the two shifted
# forms start at 641 -- tests/test_tridiag_gpu.py holds the refusal below that)
CASES = [(n, C, form) for n, C in [(640, 3), (1280, 3), (641, 3), (1279, 3), (1281, 3), (10000, 4)] for form in FORMS
         if not (n == 640 and form.startswith("shifted"))]


@pytest.mark.parametrize("n,C,form", CASES)
def test_staging_paths_leave_the_same_draw(form, n, C):
    p = Problem(n, C, form)
    x = p.draw(2)
    x8 = p.draw(2, misaligned=True)  # vectors at base + 8 bytes: the 8-byte path, no LDS-DMA parking
    xs = p.draw(1)
    e_serial = relerr(x, xs)
    e_oracle = max(relerr(x[c], p.oracle(c)) for c in (0, C - 1))
    print(f"{form} n={n}: vs serial {e_serial:.2e}, vs oracle {e_oracle:.2e}, differing entries aligned/offset {int(np.sum(x != x8))}")
    assert np.all(np.isfinite(x))
    assert np.array_equal(x, x8)
    assert e_serial < TOL
    assert e_oracle < TOL


# ---------------------------------------------------------------------------------------------------
def scaled_problem(n, lam, tau, seed=5, cut=None):
    rng = np.random.default_rng(seed)
    pd = np.full(n, 2.0)
    pd[0] = pd[-1] = 1.0
    pd[0] += 1e-3
    pd = pd * (1 + 0.1 * rng.random(n))
    po = -np.ones(n - 1)
    if cut is not None:
        po[cut] = 0.0  # the chain falls apart behind node `cut`
    y = rng.standard_normal(n) + 2
    z = rng.standard_normal(n)
    return pd, po, y, z, lam * pd + tau, lam * po, tau * y


def gpu_draw(n, pd, po, y, z, lam, tau, algo, seg):
    eng = make_engine(2)
    eng.set_option("tridiag_algo", algo)
    eng.set_option("tridiag_seg", seg)
    terms = [{"diag": eng.to_device(pd), "off": eng.to_device(po), "scale": eng.full((2,), lam)},
             {"rhs": eng.to_device(y), "center": eng.to_device(y), "scale": eng.full((2,), tau)}]
    x, mean, logdet = eng.empty(2, n), eng.empty(2, n), eng.empty(2)
    eng.tridiag_sample_canonical(n, terms, x, z=eng.to_device(np.tile(z, (2, 1))), mean_out=mean, logdet_out=logdet)
    eng.check_status()
    fb = eng.counter("tridiag_join_fallbacks")
    out = x[1].cpu().numpy(), mean[1].cpu().numpy(), float(logdet[1].item()), fb
    eng.close()
    return out


def check_against_extended_precision(n, lam, tau, cut=None):
    """The bound of tests/test_tridiag_joins_gpu.py: within 20 times the serial fp64 kernel's own distance from the
    longdouble answer (at least 2e-13), the log determinant likewise; and the sequential join sweep never ran (the parent
    commit's kernel runs none on any of these chains)."""
    pd, po, y, z, a, b, r = scaled_problem(n, lam, tau, cut=cut)
    x_ld, mu_ld, logdet_ld = longdouble_ref.tridiag_draw(a, b, r, z)
    xs, ms, lds, _ = gpu_draw(n, pd, po, y, z, lam, tau, 1, 0)
    e_serial = max(relerr(xs, x_ld), relerr(ms, mu_ld))
    xg, mg, ldg, fb = gpu_draw(n, pd, po, y, z, lam, tau, 2, 10)
    e = max(relerr(xg, x_ld), relerr(mg, mu_ld))
    print(f"n={n} lam={lam:g} cut={cut}: serial {e_serial:.2e}, segmented {e:.2e}, log det {abs(ldg - logdet_ld) / abs(logdet_ld):.2e}, "
          f"join fallbacks {fb}")
    assert e_serial < 1e-12
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(mg))
    assert e <= max(20 * e_serial, 2e-13), (e, e_serial)
    assert abs(ldg - logdet_ld) <= 2e-13 * abs(logdet_ld) + 20 * abs(lds - logdet_ld)
    assert fb == 0


@pytest.mark.parametrize("n", [7680, 10000])  # twelve full waves; sixteen, the last one partly empty
@pytest.mark.parametrize("lam", [1e-8, 1.0, 1e6, 1e9])
def test_precision_scales_against_extended_precision(n, lam):
    check_against_extended_precision(n, lam, 1.0)


@pytest.mark.parametrize("n,cut", [(7680, 3839), (10000, 4999), (10000, 5003)])  # at a wave's last node, at a segment's last, inside one
def test_zero_off_diagonal_in_mid_chain(n, cut):
    check_against_extended_precision(n, 100.0, 1.0, cut=cut)
