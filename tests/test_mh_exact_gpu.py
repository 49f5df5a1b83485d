"""The five fused Metropolis-Hastings steps and their own fp64-MFMA GEMM (csrc/omc_gemm.hip) against a plain NumPy reference,
bit for bit, on problems where every product and every sum is exact in float64 (tests/mh_exact_problem.py; its exactness is shown
on the host by tests/test_mh_exact_host.py).  On such data the answer does not depend on the order of summation, so one
np.array_equal holds every k-split, both load forms (scalar and 16-byte), both tile shapes and the rocBLAS route to the same
numbers -- and a wrong tile edge, a skipped slab or a misplaced accumulator row cannot hide below a tolerance.

Shapes straddle the tile edges in M (64), N (16 and 64) and K (32) and the k-split's idle groups.  The state is given packed, with
a row stride of d + 1, and as a view into a strided buffer that starts at an odd (8-byte aligned only) and at an even element;
everything outside the view is NaN before and must be NaN after.

Which kernels the groups reach (from the dispatch in omc_dgemm_small / omc_dgemm_wide: 16-byte loads need M, K and every leading
dimension even and 16-byte aligned bases):
  * whitened steps and small-tile runs: k_dgemm_64x16<false, 1 | 2 | 4> at every odd d and, for the products that read the state,
    at every layout with an odd row stride or an odd start; k_dgemm_64x16<true, 1 | 2 | 4> at even d on the packed and the
    (d + 2, start 2) layouts, and for L^-T a whatever the layout of x;
  * products steps: the same six through the fused two-pair launch (x' = A1p x + L^-T z + c0) and the `tri` products, plus rocBLAS;
  * runs with 32 steps x C >= 4096 columns: k_dgemm_64x64<false> (d = 65, 257, 513), k_dgemm_64x64<true> (d = 64, 130), the
    remainder block of one or two steps on k_dgemm_64x16.

Last: one float-data check per entry point against np.longdouble, where a rejected chain's untouched state shows whether the
column mask of the epilogue is honoured (on exact data a rewritten state would carry the same bits).

Slips tried by hand, one at a time, and the cases here that fail on each (none was caught by nothing):
  * rows of the f32 C/D map, 4 (lane >> 4) + r, in k_dgemm_64x16: every MALA group, the runs, the float checks (the random
    walks form only sums of squares of the product, which a permutation of rows within a tile leaves alone: there it shows
    at partial row tiles only); in k_dgemm_64x64: all five wide-tile runs;
  * `tri` starting one slab late: in k_dgemm_64x16 every group at every shape; in k_dgemm_64x64 all five wide-tile runs;
  * the last k-split group's partial tile left out of the sum: every group from d = 33 on (below, that group is idle);
  * acc[0] alone instead of the four accumulators: every group from d = 5 on;
  * addv dropped in k_dgemm_64x64: all five wide-tile runs (the mean is not zero);
  * kappa without its sign in rv: the whitened MALA steps (k_mala_white) and the runs (k_mala_white_run), each in its own tests;
  * the column mask ignored: test_step_on_float_data_against_longdouble[mala_white-*] alone, as said above.
mh_normal_pair handing out z[1] beyond an odd d changes no result: all three consumers stop at d before they use it.
"""

import numpy as np
import pytest

import mh_exact_problem as P

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LAYOUTS = [("packed", 0, 0), ("stride d+1", 1, 0), ("stride d+2 from 1", 2, 1), ("stride d+2 from 2", 2, 2)]
KSPLITS = (1, 2, 4)


def make_engine(C):
    from openmcmc_amd.engine import Engine

    return Engine(C)


class View:
    """A (C, d) view with row stride d + pad that starts at element `off` of a NaN-filled buffer."""

    def __init__(self, C, d, pad, off):
        import torch

        self.C, self.d, self.ld, self.off = C, d, d + pad, off
        self.buf = torch.full((off + C * self.ld,), float("nan"), dtype=torch.float64, device="cuda")
        self.t = self.buf.as_strided((C, d), (self.ld, 1), off)
        assert self.t.data_ptr() == self.buf.data_ptr() + 8 * off

    def fill(self, host):
        import torch

        self.t.copy_(torch.as_tensor(np.ascontiguousarray(host), device="cuda"))
        return self.t

    def numpy(self):
        return self.t.cpu().numpy()

    def padding_is_nan(self):
        b = self.buf.cpu().numpy()
        inside = np.zeros(b.shape, dtype=bool)
        for c in range(self.C):
            inside[self.off + c * self.ld: self.off + c * self.ld + self.d] = True
        return bool(np.isnan(b[~inside]).all()) and not np.isnan(b[inside]).any()


def same(got, want, tag):
    """np.array_equal, with the place of the damage in the message: rows are chains, columns are elements of the state."""
    if np.array_equal(got, want):
        return
    bad = np.argwhere(~(got == want))
    rows, cols = np.unique(bad[:, -2]), np.unique(bad[:, -1])
    first = tuple(bad[0])
    raise AssertionError(f"{tag}: {len(bad)} of {got.size} entries differ; chains {rows[:12].tolist()}, elements {cols[:24].tolist()} "
                         f"(first {first}: got {got[first]!r}, want {want[first]!r})")


def device_problem(eng, case, with_mu=True):
    """L as the library takes it (column-major, i.e. the row-major image of L'), sum log diag L, mu."""
    prob = case.prob
    L = eng.to_device(np.ascontiguousarray(prob.L.T))
    sl = eng.to_device(np.array([prob.sumlogL]))
    mu = eng.to_device(prob.mu) if with_mu else None
    return L, sl, mu


def logp_bound(rec):
    """Three roundings of MhTarget::lp = 0.5 (logdetQ - d log 2 pi - scale ss), contracted or not."""
    d = rec["x_prop"].shape[1]
    return 4 * EPS * (abs(rec["logdetQ"]) + 1.8379 * d + rec["lp_scale"] * rec["ss"])


def _white_steps(kind, d, C, step, steps, mus=(True, False)):
    import torch

    eng = make_engine(C)
    views = [View(C, d, pad, off) for _, pad, off in LAYOUTS]
    zview = [View(C, d, 3, 1) for _ in range(steps)]
    acc = torch.zeros(C, dtype=torch.int64, device="cuda")
    prop = torch.zeros(C, dtype=torch.int64, device="cuda")
    logp = eng.empty(C)
    call = eng.mala_step_white if kind == "mala_white" else eng.rw_step_white
    for with_mu in mus:
        case = P.get_case(kind, d, C, step, steps, with_mu)
        L, sl, mu = device_problem(eng, case, with_mu)
        z_packed = [eng.to_device(case.z[t]) for t in range(steps)]
        z_strided = [zview[t].fill(case.z[t]) for t in range(steps)]
        u = eng.to_device(case.u)
        want_acc = np.cumsum(case.accepts, axis=0)
        for ks in KSPLITS:
            eng.set_option("mh_gemm_ksplit", ks)
            eng.mh_invalidate()
            for (name, _, _), v in zip(LAYOUTS, views):
                x = v.fill(case.x0)
                acc.zero_()
                prop.zero_()
                zs = z_strided if ks == 2 else z_packed  # the injected z once with a row stride (d + 3, from an odd element)
                for t in range(steps):
                    tag = (kind, d, C, step, "mu" if with_mu else "no mu", f"ksplit {ks}", name, f"step {t}")
                    rec = case.trace[t]
                    # a = L'(x - mu) formed anew on the first step and on one later step, carried otherwise
                    call(mu, L, sl, step, x, state_is_current=t not in (0, 2), z=zs[t], u=u[t], accept_count=acc, proposal_count=prop,
                         log_p_out=logp)
                    same(v.numpy(), rec["x"], tag)
                    assert np.array_equal(acc.cpu().numpy(), want_acc[t]), tag
                    assert np.array_equal(prop.cpu().numpy(), np.full(C, t + 1)), tag
                    assert np.all(np.abs(logp.cpu().numpy() - rec["logp"]) <= logp_bound(rec)), tag
                assert v.padding_is_nan(), (kind, d, C, ks, name)
        assert all(zv.padding_is_nan() for zv in zview)
    eng.check_status()
    eng.close()


@pytest.mark.parametrize("d,C", P.SHAPES)
def test_mala_step_white_exact(d, C):
    """Four steps at step = 2 (kappa = -1: a' = z - a gains no fraction bits) x k-split 1, 2, 4 x four layouts x with and without
    mu: the state after every step, accepted or rejected, equals the reference bit for bit; counters equal; log p to rounding."""
    _white_steps("mala_white", d, C, 2.0, 4)


@pytest.mark.parametrize("d,C", P.HALF_STEP_SHAPES)
def test_mala_step_white_exact_at_half_kappa(d, C):
    """Three steps at step = 1 (kappa = 1/2: one more fraction bit per acceptance, and -kappa differs from kappa in more than sign)."""
    _white_steps("mala_white", d, C, 1.0, 3, mus=(True,))


@pytest.mark.parametrize("d,C", P.SHAPES)
def test_rw_step_white_exact(d, C):
    _white_steps("rw_white", d, C, 0.5, 4)


@pytest.mark.parametrize("d,C", P.SHAPES)
@pytest.mark.parametrize("kind", ["mala", "rw"])
def test_products_step_exact_on_every_route(kind, d, C):
    """omc_mala_step (Q = step^2 L L', so the drift matrix is -step^2 I exactly) and omc_rw_step through the own GEMM at k-split
    1, 2, 4 and through rocBLAS: every route equals the reference bit for bit, and therefore every other route.  d = 1025 is the
    order from which k_lower_copy, k_lower_transpose and k_set_identity need their grid stride."""
    import torch

    step, steps = (2.0, 4) if kind == "mala" else (0.5, 4)
    case = P.get_case(kind, d, C, step, steps)
    eng = make_engine(C)
    L, sl, mu = device_problem(eng, case)
    Q = eng.to_device(case.prob.Q(step)) if kind == "mala" else None
    views = [View(C, d, pad, off) for _, pad, off in LAYOUTS]
    zview = [View(C, d, 3, 1) for _ in range(steps)]
    z_packed = [eng.to_device(case.z[t]) for t in range(steps)]
    z_strided = [zview[t].fill(case.z[t]) for t in range(steps)]
    u = eng.to_device(case.u)
    acc = torch.zeros(C, dtype=torch.int64, device="cuda")
    prop = torch.zeros(C, dtype=torch.int64, device="cuda")
    want_acc = np.cumsum(case.accepts, axis=0)
    for rocblas, ks in ((0, 1), (0, 2), (0, 4), (1, 4)):
        eng.set_option("mh_use_rocblas", rocblas)
        eng.set_option("mh_gemm_ksplit", ks)
        eng.mh_invalidate()
        zs = z_strided if ks == 2 else z_packed  # the injected z once with a row stride (k_draw_normals reads it)
        for (name, _, _), v in zip(LAYOUTS, views):
            x = v.fill(case.x0)
            acc.zero_()
            prop.zero_()
            for t in range(steps):
                tag = (kind, d, C, "rocBLAS" if rocblas else f"ksplit {ks}", name, f"step {t}")
                if kind == "mala":
                    eng.mala_step(Q, mu, L, sl, step, x, z=zs[t], u=u[t], accept_count=acc, proposal_count=prop)
                else:
                    eng.rw_step(mu, L, sl, step, x, z=zs[t], u=u[t], accept_count=acc, proposal_count=prop)
                same(v.numpy(), case.trace[t]["x"], tag)
                assert np.array_equal(acc.cpu().numpy(), want_acc[t]), tag
                assert np.array_equal(prop.cpu().numpy(), np.full(C, t + 1)), tag
            assert v.padding_is_nan(), (kind, d, C, rocblas, ks, name)
    assert all(zv.padding_is_nan() for zv in zview)
    eng.check_status()
    eng.close()


def _run_white(d, C, steps, ksplits, layouts):
    import torch

    step = 2.0
    case = P.get_case("mala_white", d, C, step, steps)
    want = np.stack([rec["x"] for rec in case.trace])
    want_lp = np.stack([rec["logp"] for rec in case.trace])
    bound = np.stack([logp_bound(rec) for rec in case.trace])
    eng = make_engine(C)
    L, sl, mu = device_problem(eng, case)
    z, u = eng.to_device(case.z), eng.to_device(case.u)
    xs, lps, logp = eng.empty(steps, C, d), eng.empty(steps, C), eng.empty(C)
    acc = torch.zeros(C, dtype=torch.int64, device="cuda")
    prop = torch.zeros(C, dtype=torch.int64, device="cuda")
    for ks in ksplits:
        eng.set_option("mh_gemm_ksplit", ks)
        eng.mh_invalidate()
        for name, pad, off in layouts:
            tag = ("run", d, C, steps, f"ksplit {ks}", name)
            v = View(C, d, pad, off)
            x = v.fill(case.x0)
            xs.fill_(float("nan"))
            lps.fill_(float("nan"))
            acc.zero_()
            prop.zero_()
            eng.mala_run_white(mu, L, sl, step, x, steps, z=z, u=u, draw_index0=5, draw_stride=P.RUN_DRAW_STRIDE, x_store=xs,
                               logp_store=lps, accept_count=acc, proposal_count=prop, log_p_out=logp)
            # every stored state, also those in front of a chain's first acceptance: mu + L^-T L'(x0 - mu) = x0 on exact data
            same(xs.cpu().numpy(), want, tag)
            same(v.numpy(), want[-1], tag + ("state left behind",))
            assert np.array_equal(acc.cpu().numpy(), case.accepts.sum(axis=0)), tag
            assert np.array_equal(prop.cpu().numpy(), np.full(C, steps)), tag
            assert np.all(np.abs(lps.cpu().numpy() - want_lp) <= bound), tag
            assert np.all(np.abs(logp.cpu().numpy() - want_lp[-1]) <= bound[-1]), tag
            # the same run without a store ends in the same state
            x = v.fill(case.x0)
            eng.mala_run_white(mu, L, sl, step, x, steps, z=z, u=u, draw_index0=5, draw_stride=P.RUN_DRAW_STRIDE)
            same(v.numpy(), want[-1], tag + ("no store",))
            # zero steps change nothing
            eng.mala_run_white(mu, L, sl, step, x, 0, state_is_current=True)
            eng.mala_run_white(mu, L, sl, step, x, 0)
            same(v.numpy(), want[-1], tag + ("zero steps",))
            assert v.padding_is_nan(), tag
    eng.check_status()
    eng.close()


@pytest.mark.parametrize("d,C", P.RUN_SMALL_SHAPES)
def test_mala_run_white_exact_small_tile(d, C):
    """Seven steps in one launch (one, two and four pairs of elements per thread), one small-tile product into the store."""
    _run_white(d, C, P.RUN_SMALL_STEPS, KSPLITS, [LAYOUTS[0], LAYOUTS[2]])


@pytest.mark.parametrize("d,C,steps", P.RUN_WIDE_CASES)
def test_mala_run_white_exact_wide_tile(d, C, steps):
    """A block of 32 steps x C >= 4096 columns goes through k_dgemm_64x64 (scalar loads at odd d, 16-byte loads at d = 64 and 130;
    a partial last column tile at C = 131), the remainder of one or two steps through the small tile."""
    assert 32 * C >= 4096
    _run_white(d, C, steps, (4,), [LAYOUTS[0]])


# ---- float data against np.longdouble --------------------------------------------------------------------------------------

def _float_check(kind, d, run=False):
    """Returns the worst ratio of max|x_gpu - x_ld| to the bar 8 max|x_np64 - x_ld| + 4 eps max|x| over chains and steps."""
    import torch

    case = P.get_float_case(kind, d)
    case.check_decisions()
    C, steps, step = case.C, case.steps, case.step
    eng = make_engine(C)
    L = eng.to_device(np.ascontiguousarray(case.L.T))
    sl = eng.to_device(np.array([case.sumlogL]))
    mu = eng.to_device(case.mu)
    Q = eng.to_device(case.Q)
    x = eng.to_device(case.x0)
    u = eng.to_device(case.u)
    acc = torch.zeros(C, dtype=torch.int64, device="cuda")
    got = []
    if run:
        xs = eng.empty(steps, C, d)
        eng.mala_run_white(mu, L, sl, step, x, steps, z=eng.to_device(case.z), u=u, x_store=xs, accept_count=acc)
        got = list(xs.cpu().numpy())
        assert np.array_equal(got[-1], x.cpu().numpy())
    else:
        for t in range(steps):
            z = eng.to_device(case.z[t])
            if kind == "mala":
                eng.mala_step(Q, mu, L, sl, step, x, z=z, u=u[t], accept_count=acc)
            elif kind == "rw":
                eng.rw_step(mu, L, sl, step, x, z=z, u=u[t], accept_count=acc)
            elif kind == "mala_white":
                eng.mala_step_white(mu, L, sl, step, x, state_is_current=t > 0, z=z, u=u[t], accept_count=acc)
            else:
                eng.rw_step_white(mu, L, sl, step, x, state_is_current=t > 0, z=z, u=u[t], accept_count=acc)
            got.append(x.cpu().numpy())
    eng.check_status()
    eng.close()
    assert np.array_equal(acc.cpu().numpy(), np.sum([r["accept"] for r in case.trace_ld], axis=0))  # decisions equal
    worst = 0.0
    before = case.x0
    moved = np.zeros(C, dtype=bool)
    for t in range(steps):
        ok = case.trace_ld[t]["accept"]
        moved |= ok
        xl = case.trace_ld[t]["x"]
        if not run:  # rejected chains keep their x bit for bit (the run's store is written for every chain)
            same(got[t][~ok], before[~ok], (kind, d, f"step {t}", "rejected chains"))
        err = np.abs(got[t].astype(np.longdouble) - xl).max(axis=1).astype(np.float64)
        own = np.abs(case.trace_64[t]["x"].astype(np.longdouble) - xl).max(axis=1).astype(np.float64)
        bar = 8 * own + 4 * EPS * np.abs(got[t]).max(axis=1)
        ratio = float((err / bar)[moved if run else slice(None)].max())
        print(f"{kind} d={d} step {t}: worst max|x_gpu - x_ld| / bar = {ratio:.3f}")
        worst = max(worst, ratio)
        if run:  # in front of a chain's first acceptance the store holds mu + L^-T L'(x0 - mu), not x0 itself: not an accepted state
            err, bar = err[moved], bar[moved]
        assert np.all(err <= bar), (kind, d, t, ratio)
        before = got[t]
    return worst


@pytest.mark.parametrize("d", [137, 500])
@pytest.mark.parametrize("kind", ["mala", "mala_white", "rw", "rw_white"])
def test_step_on_float_data_against_longdouble(kind, d):
    """Random SPD Q, L = chol(Q / step^2) from the host, three steps with injected z and u: decisions as the np.longdouble
    restatement (which keeps every log u a margin of 1e-6 from its odds), rejected chains untouched bit for bit -- an ignored
    column mask shows here and only here --, and every chain's state within 8 times the float64 restatement's own distance from
    np.longdouble plus 4 eps max|x|.  Worst measured ratio of a chain's distance to that bar: 0.24 (mala, d = 500, third step);
    whitened MALA 0.11, both random walks 0.09."""
    _float_check(kind, d)


@pytest.mark.parametrize("d", [137, 500])
def test_run_on_float_data_against_longdouble(d):
    """omc_mala_run_white with a store, same bar for every chain from its first acceptance on (worst measured ratio 0.11)."""
    _float_check("mala_white", d, run=True)
