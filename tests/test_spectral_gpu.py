"""The spectral dense draw (omc_dense_spectral_sample, csrc/omc_spectral.hip) held path-wise, element by element, to the host
evaluation of x_c = V (V'b_c / d_c + z_c / sqrt(d_c)) of tests/spectral_problem.py, at the sizes where its kernels change path.

The rest of the suite checks this draw through its mean, its log-determinant and (x - m)'Q(x - m) = |z|^2, which no permutation
of z changes, and compares the in-kernel draw with the same kernel fed omc_fill_normal: a swapped pair of normals, a wrong
stride of z, V where V' is wanted inside an eigenspace or a scale off on the same lanes in both runs pass all of that.

Shapes (p, C) and the edge each one is:
  (1, 1)     k_spectral_scale: one half pair of sites; one element in every tile
  (2, 5)     one full pair; the even (16-byte) instantiation of the products at its smallest
  (3, 17)    an odd last pair; chains 16 + 1: a second chain tile of the products with one column
  (31, 5)    one transpose tile, partly empty; one slab of the contraction, partly empty
  (32, 16)   the transpose tile, the slab and the chain tile exactly full
  (33, 17)   a second transpose tile (row and column) and a second slab with one element; chain tile 17
  (63, 5)    the product's row tile of 64 one short
  (64, 65)   the row tile exactly full; chains 64 + 1: a fifth chain tile, and the second group of 64 of a grid over chains
  (65, 17)   a second row tile with one row; three slabs over the four split groups (one group idle)
  (130, 5)   five slabs over four split groups (two slabs a group, the last group idle, the third a partial one)
  (513, 3)   k_spectral_scale strides: 257 pairs over 256 threads; odd, so the 8-byte path of the products
  (514, 3)   the same with the last pair full, and the even 16-byte path

(a) exact data, bits, four ways; (b) layouts of terms, bits; (c) random orthogonal V against np.longdouble; (d) the in-kernel
normals; (e) a failed chain; (f) refusals; (g) omc_dense_spectral_prepare's layout contract.
Bars of (c), (d), (e), (g): tests/test_dense_gpu.py's own, 1e-11 max|ref| for x and the mean, 1e-12 relative for the
log-determinant."""

import ctypes

import numpy as np
import pytest

import spectral_problem as sp

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0123_4567_89AB
DRAW = (5 << 32) | 7         # a draw index with a non-zero high word
SENTINEL = -7.25             # what a call must leave alone (an exact binary fraction no case here produces)
X_BAR, LOGDET_BAR = 1e-11, 1e-12
INPUT_BAR = 1e-13            # float64 NumPy against np.longdouble on the same inputs: a condition on the inputs of (c)
RANDOM_SHAPES = [(3, 17), (33, 17), (65, 17), (130, 5), (513, 3)]


def make_engine(C, opts=()):
    from openmcmc_amd.engine import Engine

    eng = Engine(C, seed=SEED)
    for name, value in dict(opts).items():
        eng.set_option(name, value)
    return eng


def host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def padded(eng, a, pad=3):
    """(view of the first n columns, the whole tensor): rows of stride n + pad, the padding filled with SENTINEL."""
    full = eng.full((a.shape[0], a.shape[1] + pad), SENTINEL)
    full[:, : a.shape[1]] = eng.to_device(a)
    return full[:, : a.shape[1]], full


def padding_untouched(full, n):
    return bool((full[:, n:] == SENTINEL).all().item())


def device_terms(eng, case):
    """The case's terms as the library takes them.  The matrix term carries M = V diag(ev) V' itself."""
    E = case.V.T
    out = []
    for t in case.terms:
        d = {"mat": eng.to_device((E * case.ev) @ E.T) if t["kind"] == "M" else None}
        if t["rhs"] is not None:
            d["rhs"] = eng.to_device(t["rhs"])
        if t["scale"] is not None:
            d["scale"] = eng.to_device(t["scale"])
        out.append(d)
    return out


def draw(eng, case, pad=False, z="case", mean=True, logdet=True, draw_index=0):
    """One call.  z: "case" injects case.z, None lets the kernel draw, a tensor is injected as it is.  pad: x, z, rhs_chain and
    mean_out are row-padded views (stride p + 3), and the padding and the two inputs are checked afterwards."""
    p, C = case.p, case.C
    fulls = {}

    def arg(name, a):
        if a is None:
            return None
        if not pad:
            return eng.to_device(a)
        view, fulls[name] = padded(eng, a)
        return view

    sent = np.full((C, p), SENTINEL)
    x = arg("x", sent)
    m = arg("mean", sent) if mean else None
    ld = eng.full((C,), SENTINEL) if logdet else None
    zt = arg("z", case.z) if isinstance(z, str) else z
    rc = arg("rhs_chain", case.rhs_chain)
    eng.dense_spectral_sample(p, device_terms(eng, case), case.k_mat, eng.to_device(case.V), eng.to_device(case.ev), x, z=zt,
                              rhs_chain=rc, draw_index=draw_index, mean_out=m, logdet_out=ld)
    out = {"x": host(x), "mean": host(m) if mean else None, "logdet": host(ld) if logdet else None}
    for name, full in fulls.items():
        assert padding_untouched(full, p), name
    if pad:
        assert np.array_equal(host(zt), case.z)
        assert case.rhs_chain is None or np.array_equal(host(rc), case.rhs_chain)
    return out


def assert_bits(got, case, what):
    x, mean, logdet = sp.reference_all(case, np.float64)
    bad = np.argwhere(got["x"] != x)
    assert bad.size == 0, (what, "x", len(bad), bad[:5].tolist())
    bad = np.argwhere(got["mean"] != mean)
    assert bad.size == 0, (what, "mean", len(bad), bad[:5].tolist())
    err = np.abs(got["logdet"] - logdet)
    assert np.all(err <= LOGDET_BAR * np.abs(logdet)), (what, "logdet", float(np.max(err / np.maximum(np.abs(logdet), 1e-300))))


def assert_close(got, case, what, chains=None):
    """(c)'s bars against the np.longdouble reference; first the condition on the inputs."""
    chains = list(range(case.C)) if chains is None else chains
    ref, f64 = ([np.array(v) for v in zip(*(sp.reference(case, c, dt) for c in chains))] for dt in (np.longdouble, np.float64))
    figures = {}
    for key, r, h, bar in (("x", ref[0], f64[0], X_BAR), ("mean", ref[1], f64[1], X_BAR)):
        g = got[key][chains]
        scale = float(np.abs(r).max())
        assert float(np.abs(h - r).max()) <= INPUT_BAR * scale, (what, key, "the inputs are too ill-conditioned for the bar")
        figures[key] = float(np.abs(g - r).max()) / scale
        assert figures[key] < bar, (what, key, figures[key])
    r, g = ref[2], got["logdet"][chains]
    figures["logdet"] = float(np.max(np.abs(g - r) / np.abs(r)))
    assert figures["logdet"] < LOGDET_BAR, (what, "logdet", figures["logdet"])
    print(what, {k: f"{v:.2e}" for k, v in figures.items()})
    return figures


# -------------------------------------------------------------------------------------------------------- (a) exact, bits
@pytest.mark.parametrize("p,C", sp.GPU_SHAPES)
def test_exact_draw_is_the_reference_bit_for_bit(p, C):
    """Four ways, the same bits each time: the default route; the products through the library GEMM (on this data any correct
    GEMM is exact); mh_gemm_ksplit 1 (the option tunes the Metropolis-Hastings steps and must not move this draw); and x, z,
    rhs_chain, mean_out as row-padded views of stride p + 3 -- odd for even p, so the other instantiation of the products --
    whose padding and inputs are left alone."""
    case = sp.get_exact(p, C)
    eng = make_engine(C)
    runs = {"default": draw(eng, case)}
    eng.set_option("spectral_use_rocblas", 1)
    runs["rocblas"] = draw(eng, case)
    eng.set_option("spectral_use_rocblas", 0)
    eng.set_option("mh_gemm_ksplit", 1)
    runs["ksplit1"] = draw(eng, case)
    eng.set_option("mh_gemm_ksplit", 4)
    runs["padded"] = draw(eng, case, pad=True)
    eng.check_status()
    eng.close()
    for what, got in runs.items():
        assert_bits(got, case, (p, C, what))
    for what, got in runs.items():
        assert np.array_equal(got["x"], runs["default"]["x"]) and np.array_equal(got["mean"], runs["default"]["mean"]), what


# ------------------------------------------------------------------------------------------------------ (b) term layouts
@pytest.mark.parametrize("name", list(sp.LAYOUTS))
def test_term_layouts_bit_for_bit(name):
    """k_mat at each position of four terms; one, two, three identity terms; an absent scale (counts 1) on an identity and on
    the matrix term; identity terms with and without a rhs; rhs_chain absent (an absent rhs counts 0)."""
    p, C = sp.LAYOUT_SHAPE
    case = sp.get_exact(p, C, name=name)
    eng = make_engine(C)
    got = draw(eng, case)
    eng.check_status()
    eng.close()
    assert_bits(got, case, name)


def test_x_does_not_depend_on_the_outputs_requested():
    p, C = sp.LAYOUT_SHAPE
    case = sp.get_exact(p, C)
    eng = make_engine(C)
    full = draw(eng, case)
    for mean, logdet in ((False, False), (True, False), (False, True)):
        got = draw(eng, case, mean=mean, logdet=logdet)
        assert np.array_equal(got["x"], full["x"]), (mean, logdet)
        assert not mean or np.array_equal(got["mean"], full["mean"])
        assert not logdet or np.array_equal(got["logdet"], full["logdet"])
    eng.check_status()
    eng.close()
    assert_bits(full, case, "all outputs")


# -------------------------------------------------------------------------------------------- (c) random orthogonal V
@pytest.mark.parametrize("p,C", RANDOM_SHAPES)
def test_random_orthogonal_draw_against_longdouble(p, C):
    case = sp.get_random(p, C)
    eng = make_engine(C)
    got = draw(eng, case)
    eng.check_status()
    eng.close()
    assert_close(got, case, ("random", p, C))


# ------------------------------------------------------------------------------------------------ (d) in-kernel normals
@pytest.mark.parametrize("p,C", [(33, 17), (513, 3)])
def test_in_kernel_normals_are_the_stream_and_the_host_formula(p, C):
    """z = None against z = omc_fill_normal of the same seed and draw index: bits.  The injected run against the reference fed
    the z read back: (c)'s bars.  (tests/test_draw_streams_gpu.py does the first half at p = 70.)"""
    base = sp.get_random(p, C)
    eng = make_engine(C)
    z = eng.fill_normal(p, DRAW)
    drawn = draw(eng, base, z=None, draw_index=DRAW)
    injected = draw(eng, base, z=z, draw_index=DRAW)
    other = draw(eng, base, z=None, draw_index=DRAW + 1)
    zh = host(z)
    eng.check_status()
    eng.close()
    for key in ("x", "mean", "logdet"):
        assert np.array_equal(drawn[key], injected[key]), key
    assert not np.array_equal(other["x"], drawn["x"]) and np.array_equal(other["mean"], drawn["mean"])
    assert np.all(np.isfinite(zh)) and abs(zh.std() - 1.0) < 0.2 and len(np.unique(zh)) == zh.size
    assert_close(injected, base.replace(z=zh), ("in-kernel", p, C))


# ------------------------------------------------------------------------------------------------------ (e) a failed chain
def test_failed_chain_is_named_and_the_others_are_right():
    """One chain of five has a negative scale on the matrix term, so that d <= 0 at some of its sites (and > 0 at others: the
    latch must not depend on every site failing)."""
    p, C, bad = 33, 5, 3
    base = sp.get_random(p, C)
    terms = [dict(t) for t in base.terms]
    s = terms[base.k_mat]["scale"].copy()
    s[bad] = -0.5
    terms[base.k_mat]["scale"] = s
    case = base.replace(terms=terms)
    a = sum(t["scale"][bad] for k, t in enumerate(terms) if k != case.k_mat)
    assert np.any(a + s[bad] * case.ev <= 0) and np.any(a + s[bad] * case.ev > 0)
    eng = make_engine(C)
    got = draw(eng, case)
    with pytest.raises(np.linalg.LinAlgError, match=rf"chain {bad}\b"):
        eng.check_status()
    eng.check_status()  # the latch is cleared by reading it
    eng.close()
    assert_close(got, case, "failed chain", chains=[c for c in range(C) if c != bad])


# ------------------------------------------------------------------------------------------------------------ (f) refusals
def test_refusals_leave_the_outputs_alone():
    from openmcmc_amd import _abi

    p, C = 12, 3
    case = sp.get_random(p, C)
    eng = make_engine(C)
    dev = eng.to_device
    good = device_terms(eng, case)   # identity, matrix, identity
    ident, M = good[0], good[1]
    V, ev, z, rc = dev(case.V), dev(case.ev), dev(case.z), dev(case.rhs_chain)

    def refused(call):
        x, mean = eng.full((C, p), SENTINEL), eng.full((C, p), SENTINEL)
        with pytest.raises(ValueError):
            call(x, mean)
        eng.check_status()
        assert bool((x == SENTINEL).all().item()) and bool((mean == SENTINEL).all().item())

    def through_wrapper(terms, k_mat):
        return lambda x, mean: eng.dense_spectral_sample(p, terms, k_mat, V, ev, x, z=z, rhs_chain=rc, mean_out=mean)

    refused(through_wrapper([ident, M, dict(M)], 1))   # two terms with a matrix
    refused(through_wrapper(good, 0))                  # k_mat at an identity term
    refused(through_wrapper(good, 2))
    refused(through_wrapper(good, -1))                 # k_mat out of range
    refused(through_wrapper(good, 3))

    T = eng.dense_terms(good, p)

    def through_abi(terms=T, ld_rhs=p, ld_z=p, ld_x=p, ld_mean=p):
        def call(x, mean):
            vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
            _abi.check(_abi.lib.omc_dense_spectral_sample(eng._ctx, p, ctypes.byref(terms), 1, vp(V), vp(ev), vp(rc), ld_rhs, vp(z), ld_z,
                                                          0, vp(x), ld_x, vp(mean), ld_mean, None))
        return call

    with_diag = eng.dense_terms(good, p)
    diag = eng.full((C, p), 1.0)
    with_diag.diag_chain = diag.data_ptr()             # a per-chain diagonal: the route has none
    refused(through_abi(terms=with_diag))
    for name in ("ld_x", "ld_rhs", "ld_z", "ld_mean"):  # a row stride below p
        refused(through_abi(**{name: p - 1}))
    # the same call with nothing wrong is taken: the refusals above are the arguments', not the harness's
    x, mean = eng.full((C, p), SENTINEL), eng.full((C, p), SENTINEL)
    through_abi()(x, mean)
    eng.check_status()
    got = {"x": host(x), "mean": host(mean)}
    eng.close()
    ref = sp.reference_all(case)
    for key, r in zip(("x", "mean"), ref):
        assert float(np.abs(got[key] - r).max()) < X_BAR * float(np.abs(r).max()), key


# ----------------------------------------------------------------------------------------- (g) omc_dense_spectral_prepare
def random_spd(rng, p):
    A = rng.standard_normal((p, 2 * p))
    M = A @ A.T / (2 * p) + 0.5 * np.eye(p)
    return 0.5 * (M + M.T)


def repeated_spd(rng, p):
    """V diag(ev) V' with a three-fold eigenvalue in the middle of the spectrum."""
    V, _ = np.linalg.qr(rng.standard_normal((p, p)))
    ev = np.sort(rng.uniform(0.5, 4.0, size=p))
    ev[p // 2 - 1: p // 2 + 2] = ev[p // 2]
    M = (V * ev) @ V.T
    return 0.5 * (M + M.T)


def eig_residuals(M, E, ev):
    """(eigenvalues against np.linalg.eigvalsh, |E'E - I|_2, |E diag(ev) E' - M|_2) of eigenvectors in columns."""
    p = M.shape[0]
    return (float(np.abs(ev - np.linalg.eigvalsh(M)).max()), float(np.linalg.norm(E.T @ E - np.eye(p), 2)),
            float(np.linalg.norm((E * ev) @ E.T - M, 2)))


@pytest.mark.parametrize("p,kind", [(1, "random"), (2, "random"), (33, "random"), (33, "repeated"), (130, "random")])
def test_prepare_meets_the_layout_contract(p, kind):
    """V comes back with eigenvector j in memory row j and ev ascending, as the sampler and omc_dense_spectral_sample read them.
    Each residual of the device's pair is at most 10 times that of np.linalg.eigh on the same M (two algorithms of the same
    backward-stable class), with a floor of p 2^-52 |M|_2 (for the orthogonality p 2^-52 min(1, |M|_2): |I|_2 = 1) so that a
    lucky NumPy result cannot fail the device.  Then the draw with the device's own V, ev against the reference built from the
    values read back: path-wise, so neither the signs nor the basis of an eigenspace matter.

    Measured on an MI355X (eigenvalues, orthogonality, reconstruction), device / NumPy:
      p = 1              0 / 0,              0 / 0,              0 / 0
      p = 2              1.1e-16 / 0,        2.3e-16 / 2.3e-16,  4.5e-16 / 4.5e-16   (floors 5.4e-16, 4.4e-16, 5.4e-16)
      p = 33             3.6e-15 / 4.0e-15,  2.3e-15 / 2.7e-15,  4.5e-15 / 7.7e-15
      p = 33, repeated   2.7e-15 / 3.1e-15,  2.1e-15 / 2.8e-15,  1.1e-14 / 9.4e-15
      p = 130            6.2e-15 / 6.2e-15,  4.2e-15 / 4.0e-15,  9.7e-15 / 8.8e-15
    and the draw from the device's own V, ev: at most 3.4e-16 (x), 3.8e-16 (mean), 1.5e-16 (log-determinant) of the bars' scale.
    """
    C = 5
    rng = np.random.default_rng([p, 777])
    M = random_spd(rng, p) if kind == "random" else repeated_spd(rng, p)
    eng = make_engine(C)
    Vd, evd = eng.dense_spectral_prepare(eng.to_device(M))
    eng.check_status()
    V, ev = host(Vd), host(evd)
    base = sp.random_case(p, C, 1)
    case = base.replace(V=V, ev=ev)
    got = draw(eng, case)
    eng.check_status()
    eng.close()

    assert V.shape == (p, p) and ev.shape == (p,) and np.all(np.diff(ev) >= 0)
    norm = float(np.linalg.norm(M, 2))
    evn, En = np.linalg.eigh(M)
    dev_res, np_res = eig_residuals(M, V.T, ev), eig_residuals(M, En, evn)
    floors = (p * 2.0 ** -52 * norm, p * 2.0 ** -52 * min(1.0, norm), p * 2.0 ** -52 * norm)
    print(("prepare", p, kind), "device", [f"{r:.2e}" for r in dev_res], "numpy", [f"{r:.2e}" for r in np_res],
          "floor", [f"{f:.2e}" for f in floors])
    for what, d, n, f in zip(("eigenvalues", "orthogonality", "reconstruction"), dev_res, np_res, floors):
        assert d <= max(10.0 * n, f), (what, d, n, f)
    if kind == "repeated":  # the three-fold eigenvalue is there, to rounding
        assert ev[p // 2 + 1] - ev[p // 2 - 1] < 100 * p * 2.0 ** -52 * norm
    assert_close(got, case, ("prepare", p, kind))
