"""Engine.kde_binned (omc_kde_binned) on made-up bin counts against the restatement of tests/kde_model.py at np.longdouble: flags
array_equal; bandwidth, density and mode within 1e-10 relative, the project's bound for fp64 quantities (densities with an absolute
floor of 1e-300).  No chain is run.  The cases (tests/kde_cases.py): G = 8, 64, 65, 100, 512, 1024 -- below, at and just above one
wave, no multiple of anything, the default, the limit --, 1, 3 and 257 columns, every rule, all four reflections, counts up to
2^40, degenerate columns among good ones, columns on which ISJ falls back.

A condition on the inputs, not a measurement: the root ISJ picks depends on the signs of Phi at the scan points.  Every ISJ and
experimental column used here has |Phi(t_i)| / t_i >= 1e-3 at every scan point up to its bracket and the same bracket at fp64 and
at longdouble, in the restatement alone: rounding (1e-15) cannot move the bracket, and 60 bisection steps then pin the root."""

import numpy as np
import pytest
from kde_cases import cases, reference

pytestmark = pytest.mark.gpu

CASES = cases()


@pytest.fixture(scope="module")
def eng():
    from openmcmc_amd.engine import Engine

    e = Engine(1, seed=1)
    yield e
    e.close()


def run(eng, c, **over):
    import torch

    a = dict(c, **over)
    dev = eng.device
    out = eng.kde_binned(torch.as_tensor(a["counts"], device=dev), eng.to_device(a["lo"]), eng.to_device(a["hi"]), rule=a["rule"],
                         bw=None if a["bw"] is None else eng.to_device(a["bw"]), bw_fct=a["bw_fct"], reflect=a["reflect"])
    return [t.cpu().numpy() for t in out]


def held(got, want, floor=0.0):
    want = np.asarray(want)
    err = np.abs(got.astype(np.longdouble) - want) / np.maximum(np.abs(want), np.longdouble(floor) if floor else np.abs(want))
    return float(np.max(err)) if err.size else 0.0


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_against_the_restatement(eng, i):
    c, want = CASES[i], reference(i)
    good = want["flag"] != 2
    if c["rule"] in ("isj", "experimental"):  # the condition on the inputs
        assert want["margin"][good].min() >= 1e-3, want["margin"]
        assert np.array_equal(want["bracket"], reference(i, np.float64)["bracket"])
    # what is degenerate: under a rule fewer than two draws or non-empty bins; with given bandwidths no draw or no bandwidth
    degenerate = ("zeros", "empty_range", "flat") if c["rule"] == "given" else ("zeros", "empty_range", "one_draw", "one_bin")
    assert np.array_equal(~good, np.array([name in degenerate for name in c["kinds"]]))
    density, bw, mode, flag = run(eng, c)
    assert density.shape == c["counts"].shape and bw.shape == mode.shape == flag.shape == c["counts"].shape[:-1]
    assert flag.dtype == np.int32 and np.array_equal(flag, want["flag"])
    assert np.isnan(bw[~good]).all() and np.isnan(mode[~good]).all() and np.isnan(density[~good]).all()
    errs = held(bw[good], want["bw"][good]), held(density[good], want["density"][good], 1e-300), held(mode[good], want["mode"][good])
    print(c["name"], "bw %.2e density %.2e mode %.2e" % errs, "flags", np.bincount(flag, minlength=3))
    assert max(errs) <= 1e-10, errs


def test_the_cases_cover_what_they_should():
    fallback = big = 0
    for i, c in enumerate(CASES):
        want = reference(i)
        if c["rule"] in ("isj", "experimental"):
            fallback += int((want["flag"] == 1).sum())
        big += int((c["counts"].max(axis=-1) > 2**39).sum())
    assert fallback > 0 and big > 0
    assert {c["G"] for c in CASES} == {8, 64, 65, 100, 512, 1024} and {len(c["kinds"]) for c in CASES} >= {1, 3, 257}
    assert {c["reflect"] for c in CASES} == {(False, False), (True, False), (False, True), (True, True)}
    assert {c["rule"] for c in CASES} == {"given", "scott", "silverman", "isj", "experimental"}


def test_a_column_does_not_depend_on_its_neighbours(eng):
    """every good column of a mixed call, handed over alone, gives the same bits"""
    for name in ("mixed-G65-experimental", "mixed-G1024-given"):
        c = next(x for x in CASES if x["name"] == name)
        whole = run(eng, c)
        for k in range(len(c["kinds"])):
            one = run(eng, c, counts=c["counts"][k:k + 1], lo=c["lo"][k:k + 1], hi=c["hi"][k:k + 1],
                      bw=None if c["bw"] is None else c["bw"][k:k + 1])
            assert all(np.array_equal(w[k:k + 1], o, equal_nan=True) for w, o in zip(whole, one)), (name, k)


def test_repeated_calls_are_bit_equal(eng):
    for name in ("mixed-G64-isj", "mixed-G512-experimental", "many-isj", "reflect-11-silverman"):
        c = next(x for x in CASES if x["name"] == name)
        first = run(eng, c)
        for _ in range(2):
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, run(eng, c)))


def test_one_wave_and_four_waves_add_in_the_same_order(eng):
    """G = 128 runs on one wave and G = 129 on four.  A column of 128 bins and the same counts with an empty 129th bin, the grid
    longer by one bin width, share delta and every bin centre; the sums over the bins meet the same values in the same blocks of 64
    (the extra block adds zeros), so a given bandwidth must give the same density bit for bit."""
    from openmcmc_amd.engine import Engine

    assert Engine.kde_layout(128)[0] == 64 and Engine.kde_layout(129)[0] == 256
    rng = np.random.default_rng(4)
    c128 = np.histogram(rng.standard_normal(5000), 128, (-4.0, 4.0))[0].astype(np.int64)[None, :]
    c129 = np.concatenate([c128, np.zeros((1, 1), dtype=np.int64)], axis=1)
    base = dict(rule="given", bw=np.array([0.25]), bw_fct=1.0, reflect=(True, False), lo=np.array([-4.0]))
    d128 = run(eng, dict(base, counts=c128, hi=np.array([4.0])))
    d129 = run(eng, dict(base, counts=c129, hi=np.array([4.0 + 8.0 / 128])))
    assert 8.0 / 128 * 129 - 4.0 == 4.0 + 8.0 / 128  # (dyadic: both grids have exactly the same delta)
    assert np.array_equal(d128[0][0], d129[0][0, :128]) and d128[2][0] == d129[2][0]


def test_invalid_arguments_leave_the_outputs_untouched(eng):
    import torch

    from openmcmc_amd import _abi

    G, n = 16, 3
    dev = eng.device
    counts = torch.as_tensor(np.arange(n * G, dtype=np.int64).reshape(n, G), device=dev)
    negative = counts.clone()
    negative[1, 5] = -1
    lo, hi, h = eng.to_device(np.zeros(n)), eng.to_device(np.ones(n)), eng.to_device(np.full(n, 0.1))
    density, bw, mode = eng.full((n, G), -7.0), eng.full((n,), -7.0), eng.full((n,), -7.0)
    flag = torch.full((n,), -7, dtype=torch.int32, device=dev)

    def call(cnt=counts, G=G, rule=1, bw_in=None, bw_fct=1.0, reflect=0, n_cols=n):
        st = _abi.lib.omc_kde_binned(eng._ctx, n_cols, G, cnt.data_ptr(), lo.data_ptr(), hi.data_ptr(), rule,
                                     None if bw_in is None else bw_in.data_ptr(), bw_fct, reflect, density.data_ptr(), bw.data_ptr(),
                                     flag.data_ptr(), mode.data_ptr())
        torch.cuda.synchronize()
        return st

    assert call(G=7) == _abi.INVALID_ARG and call(G=1025) == _abi.INVALID_ARG
    assert call(rule=5) == _abi.INVALID_ARG and call(rule=-1) == _abi.INVALID_ARG
    assert call(rule=0) == _abi.INVALID_ARG  # no bandwidths
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(bw_fct=bad) == _abi.INVALID_ARG
    assert call(cnt=negative) == _abi.INVALID_ARG and call(cnt=negative, rule=0, bw_in=h) == _abi.INVALID_ARG
    assert call(n_cols=0) == _abi.INVALID_ARG and call(reflect=4) == _abi.INVALID_ARG
    for t in (density, bw, mode, flag):
        assert np.all(t.cpu().numpy() == -7)
    assert call(rule=0, bw_in=h) == _abi.OK and np.all(flag.cpu().numpy() == 0) and np.all(bw.cpu().numpy() == 0.1)
    # any output may be NULL
    st = _abi.lib.omc_kde_binned(eng._ctx, n, G, counts.data_ptr(), lo.data_ptr(), hi.data_ptr(), 2, None, 1.0, 0, None, bw.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert st == _abi.OK and np.all(bw.cpu().numpy() > 0) and np.all(bw.cpu().numpy() != 0.1)
    with pytest.raises(ValueError):
        eng.kde_binned(counts, lo, hi, rule="no such rule")
    with pytest.raises(ValueError):
        eng.kde_binned(counts[:, :7], lo, hi)
    with pytest.raises(ValueError):
        eng.kde_binned(counts, lo[:2], hi)
    with pytest.raises(ValueError):
        eng.kde_binned(counts, lo, hi, rule="given")
