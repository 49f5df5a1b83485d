"""Engine.kde2d_binned (omc_kde2d_binned) on made-up 2-D bin counts against the restatement of tests/kde2d_model.py at np.longdouble:
flags and level_pos array_equal; level array_equal to the kernel's own density sorted, at level_pos; the mode array_equal to the
centre of the restatement's cell (its two largest densities are further than 1e-9 apart); kernel covariance and density within 1e-10
relative, the project's bound for fp64 quantities (densities with an absolute floor of 1e-300: below it fp64 has no full
precision).  No chain is run.  The cases and what they cover: tests/kde2d_cases.py; that every level_pos is out of rounding's reach
is asserted on the host, for every case (tests/test_kde2d_model_host.py)."""

import numpy as np
import pytest
from kde2d_cases import cases, reference

pytestmark = pytest.mark.gpu

CASES = cases()
NAMES = ("density", "bw", "mode", "level", "level_pos", "flag")


@pytest.fixture(scope="module")
def eng():
    from openmcmc_amd.engine import Engine

    e = Engine(1, seed=1)
    yield e
    e.close()


def run(eng, c, **over):
    import torch

    a = dict(c, **over)
    out = eng.kde2d_binned(torch.as_tensor(a["counts"], device=eng.device), a["lo_x"], a["hi_x"], a["lo_y"], a["hi_y"], rule=a["rule"],
                           bw=a["bw"], bw_fct=a["bw_fct"], probs=a["probs"])
    return dict(zip(NAMES, (t.cpu().numpy() for t in out)))


def held(got, want, floor=0.0):
    want = np.asarray(want)
    err = np.abs(got.astype(np.longdouble) - want) / np.maximum(np.abs(want), np.longdouble(floor) if floor else np.abs(want))
    return float(np.max(err)) if err.size else 0.0


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in NAMES)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_against_the_restatement(eng, i):
    c, want = CASES[i], reference(i)
    good = want["flag"] == 0
    got = run(eng, c)
    n, nx, ny = c["counts"].shape
    assert got["density"].shape == (n, nx, ny) and got["bw"].shape == (n, 3) and got["mode"].shape == (n, 2)
    assert got["level"].shape == got["level_pos"].shape == (n, len(c["probs"])) and got["level_pos"].dtype == np.int64
    assert got["flag"].dtype == np.int32 and np.array_equal(got["flag"], want["flag"])
    assert np.array_equal(got["level_pos"], want["level_pos"])
    for k in ("density", "bw", "mode", "level"):
        assert np.isnan(got[k][~good]).all(), k
    assert want["gap"][good].min() > 1e-9
    assert np.array_equal(got["mode"][good], want["mode"][good])
    for g in np.nonzero(good)[0]:  # the level is the kernel's own density at that position of its own descending order
        D = np.sort(got["density"][g].ravel())[::-1]
        assert np.array_equal(got["level"][g], D[got["level_pos"][g]]), g
    errs = held(got["bw"][good], want["bw"][good]), held(got["density"][good], want["density"][good], 1e-300)
    print(c["name"], "bw %.2e density %.2e" % errs, "flags", np.bincount(got["flag"], minlength=3))
    assert max(errs) <= 1e-10, errs


def test_a_grid_does_not_depend_on_its_neighbours(eng):
    """every grid of a batch, handed over alone, gives the same bits: the degenerate grid between two good ones changes nothing"""
    for name, picks in (("24x20-dense-scott", (0, 1, 2)), ("24x20-given-negative", (0, 1, 2)), ("many-8x8", (0, 5, 6, 7, 511, 1024))):
        c = next(x for x in CASES if x["name"] == name)
        whole = run(eng, c)
        for g in picks + ((len(c["counts"]) - 1,) if name == "many-8x8" else ()):
            one = run(eng, c, counts=c["counts"][g:g + 1], **{k: c[k][g:g + 1] for k in ("lo_x", "hi_x", "lo_y", "hi_y")},
                      bw=None if c["bw"] is None else c["bw"][g:g + 1])
            assert all(np.array_equal(whole[k][g:g + 1], one[k], equal_nan=True) for k in NAMES), (name, g)


def test_chunks_of_grids_give_the_bits_of_one_chunk():
    """option "rank_chunk" = grids per chunk of the workspace (0: what fits the budget, here all of them): several chunks, an uneven
    last one and one grid per chunk give the bits of the single chunk -- with the densities in the caller's array, and with
    density_out NULL, when they live in the chunk's workspace beside the sort keys"""
    import torch

    from openmcmc_amd import _abi
    from openmcmc_amd.engine import Engine

    for name, chunks in (("24x20-dense-scott", (0, 1, 2)), ("many-8x8", (0, 700, 1024))):
        c = next(x for x in CASES if x["name"] == name)
        n, n_probs = len(c["counts"]), len(c["probs"])
        first = None
        for chunk in chunks:
            e = Engine(1, seed=1)
            e.set_option("rank_chunk", chunk)
            got = run(e, c)
            # the same call without density_out
            counts = torch.as_tensor(c["counts"], device=e.device)
            ends = [e.to_device(c[k]) for k in ("lo_x", "hi_x", "lo_y", "hi_y")]
            probs = e.to_device(np.array(c["probs"]))
            mode, level = e.full((n, 2), -7.0), e.full((n, n_probs), -7.0)
            pos = torch.full((n, n_probs), -7, dtype=torch.int64, device=e.device)
            st = _abi.lib.omc_kde2d_binned(e._ctx, n, *c["counts"].shape[1:], counts.data_ptr(), *(v.data_ptr() for v in ends), 1, None,
                                           c["bw_fct"], n_probs, probs.data_ptr(), None, None, mode.data_ptr(), level.data_ptr(),
                                           pos.data_ptr(), None)
            torch.cuda.synchronize()
            assert st == _abi.OK
            bare = dict(mode=mode.cpu().numpy(), level=level.cpu().numpy(), level_pos=pos.cpu().numpy())
            e.close()
            assert all(np.array_equal(bare[k], got[k], equal_nan=True) for k in bare), (name, chunk)
            if first is None:
                first = got
            assert same(first, got), (name, chunk)


def test_repeated_calls_are_bit_equal(eng):
    for name in ("256x256-scott", "24x20-dense-scott", "many-8x8"):
        c = next(x for x in CASES if x["name"] == name)
        first = run(eng, c)
        for _ in range(2):
            assert same(first, run(eng, c))


def test_a_transposed_grid_gives_the_transposed_answer_and_a_flipped_one_does_not(eng):
    c = next(x for x in CASES if x["name"] == "24x20-dense-scott")
    got = run(eng, c)
    t = run(eng, c, counts=np.ascontiguousarray(c["counts"].transpose(0, 2, 1)), lo_x=c["lo_y"], hi_x=c["hi_y"], lo_y=c["lo_x"], hi_y=c["hi_x"])
    assert np.array_equal(t["flag"], got["flag"])
    for g in (0, 2):
        assert held(t["density"][g].T, got["density"][g].astype(np.longdouble)) <= 1e-10
        assert np.array_equal(t["mode"][g][::-1], got["mode"][g]) and held(t["bw"][g][::-1], got["bw"][g].astype(np.longdouble)) <= 1e-10
        assert got["bw"][g, 1] * (1 if g == 0 else -1) > 0  # the first grid's correlation is positive, the last one's negative
    f = run(eng, c, counts=np.ascontiguousarray(c["counts"][:, :, ::-1]))
    assert held(f["bw"][0, 1:2], -got["bw"][0, 1:2].astype(np.longdouble)) <= 1e-10  # the flipped grid: the other sign
    assert not np.allclose(f["density"][0], got["density"][0], rtol=1e-3)


def test_null_outputs_and_invalid_arguments(eng):
    import itertools

    import torch

    from openmcmc_amd import _abi

    dev = eng.device
    c = next(x for x in CASES if x["name"] == "24x20-dense-scott")
    n, nx, ny = c["counts"].shape
    n_probs = len(c["probs"])
    counts = torch.as_tensor(c["counts"], device=dev)
    negative = counts.clone()
    negative[2, 3, 4] = -1
    ends = [eng.to_device(c[k]) for k in ("lo_x", "hi_x", "lo_y", "hi_y")]
    probs = eng.to_device(np.array(c["probs"]))
    bad_probs = [eng.to_device(np.array(p)) for p in ((0.3, 0.0, 0.9, 0.99), (0.3, 0.5, 1.0, 0.99), (0.3, 0.5, 0.9, float("nan")))]
    H = eng.to_device(np.tile([0.3, 0.05, 0.02], (n, 1)))
    want = run(eng, c)

    def fresh():
        f64 = {k: eng.full(want[k].shape, -7.0) for k in ("density", "bw", "mode", "level")}
        return dict(f64, level_pos=torch.full(want["level_pos"].shape, -7, dtype=torch.int64, device=dev),
                    flag=torch.full((n,), -7, dtype=torch.int32, device=dev))

    def call(out, keep=NAMES, cnt=counts, nx=nx, ny=ny, rule=1, bw_in=None, bw_fct=c["bw_fct"], n_probs=n_probs, probs=probs, n_grids=n):
        p = {k: (out[k].data_ptr() if k in keep else None) for k in NAMES}
        st = _abi.lib.omc_kde2d_binned(eng._ctx, n_grids, nx, ny, cnt.data_ptr(), *(e.data_ptr() for e in ends), rule,
                                       None if bw_in is None else bw_in.data_ptr(), bw_fct, n_probs,
                                       None if probs is None else probs.data_ptr(), p["density"], p["bw"], p["mode"], p["level"],
                                       p["level_pos"], p["flag"])
        torch.cuda.synchronize()
        return st

    out = fresh()
    assert call(out, nx=7) == _abi.INVALID_ARG and call(out, ny=257) == _abi.INVALID_ARG and call(out, nx=257) == _abi.INVALID_ARG
    assert call(out, rule=2) == _abi.INVALID_ARG and call(out, rule=-1) == _abi.INVALID_ARG
    assert call(out, rule=0) == _abi.INVALID_ARG  # no covariance
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(out, bw_fct=bad) == _abi.INVALID_ARG
    assert call(out, cnt=negative) == _abi.INVALID_ARG and call(out, cnt=negative, rule=0, bw_in=H) == _abi.INVALID_ARG
    assert call(out, n_grids=0) == _abi.INVALID_ARG and call(out, n_probs=17) == _abi.INVALID_ARG and call(out, n_probs=-1) == _abi.INVALID_ARG
    assert call(out, probs=None) == _abi.INVALID_ARG
    for p in bad_probs:
        assert call(out, probs=p) == _abi.INVALID_ARG
    for k in NAMES:
        assert np.all(out[k].cpu().numpy() == -7), k
    # every combination of NULL outputs: what is asked for comes out with the bits of the full call, the rest stays untouched
    for r in range(len(NAMES) + 1):
        for keep in itertools.combinations(NAMES, r):
            out = fresh()
            assert call(out, keep=keep) == _abi.OK, keep
            for k in NAMES:
                got = out[k].cpu().numpy()
                assert np.array_equal(got, want[k], equal_nan=True) if k in keep else np.all(got == -7), (keep, k)
    out = fresh()
    assert call(out, n_probs=0, probs=None) == _abi.OK  # no levels
    assert np.all(out["level"].cpu().numpy() == -7) and np.array_equal(out["density"].cpu().numpy(), want["density"], equal_nan=True)
    counts_t = counts
    with pytest.raises(ValueError):
        eng.kde2d_binned(counts_t, *ends, rule="no such rule")
    with pytest.raises(ValueError):
        eng.kde2d_binned(counts_t[:, :7], *ends)
    with pytest.raises(ValueError):
        eng.kde2d_binned(counts_t, ends[0][:2], *ends[1:])
    with pytest.raises(ValueError):
        eng.kde2d_binned(counts_t, *ends, rule="given")
    with pytest.raises(ValueError):
        eng.kde2d_binned(counts_t, *ends, probs=(0.5, 1.0))
    with pytest.raises(ValueError):
        eng.kde2d_binned(counts_t, *ends, rule="given", bw=np.ones((n, 2)))
    a, b = eng.kde2d_binned(counts_t, *ends, rule="silverman", bw_fct=c["bw_fct"]), eng.kde2d_binned(counts_t, *ends, bw_fct=c["bw_fct"])
    assert all(np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True) for x, y in zip(a, b)) and a[3].shape == (n, 0)
