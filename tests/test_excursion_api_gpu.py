"""MCMC.excursion and MCMC.contour_map on a small stored GMRF smoother run (6 chains) against the numpy restatement of
tests/excursion_model.py applied to MCMC.collect()'s host copy: every result is an integer or one IEEE division of integers, so
every comparison is np.array_equal.  Also: a sequence of levels against the calls one by one, offset and order=, chains split over
two engines with a common order, ties and NaN draws on a planted store, and the errors."""

import numpy as np
import pytest
from excursion_model import KINDS, contour_map, excursion

pytestmark = pytest.mark.gpu

KEYS = ("marginal", "F", "set", "order", "counts")


def store_of(out, key):
    """(n_iter, C, size) host array of a collect() entry"""
    return np.ascontiguousarray(np.transpose(out[key], (2, 0, 1)))


def same(got, want, keys=KEYS):
    return all(got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in keys)


@pytest.fixture(scope="module")
def gmrf_run(golden):
    from test_mcmc_api_gpu import build

    M, _ = build(golden("gmrf_chain"), "sparse_", True, 6, fuse=True, n_burn=5, n_iter=60, seed=5)
    M.run_mcmc()
    yield M, store_of(M.collect(), "b")
    M.engine.close()


def shard(x, chains):
    """an MCMC that holds the chains `chains` of the host store x on an engine of its own (the summaries need no more)"""
    from openmcmc_amd.engine import Engine
    from openmcmc_amd.mcmc import MCMC

    sub = np.ascontiguousarray(x[:, chains, :])
    M = MCMC.__new__(MCMC)
    M.engine = Engine(sub.shape[1], seed=1)
    M.store, M._derived, M.store_ring, M._n_dev, M.n_iter = {"f": M.engine.to_device(sub)}, set(), 0, sub.shape[0], sub.shape[0]
    return M, sub


def levels_of(x):
    return [float(v) for v in np.quantile(x, [0.35, 0.5, 0.7])]


@pytest.mark.parametrize("kind", KINDS)
def test_excursion_matches_the_restatement(gmrf_run, kind):
    M, x = gmrf_run
    n = x.shape[2]
    rng = np.random.default_rng(3)
    index = [n - 1, 0, 3, 0, 7, 3]  # repeats: tied marginal counts
    lv = levels_of(x)
    for idx in (None, index):
        k = n if idx is None else len(idx)
        offset = 0.1 * rng.standard_normal(k)
        for level, off, alpha in ((lv[1], None, 0.05), (lv[0], offset, 0.3), (lv[2], None, 0.6)):
            got = M.excursion("b", level, kind=kind, alpha=alpha, index=idx, offset=off)
            want = excursion(x, level, kind=kind, alpha=alpha, index=idx, offset=off)
            assert same(got, want), (kind, idx is None, level)
            assert got["counts"].sum() == x.shape[0] * x.shape[1]
    # a given order is used as it is, also with an offset
    given = rng.permutation(n)
    got = M.excursion("b", lv[1], kind=kind, order=given, offset=0.05 * np.arange(n))
    assert same(got, excursion(x, lv[1], kind=kind, order=given, offset=0.05 * np.arange(n))) and np.array_equal(got["order"], given)
    assert not np.array_equal(got["counts"], M.excursion("b", lv[1], kind=kind, offset=0.05 * np.arange(n))["counts"])


def test_a_sequence_of_levels_equals_the_calls_one_by_one(gmrf_run):
    M, x = gmrf_run
    n = x.shape[2]
    lv = levels_of(x)
    lv = [lv[2], lv[0], lv[1]]  # in no order
    for kind in KINDS:
        both = M.excursion("b", lv, kind=kind, alpha=0.2)
        assert both["F"].shape == (3, n) and both["counts"].shape == (3, n + 1) and both["order"].shape == (3, n)
        for i, level in enumerate(lv):
            one = M.excursion("b", level, kind=kind, alpha=0.2)
            assert all(np.array_equal(both[k][i], one[k]) for k in KEYS), (kind, i)
            assert same(one, excursion(x, level, kind=kind, alpha=0.2))
    one = M.excursion("b", [lv[0]])
    assert one["F"].shape == (1, n)  # a sequence of one keeps the axis
    eight = M.excursion("b", list(np.quantile(x, np.linspace(0.2, 0.8, 8))))
    assert eight["F"].shape == (8, n) and np.array_equal(eight["F"][3], M.excursion("b", float(np.quantile(x, np.linspace(0.2, 0.8, 8))[3]))["F"])


def test_contour_map_matches_the_restatement(gmrf_run):
    M, x = gmrf_run
    n = x.shape[2]
    mean = M.summary("b")[0]
    np.testing.assert_allclose(mean, x.reshape(-1, n).mean(axis=0), rtol=1e-12)  # the restatement's input: the device means
    for levels, idx in ((levels_of(x), None), ([float(np.median(x))], None), (list(np.quantile(x, np.linspace(0.1, 0.9, 9))), [n - 1, 0, 3, 0, 7])):
        got = M.contour_map("b", levels[::-1], index=idx)
        if idx is not None:  # (the means of the selected columns are taken on a store of those columns)
            mean = M.engine.store_moments(M._store_3d("b").index_select(2, M.engine._int64(idx, "index")).contiguous(), pooled=True)[0].cpu().numpy()
            np.testing.assert_allclose(mean, x.reshape(-1, n)[:, idx].mean(axis=0), rtol=1e-12)
        want = contour_map(x, levels, index=idx, mean=mean)
        assert np.array_equal(got["band"], want["band"]) and got["band"].dtype == np.int64
        for k in ("P0", "P1"):
            assert isinstance(got[k], float) and got[k] == want[k], (k, got[k], want[k])
        for k in ("F0", "F1"):
            assert np.array_equal(got[k], want[k]), k
        assert set(got) == {"band", "P0", "P1", "F0", "F1"} and 0.0 <= got["P0"] <= got["P1"] <= 1.0
        print("levels", len(levels), "P0", got["P0"], "P1", got["P1"])


def test_counts_of_two_shards_with_a_common_order_add(gmrf_run):
    _, x = gmrf_run
    R = x.shape[0] * x.shape[1]
    level = levels_of(x)[1]
    A, xa = shard(x, [0, 1, 2])
    B, xb = shard(x, [3, 4, 5])
    W, _ = shard(x, list(range(6)))
    for kind in (">", "<"):
        whole = W.excursion("f", level, kind=kind)
        assert same(whole, excursion(x, level, kind=kind))
        # the ranks' agreeing counts add to the whole run's, and the common order comes from their sum
        counts = [np.rint(S.excursion("f", level, kind=kind)["marginal"] * (R // 2)).astype(np.int64) for S in (A, B)]
        order = np.argsort(-(counts[0] + counts[1]), kind="stable")
        assert np.array_equal(order, whole["order"])
        parts = [S.excursion("f", level, kind=kind, order=order) for S in (A, B)]
        h = parts[0]["counts"] + parts[1]["counts"]
        assert np.array_equal(h, whole["counts"])
        pos = np.empty_like(order)
        pos[order] = np.arange(order.size)
        assert np.array_equal((R - np.cumsum(h)[:-1])[pos] / float(R), whole["F"])
    for S in (A, B, W):
        S.engine.close()


def test_ties_nan_draws_and_the_denominator():
    """a planted store: two elements with equal counts keep their order, and a NaN draw counts against both sides"""
    N, C, n = 10, 2, 4
    x = np.zeros((N, C, n))
    x[:, :, 0] = 1.0                  # always above 0.5
    x[:, :, 1] = 1.0
    x[0, 0, 1] = np.nan               # one draw on no side
    x[:5, :, 2] = 1.0                 # half above, half below: the tie of "!=" takes the upper side
    x[:, :, 3] = 1.0                  # tied with element 0
    M, _ = shard(x, [0, 1])
    for kind in KINDS:
        got = M.excursion("f", 0.5, kind=kind)
        assert same(got, excursion(x, 0.5, kind=kind)), kind
    up = M.excursion("f", 0.5)
    assert up["order"].tolist() == [0, 3, 1, 2] and up["marginal"].tolist() == [1.0, 19 / 20, 0.5, 1.0]
    assert up["F"].tolist() == [1.0, 19 / 20, 9 / 20, 1.0] and up["counts"].tolist() == [0, 0, 1, 10, 9]
    assert M.exceedance("f", 0.5)[0].tolist() == [1.0, 1.0, 0.5, 1.0]  # divides by the non-NaN draws
    avoid = M.excursion("f", 0.5, kind="!=")
    assert avoid["marginal"][2] == 0.5 and avoid["counts"].tolist() == up["counts"].tolist()  # element 2 sides with "above"
    down = M.excursion("f", 0.5, kind="<")
    assert down["marginal"].tolist() == [0.0, 0.0, 0.5, 0.0] and down["order"].tolist() == [2, 0, 1, 3]
    cm = M.contour_map("f", [0.25])  # (the NaN mean of element 1 sorts above every level)
    assert cm["band"].tolist() == [1, 1, 1, 1] and cm["P0"] == 9 / 20 and cm["P1"] == 19 / 20
    M.engine.close()


def test_infinite_and_nan_draws_through_the_api():
    """+-inf draws are ordinary values in the marginal counts, the sides and the bands; NaN draws are on no side"""
    rng = np.random.default_rng(17)
    N, C, n = 30, 3, 12
    x = np.round(2 * rng.standard_normal((N, C, n))) / 2 + np.linspace(-1, 1, n).round(1)  # draws on the levels too
    u = rng.random(x.shape)
    x[u < 0.05] = np.nan
    x[(u >= 0.05) & (u < 0.10)] = np.inf
    x[(u >= 0.10) & (u < 0.15)] = -np.inf
    x[:, :, 3] = np.where(np.isfinite(x[:, :, 3]), x[:, :, 3], 0.5)  # one element without them
    M, _ = shard(x, [0, 1, 2])
    for kind in KINDS:
        for level, idx in ((0.5, None), (0.0, [11, 3, 3, 0]), ([-0.5, 0.5, 1.0], None)):
            got = M.excursion("f", level, kind=kind, index=idx, alpha=0.4)
            if np.ndim(level):
                assert all(same({k: got[k][i] for k in KEYS}, excursion(x, v, kind=kind, index=idx, alpha=0.4)) for i, v in enumerate(level)), kind
            else:
                assert same(got, excursion(x, level, kind=kind, index=idx, alpha=0.4)), (kind, level)
    mean = M.summary("f")[0]  # NaN, +inf or -inf where an element has such draws: the restatement's input
    assert not np.isfinite(mean).all() and np.isfinite(mean[3])
    for levels in ([0.0], [-0.5, 0.5, 1.0]):
        got, want = M.contour_map("f", levels), contour_map(x, levels, mean=mean)
        assert np.array_equal(got["band"], want["band"]) and got["P0"] == want["P0"] and got["P1"] == want["P1"]
        assert np.array_equal(got["F0"], want["F0"]) and np.array_equal(got["F1"], want["F1"])
    M.engine.close()


def test_errors(gmrf_run):
    M, x = gmrf_run
    n = x.shape[2]
    with pytest.raises(ValueError, match="pooled=False"):
        M.excursion("b", 0.0, pooled=False)
    with pytest.raises(ValueError, match="pooled=False"):
        M.contour_map("b", [0.0], pooled=False)
    with pytest.raises(ValueError, match="unknown kind"):
        M.excursion("b", 0.0, kind=">=")
    with pytest.raises(ValueError, match="1 to 8"):
        M.excursion("b", list(range(9)))
    with pytest.raises(ValueError, match="finite"):
        M.excursion("b", np.inf)
    with pytest.raises(ValueError, match="levels must differ"):
        M.excursion("b", [0.5, 0.5])
    with pytest.raises(ValueError, match="offset"):
        M.excursion("b", 0.0, offset=np.zeros(n + 1))
    with pytest.raises(ValueError, match="permutation"):
        M.excursion("b", 0.0, order=np.zeros(n, dtype=np.int64))
    with pytest.raises(ValueError, match="alpha"):
        M.excursion("b", 0.0, alpha=1.0)
    with pytest.raises(ValueError, match="distinct"):
        M.contour_map("b", [0.5, 0.5])
    with pytest.raises(ValueError):
        M.excursion("b", 0.0, index=[n])
