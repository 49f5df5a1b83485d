"""Joint 2-D histograms and occupancy maps of the device store (omc_store_histogram2d, Engine.store_histogram2d,
MCMC.histogram2d / occupancy) against numpy on the host copy of the same stores: np.histogram2d(x, y, bins=[ex, ey]) of the pair's
draws without the pairs that have a NaN coordinate, and for occupancy the loop over rows of np.histogram2d(...)[0] > 0.  Counts are
integers: every comparison is np.array_equal; edges and densities are built by the same numpy operations and compared with ==.

Shapes sit at the edges of the tiling: TE pairs of a workgroup's tile and RB rows of a slice, both a function of the grid, the
edge mode and the shape (Engine.hist2d_tile); the largest grid the LDS form takes and the first one it does not are read from the
layout.  Every check runs the default form, the forced direct form and the forced bisection (option "hist2d_algo") and holds the
three against each other bit for bit before comparing with numpy."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def engine(C):
    from openmcmc_amd.engine import Engine
    return Engine(C, seed=1)


def hist2d(xv, yv, ex, ey):
    """np.histogram2d of the valid pairs as int64, and the two outside counts"""
    ok = ~(np.isnan(xv) | np.isnan(yv))
    with np.errstate(all="ignore"):  # (numpy takes differences of infinite edges on the way)
        H = np.histogram2d(xv[ok], yv[ok], bins=[ex, ey])[0].astype(np.int64)
    return H, [ok.sum() - H.sum(), (~ok).sum()]


def reference(x, y, ex, ey, ix=None, iy=None, pooled=True, pool_pairs=False, occupancy=False):
    """(counts, outside[, occupied]) of host stores x (n_iter, C, size_x), y (n_iter, C, size_y) by np.histogram2d"""
    n_iter, C = x.shape[:2]
    xs = x if ix is None else x[:, :, np.asarray(ix)]
    ys = y if iy is None else y[:, :, np.asarray(iy)]
    n = xs.shape[2]
    assert ys.shape[2] == n
    batches = [(xs.reshape(-1, n), ys.reshape(-1, n))] if pooled else [(xs[:, c], ys[:, c]) for c in range(C)]
    nx, ny = ex.shape[-1] - 1, ey.shape[-1] - 1
    counts, outside, occupied = [], [], []
    for bx, by in batches:
        if pool_pairs:
            H, o = hist2d(bx.ravel(), by.ravel(), ex, ey)
            if occupancy:
                occ = np.zeros((nx, ny), dtype=np.int64)
                for r in range(bx.shape[0]):
                    occ += hist2d(bx[r], by[r], ex, ey)[0] > 0
                occupied.append(occ)
        else:
            res = [hist2d(bx[:, k], by[:, k], ex if ex.ndim == 1 else ex[k], ey if ey.ndim == 1 else ey[k]) for k in range(n)]
            H, o = np.stack([r[0] for r in res]), np.array([r[1] for r in res])
        counts.append(H)
        outside.append(np.asarray(o, dtype=np.int64))
    out = [np.stack(counts), np.stack(outside)] + ([np.stack(occupied)] if occupancy else [])
    return [v[0] for v in out] if pooled else out


def check(eng, x, y, ex, ey, ix=None, iy=None, pooled=True, pool_pairs=False, occupancy=False, dx=None, dy=None):
    dx = eng.to_device(x) if dx is None else dx
    dy = (dx if y is x else eng.to_device(y)) if dy is None else dy
    got = []
    for algo in (0, 1, 2):  # as the layout decides; always the direct form; always the bisection
        eng.set_option("hist2d_algo", algo)
        got.append([t.cpu().numpy() for t in eng.store_histogram2d(dx, dy, ex, ey, index_x=ix, index_y=iy, pooled=pooled,
                                                                    pool_pairs=pool_pairs, occupancy=occupancy)])
    eng.set_option("hist2d_algo", 0)
    for other in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got[0], other))
    want = reference(x, y, np.asarray(ex), np.asarray(ey), ix, iy, pooled, pool_pairs, occupancy)
    assert len(got[0]) == len(want)
    for g, w in zip(got[0], want):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w)
    counts, outside = got[0][:2]
    rows = x.shape[0] * (x.shape[1] if pooled else 1)
    n = x.shape[2] if ix is None else len(ix)
    assert np.all(counts.sum(axis=(-2, -1)) + outside.sum(axis=-1) == rows * (n if pool_pairs else 1))
    if occupancy:
        assert np.all(got[0][2] <= counts) and np.all(got[0][2] <= rows) and np.all(got[0][2] >= (counts > 0))
    return got[0]


def make_edges(rng, nb, rows, uniform):
    """(nb + 1,) for rows None, else (rows, nb + 1): evenly spaced, or sorted normal deviates (with a repeated edge)"""
    n = 1 if rows is None else rows
    if uniform:
        lo, hi = rng.uniform(-2.5, -0.5, n), rng.uniform(0.5, 2.5, n)
        e = np.stack([np.linspace(a, b, nb + 1) for a, b in zip(lo, hi)])
    else:
        e = np.sort(rng.standard_normal((n, nb + 1)) * 1.3, axis=-1)
        if nb >= 3:
            e[:, nb // 2] = e[:, nb // 2 + 1]
    return e[0] if rows is None else e


def lds_limit(per, shape):
    """the largest n for which the n x n grid is counted in LDS"""
    from openmcmc_amd.engine import Engine

    n = 1
    while not Engine.hist2d_layout(n + 1, n + 1, per, shape)[0]:
        n += 1
    return n


# ---------------------------------------------------------------------------------------------------------- tile edges
GRIDS = ((1, 1), (1, 7), (7, 1), (13, 13), (64, 64), "lds_max", "direct_min", (300, 300))
SIZES = ("1", "TE-1", "TE", "TE+1", "2TE+3")
POOLED_PAIRS = (1, 5, 32, 33, 65, 129, 257, 600)  # a row in one to 64 lanes of a wave, in two to four slots, in several trips
FORMS = ((1, "3RB+7", True), (3, "RB-1", True), (1, "RB", True), (65, "1", False), (3, "RB+1", False), (1, "1", True),
         (65, ">3RB+7", True), (1, "RB-1", True), (1, "RB+1", False))


def tile_cases():
    out = []
    for i, grid in enumerate(GRIDS):
        for j in range(5):
            k = 5 * i + j
            pool_pairs = j in (1, 3)
            per = not pool_pairs and (i + j) % 4 == 0
            C, rows, pooled = FORMS[(2 * i + j) % len(FORMS)]
            size = str(POOLED_PAIRS[k % len(POOLED_PAIRS)]) if pool_pairs else SIZES[(i + j) % 5]
            name = grid if isinstance(grid, str) else "x".join(map(str, grid))
            out.append(pytest.param(grid, per, pool_pairs, size, C, rows, pooled, (k // 2) % 2 == 0,
                                    id=f"grid{name}-{'pool' if pool_pairs else 'per' if per else 'shared'}-pairs{size}-C{C}-rows{rows}-"
                                       f"{'pooled' if pooled else 'chain'}"))
    return out


@pytest.mark.parametrize("grid,per,pool_pairs,size_kind,C,rows_kind,pooled,uniform", tile_cases())
def test_tile_edges(grid, per, pool_pairs, size_kind, C, rows_kind, pooled, uniform):
    from openmcmc_amd.engine import Engine

    direct = grid in ("direct_min", (300, 300))
    if isinstance(grid, str):
        n = lds_limit(per, int(pool_pairs)) + (grid == "direct_min")
        grid = (n, n)
    nx, ny = grid
    form, TE, RB = Engine.hist2d_layout(nx, ny, per, pool_pairs)[:3]
    assert form == int(direct)
    rows = {"1": 1, "RB-1": RB - 1, "RB": RB, "RB+1": RB + 1, "3RB+7": 3 * RB + 7, ">3RB+7": -(-(3 * RB + 7) // C) * C}[rows_kind]
    n_iter = -(-rows // C) if pooled else rows  # (pooled: the row count itself where C divides it, else the next multiple of C)
    if pool_pairs:
        n = max(1, min(int(size_kind), 2_000_000 // (n_iter * C)))  # (the host reference walks every pair)
    else:
        n = max(1, {"1": 1, "TE-1": TE - 1, "TE": TE, "TE+1": TE + 1, "2TE+3": 2 * TE + 3}[size_kind])
        n = max(1, min(n, 4_000_000 // (nx * ny * (1 if pooled else C))))  # (the output is a grid per pair and chain)
    rng = np.random.default_rng(1000 * nx + 10 * C + len(size_kind) + int(per))
    x = rng.standard_normal((n_iter, C, n)) * rng.uniform(0.5, 1.5, n) + rng.uniform(-0.5, 0.5, n)
    y = 0.6 * x + rng.standard_normal((n_iter, C, n)) * rng.uniform(0.5, 1.5, n)
    ex, ey = make_edges(rng, nx, n if per else None, uniform), make_edges(rng, ny, n if per else None, uniform)
    eng = engine(C)
    check(eng, x, y, ex, ey, pooled=pooled, pool_pairs=pool_pairs)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- the bin rule
@pytest.mark.parametrize("pool_pairs", (False, True))
def test_draws_on_the_edges(pool_pairs):
    """Coordinates drawn from the edge values themselves, their neighbours in fp64 and the midpoints: a repeated edge, infinite
    first and last edges with infinite draws, an edge at 0.0 with draws of -0.0."""
    rng = np.random.default_rng(21)
    ex = np.array([-np.inf, -1.5, -0.25, 0.0, 0.0, 0.75, 1.0, 1.0, 1.0, 3.0, np.inf])
    ey = np.array([-2.0, -1.0, -1.0, 0.0, 0.5, 2.0])
    ez = np.linspace(-1.0, 1.0, 11)  # evenly spaced: the arithmetic guess lands on or beside the edge

    def pool(e):
        fin = e[np.isfinite(e)]
        return np.concatenate([e, np.nextafter(fin, np.inf), np.nextafter(fin, -np.inf), (fin[1:] + fin[:-1]) / 2,
                               [-0.0, 0.0, -np.inf, np.inf, fin[0] - 1.0, fin[-1] + 1.0]])

    n_iter, C, n = 700, 3, 6
    eng = engine(C)
    for ea, eb in ((ex, ey), (ey, ex), (ez, ez), (ez, ex), (ex, ex)):
        x = rng.choice(pool(ea), size=(n_iter, C, n))
        y = rng.choice(pool(eb), size=(n_iter, C, n))
        counts, outside = check(eng, x, y, ea, eb, pool_pairs=pool_pairs)
        assert counts.sum() > 0 and (outside[..., 0].sum() > 0 or not (np.isfinite(ea[0]) or np.isfinite(eb[0])))
        if not pool_pairs:
            check(eng, x, y, np.tile(ea, (n, 1)), np.tile(eb, (n, 1)), pooled=False)
    # the last edge closes the last bin, +inf == +inf included; -0.0 sits in the bin that starts at 0.0
    one = np.full((1, C, 1), np.inf)
    counts, _ = check(eng, one, one, ex, ex, pool_pairs=pool_pairs)
    assert counts.reshape(10, 10)[9, 9] == C
    zero = np.full((1, C, 1), -0.0)
    counts, _ = check(eng, zero, zero, ex, ey, pool_pairs=pool_pairs)
    assert counts.reshape(10, 5)[4, 3] == C  # (the last of the equal bins at 0.0 in x; [0.0, 0.5) in y)
    eng.close()


@pytest.mark.parametrize("pool_pairs", (False, True))
def test_nan_coordinates_drop_the_pair(pool_pairs):
    n_iter, C, n = 300, 3, 5
    rng = np.random.default_rng(22)
    x, y = rng.standard_normal((n_iter, C, n)), rng.standard_normal((n_iter, C, n))
    x[rng.random(x.shape) < 0.2] = np.nan  # in x only, in y only and, where the two meet, in both
    y[rng.random(y.shape) < 0.2] = np.nan
    x[:, :, 3] = np.nan  # a pair that is NaN throughout in one coordinate, one that is so in both
    x[:, :, 4] = np.nan
    y[:, :, 4] = np.nan
    assert (np.isnan(x) & np.isnan(y)).any() and (np.isnan(x) & ~np.isnan(y)).any() and (~np.isnan(x) & np.isnan(y)).any()
    eng = engine(C)
    ex, ey = np.linspace(-1.5, 1.5, 8), np.sort(rng.standard_normal(6))
    for pooled in (True, False):
        counts, outside = check(eng, x, y, ex, ey, pooled=pooled, pool_pairs=pool_pairs)
        if not pool_pairs:
            assert not counts[..., 3:, :, :].any() and np.all(outside[..., 3:, 1] == (n_iter * C if pooled else n_iter))
    eng.close()


# ---------------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("pooled", (True, False))
def test_indices_reversed_repeated_and_from_two_stores(pooled):
    n_iter, C, sx, sy = 257, 3, 11, 29
    rng = np.random.default_rng(23)
    x, y = rng.standard_normal((n_iter, C, sx)), rng.standard_normal((n_iter, C, sy)) + np.linspace(-1, 1, sy)
    eng = engine(C)
    dx, dy = eng.to_device(x), eng.to_device(y)
    ex, ey = np.linspace(-2, 2, 10), np.sort(rng.standard_normal(8)) * 1.2
    ix = np.concatenate([np.arange(sx), np.arange(sx)[::-1], [4, 4, 0, sx - 1]])
    iy = np.concatenate([np.arange(sx) + 7, (np.arange(sx) + 7)[::-1], [20, 20, 28, 0]])
    counts, _ = check(eng, x, y, ex, ey, ix=ix, iy=iy, pooled=pooled, dx=dx, dy=dy)
    assert np.array_equal(counts[..., :sx, :, :], counts[..., 2 * sx - 1:sx - 1:-1, :, :])  # reversed indices reverse the result
    assert np.array_equal(counts[..., 2 * sx, :, :], counts[..., 2 * sx + 1, :, :])  # a repeated pair repeats its grid
    # x and y from one store (the same tensor on both sides); swapping the sides transposes the grids
    a, _ = check(eng, x, x, ex, ey, ix=[0, 3, 5], iy=[10, 3, 0], pooled=pooled, dx=dx, dy=dx)
    b, _ = check(eng, x, x, ey, ex, ix=[10, 3, 0], iy=[0, 3, 5], pooled=pooled, dx=dx, dy=dx)
    assert np.array_equal(a, np.swapaxes(b, -1, -2))
    # pooled pairs under an index, with and without occupancy
    check(eng, x, y, ex, ey, ix=ix, iy=iy, pooled=pooled, pool_pairs=True, occupancy=True, dx=dx, dy=dy)
    with pytest.raises(ValueError, match="equally many"):
        eng.store_histogram2d(dx, dy, ex, ey)
    with pytest.raises(ValueError, match="equally many"):
        eng.store_histogram2d(dx, dy, ex, ey, index_x=[0, 1], index_y=[0])
    eng.close()


def test_pooled_pairs_are_the_sum_over_pairs():
    n_iter, C, n = 500, 3, 70
    rng = np.random.default_rng(24)
    x, y = rng.standard_normal((n_iter, C, n)), rng.standard_normal((n_iter, C, n))
    y[rng.random(y.shape) < 0.1] = np.nan
    eng = engine(C)
    dx, dy = eng.to_device(x), eng.to_device(y)
    ex, ey = np.linspace(-2, 2, 17), np.linspace(-1, 3, 10)
    for pooled in (True, False):
        each, out_each = check(eng, x, y, ex, ey, pooled=pooled, dx=dx, dy=dy)
        both, out_both = check(eng, x, y, ex, ey, pooled=pooled, pool_pairs=True, dx=dx, dy=dy)
        assert np.array_equal(each.sum(axis=-3), both) and np.array_equal(out_each.sum(axis=-2), out_both)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- occupancy
def ragged(rng, n_iter, C, n_max, scale=1.0):
    """two NaN-padded stores of a variable-size parameter: live length 0 .. n_max per (iteration, chain)"""
    k = rng.integers(0, n_max + 1, size=(n_iter, C))
    live = np.arange(n_max) < k[..., None]
    x = np.where(live, rng.uniform(0.0, 10.0, (n_iter, C, n_max)), np.nan)
    y = np.where(live, rng.standard_normal((n_iter, C, n_max)) * scale, np.nan)
    return x, y


@pytest.mark.parametrize("n_pairs,grid", ((20, (2, 2)), (1, (5, 4)), (63, (9, 3)), (64, (3, 9)), (65, (6, 6)), (256, (16, 16)),
                                          (20, (64, 64)), (20, (80, 80))))
def test_occupancy_of_a_ragged_store(n_pairs, grid):
    """20 components into 2 x 2 cells: duplicates within a row are certain; 80 x 80 with occupancy is past the LDS budget"""
    C = 3
    n_iter = 350 if n_pairs <= 65 else 120
    rng = np.random.default_rng(25 + n_pairs)
    x, y = ragged(rng, n_iter, C, n_pairs)
    ex, ey = np.linspace(0.5, 9.0, grid[0] + 1), np.linspace(-1.5, 1.5, grid[1] + 1)
    eng = engine(C)
    for pooled in (True, False):
        counts, _, occupied = check(eng, x, y, ex, ey, pooled=pooled, pool_pairs=True, occupancy=True)
        if n_pairs == 1:
            assert np.array_equal(occupied, counts)
        elif grid == (2, 2):
            assert np.all(occupied < counts)
    eng.close()


def test_occupancy_is_limited_to_256_pairs():
    C = 2
    eng = engine(C)
    d = eng.to_device(np.zeros((4, C, 257)))
    e = np.linspace(-1, 1, 3)
    with pytest.raises(NotImplementedError):
        eng.store_histogram2d(d, d, e, e, pool_pairs=True, occupancy=True)
    counts, _ = eng.store_histogram2d(d, d, e, e, pool_pairs=True)  # (without occupancy any number of pairs)
    assert counts.cpu().numpy()[1, 1] == 4 * C * 257
    with pytest.raises(ValueError, match="pool_pairs"):
        eng.store_histogram2d(d, d, e, e, occupancy=True)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- marginals
@pytest.mark.parametrize("pooled", (True, False))
def test_one_infinite_bin_in_y_gives_the_marginals_of_x(pooled):
    n_iter, C, n = 1100, 3, 67
    rng = np.random.default_rng(26)
    x, y = rng.standard_normal((n_iter, C, n)), rng.standard_normal((n_iter, C, n)) * 1e3
    x[rng.random(x.shape) < 0.05] = np.nan
    eng = engine(C)
    dx, dy = eng.to_device(x), eng.to_device(y)
    for ex in (np.linspace(-2, 2, 33), np.sort(rng.standard_normal(20))):
        counts, outside = (t.cpu().numpy() for t in eng.store_histogram2d(dx, dy, ex, np.array([-np.inf, np.inf]), pooled=pooled))
        c1, o1 = (t.cpu().numpy() for t in eng.store_histogram(dx, ex, pooled=pooled))
        assert counts.shape[-1] == 1 and np.array_equal(counts[..., 0], c1)
        assert np.array_equal(outside[..., 0], o1[..., 0] + o1[..., 1]) and np.array_equal(outside[..., 1], o1[..., 2])
    eng.close()


# ---------------------------------------------------------------------------------------------------------- contract
def test_rejections_leave_the_outputs_alone_and_null_outputs_work():
    import torch

    from openmcmc_amd import _abi

    n_iter, C, sx, sy, nx, ny = 16, 3, 12, 20, 6, 4
    rng = np.random.default_rng(27)
    x, y = rng.standard_normal((n_iter, C, sx)), rng.standard_normal((n_iter, C, sy))
    eng = engine(C)
    dx, dy = eng.to_device(x), eng.to_device(y)
    good_x, good_y = np.linspace(-2, 2, nx + 1), np.linspace(-2, 2, ny + 1)
    nan_edge, decreasing = good_x.copy(), good_y.copy()
    nan_edge[3] = np.nan
    decreasing[2] = decreasing[1] - 1e-9
    iy = np.arange(sx)
    for ex, ey in ((nan_edge, good_y), (good_x, decreasing), (good_y, nan_edge), (np.tile(nan_edge, (sx, 1)), np.tile(good_y, (sx, 1)))):
        with pytest.raises(ValueError, match="invalid argument"):
            eng.store_histogram2d(dx, dy, ex, ey, index_y=iy)
    for bad in ([0, -1], [sx, 1], [2 ** 40, 0]):
        with pytest.raises(ValueError, match="invalid argument"):
            eng.store_histogram2d(dx, dy, good_x, good_y, index_x=bad, index_y=[0, 1])
    for bad in ([0, -1], [sy, 1]):
        with pytest.raises(ValueError, match="invalid argument"):
            eng.store_histogram2d(dx, dy, good_x, good_y, index_x=[0, 1], index_y=bad)
    with pytest.raises(ValueError):
        eng.store_histogram2d(dx, dy, np.tile(good_x, (3, 1)), np.tile(good_y, (3, 1)), index_y=iy)  # per-pair edges of another count
    with pytest.raises(ValueError):
        eng.store_histogram2d(dx, dy, np.tile(good_x, (sx, 1)), good_y, index_y=iy)  # per pair on one axis only
    with pytest.raises(ValueError):
        eng.store_histogram2d(dx, dy, np.tile(good_x, (sx, 1)), np.tile(good_y, (sx, 1)), index_y=iy, pool_pairs=True)
    with pytest.raises(ValueError):
        eng.store_histogram2d(dx, dy, np.linspace(0, 1, 1026 + 1), good_y, index_y=iy)

    def ptr(t):
        return None if t is None else t.data_ptr()

    def call(ex, ey, idx_x, idx_y, n, counts, outside, occupied=None, pool_pairs=0, per=0, nx=nx, ny=ny):
        ex, ey = eng.to_device(ex), eng.to_device(ey)
        st = _abi.lib.omc_store_histogram2d(eng._ctx, n_iter, sx, dx.data_ptr(), ptr(idx_x), sy, dy.data_ptr(), ptr(idx_y), n, 1, pool_pairs,
                                            nx, ex.data_ptr(), ny, ey.data_ptr(), per, ptr(counts), ptr(outside), ptr(occupied))
        torch.cuda.synchronize()
        return st

    def idx(v):
        return torch.as_tensor(np.array(v, dtype=np.int64), device=dx.device)

    counts = torch.full((sx, nx, ny), -7, dtype=torch.int64, device=dx.device)
    outside = torch.full((sx, 2), -7, dtype=torch.int64, device=dx.device)
    occupied = torch.full((nx, ny), -7, dtype=torch.int64, device=dx.device)
    iy_d = idx(iy)
    for pool_pairs, occ in ((0, None), (1, None), (1, occupied)):
        assert call(nan_edge, good_y, None, iy_d, sx, counts, outside, occ, pool_pairs) == _abi.INVALID_ARG
        assert call(good_x, decreasing, None, iy_d, sx, counts, outside, occ, pool_pairs) == _abi.INVALID_ARG
        assert call(good_x, good_y, idx([3, sx]), idx([0, 1]), 2, counts, outside, occ, pool_pairs) == _abi.INVALID_ARG
        assert call(good_x, good_y, idx([3, 0]), idx([-1, 1]), 2, counts, outside, occ, pool_pairs) == _abi.INVALID_ARG
        assert call(good_x, good_y, idx([3, 0]), idx([sy, 1]), 2, counts, outside, occ, pool_pairs) == _abi.INVALID_ARG
    assert call(good_x, good_y, None, iy_d, sx, counts, outside, nx=0) == _abi.INVALID_ARG
    assert call(good_x, good_y, None, iy_d, sx, counts, outside, ny=1025) == _abi.INVALID_ARG
    assert call(good_x, good_y, None, iy_d, 2, counts, outside) == _abi.INVALID_ARG  # n_pairs must equal size without an index
    assert call(good_x, good_y, None, None, sx, counts, outside) == _abi.INVALID_ARG  # ... on either side
    assert call(good_x, good_y, None, iy_d, sx, counts, outside, occupied) == _abi.INVALID_ARG  # occupancy is of pooled pairs
    assert call(good_x, good_y, None, iy_d, sx, counts, outside, None, 1, 1) == _abi.INVALID_ARG  # pooled pairs share their edges
    for t in (counts, outside, occupied):
        assert np.all(t.cpu().numpy() == -7)
    # NULL outside_out; the outputs are overwritten, not accumulated
    want = reference(x, y, good_x, good_y, None, iy)[0]
    for _ in range(2):
        assert call(good_x, good_y, None, iy_d, sx, counts, None) == _abi.OK
        assert np.array_equal(counts.cpu().numpy(), want)
    assert np.all(outside.cpu().numpy() == -7)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- public API
def test_histogram2d_through_mcmc(golden):
    """A short run of the linear-regression model: MCMC.histogram2d against np.histogram2d of the stored draws"""
    from test_mcmc_api_gpu import build_linreg

    G = golden("linreg_chain")
    C = 3
    M = build_linreg(G, "ex3_", C)
    M.run_mcmc()
    beta = M.store["beta"].cpu().numpy()
    beta = beta.reshape(beta.shape[0], C, -1)
    logp = M.store["log_post"].cpu().numpy().reshape(beta.shape[0], C)
    p = beta.shape[2]
    flat, flat_lp = beta.reshape(-1, p), logp.ravel()
    ix, iy = [0, p - 1, 0], [1, 0, 0]
    # int bins without a range: every coordinate gets numpy's own edges; key_y=None pairs elements of one entry
    for bins in (10, (4, 7), 1):
        hist, xe, ye = M.histogram2d("beta", index_x=ix, index_y=iy, bins=bins)
        dens, xd, yd = M.histogram2d("beta", index_x=ix, index_y=iy, bins=bins, density=True)
        nx, ny = (bins, bins) if np.ndim(bins) == 0 else bins
        assert hist.shape == (3, nx, ny) and hist.dtype == np.int64 and xe.shape == (3, nx + 1) and ye.shape == (3, ny + 1)
        assert np.array_equal(xe, xd) and np.array_equal(ye, yd)
        for k, (i, j) in enumerate(zip(ix, iy)):
            want, wx, wy = np.histogram2d(flat[:, i], flat[:, j], bins=bins)
            assert np.array_equal(hist[k], want) and np.all(xe[k] == wx) and np.all(ye[k] == wy)
            assert np.all(dens[k] == np.histogram2d(flat[:, i], flat[:, j], bins=bins, density=True)[0])
        per, xp, yp = M.histogram2d("beta", index_x=ix, index_y=iy, bins=bins, pooled=False)  # the chains share the pooled range's edges
        assert per.shape == (C, 3, nx, ny) and np.array_equal(xp, xe) and np.array_equal(per.sum(axis=0), hist)
        for c in range(C):
            assert np.array_equal(per[c, 1], np.histogram2d(beta[:, c, ix[1]], beta[:, c, iy[1]], bins=[xe[1], ye[1]])[0])
    # a range: shared edges; a 2-D entry as one element against every element of another entry
    lo, hi = np.quantile(beta, 0.2), np.quantile(beta, 0.9)
    rng_lp = [flat_lp.min(), np.quantile(flat_lp, 0.8)]
    hist, xe, ye = M.histogram2d("beta", "log_post", index_y=[0] * p, bins=(12, 5), range=[[lo, hi], rng_lp])
    assert hist.shape == (p, 12, 5) and xe.shape == (13,) and ye.shape == (6,)
    with np.errstate(all="ignore"):
        dens, _, _ = M.histogram2d("beta", "log_post", index_y=[0] * p, bins=(12, 5), range=[[lo, hi], rng_lp], density=True)
        for i in range(p):
            want, wx, wy = np.histogram2d(flat[:, i], flat_lp, bins=(12, 5), range=[[lo, hi], rng_lp])
            assert np.array_equal(hist[i], want) and np.all(xe == wx) and np.all(ye == wy)
            want = np.histogram2d(flat[:, i], flat_lp, bins=(12, 5), range=[[lo, hi], rng_lp], density=True)[0]
            assert np.array_equal(dens[i], want, equal_nan=True)
    # a range on one axis only; pool_elements: one map and one range over all selected elements
    hist, xe, ye = M.histogram2d("beta", "log_post", index_x=[p - 1], bins=6, range=[None, rng_lp])
    want, wx, wy = np.histogram2d(flat[:, p - 1], flat_lp, bins=6, range=[None, rng_lp])
    assert np.array_equal(hist[0], want) and np.all(xe[0] == wx) and np.all(ye == wy)
    hist, xe, ye = M.histogram2d("beta", index_x=[0, 1], index_y=[1, 0], bins=9, pool_elements=True)
    want, wx, wy = np.histogram2d(flat[:, [0, 1]].ravel(), flat[:, [1, 0]].ravel(), bins=9)
    assert np.array_equal(hist, want) and np.all(xe == wx) and np.all(ye == wy)
    # edge arrays: one for both axes, one per axis, per pair
    mine = np.sort(np.random.default_rng(3).standard_normal(8)) * 3.0
    hist, xe, ye = M.histogram2d("beta", index_x=ix, index_y=iy, bins=mine)
    assert np.array_equal(xe, mine) and np.array_equal(ye, mine) and hist.shape == (3, 7, 7)
    for k, (i, j) in enumerate(zip(ix, iy)):
        assert np.array_equal(hist[k], np.histogram2d(flat[:, i], flat[:, j], bins=mine)[0])
    per_pair = np.stack([mine + 0.1 * k for k in range(3)])
    hist, xe, ye = M.histogram2d("beta", index_x=ix, index_y=iy, bins=[per_pair, mine[:5]], pooled=False)
    assert np.array_equal(xe, per_pair) and np.array_equal(ye, mine[:5]) and hist.shape == (C, 3, 7, 4)
    for c in range(C):
        for k, (i, j) in enumerate(zip(ix, iy)):
            assert np.array_equal(hist[c, k], np.histogram2d(beta[:, c, i], beta[:, c, j], bins=[per_pair[k], mine[:5]])[0])
    with pytest.raises(ValueError):
        M.histogram2d("beta", index_x=ix, index_y=iy, bins=mine[::-1])
    with pytest.raises(ValueError):
        M.histogram2d("beta", index_x=ix, index_y=iy, bins=0)
    with pytest.raises(ValueError):
        M.histogram2d("beta", index_x=ix, index_y=iy, bins=5, range=[[1.0, 0.0], None])
    M.store["beta"][0, 0, 0] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        M.histogram2d("beta", index_x=ix, index_y=iy, bins=5)
    M.engine.close()
    # a ring store holds the last iterations only: nothing to reduce on the device
    M = build_linreg(G, "ex3_", C, store_ring=6)
    M.run_mcmc()
    for call in (lambda: M.histogram2d("beta", index_x=[0], index_y=[1]), lambda: M.occupancy("beta", index_x=[0], index_y=[1])):
        with pytest.raises(ValueError, match="store_ring"):
            call()
    M.engine.close()


def test_occupancy_of_a_reversible_jump_run(golden):
    """Knot location against coefficient over a short run of the reversible-jump problem: per stored state
    np.histogram2d(theta, beta)[0] > 0 over the live knots, averaged over the states."""
    from test_rj_chain_gpu import run_with_tape

    G = golden("rj_gmrf_chain")
    chains = np.arange(min(4, G["init_k"].shape[0]))
    n_iter = 40
    M, _, _ = run_with_tape(G, chains, n_iter)
    M.run_mcmc()
    C = len(chains)
    theta, beta = (M.store[k].cpu().numpy().reshape(n_iter, C, -1) for k in ("theta", "beta"))
    assert np.isnan(theta).any() and np.array_equal(np.isnan(theta), np.isnan(beta))
    for bins, rng in ((6, None), ((8, 3), [[np.nanmin(theta), np.nanmax(theta)], [-1.0, 1.0]])):
        for pooled in (True, False):
            prob, xe, ye = M.occupancy("theta", "beta", bins=bins, range=rng, pooled=pooled)
            fx, fy = theta[~np.isnan(theta)], beta[~np.isnan(beta)]
            _, wx, wy = np.histogram2d(fx, fy, bins=bins, range=rng)
            assert np.all(xe == wx) and np.all(ye == wy)
            want = np.zeros((C,) + prob.shape[-2:])
            for it in range(n_iter):
                for c in range(C):
                    live = ~np.isnan(theta[it, c])
                    want[c] += np.histogram2d(theta[it, c][live], beta[it, c][live], bins=[xe, ye])[0] > 0
            want = want.sum(axis=0) / (n_iter * C) if pooled else want / n_iter
            assert prob.shape == want.shape and np.all(prob == want) and prob.max() > 0
            hist, xh, yh = M.histogram2d("theta", "beta", bins=bins, range=rng, pooled=pooled, pool_elements=True)
            assert np.all(xh == xe) and np.all(yh == ye)
            if pooled:
                assert np.array_equal(hist, np.histogram2d(fx, fy, bins=[xe, ye])[0])
    M.engine.close()
