"""The made-up 2-D bin counts that tests/test_store_kde2d_gpu.py hands to Engine.kde2d_binned, and their restatement
(tests/kde2d_model.py) at np.longdouble and np.float64, computed once per process.  tests/test_kde2d_model_host.py holds the two
precisions together on the same cases without a GPU, and asserts for every case and prob that the level's position is out of
rounding's reach.

Shapes: 8 x 8, 8 x 256, 256 x 8, 256 x 256, and one bin either side of every edge the tiling has -- the columns of an output tile
(both lane widths), the rows of a count block, the rows of an output tile -- read from omc_kde2d_layout, not written down here.
Large grids are sparse (at most about 200 non-empty cells, so that the longdouble restatement takes seconds): the four corners, a
cell either side of every tile and block seam, strung along a diagonal (rising: a strong positive correlation; falling: a strong
negative one) with counts that differ from cell to cell, and a dense 5 x 5 clump.  One 24 x 20 grid has every cell non-empty.  No
grid is symmetric under a swap or a flip of its axes, the two axes have different widths, and no two cells that could hold the
mode carry the same count: a transposed grid, a swapped axis or a sign slip in the cross term changes the answer."""

import functools

import numpy as np
from kde2d_model import kde2d_model

PROBS = (0.5, 0.9)
LAYOUT_NAMES = "tx ty ry rb threads tiles_x tiles_y cs pl counts_off rownz_off mask_off weights_off wave_weights end budget".split()
# What a launch can hold at once, whatever a kernel's registers and LDS allow: every kernel of the call runs workgroups of 256
# threads = 4 waves, a CU holds at most 32 waves, the device has 256 CUs.  One grid more than that, at one workgroup per grid
# (8 x 8: one tile), and a second round of workgroups must run in every kernel of the call.
RESIDENT_WORKGROUPS_MAX = 256 * (32 // 4)
MANY = RESIDENT_WORKGROUPS_MAX + 1


def layout(nx, ny):
    """the sixteen numbers of Engine.kde2d_layout (static: no GPU) by name"""
    from openmcmc_amd.engine import Engine

    return dict(zip(LAYOUT_NAMES, Engine.kde2d_layout(nx, ny)))


def sparse_grid(nx, ny, falling=False, big=False):
    """corners, both sides of every seam along a diagonal, a 5 x 5 clump"""
    L = layout(nx, ny)
    c = np.zeros((nx, ny), dtype=np.int64)

    def col(i):  # the diagonal: column of row i
        j = (i * (ny - 1)) // max(nx - 1, 1)
        return ny - 1 - j if falling else j

    for k, i in enumerate(sorted({s + d for step in (L["tx"], L["rb"]) for s in range(step, nx, step) for d in (-1, 0)})):
        # (a fifth of the width either side of the diagonal in turn: a correlation near +-0.8, not +-0.99, whose det H would cancel)
        c[i, min(max(col(i) + (ny // 5 if k & 1 else -(ny // 5)), 0), ny - 1)] += 40 + (7 * k) % 23
    for k, j in enumerate(sorted({s + d for s in range(L["ty"], ny, L["ty"]) for d in (-1, 0)})):
        i = next(r for r in range(nx) if col(r) == j) if any(col(r) == j for r in range(nx)) else nx // 2
        c[i, j] += 31 + 5 * k
    for i, j, v in ((0, 0, 3), (0, ny - 1, 2), (nx - 1, 0, 1), (nx - 1, ny - 1, 4)):
        c[i, j] += v
    i0, j0 = min(max(nx // 3 - 2, 0), nx - 5), min(max(col(nx // 3) - 2, 0), ny - 5)
    c[i0:i0 + 5, j0:j0 + 5] += 200 + np.arange(25).reshape(5, 5) * 3 + np.arange(5)[:, None] * 11  # (its largest count stands alone)
    if big:
        c[i0 + 2, j0 + 2] = 2**31 - 5
    assert 0 < (c > 0).sum() <= 200
    return c


def dense_grid(nx, ny, rho, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((4000, 2))
    x, y = 0.3 + z[:, 0], -0.2 + 0.6 * (rho * z[:, 0] + np.sqrt(1 - rho * rho) * z[:, 1])
    c = np.histogram2d(x, y, bins=[nx, ny], range=[[-4.0, 4.5], [-3.0, 2.6]])[0].astype(np.int64)
    return c


def _case(name, grids, rule="scott", bw=None, bw_fct=1.0, probs=PROBS, ends=None):
    counts = np.stack(grids)
    n = len(grids)
    lo_x, hi_x, lo_y, hi_y = ends if ends is not None else (np.full(n, -3.1), np.full(n, 4.3), np.full(n, 0.7), np.full(n, 2.9))
    return dict(name=name, counts=counts, lo_x=np.array(lo_x, dtype=float), hi_x=np.array(hi_x, dtype=float),
                lo_y=np.array(lo_y, dtype=float), hi_y=np.array(hi_y, dtype=float), rule=rule,
                bw=None if bw is None else np.array(bw, dtype=float), bw_fct=bw_fct, probs=tuple(probs))


def edge_shapes():
    """(nx, ny) one bin either side of every edge of the tiling, from the layout"""
    shapes = []
    for ty in sorted({layout(256, ny)["ty"] for ny in (8, 256)}):  # the columns of a tile at either lane width
        for ny in (ty - 1, ty + 1):
            L = layout(256, ny)
            shapes += [(L["rb"] - 1, ny), (L["rb"] + 1, ny), (L["tx"] + 1, ny)]
    return shapes


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for k, (nx, ny) in enumerate(((8, 8), (8, 256), (256, 8), (256, 256))):
        out.append(_case(f"{nx}x{ny}-scott", [sparse_grid(nx, ny, falling=bool(k & 1))]))
    for k, (nx, ny) in enumerate(edge_shapes()):
        out.append(_case(f"{nx}x{ny}-edge", [sparse_grid(nx, ny, falling=bool(k & 1))], bw_fct=0.8 if k & 2 else 1.0))
    # every cell non-empty, both signs of the correlation, a degenerate grid between two good ones
    pos, neg = dense_grid(24, 20, 0.85, 3) + 1, dense_grid(24, 20, -0.9, 4) + 1
    one_row = np.zeros((24, 20), dtype=np.int64)
    one_row[5] = 7
    out.append(_case("24x20-dense-scott", [pos, one_row, neg], bw_fct=0.7, probs=(0.3, 0.5, 0.9, 0.99)))
    dx, dy = 7.4 / 24, 2.2 / 20
    out.append(_case("24x20-given-negative", [pos, neg, pos], rule="given", bw_fct=1.3,
                     bw=[[(2 * dx) ** 2, -0.6 * 2 * dx * 1.5 * dy, (1.5 * dy) ** 2], [(3 * dx) ** 2, -0.9 * 3 * dx * 2 * dy, (2 * dy) ** 2],
                         [dx * dx, dx * dy, dy * dy]]))  # (the last one singular: flag 2)
    bx, by = 7.4 / 128, 2.2 / 128  # (a given kernel of a few bins: under a rule 2^31 draws in one cell leave H a spike)
    out.append(_case("128x128-big-count", [sparse_grid(128, 128, big=True)], rule="given", probs=(0.5, 0.999999),
                     bw=[[(6 * bx) ** 2, 0.5 * 6 * bx * 4 * by, (4 * by) ** 2]]))
    # more grids than a launch can hold workgroups at once (MANY, above)
    rng = np.random.default_rng(11)
    many = []
    for g in range(MANY):
        c = rng.integers(0, 9, size=(8, 8)) * (rng.random((8, 8)) < 0.4)
        if g % 97 == 5:
            c[:] = 0
        if g % 97 == 6:
            c[:] = 0
            c[3, 4] = 1
        many.append(c.astype(np.int64))
    ends = (-1.0 - 0.01 * np.arange(MANY), 2.0 + 0.02 * np.arange(MANY), np.full(MANY, 10.0), 10.5 + 0.01 * np.arange(MANY))
    out.append(_case("many-8x8", many, ends=ends))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(i, dtype=np.longdouble):
    """kde2d_model of cases()[i] at dtype"""
    c = cases()[i]
    return kde2d_model(c["counts"], c["lo_x"], c["hi_x"], c["lo_y"], c["hi_y"], c["rule"], c["bw"], c["bw_fct"], c["probs"], dtype=dtype)
