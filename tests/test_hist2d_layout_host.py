"""The LDS images of k_hist2d_pair / k_hist2d_pool as host arithmetic (openmcmc_amd/csrc/omc_hist2d_layout.h through the exported
query omc_store_histogram2d_layout; no GPU): for every grid, both edge modes and every shape the regions the kernels index --
spelled out here, independently of the header -- are 8-byte aligned, lie inside the image in order without overlap, the image's
end (what the host launches with) stays inside the budget, TE is a power of two, and the direct form is reported exactly where
the counters of one pair (TE = 1) do not fit."""

import ctypes
import itertools

import pytest

LDS_WORKGROUP = 64 * 1024
BINS = (1, 2, 7, 63, 64, 65, 1024)
NAMES = "direct TE RB EXS EYS CS ex_off ey_off counts_off occ_off outside_off end budget threads".split()
PER_PAIR, POOLED, POOLED_OCC = 0, 1, 2


def layout(nx, ny, per, shape):
    from openmcmc_amd import _abi

    out = (ctypes.c_int32 * 14)()
    assert _abi.lib.omc_store_histogram2d_layout(nx, ny, per, shape, out) == _abi.OK
    return dict(zip(NAMES, out))


def image_bytes(nx, ny, per, shape, direct, te):
    """bytes of the image with te pairs, region by region as the kernels index them: [(name, bytes), ...]"""
    cells = nx * ny
    ex = 8 * ((te - 1) * ((nx + 1) | 1) + nx + 1) if per else 8 * (nx + 1)
    ey = 8 * ((te - 1) * ((ny + 1) | 1) + ny + 1) if per else 8 * (ny + 1)
    counts = 0 if direct else 4 * ((te - 1) * (cells | 1) + cells)
    occ = 4 * cells if (shape == POOLED_OCC and not direct) else 0
    return [("ex_off", ex), ("ey_off", ey), ("counts_off", counts), ("occ_off", occ), ("outside_off", 16 * te)]


@pytest.mark.parametrize("per,shape", ((0, PER_PAIR), (1, PER_PAIR), (0, POOLED), (0, POOLED_OCC)))
def test_every_grid_fits(per, shape):
    for nx, ny in itertools.product(BINS, BINS):
        l = layout(nx, ny, per, shape)
        te, cells = l["TE"], nx * ny
        assert te >= 1 and te & (te - 1) == 0 and l["threads"] % te == 0 and te <= 64, (nx, ny, l)
        assert te == 1 or shape == PER_PAIR
        assert l["budget"] <= LDS_WORKGROUP and l["threads"] == 256
        # the direct form exactly where one pair's counters do not fit beside its edges and outside counts
        lds_one = sum(-(-b // 8) * 8 for _, b in image_bytes(nx, ny, per, shape, 0, 1))
        assert l["direct"] == int(lds_one > l["budget"]), (nx, ny, l, lds_one)
        # regions: aligned, in order, none reaching into the next, the last one ending inside the image
        regions = image_bytes(nx, ny, per, shape, l["direct"], te)
        assert l["ex_off"] == 0
        for (name, size), (nxt, _) in zip(regions, regions[1:] + [("end", 0)]):
            assert l[name] % 8 == 0 and l[name] + size <= l[nxt], (nx, ny, l, name)
        assert l["end"] % 8 == 0 and l["end"] <= l["budget"], (nx, ny, l)
        # strides: odd, at least the row they hold
        if per:
            assert l["EXS"] >= nx + 1 and l["EXS"] % 2 == 1 and l["EYS"] >= ny + 1 and l["EYS"] % 2 == 1
        else:
            assert l["EXS"] == 0 and l["EYS"] == 0
        assert (l["CS"] == 0) if l["direct"] else (l["CS"] >= cells and l["CS"] % 2 == 1)
        # rows of a slice: a power of two, at least 1024; in the LDS form enough rows per cell to pay for the flush
        rb = l["RB"]
        assert rb >= 1024 and rb & (rb - 1) == 0
        if not l["direct"]:
            assert rb >= (8 if shape == PER_PAIR else 1) * cells
        # the tile is the largest that fits: the next power of two would not (or is past the 64 lanes of a wave)
        if shape == PER_PAIR and te < 64:
            assert sum(-(-b // 8) * 8 for _, b in image_bytes(nx, ny, per, shape, l["direct"], 2 * te)) > l["budget"], (nx, ny, l)


def test_the_forms_meet_where_one_grid_fills_the_budget():
    """shared edges, one pair: 8 (nx + ny + 2) + 4 (nx ny | 1) (+ 4 to the next 8) + 16 bytes against 48 KiB"""
    assert layout(1024, 9, 0, PER_PAIR)["direct"] == 0 and layout(1024, 10, 0, PER_PAIR)["direct"] == 1
    assert layout(9, 1024, 1, PER_PAIR)["direct"] == 0 and layout(10, 1024, 1, PER_PAIR)["direct"] == 1
    assert layout(108, 108, 0, POOLED)["direct"] == 0 and layout(109, 109, 0, POOLED)["direct"] == 1
    assert layout(77, 77, 0, POOLED_OCC)["direct"] == 0 and layout(78, 78, 0, POOLED_OCC)["direct"] == 1
    assert layout(13, 13, 0, PER_PAIR)["TE"] == 64 and layout(32, 32, 0, PER_PAIR)["TE"] == 8


def test_out_of_range_grids_are_rejected():
    from openmcmc_amd import _abi

    out = (ctypes.c_int32 * 14)()
    for nx, ny in ((0, 8), (8, 0), (1025, 8), (8, 1025), (-1, 8)):
        for shape in (PER_PAIR, POOLED, POOLED_OCC):
            assert _abi.lib.omc_store_histogram2d_layout(nx, ny, 0, shape, out) == _abi.INVALID_ARG
    assert _abi.lib.omc_store_histogram2d_layout(8, 8, 0, 3, out) == _abi.INVALID_ARG
    assert _abi.lib.omc_store_histogram2d_layout(8, 8, 1, POOLED, out) == _abi.INVALID_ARG  # pooled pairs share their edges
    assert _abi.lib.omc_store_histogram2d_layout(8, 8, 0, PER_PAIR, None) == _abi.INVALID_ARG
