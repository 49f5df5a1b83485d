"""The tiling and LDS image of the joint density's convolution as host arithmetic (openmcmc_amd/csrc/omc_kde2d_layout.h through the
exported query omc_kde2d_layout; no GPU): at every (nx, ny) the regions the kernel indexes -- spelled out here, independently of the
header -- lie inside the image in order and on 16-byte boundaries, every index the kernel forms stays inside its region, and the
image's end, which is what the host launches with, stays inside the budget it states, with room for three workgroups on a CU of
160 KiB."""

import ctypes

import pytest

from kde2d_cases import layout

LDS_CU, LDS_WORKGROUP = 160 * 1024, 64 * 1024


def check(nx, ny):
    l = layout(nx, ny)
    where = (nx, ny, l)
    waves = l["threads"] // 64
    assert l["threads"] == 256 and l["ry"] == (1 if ny <= 64 else 2) and l["ty"] == 64 * l["ry"] and l["tx"] % 4 == 0, where
    assert l["tiles_x"] * l["tx"] >= nx > (l["tiles_x"] - 1) * l["tx"] and l["tiles_y"] * l["ty"] >= ny > (l["tiles_y"] - 1) * l["ty"], where
    assert 1 <= l["rb"] <= nx and l["cs"] % l["ry"] == 0 and ny <= l["cs"] < ny + l["ry"], where
    # counts: rows 0 .. rb (the last one all zero), columns < cs; the partial tiles of the waves: tx x ty doubles in the same place
    assert l["counts_off"] == 0 and 8 * max((l["rb"] + 1) * l["cs"], l["tx"] * l["ty"]) <= l["rownz_off"], where
    assert l["rownz_off"] + 4 * (l["rb"] + 1) <= l["mask_off"] and l["mask_off"] + 16 * (l["rb"] + 1) <= l["weights_off"], where
    assert l["cs"] // l["ry"] <= 128, where  # a row's runs of ry cells: one bit each of its two 64-bit words
    # weights of a wave: ry planes of pl slots; a lane reads slot lane - jb + nyp / ry and the one below, jb < nyp / ry: 0 .. pl - 1
    njb = l["cs"] // l["ry"]
    assert 63 - 0 + njb <= l["pl"] - 1 and 0 - (njb - 1) + njb - 1 >= 0, where
    assert 8 * l["ry"] * l["pl"] <= l["wave_weights"] and l["weights_off"] + waves * l["wave_weights"] <= l["end"], where
    # the column offsets a vector covers reach every pair (output column of the widest tile row, count column)
    lt_max = (l["tiles_y"] - 1) * l["ty"]
    assert l["ry"] * (l["pl"] - 1) + (l["ry"] - 1) - l["cs"] >= l["ty"] - 1 and 0 - l["cs"] <= -(l["cs"] - 1) - (l["ry"] - 1), where
    assert lt_max + l["ty"] >= ny, where
    assert all(l[k] % 16 == 0 for k in ("counts_off", "rownz_off", "mask_off", "weights_off", "wave_weights", "end")), where
    assert l["end"] <= l["budget"] <= LDS_WORKGROUP and 3 * l["budget"] <= LDS_CU, where


@pytest.mark.parametrize("nx,ny", ((8, 8), (8, 256), (256, 8), (256, 256), (100, 64), (100, 65), (33, 128), (33, 129)))
def test_the_image_fits_its_budget(nx, ny):
    check(nx, ny)


def test_every_grid_fits():
    for ny in range(8, 257):
        for nx in (8, 9, 15, 16, 17, 31, 32, 33, 100, 255, 256):
            check(nx, ny)
    for nx in range(8, 257):
        for ny in (8, 64, 65, 128, 129, 256):
            check(nx, ny)


def test_out_of_range_grids_are_rejected():
    from openmcmc_amd import _abi

    out = (ctypes.c_int32 * 16)()
    for nx, ny in ((7, 8), (8, 7), (0, 8), (-1, 8), (257, 8), (8, 257)):
        assert _abi.lib.omc_kde2d_layout(nx, ny, out) == _abi.INVALID_ARG
    assert _abi.lib.omc_kde2d_layout(8, 8, None) == _abi.INVALID_ARG
