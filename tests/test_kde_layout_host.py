"""The LDS image of the kernel density kernel as host arithmetic (openmcmc_amd/csrc/omc_kde_layout.h through the exported query
omc_kde_layout; no GPU): at every grid length the regions the kernel indexes -- spelled out here, independently of the header -- lie
inside the image in order and on 16-byte boundaries, and the image's end, which is what the host launches with, stays inside the
budget it states, with room for at least two workgroups on a CU of 160 KiB."""

import ctypes

import pytest

LDS_CU, LDS_WORKGROUP = 160 * 1024, 64 * 1024
NAMES = "threads counts_off a2_off cos_off gauss_off red_off end budget".split()


def layout(G):
    from openmcmc_amd import _abi

    out = (ctypes.c_int32 * 8)()
    assert _abi.lib.omc_kde_layout(G, out) == _abi.OK
    return dict(zip(NAMES, out))


def check(G):
    l = layout(G)
    assert l["threads"] == (64 if G <= 128 else 256), (G, l)
    # counts: doubles, index j < G; A2 (and the prefix sums before it): index k < G; cosines: index m <= G; Gaussians: index d < 2 G
    assert l["counts_off"] == 0 and l["counts_off"] + 8 * G <= l["a2_off"], (G, l)
    assert l["a2_off"] + 8 * G <= l["cos_off"] and l["cos_off"] + 8 * (G + 1) <= l["gauss_off"], (G, l)
    assert l["gauss_off"] + 8 * 2 * G <= l["red_off"], (G, l)
    # block sums: two buffers of ceil(G / 64) <= 16 doubles, then the quartiles and (value, bin) of every wave's maximum
    assert -(-G // 64) <= 16 and l["red_off"] + 8 * (2 * 16 + 2 + 2 * (l["threads"] // 64)) <= l["end"], (G, l)
    assert all(l[k] % 16 == 0 for k in NAMES[1:7]), (G, l)
    assert l["end"] <= l["budget"] <= LDS_WORKGROUP and 2 * l["budget"] <= LDS_CU, (G, l)


@pytest.mark.parametrize("G", (8, 100, 1024))
def test_the_image_fits_its_budget(G):
    check(G)


def test_every_grid_length_fits():
    for G in range(8, 1025):
        check(G)


def test_out_of_range_grid_lengths_are_rejected():
    from openmcmc_amd import _abi

    out = (ctypes.c_int32 * 8)()
    for G in (7, 0, -1, 1025):
        assert _abi.lib.omc_kde_layout(G, out) == _abi.INVALID_ARG
    assert _abi.lib.omc_kde_layout(8, None) == _abi.INVALID_ARG
