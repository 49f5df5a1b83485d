"""The LDS image of k_hist_count as host arithmetic (openmcmc_amd/csrc/omc_hist_layout.h through the exported query
omc_store_histogram_layout; no GPU): for every n_bins and both edge modes the tile holds at least one element, the regions the
kernel indexes -- spelled out here, independently of the header -- lie inside the image in order, and the image's end, which is
what the host launches with, stays inside the budget and inside one workgroup's LDS."""

import ctypes

import pytest

LDS_WORKGROUP = 64 * 1024


def layout(n_bins, per):
    from openmcmc_amd import _abi

    out = (ctypes.c_int32 * 10)()
    assert _abi.lib.omc_store_histogram_layout(n_bins, per, out) == _abi.OK
    return dict(zip("TE RB ES CS edges_off counts_off outside_off end budget threads".split(), out))


@pytest.mark.parametrize("per", (0, 1))
def test_every_bin_count_fits(per):
    for n_bins in range(1, 1025):
        l = layout(n_bins, per)
        te = l["TE"]
        assert te >= 1 and te & (te - 1) == 0 and l["threads"] % te == 0 and te <= 64, (n_bins, l)
        # edges: doubles, index j <= n_bins of the shared array, or element * ES + j
        edge_doubles = (te - 1) * l["ES"] + n_bins + 1 if per else n_bins + 1
        assert (l["ES"] >= n_bins + 1 and l["ES"] % 2 == 1) if per else l["ES"] == 0
        assert l["edges_off"] == 0 and l["edges_off"] + 8 * edge_doubles <= l["counts_off"], (n_bins, l)
        # counters: words, element * CS + j, j < n_bins; zeroed as TE * CS words
        assert l["CS"] >= n_bins and l["CS"] % 2 == 1
        assert l["counts_off"] % 4 == 0 and l["counts_off"] + 4 * te * l["CS"] <= l["outside_off"], (n_bins, l)
        # outside counts: words, element * 3 + k
        assert l["outside_off"] % 4 == 0 and l["outside_off"] + 4 * 3 * te <= l["end"], (n_bins, l)
        assert l["end"] <= l["budget"] <= LDS_WORKGROUP, (n_bins, l)
        # a block's 32-bit counters: RB is what the host cuts the rows into; sixteen rows per bin, a power of two
        assert l["RB"] >= 1024 and l["RB"] >= 16 * n_bins and l["RB"] & (l["RB"] - 1) == 0
        # the tile is the largest that fits: the next power of two would not (or is past the 64 lanes of a wave)
        if te < 64:
            per_el = 4 * l["CS"] + 12 + (8 * l["ES"] if per else 0)
            assert 2 * te * per_el + (0 if per else 8 * (n_bins + 1)) > l["budget"], (n_bins, l)


def test_out_of_range_bin_counts_are_rejected():
    from openmcmc_amd import _abi

    out = (ctypes.c_int32 * 10)()
    for n_bins in (0, -1, 1025):
        assert _abi.lib.omc_store_histogram_layout(n_bins, 0, out) == _abi.INVALID_ARG
    assert _abi.lib.omc_store_histogram_layout(8, 0, None) == _abi.INVALID_ARG
