"""openmcmc_amd/summary/ranges.py against the expressions it replaced: `histogram`, `kde`, the axes of `histogram2d` and of `kde2d` each
spelled the range rule out, and the functions below named `was_*` are those four spellings, line for line as they stood in mcmc.py.
Everything is compared bit for bit (tobytes).  No GPU: numpy only."""

import numpy as np
import pytest

from openmcmc_amd.summary.ranges import auto_range, bin_edges, linspace_edges, widen

MSG = ("the caller's words for a bad int", "the caller's words for a bad shape")

BIG = 1.7e308
# six elements: generic, never moved, no draw (the device reports NaN, NaN, 0), -0.0 .. 0.0, the ends of fp64, a maximum of -0.0
MN = np.array([-1.25, 3.0, np.nan, -0.0, -BIG, -1.0])
MX = np.array([2.5, 3.0, np.nan, 0.0, BIG, -0.0])
CNT = np.array([12, 12, 0, 12, 12, 12], dtype=np.int64)


def was_histogram(mn, mx, cnt, n_bins):
    lo, hi = np.where(cnt > 0, mn, 0.0), np.where(cnt > 0, mx, 1.0)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("autodetected range is not finite")
    same = lo == hi
    lo, hi = np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)
    return np.stack([np.linspace(a, b, n_bins + 1) for a, b in zip(lo, hi)])


def was_histogram_given(range, n_bins):
    lo, hi = (float(v) for v in range)
    if lo > hi:
        raise ValueError("max must be larger than min in range parameter.")
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"supplied range of [{lo}, {hi}] is not finite")
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, n_bins + 1)


def was_kde(mn, mx, cnt, extend, G):
    lo, hi = np.where(cnt > 0, mn, 0.0), np.where(cnt > 0, mx, 1.0)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("autodetected range is not finite")
    same = lo == hi
    pad = extend * (hi - lo)
    a, b = np.where(same, lo - 0.5, lo - pad), np.where(same, hi + 0.5, hi + pad)
    return a, b, np.stack([np.linspace(x, y, G + 1) for x, y in zip(a, b)])


def was_axis_edges(mn, mx, cnt, n, rng, pool_elements):
    if rng is not None:
        lo, hi = (float(v) for v in rng)
        if lo > hi:
            raise ValueError("max must be larger than min in range parameter.")
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"supplied range of [{lo}, {hi}] is not finite")
        lo, hi = np.array([lo]), np.array([hi])
    else:
        lo, hi = np.where(cnt > 0, mn, 0.0), np.where(cnt > 0, mx, 1.0)
        if pool_elements:
            have = cnt > 0
            lo, hi = (np.array([lo[have].min()]), np.array([hi[have].max()])) if have.any() else (np.zeros(1), np.ones(1))
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError("autodetected range is not finite")
    same = lo == hi
    lo, hi = np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)
    edges = np.stack([np.linspace(a, b, n + 1) for a, b in zip(lo, hi)])
    return edges[0] if (rng is not None or pool_elements) else edges


def was_kde2d_axis(mn, mx, cnt, extend, n, pool_elements):
    lo, hi = np.where(cnt > 0, mn, 0.0), np.where(cnt > 0, mx, 1.0)
    if pool_elements:
        have = cnt > 0
        lo, hi = (np.array([lo[have].min()]), np.array([hi[have].max()])) if have.any() else (np.zeros(1), np.ones(1))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("autodetected range is not finite")
    same = lo == hi
    pad = extend * (hi - lo)
    a, b = np.where(same, lo - 0.5, lo - pad), np.where(same, hi + 0.5, hi + pad)
    edges = np.stack([np.linspace(p, q, n + 1) for p, q in zip(a, b)])
    return (a[0], b[0], edges[0]) if pool_elements else (a, b, edges)


def same_bits(got, expected):
    got, expected = np.asarray(got), np.asarray(expected)
    assert got.dtype == expected.dtype and got.shape == expected.shape
    assert got.tobytes() == expected.tobytes()


def test_without_extend_nothing_is_padded_and_the_ends_of_fp64_stay_finite():
    lo, hi = widen(*auto_range(MN, MX, CNT))
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and lo[4] == -BIG and hi[4] == BIG  # (no extend * (hi - lo) = 0 * inf)
    with np.errstate(over="ignore", invalid="ignore"):
        edges = linspace_edges(lo, hi, 8)
        same_bits(edges, was_histogram(MN, MX, CNT, 8))
        same_bits(edges, was_axis_edges(MN, MX, CNT, 8, None, False))
    # a constant element and one without a draw have the edges numpy gives them; -0.0 .. 0.0 counts as constant
    same_bits(edges[1], np.linspace(2.5, 3.5, 9))
    same_bits(edges[2], np.linspace(0.0, 1.0, 9))
    same_bits(edges[3], np.linspace(-0.5, 0.5, 9))
    # the element is accepted as before; np.linspace forms hi - lo itself, so only the last of its edges is a number (as before)
    assert edges[4, -1] == BIG and not np.isfinite(edges[4, :-1]).any()
    # half the range does not overflow: every edge is finite
    half = linspace_edges(*widen(*auto_range(MN / 2, MX / 2, CNT)), 8)
    same_bits(half, was_histogram(MN / 2, MX / 2, CNT, 8))
    assert np.isfinite(half[4]).all() and half[4, 0] == -BIG / 2 and half[4, -1] == BIG / 2


@pytest.mark.parametrize("extend", (0, 0.0, 0.1))
def test_with_extend_the_kernel_estimates_pad_as_they_did(extend):
    with np.errstate(over="ignore", invalid="ignore"):
        a, b = widen(*auto_range(MN, MX, CNT), extend=extend)
        edges = linspace_edges(a, b, 8)
        wa, wb, wedges = was_kde(MN, MX, CNT, extend, 8)
        xa, xb, xedges = was_kde2d_axis(MN, MX, CNT, extend, 8, False)
    for got, one, two in ((a, wa, xa), (b, wb, xb), (edges, wedges, xedges)):
        same_bits(got, one)
        same_bits(got, two)
    # hi - lo overflows at the ends of fp64: extend = 0 gives 0 * inf = NaN there, which kde keeps (and then refuses on its own)
    assert not np.isfinite(a[4]) and not np.isfinite(b[4])
    assert np.isfinite(a[[0, 1, 2, 3, 5]]).all() and np.isfinite(b[[0, 1, 2, 3, 5]]).all()
    if extend == 0:
        same_bits(a[:4], np.array([-1.25, 2.5, 0.0, -0.5]))


@pytest.mark.parametrize("cnt", ([12, 12, 0, 12, 0, 12], [0, 0, 0, 0, 0, 0]), ids=("some_empty", "all_empty"))
def test_one_range_over_the_elements_that_have_a_draw(cnt):
    cnt = np.array(cnt, dtype=np.int64)
    mn, mx = np.where(cnt > 0, MN, np.nan), np.where(cnt > 0, MX, np.nan)
    lo, hi = auto_range(mn, mx, cnt, pool=True)
    assert lo.shape == hi.shape == (1,)
    same_bits(linspace_edges(*widen(lo, hi), 8)[0], was_axis_edges(mn, mx, cnt, 8, None, True))
    for extend in (0, 0.1):
        a, b = widen(lo, hi, extend=extend)
        wa, wb, wedges = was_kde2d_axis(mn, mx, cnt, extend, 8, True)
        same_bits(a[0], wa)
        same_bits(b[0], wb)
        same_bits(linspace_edges(a, b, 8)[0], wedges)
    expected = (-1.25, 3.0) if cnt.any() else (0.0, 1.0)
    assert (lo[0], hi[0]) == expected


@pytest.mark.parametrize("pool", (False, True))
def test_an_infinite_draw_is_refused_in_numpys_words(pool):
    mn = np.array([-np.inf, 0.0])
    mx = np.array([1.0, 1.0])
    cnt = np.array([3, 3], dtype=np.int64)
    for was in (lambda: was_histogram(mn, mx, cnt, 4), lambda: was_kde(mn, mx, cnt, 0.1, 8),
                lambda: was_axis_edges(mn, mx, cnt, 4, None, pool), lambda: was_kde2d_axis(mn, mx, cnt, 0.1, 8, pool),
                lambda: auto_range(mn, mx, cnt, pool=pool)):
        with pytest.raises(ValueError) as e:
            was()
        assert str(e.value) == "autodetected range is not finite"
    # an infinite draw of an element that is not counted does not matter
    auto_range(mn, mx, np.array([0, 3], dtype=np.int64), pool=pool)


@pytest.mark.parametrize("rng, text", [((2.0, 1.0), "max must be larger than min in range parameter."),
                                       ((0.0, np.inf), "supplied range of [0.0, inf] is not finite"),
                                       ((np.nan, 1.0), "supplied range of [nan, 1.0] is not finite")])
def test_a_given_range_is_refused_in_numpys_words(rng, text):
    for fn in (lambda: was_histogram_given(rng, 4), lambda: was_axis_edges(None, None, None, 4, rng, False), lambda: bin_edges(4, rng, None, MSG)):
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == text


@pytest.mark.parametrize("rng", [(-1.5, 2.25), (3.0, 3.0), (-0.0, 0.0), (0.1, 0.3), (-BIG, BIG), (1e-320, 1e-320), (np.float32(0.1), 7)])
def test_a_given_range_gives_the_edges_of_both_callers(rng):
    with np.errstate(over="ignore", invalid="ignore"):
        edges = bin_edges(7, rng, None, MSG)
        same_bits(edges, was_histogram_given(rng, 7))  # (+-0.5 on the floats, before np.linspace)
        same_bits(edges, was_axis_edges(None, None, None, 7, rng, False))  # (+-0.5 on one-element arrays)


def test_arrays_of_edges():
    text = MSG[1]

    def check_edges(bins, _, per_element=True):
        return bin_edges(bins, None, None, MSG, pool=not per_element)

    same_bits(check_edges([0, 1, 1, 2], text), np.array([0.0, 1.0, 1.0, 2.0]))
    same_bits(check_edges([[0, 1], [5, 6]], text), np.array([[0.0, 1.0], [5.0, 6.0]]))
    given = np.array([0.0, 0.5, 4.0])
    assert check_edges(given, text) is not given  # (a copy, as np.array(bins, dtype=np.float64) was)
    for bad in ([1.0], np.zeros((2, 2, 2)), [[0.0], [1.0]]):
        with pytest.raises(ValueError) as e:
            check_edges(bad, text)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        check_edges([[0, 1], [5, 6]], text, per_element=False)
    assert str(e.value) == text
    for bad in ([0.0, np.nan, 1.0], [0.0, 2.0, 1.0], [[0.0, 1.0], [1.0, 0.0]]):
        with pytest.raises(ValueError) as e:
            check_edges(bad, text)
        assert str(e.value) == "`bins` must increase monotonically, when an array"
    with pytest.raises(ValueError) as e:  # the shape is judged first
        check_edges([[0.0, np.nan], [0.0, 1.0]], text, per_element=False)
    assert str(e.value) == text


def test_int_bins_through_bin_edges_are_the_edges_of_both_histograms():
    with np.errstate(over="ignore", invalid="ignore"):
        same_bits(bin_edges(8, None, lambda: (MN, MX, CNT), MSG), was_histogram(MN, MX, CNT, 8))
        same_bits(bin_edges(np.int64(8), None, lambda: (MN, MX, CNT), MSG), was_axis_edges(MN, MX, CNT, 8, None, False))
    cnt = np.array([12, 12, 0, 12, 0, 12], dtype=np.int64)
    same_bits(bin_edges(8.0, None, lambda: (MN, MX, cnt), MSG, pool=True), was_axis_edges(MN, MX, cnt, 8, None, True))
    for bad in (0, 1025, 2.5):
        with pytest.raises(ValueError) as e:  # before the store would be read
            bin_edges(bad, None, None, MSG)
        assert str(e.value) == MSG[0]
