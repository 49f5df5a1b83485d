"""The numpy restatement of tests/excursion_model.py against the definition, by brute force on small cases (no GPU): for every
element F_k R is the number of rows that agree at every element of order[: pos[k] + 1], counted with Python loops; F does not
increase along the order and never exceeds the marginal; the returned set holds whole rows with probability >= 1 - alpha; and on a
planted smooth field the joint set is a strict subset of the pointwise one."""

import math

import numpy as np
import pytest
from excursion_model import (KINDS, agree, band_sides, bands_of, contour_map, excursion, excursion_function, first_failure, joint_counts,
                             order_of, sides)


def agrees(x, lo, hi):
    """the definition, one draw at a time"""
    return x == x and (lo == -math.inf or x > lo) and (hi == math.inf or x < hi)


def small_store(seed, N=7, C=3, size=9):
    rng = np.random.default_rng(seed)
    x = np.round(rng.standard_normal((N, C, size)) * 2) / 2 + np.linspace(-1, 1, size)  # a coarse grid: ties with the levels
    x[rng.random(x.shape) < 0.05] = np.nan
    x[rng.random(x.shape) < 0.03] = np.inf
    x[rng.random(x.shape) < 0.03] = -np.inf
    return x


@pytest.mark.parametrize("seed", range(4))
def test_first_failure_is_the_definition(seed):
    x = small_store(seed).reshape(-1, 9)
    rng = np.random.default_rng(100 + seed)
    lo = rng.choice([-np.inf, -0.5, 0.0, 0.5], 9)
    hi = np.where(rng.random(9) < 0.5, np.inf, np.where(np.isneginf(lo), 0.0, lo) + rng.choice([0.5, 1.0, np.inf], 9))
    pos = rng.permutation(9)
    h, r = first_failure(x, lo, hi, pos)
    for s in range(x.shape[0]):
        fails = [int(pos[k]) for k in range(9) if not agrees(float(x[s, k]), float(lo[k]), float(hi[k]))]
        assert r[s] == min(fails + [9])
    assert h.sum() == x.shape[0] and all(h[j] == sum(1 for v in r if v == j) for j in range(10))
    a = agree(x, lo, hi)
    assert all(bool(a[s, k]) == agrees(float(x[s, k]), float(lo[k]), float(hi[k])) for s in range(x.shape[0]) for k in range(9))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", range(3))
def test_excursion_function_counts_rows_that_agree_along_the_order(seed, kind):
    store = small_store(seed)
    rows = store.reshape(-1, store.shape[2])
    R, n = rows.shape
    offset = 0.25 * np.arange(n) if seed == 1 else None
    level = 0.5
    u = np.full(n, level) + (0.0 if offset is None else offset)
    lo, hi, count = sides(rows, u, kind)
    for k in range(n):  # sides and tie rule, one element at a time
        above = sum(1 for s in range(R) if rows[s, k] > u[k])
        below = sum(1 for s in range(R) if rows[s, k] < u[k])
        up = kind == ">" or (kind != "<" and above >= below)
        assert (lo[k], hi[k], count[k]) == ((u[k], np.inf, above) if up else (-np.inf, u[k], below))
    order, pos = order_of(count)
    assert sorted(order.tolist()) == list(range(n)) and all(pos[order[j]] == j for j in range(n))
    assert all((count[order[j]], -order[j]) >= (count[order[j + 1]], -order[j + 1]) for j in range(n - 1))
    h, _ = first_failure(rows, lo, hi, pos)
    F = excursion_function(h, pos)
    for k in range(n):
        first = order[: pos[k] + 1]
        joint = sum(1 for s in range(R) if all(agrees(float(rows[s, e]), float(lo[e]), float(hi[e])) for e in first))
        assert F[k] * R == joint and F[k] == joint / float(R)
    assert np.all(np.diff(F[order]) <= 0) and np.all(F <= count / float(R))
    for alpha in (0.05, 0.2, 0.5, 0.9):
        out = excursion(store, level, kind=kind, alpha=alpha, offset=offset)
        assert np.array_equal(out["counts"], h) and np.array_equal(out["order"], order)
        avoid = out["set"] if kind != "=" else ~out["set"]
        assert np.array_equal(avoid, F >= 1 - alpha)
        members = np.flatnonzero(avoid)
        share = sum(1 for s in range(R) if all(agrees(float(rows[s, e]), float(lo[e]), float(hi[e])) for e in members)) / R
        assert share >= 1 - alpha
        if kind == "=":
            assert np.array_equal(out["F"], 1.0 - F) and np.array_equal(out["marginal"], 1.0 - count / float(R))
        else:
            assert np.array_equal(out["F"], F) and np.array_equal(out["marginal"], count / float(R))


def test_a_given_order_is_used_as_it_is():
    store = small_store(9)
    n = store.shape[2]
    given = np.arange(n)[::-1].copy()
    out = excursion(store, 0.0, order=given)
    rows = store.reshape(-1, n)
    for k in range(n):
        joint = sum(1 for s in range(rows.shape[0]) if all(rows[s, e] > 0.0 for e in given[: n - k]))
        assert out["F"][k] * rows.shape[0] == joint
    assert np.array_equal(out["order"], given)


def test_the_joint_set_is_a_strict_subset_of_the_pointwise_one():
    rng = np.random.default_rng(5)
    N, C, n = 100, 4, 60
    field = 1.6 * np.sin(np.linspace(0, np.pi, n))  # planted: above 0 in the middle, near it at the ends
    store = field + 0.45 * rng.standard_normal((N, C, n))
    out = excursion(store, 0.0, alpha=0.05)
    pointwise = out["marginal"] >= 0.95
    assert out["set"].any() and np.all(pointwise[out["set"]]) and pointwise.sum() > out["set"].sum()
    rows = store.reshape(-1, n)
    assert np.all(rows[:, out["set"]] > 0.0, axis=1).mean() >= 0.95 > np.all(rows[:, pointwise] > 0.0, axis=1).mean()


def test_band_rules_and_contour_map():
    levels = [-0.5, 0.5, 1.5]
    mean = np.array([-3.0, -0.5, 0.0, 0.5, 1.0, 1.5, 9.0])
    band = bands_of(mean, levels)
    assert band.tolist() == [0, 1, 1, 2, 2, 3, 3]  # a mean on a level belongs to the band above it
    lo, hi = band_sides(band, levels, 0)
    assert lo.tolist() == [-np.inf, -0.5, -0.5, 0.5, 0.5, 1.5, 1.5] and hi.tolist() == [-0.5, 0.5, 0.5, 1.5, 1.5, np.inf, np.inf]
    lo, hi = band_sides(band, levels, 1)
    assert lo.tolist() == [-np.inf, -np.inf, -np.inf, -0.5, -0.5, 0.5, 0.5] and hi.tolist() == [0.5, 1.5, 1.5, np.inf, np.inf, np.inf, np.inf]
    store = small_store(11, N=9, C=2, size=7) + mean / 3
    out = contour_map(store, levels)
    rows = store.reshape(-1, 7)
    R = rows.shape[0]
    b = bands_of(np.mean(rows, axis=0), levels)
    assert np.array_equal(out["band"], b)
    for w in (0, 1):
        lo, hi = band_sides(b, levels, w)
        inside = [all(agrees(float(rows[s, k]), float(lo[k]), float(hi[k])) for k in range(7)) for s in range(R)]
        assert out[f"P{w}"] == sum(inside) / float(R)
        count = np.array([sum(1 for s in range(R) if agrees(float(rows[s, k]), float(lo[k]), float(hi[k]))) for k in range(7)])
        order, pos = order_of(count)
        for k in range(7):
            joint = sum(1 for s in range(R) if all(agrees(float(rows[s, e]), float(lo[e]), float(hi[e])) for e in order[: pos[k] + 1]))
            assert out[f"F{w}"][k] * R == joint
    assert out["P1"] >= out["P0"] and np.all(out["F1"] >= 0)


def test_joint_counts_of_added_histograms():
    """the h of two halves of the rows over the same tables add to the h of all rows"""
    x = small_store(21, N=10, C=4).reshape(-1, 9)
    lo, hi, pos = np.full(9, 0.0), np.full(9, np.inf), np.random.default_rng(2).permutation(9)
    whole, _ = first_failure(x, lo, hi, pos)
    a, _ = first_failure(x[:17], lo, hi, pos)
    b, _ = first_failure(x[17:], lo, hi, pos)
    assert np.array_equal(a + b, whole) and np.array_equal(joint_counts(a) + joint_counts(b), joint_counts(whole))
