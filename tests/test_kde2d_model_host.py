"""The restatement of the joint density (tests/kde2d_model.py) held to an outside reference and to itself, without a GPU:
  - draws on bin centres under Scott's rule: the restatement equals scipy.stats.gaussian_kde of the centres repeated by their
    counts (unweighted; scipy's default is Scott's factor N^(-1/6) on the ddof-1 covariance: the same definition) within 1e-12;
  - level_pos and level equal a direct sort / cumsum;
  - fp64 and longdouble agree within 1e-12 on every GPU case (tests/kde2d_cases.py);
  - the flag rules;
  - the completed square that the restatement and the kernel evaluate equals the contract's three-term quadratic form summed as
    written at longdouble (1e-12), on GPU cases of both signs of the correlation;
  - for every GPU case and every prob the running sum at level_pos and at level_pos - 1 is further than 1e-9 S from prob S: out of
    the reach of the running sum's rounding, nx ny 2^-53 <= 7.3e-12, so that the kernel's level_pos must equal the restatement's."""

import numpy as np
import pytest
from kde2d_cases import cases, reference
from kde2d_model import kde2d_model
from scipy import stats

CASES = cases()


def scipy_density(c, lo_x, hi_x, lo_y, hi_y):
    nx, ny = c.shape
    X = lo_x + (np.arange(nx) + 0.5) * (hi_x - lo_x) / nx
    Y = lo_y + (np.arange(ny) + 0.5) * (hi_y - lo_y) / ny
    gx, gy = np.meshgrid(X, Y, indexing="ij")
    pts = np.vstack([np.repeat(gx.ravel(), c.ravel()), np.repeat(gy.ravel(), c.ravel())])
    return stats.gaussian_kde(pts)(np.vstack([gx.ravel(), gy.ravel()])).reshape(nx, ny)


def correlated_counts(nx, ny, n, rho, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 2))
    x, y = z[:, 0], rho * z[:, 0] + np.sqrt(1 - rho * rho) * z[:, 1]
    return np.histogram2d(x, y, bins=[nx, ny], range=[[-3, 3], [-3, 3]])[0].astype(np.int64)


@pytest.mark.parametrize("nx,ny,rho,ends", [(12, 9, 0.6, (-1.0, 2.0, 0.5, 4.0)), (12, 9, -0.8, (-1.0, 2.0, 0.5, 4.0)),
                                              (9, 17, -0.5, (0.0, 1.0, -30.0, 50.0)), (16, 16, 0.0, (2.0, 3.0, 2.0, 3.0))])
def test_scott_equals_scipy_on_the_repeated_centres(nx, ny, rho, ends):
    c = correlated_counts(nx, ny, 97, rho, nx + ny)
    m = kde2d_model(c, *ends, rule="scott")
    assert m["flag"] == 0
    want = scipy_density(c, *ends)
    err = float(np.max(np.abs(m["density"] - want) / want))
    print(nx, ny, rho, "max relative difference %.2e" % err)
    assert err <= 1e-12
    if rho:
        assert np.sign(m["bw"][1]) == np.sign(rho)
    # the transposed problem is the transposed answer, and nothing else is
    t = kde2d_model(c.T, ends[2], ends[3], ends[0], ends[1], rule="scott")
    assert np.max(np.abs(t["density"].T - m["density"]) / m["density"]) <= 1e-12
    assert np.array_equal(t["mode_index"][::-1], m["mode_index"])


def test_levels_equal_a_direct_sort_and_cumsum():
    c = correlated_counts(12, 9, 97, 0.6, 21)
    probs = (0.1, 0.5, 0.9, 0.999)
    m = kde2d_model(c, -1.0, 2.0, 0.5, 4.0, probs=probs)
    D = np.sort(m["density"].ravel())[::-1]
    S = np.cumsum(D)
    for q, p in enumerate(probs):
        r = int(np.searchsorted(S, p * S[-1], side="left"))
        assert m["level_pos"][q] == r and m["level"][q] == D[r]
        held = m["density"][m["density"] >= m["level"][q]].sum() / S[-1]
        assert held >= p and held - D[r] / S[-1] < p
    assert np.all(np.diff(m["level"]) <= 0) and np.all(np.diff(m["level_pos"]) >= 0)


def test_flag_rules():
    good = correlated_counts(10, 10, 200, 0.3, 5)
    e = (0.0, 1.0, 0.0, 2.0)
    assert kde2d_model(good, *e)["flag"] == 0
    one_row, one_col, diag = np.zeros_like(good), np.zeros_like(good), np.diag(np.arange(1, 11)).astype(np.int64)
    one_row[4], one_col[:, 7] = 3, 2
    single = np.zeros_like(good)
    single[2, 3] = 1
    for c in (one_row, one_col, diag, diag[::-1].copy(), single, np.zeros_like(good)):
        m = kde2d_model(c, *e, probs=(0.5,))
        assert m["flag"] == 2 and np.isnan(m["density"].astype(float)).all() and m["level_pos"][0] == -1
        assert np.isnan(m["bw"].astype(float)).all() and np.isnan(m["mode"]).all() and np.isnan(m["level"].astype(float)).all()
    for ends in ((1.0, 1.0, 0.0, 2.0), (0.0, 1.0, 2.0, 1.0), (0.0, np.inf, 0.0, 2.0), (np.nan, 1.0, 0.0, 2.0)):
        assert kde2d_model(good, *ends)["flag"] == 2
    # given H: a row or a diagonal is fine, N == 0 and a singular or improper H are not
    H = [0.04, 0.01, 0.09]
    assert kde2d_model(one_row, *e, rule="given", bw=H)["flag"] == 0 and kde2d_model(single, *e, rule="given", bw=H)["flag"] == 0
    assert kde2d_model(np.zeros_like(good), *e, rule="given", bw=H)["flag"] == 2
    for bad in ([0.04, 0.06, 0.09], [0.04, -0.06, 0.09], [0.0, 0.0, 1.0], [1.0, 0.0, -1.0], [np.inf, 0.0, 1.0], [1.0, np.nan, 1.0]):
        assert kde2d_model(good, *e, rule="given", bw=bad)["flag"] == 2, bad
    assert kde2d_model(good, *e, rule="given", bw=[0.04, 0.0599, 0.09])["flag"] == 0  # (correlation 0.998: inside)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_the_gpu_cases_are_out_of_roundings_reach(i):
    c, want, w64 = CASES[i], reference(i), reference(i, np.float64)
    good = want["flag"] == 0
    assert np.array_equal(want["flag"], w64["flag"]) and good.any()
    d, d64 = want["density"][good], w64["density"][good].astype(np.longdouble)
    err = float(np.max(np.abs(d64 - d) / np.maximum(np.abs(d), np.longdouble(1e-300))))
    print(c["name"], "fp64 against longdouble %.2e" % err, "margin %.2e" % want["margin"][good].min(), "gap %.2e" % want["gap"][good].min())
    assert err <= 1e-12
    assert np.array_equal(want["level_pos"], w64["level_pos"]) and np.array_equal(want["mode_index"], w64["mode_index"])
    assert want["margin"][good].min() > 1e-9, want["margin"]
    assert want["gap"][good].min() > 1e-9


@pytest.mark.parametrize("name,g", [("24x20-dense-scott", 0), ("24x20-given-negative", 1), ("33x127-edge", 0), ("8x256-scott", 0)])
def test_the_completed_square_is_the_contracts_quadratic_form(name, g):
    """the restatement and the kernel evaluate q = A u^2 + 2 B u v + C v^2 as A (u + (B / A) v)^2 + v^2 / h_yy; here the contract's
    three terms are summed as written, at longdouble, with (A, B, C) = (h_yy, -h_xy, h_xx) / det H from the restatement's own H --
    on GPU cases of both signs of the correlation, up to 0.9 in size -- and must give the restatement's density within 1e-12
    (longdouble keeps 1e-19 of the largest term: the cancellation that costs fp64 its digits costs it nothing that shows)"""
    f = np.longdouble
    i = next(k for k, c in enumerate(CASES) if c["name"] == name)
    c, want = CASES[i], reference(i)
    assert want["flag"][g] == 0
    cnt = c["counts"][g]
    nx, ny = cnt.shape
    hxx, hxy, hyy = want["bw"][g]
    det = hxx * hyy - hxy * hxy
    A, B, C = hyy / det, -hxy / det, hxx / det
    dx, dy = (f(c["hi_x"][g]) - f(c["lo_x"][g])) / f(nx), (f(c["hi_y"][g]) - f(c["lo_y"][g])) / f(ny)
    K, L = np.arange(nx)[:, None], np.arange(ny)[None, :]
    acc = np.zeros((nx, ny), dtype=f)
    for a, b in zip(*np.nonzero(cnt)):
        u, v = (K - a).astype(f) * dx, (L - b).astype(f) * dy
        acc += f(int(cnt[a, b])) * np.exp(-(A * u * u + f(2) * B * u * v + C * v * v) / f(2))
    dens = acc / (f(int(cnt.sum())) * f(2) * np.arccos(f(-1)) * np.sqrt(det))
    err = float(np.max(np.abs(dens - want["density"][g]) / np.maximum(want["density"][g], f(1e-300))))
    print(name, g, "term by term against the completed square, longdouble: %.2e" % err, "correlation %.3f" % float(hxy / np.sqrt(hxx * hyy)))
    assert err <= 1e-12


def test_the_cases_cover_what_they_should():
    from kde2d_cases import MANY, RESIDENT_WORKGROUPS_MAX, edge_shapes, layout

    shapes = {c["counts"].shape[1:] for c in CASES}
    assert {(8, 8), (8, 256), (256, 8), (256, 256), (24, 20)} <= shapes and set(edge_shapes()) <= shapes
    # more grids than workgroups of four waves fit the device at 32 waves per CU, at one workgroup per grid in every kernel of the call
    assert {len(c["counts"]) for c in CASES} >= {1, 3, MANY} and MANY > RESIDENT_WORKGROUPS_MAX == 256 * 32 // 4
    many = next(c for c in CASES if len(c["counts"]) == MANY)
    L = layout(*many["counts"].shape[1:])
    assert L["tiles_x"] * L["tiles_y"] == 1 and L["threads"] == 4 * 64
    assert {layout(*s)["ry"] for s in shapes} == {1, 2} and max(layout(*s)["tiles_y"] for s in shapes) == 2
    signs = {int(np.sign(reference(i)["bw"][g, 1])) for i, c in enumerate(CASES) for g in range(len(c["counts"])) if reference(i)["flag"][g] == 0}
    assert signs >= {-1, 1}
    assert any(c["counts"].max() > 2**31 - 10 for c in CASES) and any(c["bw_fct"] != 1.0 for c in CASES)
    assert any((c["counts"].reshape(len(c["counts"]), -1) > 0).all(axis=1).any() for c in CASES)  # every cell non-empty
    flags = [reference(i)["flag"] for i in range(len(CASES))]
    assert any(len(f) == 3 and f[1] == 2 and f[0] == 0 and f[2] == 0 for f in flags)  # a degenerate grid between two good ones
