"""MCMC.kde and MCMC.mode on a small stored run (a regression: 5 coefficients and a precision, 4 chains, 64 stored iterations) against
the restatement of tests/kde_model.py applied to collect()'s host copy of the same store: grid and counts array_equal to
np.linspace / np.histogram, bandwidth, density and mode within the project's fp64 tolerance 1e-10, flags equal.  Then the claim
that the estimate is a function of the counts: the store in two halves of chains, counts over shared edges added, one
Engine.kde_binned call -- bit-equal to the call on the whole."""

import numpy as np
import pytest
from kde_model import kde_model
from scipy import sparse

pytestmark = pytest.mark.gpu

N, P, C, N_ITER = 30, 5, 4, 64


def build_regression():
    from openmcmc_amd.distribution.distribution import Gamma
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.mcmc import MCMC
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombination, ScaledMatrix
    from openmcmc_amd.sampler.sampler import NormalGamma, NormalNormal

    rng = np.random.default_rng(42)
    X = rng.standard_normal((N, P))
    y = X @ np.arange(1.0, P + 1) + 0.3 * rng.standard_normal(N)
    mdl = Model([Normal("y", mean=LinearCombination(form={"beta": "X"}), precision=ScaledMatrix(matrix="P_tau", scalar="tau")),
                 Normal("beta", mean="mu", precision=ScaledMatrix(matrix="P_lambda", scalar="lambda")),
                 Gamma("tau", shape="a_tau", rate="b_tau")], response={"y": "mean"})
    samplers = [NormalNormal("beta", mdl), NormalGamma("tau", mdl)]
    state = {"y": y, "X": X, "beta": [0.0] * P, "P_tau": sparse.csc_matrix(np.eye(N)), "tau": 1, "P_lambda": sparse.csc_matrix(np.eye(P)),
             "mu": [0.0] * P, "lambda": 0.01, "a_tau": 1e-3, "b_tau": 1e-3}
    return MCMC(state, samplers, model=mdl, n_burn=3, n_iter=N_ITER, n_chains=C, seed=5)


@pytest.fixture(scope="module")
def run():
    M = build_regression()
    M.run_mcmc()
    M.store["beta"][5::3, :, 2] = float("nan")  # a NaN-padded element, as a variable-size parameter leaves it
    M.store["beta"][:, :, 4] = 2.5              # ... and one that never moved
    yield M, M._store_3d("beta").cpu().numpy(), M._store_3d("tau").cpu().numpy()
    M.engine.close()


def close(got, want):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= 1e-10 * np.maximum(np.abs(want), np.longdouble(1e-300))))


def expected(x, cols, pooled, G, rule, bw=None, bw_fct=1.0, extend=0.1, bounds=(None, None)):
    """The definition of MCMC.kde on the host copy x (n_iter, C, size): (grid, counts, outside, model results)"""
    flat = x.reshape(-1, x.shape[2])
    edges, counts, outside = [], [], []
    for k in cols:
        col = flat[:, k]
        mn, mx = np.nanmin(col), np.nanmax(col)
        a, b = (mn - 0.5, mx + 0.5) if mn == mx else (mn - extend * (mx - mn), mx + extend * (mx - mn))
        a, b = (a if bounds[0] is None else float(bounds[0])), (b if bounds[1] is None else float(bounds[1]))
        edges.append(np.linspace(a, b, G + 1))
        sets = [col] if pooled else [x[:, c, k] for c in range(x.shape[1])]
        counts.append([np.histogram(s[~np.isnan(s)], G, (a, b))[0] for s in sets])
        outside.append([len(s) - np.histogram(s[~np.isnan(s)], G, (a, b))[0].sum() for s in sets])
    edges = np.array(edges)
    counts, outside = np.array(counts).swapaxes(0, 1), np.array(outside).swapaxes(0, 1)  # (chains or 1, n_idx, ..)
    if pooled:
        counts, outside = counts[0], outside[0]
    lead = counts.shape[:-1]
    given = None if bw is None else np.broadcast_to(bw, lead)
    m = kde_model(counts, np.broadcast_to(edges[:, 0], lead), np.broadcast_to(edges[:, -1], lead), rule, given, bw_fct,
                  (bounds[0] is not None, bounds[1] is not None))
    if rule in ("isj", "experimental"):  # the inputs must leave ISJ's choice of a root to no rounding
        good = m["flag"] != 2
        m64 = kde_model(counts, np.broadcast_to(edges[:, 0], lead), np.broadcast_to(edges[:, -1], lead), rule, given, bw_fct,
                        (bounds[0] is not None, bounds[1] is not None), dtype=np.float64)
        assert m["margin"][good].min() >= 1e-3 and np.array_equal(m["bracket"], m64["bracket"])
    grid = np.broadcast_to(0.5 * (edges[:, :-1] + edges[:, 1:]), lead + (G,))
    return grid, counts, outside, m


def check(got, x, cols, pooled, G, rule, **kw):
    grid, counts, outside, m = expected(x, cols, pooled, G, rule, **kw)
    assert np.array_equal(got["grid"], grid) and np.array_equal(got["n"], counts.sum(axis=-1)) and np.array_equal(got["outside"], outside)
    assert got["flag"].dtype == np.int32 and np.array_equal(got["flag"], m["flag"])
    good = m["flag"] != 2
    assert np.isnan(got["bw"][~good]).all() and np.isnan(got["mode"][~good]).all() and np.isnan(got["density"][~good]).all()
    assert close(got["bw"][good], m["bw"][good]) and close(got["mode"][good], m["mode"][good])
    assert close(got["density"][good], m["density"][good])
    return m


def test_pooled_and_per_chain_with_an_index_that_repeats(run):
    M, beta, tau = run
    back = np.array([3, 0, 3, 2, 4])
    for pooled in (True, False):
        rule = "experimental" if pooled else "silverman"  # (the default rule pooled; a chain's 64 draws are few for ISJ)
        got = M.kde("beta", index=back, pooled=pooled, grid_len=64) if pooled else M.kde("beta", index=back, pooled=False, grid_len=64, bw=rule)
        lead = (5,) if pooled else (C, 5)
        assert got["density"].shape == lead + (64,) and got["bw"].shape == lead
        m = check(got, beta, back, pooled, 64, rule)
        assert np.all(m["flag"][..., 4] == 2) and np.all(m["flag"][..., :4] != 2)  # the element that never moved
        assert np.array_equal(got["density"][..., 0, :], got["density"][..., 2, :])  # the repeat
        assert np.array_equal(M.mode("beta", index=back, pooled=pooled, grid_len=64, bw=rule), got["mode"], equal_nan=True)
        # the NaN draws of element 2 are left out and reported
        nans = np.isnan(beta[:, :, 2]).sum() if pooled else np.isnan(beta[:, :, 2]).sum(axis=0)
        assert np.array_equal(got["outside"][..., 3], nans) and np.all(got["outside"][..., :3] == 0)
    # all elements, the default grid, another rule
    check(M.kde("beta", bw="silverman"), beta, np.arange(P), True, 512, "silverman")
    check(M.kde("beta", bw="scott", bw_fct=1.5, extend=0.25, grid_len=100), beta, np.arange(P), True, 100, "scott", bw_fct=1.5, extend=0.25)


def test_a_bound_and_given_bandwidths(run):
    M, beta, tau = run
    got = M.kde("tau", bounds=(0, None), grid_len=128, bw="isj")
    check(got, tau, [0], True, 128, "isj", bounds=(0, None))
    assert 0 < got["grid"][0, 0] < got["grid"][0, 1] - got["grid"][0, 0]  # the first bin starts at the bound
    upper = float(np.quantile(tau, 0.9))  # an upper bound inside the draws: what lies beyond is left out and counted
    got = M.kde("tau", bounds=(0, upper), grid_len=64, bw="silverman", pooled=False)
    check(got, tau, [0], False, 64, "silverman", bounds=(0, upper))
    assert got["outside"].sum() == (tau > upper).sum() > 0
    sd = float(np.nanstd(beta[:, :, 0]))
    check(M.kde("beta", bw=0.3 * sd, grid_len=64), beta, np.arange(P), True, 64, "given", bw=0.3 * sd)
    widths = sd * np.array([0.2, 0.3, 0.4, 0.5])
    for pooled in (True, False):
        got = M.kde("beta", index=[0, 1, 2, 3], bw=widths, bw_fct=0.5, grid_len=65, pooled=pooled)
        check(got, beta, [0, 1, 2, 3], pooled, 65, "given", bw=widths, bw_fct=0.5)
        assert np.array_equal(got["bw"], np.broadcast_to(0.5 * widths, got["bw"].shape))
    with pytest.raises(ValueError):
        M.kde("beta", grid_len=7)
    with pytest.raises(ValueError):
        M.kde("beta", bw="no such rule")
    with pytest.raises(ValueError):
        M.kde("tau", bounds=(1e9, None))
    M.store["tau"][3, 1] = float("inf")
    try:
        with pytest.raises(ValueError, match="not finite"):
            M.kde("tau")
    finally:
        M.store["tau"][3, 1] = float(tau[3, 1, 0])


def test_counts_of_two_halves_of_the_chains_add_up_to_the_whole(run):
    """what a sharded run does: every rank counts its own chains over the same edges, the counts are added, one call"""
    import torch

    from openmcmc_amd.engine import Engine

    M, beta, tau = run
    G = 128
    store = M._store_3d("beta")
    lo, hi = beta[:, :, :4].reshape(-1, 4).min(axis=0) - 0.3, beta[:, :, :4].reshape(-1, 4).max(axis=0) + 0.3
    lo, hi = np.where(np.isnan(lo), np.nanmin(beta[:, :, 2]) - 0.3, lo), np.where(np.isnan(hi), np.nanmax(beta[:, :, 2]) + 0.3, hi)
    edges = np.stack([np.linspace(a, b, G + 1) for a, b in zip(lo, hi)])
    idx = [0, 1, 2, 3]
    whole, _ = M.engine.store_histogram(store, edges, index=idx)
    half = Engine(C // 2, seed=1)
    parts = [half.store_histogram(store[:, r * (C // 2):(r + 1) * (C // 2)].contiguous(), edges, index=idx)[0] for r in range(2)]
    added = parts[0] + parts[1]
    assert torch.equal(added, whole)
    for rule in ("experimental", "scott"):
        a = M.engine.kde_binned(whole, lo, hi, rule=rule)
        b = half.kde_binned(added, lo, hi, rule=rule)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert (a[3] == 0).all()
    half.close()
