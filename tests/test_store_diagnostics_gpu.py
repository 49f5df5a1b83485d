"""Split R-hat and effective sample size of the device store (omc_store_rhat_ess, Engine.store_rhat_ess,
MCMC.diagnostics) against a plain-numpy restatement of the definitions in include/omcmc_hip.h, against known answers,
at the edges of the contract, and through the public API."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-9


# ---------------------------------------------------------------------------------------------------------- restatement
def restate(x):
    """(rhat, ess, lags) of a host store x (N, C, size): the definitions, element by element, autocovariances by direct
    sums.  Series means are taken around the series' first draw and the variance of the means around the first mean, so
    that constant series and equal means come out exactly (the contract's edge cases are exact tests)."""
    N, C, size = x.shape
    M, J = N // 2, 2 * C
    rhat, ess, lags = np.empty(size), np.empty(size), np.zeros(size, dtype=np.int32)
    for k in range(size):
        if np.isnan(x[:, :, k]).any():
            rhat[k] = ess[k] = np.nan
            continue
        xs = np.concatenate([x[:M, :, k].T, x[N - M:, :, k].T])  # (J, M)
        if np.all(xs == xs[0, 0]):
            rhat[k], ess[k] = np.nan, J * M
            continue
        m = xs[:, :1] + (xs - xs[:, :1]).mean(axis=1, keepdims=True)
        y = xs - m
        cache = {}

        def gbar(t):  # mean_j g_j(t)
            if t not in cache:
                cache[t] = np.sum(y[:, :M - t] * y[:, t:]) / (J * M)
            return cache[t]

        W = gbar(0) * M / (M - 1)
        d = m[:, 0] - m[0, 0]
        B_M = np.sum((d - d.mean()) ** 2) / (J - 1)
        var_plus = W * (M - 1) / M + B_M
        with np.errstate(divide="ignore"):
            rhat[k] = np.sqrt(var_plus / W)

        def rho(t):
            return 1.0 - (W - gbar(t)) / var_plus

        r = np.zeros(M)
        r[0] = 1.0
        even, odd = 1.0, rho(1)
        r[1] = odd
        t = 1
        while t < M - 3 and even + odd > 0:
            even, odd = rho(t + 1), rho(t + 2)
            if even + odd >= 0:
                r[t + 1], r[t + 2] = even, odd
            t += 2
        max_t = t - 2
        if even > 0:
            r[max_t + 1] = even
        t = 1
        while t <= max_t - 2:
            if r[t + 1] + r[t + 2] > r[t - 1] + r[t]:
                r[t + 1] = r[t + 2] = (r[t - 1] + r[t]) / 2
            t += 2
        tau = -1 + 2 * np.sum(r[:max_t + 1]) + r[max_t + 1]
        tau = max(tau, 1 / np.log10(J * M))
        ess[k] = J * M / tau
        lags[k] = max_t + 1
    return rhat, ess, lags


def ar1(N, C, phis, seed, mu=None):
    """seeded stationary AR(1) store (N, C, len(phis)), one coefficient per element"""
    rng = np.random.default_rng(seed)
    phis = np.asarray(phis, dtype=float)
    x = np.empty((N, C, phis.size))
    x[0] = rng.standard_normal((C, phis.size))
    s = np.sqrt(1 - phis ** 2)
    for n in range(1, N):
        x[n] = phis * x[n - 1] + s * rng.standard_normal((C, phis.size))
    return x if mu is None else x + mu


def phis_for(size, hi=0.95):
    return np.linspace(-0.7, hi, size)


def device(eng, x):
    return eng.to_device(np.ascontiguousarray(x))


def run(eng, x):
    rhat, ess, lags = eng.store_rhat_ess(device(eng, x))
    return rhat.cpu().numpy(), ess.cpu().numpy(), lags.cpu().numpy()


def assert_matches(got, want, rtol=RTOL):
    (r1, e1, l1), (r2, e2, l2) = got, want
    np.testing.assert_allclose(r1, r2, rtol=rtol, atol=0, equal_nan=True)
    np.testing.assert_allclose(e1, e2, rtol=rtol, atol=0, equal_nan=True)
    assert np.array_equal(l1, l2), (l1, l2)


def engine(C, **options):
    from openmcmc_amd.engine import Engine

    eng = Engine(C, seed=1)
    for name, value in options.items():
        eng.set_option(name, value)
    return eng


# ---------------------------------------------------------------------------------------------------------- 1. restatement
@pytest.mark.parametrize("shape", [(4, 1, 1), (5, 3, 7), (8, 2, 3), (9, 4, 5), (11, 2, 6), (64, 8, 33), (257, 16, 130),
                                   (1000, 32, 40)])
def test_matches_restatement(shape):
    N, C, size = shape
    x = ar1(N, C, phis_for(size), seed=N * 7 + size)
    eng = engine(C)
    assert_matches(run(eng, x), restate(x))
    eng.close()


def test_elements_that_stop_in_later_lag_blocks():
    N, C, size = 300, 4, 70
    x = ar1(N, C, phis_for(size, hi=0.98), seed=11)
    eng = engine(C)
    got, want = run(eng, x), restate(x)
    assert_matches(got, want)
    assert want[2].max() > 32, want[2]  # some elements need the second block of 32 lags
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 2. known answers
def test_iid_chains():
    C, N = 64, 2000
    x = np.random.default_rng(3).standard_normal((N, C, 6))
    eng = engine(C)
    rhat, ess, _ = run(eng, x)
    assert np.all(np.abs(rhat - 1) < 0.01), rhat
    assert 0.9 <= np.mean(ess / (C * N)) <= 1.1, ess / (C * N)
    eng.close()


def test_ar1_ess_known_answer():
    C, N, phi = 64, 2000, 0.9
    x = ar1(N, C, [phi] * 4, seed=5)
    eng = engine(C)
    _, ess, _ = run(eng, x)
    want = C * N * (1 - phi) / (1 + phi)
    assert np.all(np.abs(ess / want - 1) < 0.15), ess / want
    eng.close()


def test_offset_chains_have_large_rhat():
    C, N = 8, 400
    x = np.random.default_rng(6).standard_normal((N, C, 3)) + 3.0 * np.arange(C)[None, :, None]
    eng = engine(C)
    rhat, _, _ = run(eng, x)
    assert np.all(rhat > 1.5), rhat
    eng.close()


def test_split_is_applied():
    """Each chain at -1 for its first half and +1 for its second: all chain means agree (a non-split R-hat is about 1),
    the split halves do not."""
    C, N = 8, 400
    x = np.random.default_rng(7).standard_normal((N, C, 3))
    x[: N // 2] -= 1.0
    x[N // 2:] += 1.0
    eng = engine(C)
    rhat, _, _ = run(eng, x)
    assert np.all(rhat > 1.1), rhat
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("N", [9, 128, 301])
def test_constant_and_constant_per_chain_elements(N):
    C, size = 3, 5
    x = ar1(N, C, phis_for(size), seed=N)
    x[:, :, 1] = 2.5                                          # every draw equal
    x[:, :, 3] = 0.1 * np.arange(C)[None, :]                  # every series constant, the series differ
    eng = engine(C)
    got = run(eng, x)
    rhat, ess, lags = got
    M, J = N // 2, 2 * C
    assert np.isnan(rhat[1]) and ess[1] == J * M and lags[1] == 0
    assert rhat[3] == np.inf and np.isfinite(ess[3])
    assert_matches(got, restate(x))
    eng.close()


@pytest.mark.parametrize("N", [9, 130, 301])
def test_nan_draws_poison_their_element_only(N):
    C, size = 4, 6
    x = ar1(N, C, phis_for(size), seed=N + 1)
    x[N // 3, 2, 3] = np.nan
    if N % 2:
        x[N // 2, 1, 5] = np.nan  # the middle draw: dropped from the series, still a draw of the element
    eng = engine(C)
    got = run(eng, x)
    nan_el = [3, 5] if N % 2 else [3]
    assert np.all(np.isnan(got[0][nan_el])) and np.all(np.isnan(got[1][nan_el]))
    rest = [k for k in range(size) if k not in nan_el]
    assert np.all(np.isfinite(got[0][rest])) and np.all(np.isfinite(got[1][rest]))
    assert_matches(got, restate(x))
    eng.close()


def test_three_iterations_are_refused():
    eng = engine(2)
    with pytest.raises(ValueError):
        eng.store_rhat_ess(device(eng, np.zeros((3, 2, 4))))
    eng.close()


def test_slowly_mixing_element_over_several_lag_blocks():
    N, C = 4000, 4
    x = ar1(N, C, [0.995, 0.9, 0.5], seed=13)
    eng = engine(C)
    got, want = run(eng, x), restate(x)
    assert_matches(got, want)
    assert want[2][0] > 64, want[2]
    eng.close()


def test_forced_forms_agree():
    N, C, size = 128, 16, 50
    x = ar1(N, C, phis_for(size), seed=17)
    x[:, :, 7] = -1.25
    x[40, 3, 9] = np.nan
    short, blocks = engine(C, diag_algo=1), engine(C, diag_algo=2)
    a, b = run(short, x), run(blocks, x)
    assert_matches(a, b, rtol=1e-12)
    assert_matches(a, restate(x))
    long_x = ar1(130, C, phis_for(4), seed=1)  # M = 65: beyond the short-series form
    with pytest.raises(ValueError):
        short.store_rhat_ess(device(short, long_x))
    short.close()
    blocks.close()


# ---------------------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("shape", [(128, 16, 50), (257, 16, 130), (300, 4, 70)])
def test_repeat_is_bit_equal_and_store_untouched(shape):
    N, C, size = shape
    x = ar1(N, C, phis_for(size, hi=0.98), seed=19)
    eng = engine(C)
    d = device(eng, x)
    before = d.clone()
    outs = [[t.cpu().numpy() for t in eng.store_rhat_ess(d)] for _ in range(2)]
    for u, v in zip(*outs):
        assert u.tobytes() == v.tobytes()
    assert d.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 5. public API
def store_of(out, key):
    """(n_iter, C, size) host array of a collect() entry"""
    arr = out[key] if key != "log_post" else np.transpose(out[key], (0, 2, 1))  # (C, size, n_iter)
    return np.ascontiguousarray(np.transpose(arr, (2, 0, 1)))


def test_mcmc_diagnostics_gmrf(golden):
    from test_mcmc_api_gpu import build

    G = golden("gmrf_chain")
    M, _ = build(G, "sparse_", True, 6, fuse=True, n_burn=5, n_iter=300, seed=5)
    M.run_mcmc()
    out = M.collect()
    for key in ("b", "lambda", "log_post"):
        x = store_of(out, key)
        rhat, ess, _ = restate(x)
        got = M.diagnostics(key)
        np.testing.assert_allclose(got["rhat"], rhat, rtol=RTOL, atol=0)
        np.testing.assert_allclose(got["ess"], ess, rtol=RTOL, atol=0)
        sd = x.reshape(x.shape[0] * x.shape[1], -1).std(axis=0, ddof=1)
        np.testing.assert_allclose(got["mcse_mean"], sd / np.sqrt(ess), rtol=1e-8, atol=0)
        assert got["rhat"].shape == got["ess"].shape == got["mcse_mean"].shape == (x.shape[2],)


def test_mcmc_diagnostics_variable_size(golden):
    from test_rj_chain_gpu import run_with_tape

    G = golden("rj_gmrf_chain")
    chains = np.arange(G["init_k"].shape[0])
    M, _, _ = run_with_tape(G, chains, int(G["n_iter"]))
    M.run_mcmc()
    out = M.collect()
    for key in ("theta", "beta"):
        x = store_of(out, key)
        has_nan = np.isnan(x).any(axis=(0, 1))
        got = M.diagnostics(key)
        assert np.array_equal(np.isnan(got["ess"]), has_nan) and np.all(np.isnan(got["rhat"][has_nan]))
        rhat, ess, _ = restate(x)
        np.testing.assert_allclose(got["rhat"], rhat, rtol=RTOL, atol=0, equal_nan=True)
        np.testing.assert_allclose(got["ess"], ess, rtol=RTOL, atol=0, equal_nan=True)
