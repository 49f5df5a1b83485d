"""A workspace of the context that grows inside a live context (omc_ensure, omc_common.h): the call at a small size, the same call
at a larger size -- the buffer is freed and allocated anew under the stream -- and the small size again, every result bit for bit
what the same call gives on a fresh Engine.  The library promises "same call twice, same bits", and kernel, launch geometry and
(for rocSOLVER) batch count and order do not depend on what the context held before: equality, no tolerance.  Three chains,
injected draws."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
C = 3


def make_engine(options=()):
    from openmcmc_amd.engine import Engine

    eng = Engine(C, seed=5)
    for name, value in options:
        eng.set_option(name, value)
    return eng


def dense_call(eng, p):
    rng = np.random.default_rng(100 + p)
    A = rng.standard_normal((p, p))
    G = A @ A.T / p + np.eye(p)
    terms = [{"mat": eng.to_device(G), "rhs": eng.to_device(rng.standard_normal(p)), "scale": eng.to_device(0.5 + rng.random(C))},
             {"scale": eng.to_device(0.1 + rng.random(C))}]
    x, mean, logdet = eng.empty(C, p), eng.empty(C, p), eng.empty(C)
    eng.dense_sample_canonical(p, terms, x, z=eng.to_device(rng.standard_normal((C, p))),
                               rhs_chain=eng.to_device(rng.standard_normal((C, p))), mean_out=mean, logdet_out=logdet)
    return x, mean, logdet


def tridiag_call(eng, n):
    rng = np.random.default_rng(200 + n)
    d = np.full(n, 2.0)
    d[0] = d[-1] = 1.0 + 1e-3
    y = rng.standard_normal(n)
    terms = [{"diag": eng.to_device(d), "off": eng.to_device(-np.ones(n - 1)), "scale": eng.to_device(5 + 10 * rng.random(C))},
             {"rhs": eng.to_device(y), "center": eng.to_device(y), "scale": eng.to_device(0.5 + rng.random(C))}]
    x = eng.empty(C, n)
    eng.tridiag_sample_canonical(n, terms, x, z=eng.to_device(rng.standard_normal((C, n))))
    return (x,)


def mala_call(eng, d):
    import torch

    rng = np.random.default_rng(300 + d)
    A = rng.standard_normal((d, d))
    Q = A @ A.T / d + np.eye(d)
    step = 0.7
    eng.mh_invalidate()  # nothing cached from the order before
    L, sl = eng.dense_cholesky(eng.to_device(Q), 1.0 / step**2)
    x = eng.to_device(rng.standard_normal((C, d)))
    acc, prop = (torch.zeros(C, dtype=torch.int64, device="cuda") for _ in range(2))
    lp = eng.empty(C)
    mu = eng.to_device(rng.standard_normal(d))
    for i in range(2):  # the second step finds the state's whitened image cached
        eng.mala_step_white(mu, L, sl, step, x, state_is_current=i > 0, z=eng.to_device(rng.standard_normal((C, d))),
                            u=eng.to_device(rng.random(C)), accept_count=acc, proposal_count=prop, log_p_out=lp)
    return x, lp, acc, prop


def moments_call(eng, shape):
    rng = np.random.default_rng(400 + shape[0])
    return eng.store_moments(eng.to_device(rng.standard_normal(shape)))


CASES = {
    # dense_factor and dense_info grow (rocSOLVER's factorisation below "dense_blocked_min")
    "dense": (dense_call, 8, 40, ()),
    # the blocked factorisation from order 1: dense_winv is allocated, p = 70 reaches the second panel
    "dense_blocked": (dense_call, 8, 70, (("dense_blocked_min", 1),)),
    # the serial kernel's `workspace`
    "tridiag_serial": (tridiag_call, 8, 40, (("tridiag_algo", 1),)),
    # white.prep and white.a
    "mala_white": (mala_call, 3, 9, ()),
    # store_ws
    "store_moments": (moments_call, (4, C, 2), (16, C, 5), ()),
}


@pytest.mark.parametrize("case", list(CASES))
def test_grown_workspace_gives_the_bits_of_a_fresh_context(case):
    call, small, large, options = CASES[case]

    def bits(eng, size):
        out = call(eng, size)
        eng.check_status()
        return [t.cpu().numpy().copy() for t in out]

    fresh = {}
    for size in (small, large):
        eng = make_engine(options)
        fresh[size] = bits(eng, size)
        eng.close()
    live = make_engine(options)
    for size in (small, large, small):
        got = bits(live, size)
        assert len(got) == len(fresh[size])
        for k, (a, b) in enumerate(zip(got, fresh[size])):
            assert a.shape == b.shape and np.all(np.isfinite(a.astype(np.float64))), (case, size, k)
            assert np.array_equal(a, b), (case, size, k, np.abs(a - b).max())
    live.check_status()
    live.close()
