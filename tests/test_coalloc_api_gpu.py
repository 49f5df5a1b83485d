"""MCMC.coallocation and MCMC.partition on a small mixture-prior regression (K = 3, p = 40, 4 chains) run through
MCMC.run_mcmc, against the numpy restatement of coalloc_model.py applied to MCMC.collect(): array_equal counts and scores, the
number of labels read from the model's Categorical, and the errors of an entry that is no allocation."""

import numpy as np
import pytest
from coalloc_model import batches_of, canonical, coalloc, first_argmin, scores

pytestmark = pytest.mark.gpu

P, C, K, N_ITER = 40, 4, 3, 60


@pytest.fixture(scope="module")
def run():
    from normal_normal_models import mixture

    from openmcmc_amd.mcmc import MCMC

    mdl, st, samplers, _ = mixture("plain", P, C, np.random.default_rng(3), None)
    M = MCMC(st, samplers, model=mdl, n_burn=5, n_iter=N_ITER, n_chains=C, seed=2)
    M.run_mcmc()
    store = np.ascontiguousarray(np.transpose(np.asarray(M.collect()["allocation"]), (2, 0, 1)))  # (n_iter, C, p)
    assert store.shape == (N_ITER, C, P) and len(np.unique(store)) == K
    return M, store


@pytest.mark.parametrize("pooled", (True, False))
def test_coallocation_and_partition(run, pooled):
    M, store = run
    index = None if pooled else [5, 0, 39, 5, 17, 18, 19]
    Zs = batches_of(store, K, index, pooled)
    rows = N_ITER * (C if pooled else 1)
    ref = np.stack([coalloc(Z, K) for Z in Zs])
    out = M.coallocation("allocation", index=index, pooled=pooled)  # K from the Categorical's prob
    counts = out["counts"] if not pooled else out["counts"][None]
    assert out["rows"] == rows and out["counts"].dtype == np.int64 and np.array_equal(counts, ref)
    assert np.array_equal(out["prob"], out["counts"] / float(rows)) and not out["absent"].any()
    assert np.array_equal(M.coallocation("allocation", n_labels=K, index=index, pooled=pooled)["counts"], out["counts"])
    per = M.coallocation("allocation", index=index, pooled=pooled, per_label=True)
    assert np.array_equal(per["counts"].sum(axis=-3), out["counts"])
    assert np.array_equal(per["counts"] if not pooled else per["counts"][None], np.stack([coalloc(Z, K, per_label=True) for Z in Zs]))

    part = M.partition("allocation", index=index, pooled=pooled)
    sc = [scores(Z, c, rows) for Z, c in zip(Zs, ref)]
    best = [first_argmin(s) for s in sc]
    if pooled:
        assert np.array_equal(part["scores"], sc[0].reshape(N_ITER, C))
        it, ch = divmod(best[0][0], C)
        assert (part["iteration"], part["chain"], part["score"]) == (it, ch, best[0][1])
        assert np.array_equal(part["labels"], canonical(Zs[0][best[0][0]]))
    else:
        assert np.array_equal(part["scores"], np.stack(sc, axis=1))
        assert np.array_equal(part["iteration"], [b[0] for b in best]) and np.array_equal(part["chain"], np.arange(C))
        assert np.array_equal(part["score"], [b[1] for b in best])
        assert np.array_equal(part["labels"], np.stack([canonical(Z[b[0]]) for Z, b in zip(Zs, best)]))


def test_entries_that_are_no_allocation(run):
    M, store = run
    with pytest.raises(ValueError, match=r"not an allocation in \[0, 3\): element 0 "):
        M.coallocation("parameter", n_labels=K)          # a continuous entry
    first = int(np.flatnonzero((store == 2).any(axis=(0, 1)))[0])
    with pytest.raises(ValueError, match=rf"not an allocation in \[0, 2\): element {first} "):
        M.partition("allocation", n_labels=2)            # label 2 is no label of two
    with pytest.raises(ValueError, match="give n_labels"):
        M.coallocation("parameter")                     # no Categorical on this key
    with pytest.raises(ValueError, match="give n_labels"):
        M.partition("prior_precision_vector")
