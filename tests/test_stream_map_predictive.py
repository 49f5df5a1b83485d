"""The draw indices of the posterior-predictive noise (omc_store_project: (1 << 41) + it + (replicate << 44), purpose
"normal"; the field map in omc_common.h) laid out as Philox counters beside the conventions tests/test_stream_map.py lists:
they share no (c1, c2, c3) words with a sweep draw, a prior draw or each other, and stay below 2^48.  CPU only: the counters
come from tests/philox_model.py."""

import itertools

import philox_model as pm
import test_stream_map as sm

REPLICATES = range(16)


def predictive_draw(it, rep):
    return (1 << 41) + it + (rep << 44)


def test_predictive_draw_indices_fit_48_bits():
    assert max(predictive_draw(it, rep) for it in sm.T_VALS for rep in REPLICATES) < 1 << 48
    assert predictive_draw(sm.T_MAX - 1, 15) < 1 << 48


def test_predictive_draws_share_no_counter_with_other_draws_or_each_other():
    """Element j of the noise reads block j >> 1 of its counter, any block of the 32-bit word: two draws must differ in
    (c1, c2, c3) themselves."""
    others = set()
    for _, purpose, d, b0, _ in sm.draws():
        if purpose != "normal":
            continue  # (another purpose is another counter by bits 24-31 of c3: checked below on the words)
        for chain in sm.CHAIN_VALS:
            others.add(pm.counter("normal", d, chain, b0)[1:])
    assert len(others) > 1000
    mine = {}
    for it, rep, chain in itertools.product(sm.T_VALS, REPLICATES, sm.CHAIN_VALS):
        words = pm.counter("normal", predictive_draw(it, rep), chain)[1:]
        assert words not in others, (it, rep, chain)
        assert words not in mine, ((it, rep, chain), mine[words])
        mine[words] = (it, rep, chain)
    assert len(mine) == len(sm.T_VALS) * 16 * len(sm.CHAIN_VALS)
    # the purpose field keeps them apart from every gamma, uniform and raw draw whatever their draw index
    for purpose in ("gamma", "uniform", "raw"):
        for words in mine:
            assert (words[2] >> 24) != pm.PURPOSE[purpose]
