"""The exact model of omc_store_ess_indicator (tests/essq_model.py: integers and Fractions) against the centred fp64 definition of
omc_store_rhat_ess applied to the 0/1 series as plain numpy, on the inputs of the GPU tests (tests/essq_cases.py) -- and the condition
on those inputs under which a device result may be held to the model at all: no decision of Geyer's sequence is taken on a pair
sum closer to zero than 1e-9, so that the few roundings of the device's fp64 steps cannot flip one.  No GPU needed."""

import numpy as np
import pytest
from essq_cases import cases, model
from essq_model import indicator_fp64, split_series

NAMES = [c["name"] for c in cases()]


@pytest.mark.parametrize("name", NAMES)
def test_exact_model_matches_the_centred_fp64_definition(name):
    c = next(k for k in cases() if k["name"] == name)
    m = model(name)
    idx = np.arange(c["x"].shape[2]) if c["idx"] is None else c["idx"]
    for k in range(0, idx.size, 7 if name == "large" else 1):  # (the large store: every seventh element)
        if m["dead"][k]:
            continue
        xs = split_series(c["x"][:, :, idx[k]])
        for p in range(c["hi"].size):
            ess, lags = indicator_fp64(xs, c["lo"][p], c["hi"][p])
            assert lags == m["lags"][p, k], (name, k, p)
            np.testing.assert_allclose(ess, m["ess"][p, k], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_no_decision_of_the_gpu_cases_is_marginal(name):
    m = model(name)
    print(name, "smallest |even + odd| at a decision:", m["margin"])
    assert m["margin"] > 1e-9


def test_the_cases_reach_the_paths_they_are_meant_for():
    c, m = {k["name"]: k for k in cases()}, {n: model(n) for n in NAMES}
    assert sorted(k["x"].shape[0] // 2 for k in cases() if k["name"].startswith("edge")) == [63, 64, 65, 127, 128, 129]
    assert m["slow"]["lags"].max() > 192 and (m["slow"]["lags"] > 128).sum() >= 2  # blocks q >= 2, with their lane r == 0
    assert m["large"]["lags"].max() > 128
    M = c["trend"]["x"].shape[0] // 2
    assert np.all(m["trend"]["lags"][:2] == 2 * ((M - 3) // 2))  # the M - 3 limit
    assert m["trend"]["counts"][1, 0, 1] == 2 * M * M and m["trend"]["counts"][1, 0, 0] == 2 * M  # p = 0.5: two series of ones
    JM = 2 * c["ends"]["x"].shape[1] * (c["ends"]["x"].shape[0] // 2)
    assert np.all(m["ends"]["ess"][[1, 2]] == JM) and np.all(m["ends"]["lags"][[1, 2]] == 0)  # prob 1 and (0, 1): all ones
    lev = m["levels"]
    assert np.all(lev["counts"][0, :, 0] == 40) and np.all(lev["lags"][0] == 2 * ((20 - 3) // 2))  # W == 0 < B_M runs to the limit
    ties = c["ties"]["x"]
    assert np.unique(ties).size < 40  # many ties
    assert c["32-intervals"]["hi"].size == 32 and c["one-interval"]["hi"].size == 1
    assert m["non-finite"]["dead"].tolist() == [False, True, False, True, False]
