"""LinearCombinationWithTransform on host values (no GPU): the class mirrors the reference's (parameter.py:231-297), its host
predictor reproduces tests/golden/transform_parameter.npz, all-False transforms are LinearCombination, and the routes that would
have to drop the exp say so."""

import dataclasses

import numpy as np
import pytest
from scipy import sparse


def _state(G, tag, k):
    A = G[f"{tag}_A"]
    p = A.shape[1]
    return {"A": sparse.csc_matrix(A) if G[f"{tag}_sparse_A"] else A, "B": G[f"{tag}_B"], "s": G[f"{tag}_S"][k].reshape(p, 1),
            "g": G[f"{tag}_g"].reshape(-1, 1), "y": G[f"{tag}_y"]}


def _mean(G, tag):
    from openmcmc_amd.parameter import LinearCombinationWithTransform

    form, transform = {"s": "A"}, {"s": bool(G[f"{tag}_tr_s"])}
    if G[f"{tag}_second"]:
        form["g"], transform["g"] = "B", False
    return LinearCombinationWithTransform(form=form, transform=transform)


def test_class_mirrors_the_reference():
    from openmcmc_amd.parameter import LinearCombination, LinearCombinationWithTransform

    assert issubclass(LinearCombinationWithTransform, LinearCombination)
    assert [f.name for f in dataclasses.fields(LinearCombinationWithTransform)] == ["form", "transform"]
    par = LinearCombinationWithTransform(form={"beta": "X", "gamma": "Y"}, transform={"beta": True, "gamma": False})
    assert par.get_param_list() == ["beta", "gamma", "X", "Y"]
    assert par.get_grad_param_list() == ["beta", "gamma"]
    for name in ("predictor", "predictor_conditional", "grad", "get_param_list", "get_grad_param_list"):
        assert callable(getattr(par, name))


@pytest.mark.parametrize("tag", ["all", "none", "mixed", "sparseA", "nrep3", "scaled"])
def test_host_predictor_matches_the_reference(golden, tag):
    G = golden("transform_parameter")
    mean = _mean(G, tag)
    for k in range(3):
        st = _state(G, tag, k)
        np.testing.assert_allclose(np.asarray(mean.predictor(st)).ravel(), G[f"{tag}_pred"][k], rtol=1e-14, atol=0)
        cond = np.asarray(mean.predictor_conditional(st, term_to_exclude="s")).ravel() * np.ones(G[f"{tag}_A"].shape[0])
        np.testing.assert_allclose(cond, G[f"{tag}_pred_cond"][k], rtol=1e-14, atol=0)
        grad = mean.grad(st, "s")
        grad = grad.toarray() if sparse.issparse(grad) else np.asarray(grad)
        np.testing.assert_allclose(grad, G[f"{tag}_grad"][k], rtol=1e-14, atol=0)


def test_all_false_transforms_are_linear_combination(golden):
    from openmcmc_amd.parameter import LinearCombination, LinearCombinationWithTransform

    G = golden("transform_parameter")
    st = _state(G, "none", 1)
    plain = LinearCombination({"s": "A", "g": "B"})
    tr = LinearCombinationWithTransform(form={"s": "A", "g": "B"}, transform={"s": False, "g": False})
    assert np.array_equal(tr.predictor(st), plain.predictor(st))
    assert np.array_equal(tr.predictor_conditional(st, "g"), plain.predictor_conditional(st, "g"))
    assert not tr.is_transformed()


def test_guards_raise():
    torch = pytest.importorskip("torch")
    from openmcmc_amd.chains import ChainArray
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.parameter import LinearCombinationWithTransform

    mean = LinearCombinationWithTransform(form={"s": "A", "g": "B"}, transform={"s": True, "g": False})
    chain = ChainArray(torch.zeros(2, 3, 1, dtype=torch.float64))
    st = {"A": np.eye(3), "B": np.ones((3, 1)), "s": chain, "g": np.ones((1, 1))}
    with pytest.raises(NotImplementedError):   # host sums must never drop the exp of a per-chain term
        mean.predictor_conditional(st)
    with pytest.raises(NotImplementedError):
        mean.grad(st, "s")
    lik = Normal("y", mean=mean, precision="W")
    assert lik.constant_hessian("s") is False and lik.constant_hessian("g") is True
    assert mean.resid_sq_device(st, None, None) is None
