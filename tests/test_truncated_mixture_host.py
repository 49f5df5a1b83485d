"""Host-side rules of truncated mixture priors (no GPU): which limits a variable-size parameter takes, and the error that
names the parameter when it gets one limit per element."""

import numpy as np
import pytest


def _mixture_model(**limits):
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombination, MixtureParameterMatrix, MixtureParameterVector, ScaledMatrix

    return Model([
        Normal("y", mean=LinearCombination({"beta": "B"}), precision=ScaledMatrix("P", "tau")),
        Normal("beta", mean=MixtureParameterVector("mu", "alloc"), precision=MixtureParameterMatrix("prec", "alloc"), **limits),
    ])


def test_scalar_domain_limits():
    mdl = _mixture_model(domain_response_lower=np.array([[0.0]]))
    assert mdl["beta"].scalar_domain_limits() == (0.0, np.inf)
    mdl = _mixture_model(domain_response_upper=np.array([[2.5]]))
    assert mdl["beta"].scalar_domain_limits() == (-np.inf, 2.5)
    mdl = _mixture_model(domain_response_lower=np.array([[0.0], [1.0]]))
    assert mdl["beta"].scalar_domain_limits() is None


def test_ragged_limits_of_the_sampler():
    from openmcmc_amd.sampler.sampler import NormalNormal

    nn = NormalNormal("beta", _mixture_model(domain_response_lower=np.array([[0.0]])))
    assert nn._ragged_limits(nn.model["beta"]) == (0.0, np.inf)
    assert NormalNormal("beta", _mixture_model())._ragged_limits(_mixture_model()["beta"]) is None
    both_open = _mixture_model(domain_response_lower=np.array([[-np.inf]]))
    assert NormalNormal("beta", both_open)._ragged_limits(both_open["beta"]) is None
    bad = _mixture_model(domain_response_lower=np.array([[1.0]]), domain_response_upper=np.array([[1.0]]))
    with pytest.raises(ValueError, match="strictly less"):
        NormalNormal("beta", bad)._ragged_limits(bad["beta"])


def test_per_element_limits_on_a_ragged_parameter_name_it():
    from openmcmc_amd.sampler.sampler import NormalNormal

    mdl = _mixture_model(domain_response_lower=np.array([[0.0], [1.0]]))
    with pytest.raises(ValueError, match="beta: a variable-size parameter takes scalar domain limits only"):
        NormalNormal("beta", mdl)._ragged_limits(mdl["beta"])
