"""CPU tests of the host side above the C ABI: state coercion, model algebra, structure
recognition, the RW1 builders (bit-exact against the reference's output) and sharding."""

import numpy as np
import pytest
from scipy import sparse

from openmcmc_amd import gmrf
from openmcmc_amd.chains import host_2d
from openmcmc_amd.distribution.distribution import Gamma
from openmcmc_amd.distribution.location_scale import Normal, tridiagonal_bands
from openmcmc_amd.model import Model
from openmcmc_amd.parallel import shard_chains, store_to_reference_layout
from openmcmc_amd.parameter import Identity, LinearCombination, ScaledMatrix, _is_identity


@pytest.mark.parametrize("n", [1, 2, 5, 40])
def test_precision_irregular_matches_reference(golden, n):
    G = golden("precision_builders")
    P = gmrf.precision_irregular(G[f"irr{n}_s"])
    P = P.toarray() if sparse.issparse(P) else np.asarray(P, dtype=float)
    assert np.array_equal(P, G[f"irr{n}_P"])
    assert np.array_equal(np.asarray(gmrf.precision_irregular(G[f"irr{n}_s"], is_sparse=False), dtype=float), G[f"irr{n}_P"])
    if n > 1:  # reference test_precision: symmetric, rows sum to zero
        assert np.allclose(P, P.T) and np.allclose(P.sum(1), 0)


def test_precision_temporal_matches_reference(golden):
    import pandas as pd

    G = golden("precision_builders")
    t = pd.date_range(start="2022-04-01T01:00:00", end="2022-04-01T01:01:00", periods=30)
    assert np.array_equal(gmrf.precision_temporal(t).toarray(), G["temporal_P"])
    assert np.array_equal(gmrf.precision_temporal(t, unit_length=30.0).toarray(), G["temporal_P_unit30"])


def test_state_coercion_like_reference():
    """mcmc.py:69-76: scalars -> (1,1), lists and 1-D arrays -> columns, 2-D untouched."""
    assert host_2d(3).shape == (1, 1) and host_2d(3).dtype == np.float64
    assert host_2d([1, 2, 3]).shape == (3, 1)
    assert host_2d(np.arange(4.0)).shape == (4, 1)
    a = np.ones((2, 3))
    assert host_2d(a) is a


def test_tridiagonal_bands():
    n = 6
    P = sparse.diags((-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)), offsets=[-1, 0, 1], format="csc")
    d, o = tridiagonal_bands(P, n)
    assert np.array_equal(d, 2 * np.ones(n)) and np.array_equal(o, -np.ones(n - 1))
    assert tridiagonal_bands(sparse.identity(n, format="csc"), n) == (None, None)
    d, o = tridiagonal_bands(np.diag(np.arange(1.0, n + 1)), n)
    assert o is None and np.array_equal(d, np.arange(1.0, n + 1))
    wide = P.toarray()
    wide[0, 3] = wide[3, 0] = 0.5
    assert tridiagonal_bands(wide, n) is None
    asym = P.toarray()
    asym[0, 1] = 7.0
    with pytest.raises(ValueError):
        tridiagonal_bands(asym, n)
    assert _is_identity(sparse.identity(n), n) and not _is_identity(P, n)


def example4_model():
    return Model([
        Normal("y", mean="b", precision=ScaledMatrix(matrix="P_tau", scalar="tau")),
        Normal("b", mean="mu", precision=ScaledMatrix(matrix="P_lambda", scalar="lambda")),
        Gamma("lambda", shape="a_lam", rate="b_lam"),
        Gamma("tau", shape="a_tau", rate="b_tau"),
    ])


def test_model_conditional_membership():
    """model.py:41-55 and tests/test_distribution.py:253-270 of the reference."""
    mdl = example4_model()
    assert list(mdl.keys()) == ["y", "b", "lambda", "tau"]
    assert set(mdl.conditional("b").keys()) == {"y", "b"}
    assert set(mdl.conditional("lambda").keys()) == {"b", "lambda"}
    assert set(mdl.conditional("tau").keys()) == {"y", "tau"}
    assert mdl["y"].param_list == ["y", "b", "tau", "P_tau"]
    assert isinstance(mdl["y"].mean, Identity) and mdl["y"].mean.form == "b"
    assert mdl.response is None


def test_parameter_lists_and_type_errors():
    lc = LinearCombination(form={"beta": "X", "alpha": "A"})
    assert lc.get_param_list() == ["beta", "alpha", "X", "A"] and lc.get_grad_param_list() == ["beta", "alpha"]
    sm = ScaledMatrix(matrix="P", scalar="lam")
    assert sm.get_param_list() == ["lam", "P"] and sm.get_grad_param_list() == ["lam"]
    state = {"X": np.arange(6.0).reshape(3, 2), "beta": np.ones((2, 1)), "A": np.eye(3), "alpha": np.ones((3, 1)),
             "P": 2 * np.eye(3), "lam": np.array([[3.0]])}
    assert np.array_equal(lc.predictor(state), state["X"] @ state["beta"] + state["alpha"])
    assert np.array_equal(lc.predictor_conditional(state, term_to_exclude="alpha"), state["X"] @ state["beta"])
    assert np.array_equal(sm.predictor(state), 6 * np.eye(3))
    with pytest.raises(TypeError):
        Normal("y", mean=3.0, precision="P")
    with pytest.raises(TypeError):
        Normal("y", mean="m", precision=LinearCombination(form={"a": "b"}))
    with pytest.raises(TypeError):
        Gamma("g", shape=1.0, rate="r")


def test_normal_structure_recognition():
    n = 5
    mdl = example4_model()
    P = sparse.diags((-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)), offsets=[-1, 0, 1], format="csc")
    state = {"P_lambda": P, "P_tau": sparse.identity(n, format="csc"), "lambda": np.array([[2.0]]), "tau": np.array([[1.0]])}
    st = mdl["b"].structure(state)
    assert st.n == n and st.scale_key == "lambda" and st.n_pos == n and st.off is not None
    st = mdl["y"].structure(state)
    assert st.diag is None and st.off is None and st.scale_key == "tau"
    state["P_lambda"] = np.ones((n, n)) + 5 * np.eye(n)
    assert mdl["b"].structure(state).diag is False  # dense: not served by the tridiagonal path
    state["P_lambda"] = np.ones((n, n + 1))
    with pytest.raises(ValueError):
        mdl["b"].structure(state)


def test_gamma_host_log_p_matches_scipy():
    from scipy import stats

    g = Gamma("lam", shape="a", rate="b")
    state = {"lam": np.array([[2.5]]), "a": np.array([[3.0]]), "b": np.array([[0.7]])}
    assert abs(g.log_p(state) - stats.gamma.logpdf(2.5, 3.0, scale=1 / 0.7)) < 1e-13


def test_shard_chains_partitions_exactly():
    for total, world in [(1024, 8), (1024, 1), (10, 4), (3, 8)]:
        blocks = [shard_chains(total, world, r) for r in range(world)]
        assert sum(b[0] for b in blocks) == total
        off = 0
        for n_local, offset in blocks:
            assert offset == off
            off += n_local
    with pytest.raises(ValueError):
        shard_chains(8, 2, 2)


def test_store_layout():
    a = np.arange(2 * 3 * 4.0).reshape(2, 3, 4)  # (n_iter, C, size)
    out = store_to_reference_layout("b", a)
    assert out.shape == (3, 4, 2) and out[1, 2, 0] == a[0, 1, 2]
    lp = np.arange(6.0).reshape(2, 3)
    assert store_to_reference_layout("log_post", lp).shape == (3, 2, 1)


def test_ragged_chain_arrays_on_cpu_tensors():
    """The ragged description (count key + axis) and the padded constructors; torch CPU tensors stand in for
    device memory (no kernel is called)."""
    import torch

    from openmcmc_amd.chains import ChainArray, ragged_from_lists

    theta = ragged_from_lists([[1.0, 2.0], [3.0], [4.0, 5.0, 6.0]], 4, 1, "n_basis", torch.device("cpu"))
    assert theta.shape == (1, 4) and theta.ragged == ("n_basis", 1)
    assert theta.data[1, 0].tolist() == [3.0, 0.0, 0.0, 0.0]
    beta = ragged_from_lists([[1.0], [2.0, 3.0]], 3, 0, "n_basis", torch.device("cpu"))
    assert beta.shape == (3, 1) and beta.vector().shape == (2, 3)
    state = {"n_basis": ChainArray(torch.tensor([2.0, 1.0, 3.0]).reshape(3, 1, 1))}
    assert theta.count(state).tolist() == [2.0, 1.0, 3.0]
    assert theta.like(theta.data + 1).ragged == theta.ragged
    with pytest.raises(ValueError):
        ragged_from_lists([[1.0, 2.0, 3.0]], 2, 0, "k", torch.device("cpu"))
    with pytest.raises(ValueError):
        ChainArray(torch.zeros(2, 3, 1), ragged=("k", 2))
    # a basis kept column-major per chain: logical (C, n, k) view over (C, k, n) storage
    phys = torch.arange(2 * 3 * 5, dtype=torch.float64).reshape(2, 3, 5)
    B = ChainArray(phys.transpose(1, 2), ragged=("n_basis", 1))
    assert B.shape == (5, 3) and B.storage().data_ptr() == phys.data_ptr() and B.columns().is_contiguous()


def test_uniform_and_poisson_host_values_match_scipy():
    from scipy import stats

    from openmcmc_amd.distribution.distribution import Poisson, Uniform

    u = Uniform("theta", domain_response_lower=np.array([[-10.0]]), domain_response_upper=np.array([[10.0]]))
    state = {"theta": np.array([[1.0, 2.0, -3.0]])}
    assert u.log_p(state) == pytest.approx(3 * -np.log(20.0))                 # distribution.py:436-442
    assert np.allclose(u.log_p(state, by_observation=True), -np.log(20.0) * np.ones(3))
    assert u.log_p_per_replicate(state) == pytest.approx(-np.log(20.0))
    u2 = Uniform("x", domain_response_lower=np.array([0.0, -1.0]), domain_response_upper=np.array([2.0, 3.0]))
    assert u2.domain_range({"x": np.zeros((2, 1))}).ravel().tolist() == [2.0, 4.0]
    assert u2.param_list == ["x"]
    p = Poisson("n", rate="rho")
    st = {"n": np.array([[4.0]]), "rho": np.array([[5.0]])}
    assert p.log_p(st) == pytest.approx(stats.poisson.logpmf(4, 5.0))
    assert p.param_list == ["n", "rho"]
    with pytest.raises(TypeError):
        Poisson("n", rate=3.0)


def test_mixture_parameters_host_predictors():
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.parameter import MixtureParameterMatrix, MixtureParameterVector

    st = {"mu": np.array([[1.0], [5.0]]), "tau": np.array([[0.25], [4.0]]), "alloc": np.array([[0], [1], [1]])}
    v = MixtureParameterVector("mu", "alloc")
    assert v.predictor(st).ravel().tolist() == [1.0, 5.0, 5.0]                 # parameter.py:447
    m = MixtureParameterMatrix("tau", "alloc")
    assert np.array_equal(m.predictor(st).toarray(), np.diag([0.25, 4.0, 4.0]))  # parameter.py:501
    assert v.get_param_list() == ["mu", "alloc"] and v.get_grad_param_list() == ["mu"] and m.get_grad_param_list() == []
    d = Normal("beta", mean=v, precision=m)
    assert d.is_mixture and d.param_list == ["beta", "mu", "alloc", "tau", "alloc"]


def test_samplers_keep_full_model_like_reference():
    """RandomWalk with a state_update_function and ReversibleJump keep the WHOLE model
    (metropolis_hastings.py:201-210, reversible_jump.py:66-74); without the callback RandomWalk conditions."""
    import sys, os

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from openmcmc_amd.distribution.distribution import Gamma, Poisson, Uniform
    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.model import Model
    from openmcmc_amd.sampler.metropolis_hastings import RandomWalk, RandomWalkLoop
    from openmcmc_amd.sampler.reversible_jump import ReversibleJump

    mdl = Model([Normal("x", mean="mu", precision="Q"), Uniform("theta"), Poisson("n", rate="rho"), Gamma("tau", shape="a", rate="b")])
    assert set(RandomWalk("theta", mdl).model.keys()) == {"theta"}
    assert set(RandomWalkLoop("theta", mdl, state_update_function=lambda s, j: (s, 0.0, 0.0)).model.keys()) == set(mdl.keys())
    rj = ReversibleJump("n", mdl, associated_params="theta", n_max=5)
    assert set(rj.model.keys()) == set(mdl.keys()) and rj.associated_params == ["theta"]
    assert rj.accept_rate.get_acceptance_rate() == "No proposals"
    with pytest.raises(RuntimeError):
        rj.sample({})  # not bound to an engine: the product path fails loudly


def test_null_distribution_and_band_recognition():
    """NullDistribution's host behaviour (location_scale.py:63-124) and the band-structure recognition that routes a
    precision wider than tridiagonal to the band kernel (or to the dense route when the band would not pay)."""
    from scipy import sparse

    from openmcmc_amd.distribution.location_scale import Normal, NullDistribution, band_storage
    from openmcmc_amd.parameter import LinearCombination, ScaledMatrix

    nd = NullDistribution("y", mean=LinearCombination({"beta": "B"}), precision=ScaledMatrix("P", "tau"))
    assert nd.log_p({}) == 0.0 and nd.rvs({}) is None and nd.grad_log_p_diag({}, "beta", None) is None
    assert nd.param_list == ["y", "beta", "B", "tau", "P"]
    n = 12
    D = sparse.diags([np.ones(n - 2), -2 * np.ones(n - 2), np.ones(n - 2)], offsets=[0, 1, 2], shape=(n - 2, n))
    P = (D.T @ D + 1e-3 * sparse.identity(n)).tocsc()
    band = band_storage(P, n)
    assert band.shape == (3, n) and np.array_equal(band[0], P.diagonal()) and np.array_equal(band[2, : n - 2], P.diagonal(-2))
    assert band[2, n - 2:].tolist() == [0.0, 0.0]
    st = Normal("b", mean="mu", precision=ScaledMatrix("P", "lam")).structure({"P": P, "lam": 1.0})
    assert st.diag is False and st.band is not None and st.band_rows().shape == (3, n)
    assert band_storage(np.ones((6, 6)) + 6 * np.eye(6), 6) is None          # dense: the band would not pay
    tri = Normal("b", mean="mu", precision="Q").structure({"Q": sparse.diags([[-1.0] * 4, [2.0] * 5, [-1.0] * 4], [-1, 0, 1]).tocsc()})
    assert tri.band is None and tri.band_rows().shape == (2, 5)
    with pytest.raises(ValueError):
        band_storage(sparse.csc_matrix(np.triu(np.ones((8, 8)), 0) * (np.abs(np.subtract.outer(np.arange(8), np.arange(8))) <= 2)), 8)


def _structure_matrices():
    """(name, matrix as an ndarray, the kind it has): one matrix per structure class, and a band too wide to pay"""
    def rw(n, order):
        D = np.diff(np.eye(n), order, axis=0)
        return D.T @ D + 1e-2 * np.eye(n)

    A = np.random.default_rng(7).standard_normal((9, 5))
    return [("identity", np.eye(5), "identity"), ("diagonal", np.diag([1.0, 2.0, 0.5, 1.0, 3.0]), "diagonal"),
            ("rw1", rw(5, 1), "tridiagonal"), ("rw2_n12", rw(12, 2), "band"),  # (w + 1) * 2 = 6 <= 12: band_storage gives rows
            ("full_spd", A.T @ A / 5 + 0.5 * np.eye(5), "dense"),
            ("rw2_n5", rw(5, 2), "dense")]                                     # (w + 1) * 2 = 6 > 5: the band would not pay


@pytest.mark.parametrize("as_sparse", [False, True])
@pytest.mark.parametrize("name,M,kind", _structure_matrices())
def test_normal_structure_kind(name, M, kind, as_sparse):
    """NormalStructure.kind for every structure class, from a dense array and from a scipy.sparse matrix, and the booleans the
    callers ask next to the sentinel expressions they replace; NormalNormal's structure of a replicated response keeps the kind
    (n_rep times the identity is a constant diagonal)."""
    from openmcmc_amd.sampler.sampler import NormalNormal

    dist = Normal("b", mean="mu", precision=ScaledMatrix("P", "lam"))
    st = dist.structure({"P": sparse.csc_matrix(M) if as_sparse else M, "lam": 1.0})
    assert st.kind == kind
    assert st.narrow == (st.diag is not False)
    assert st.diagonal_only == (not (st.diag is False or st.off is not None))
    assert (st.kind == "dense") == (st.diag is False and st.band is None)
    assert (st.kind == "identity") == (st.diag is None and st.off is None)
    assert (st.kind == "band") == (st.band is not None) == (st.diag is False and st.band_rows() is not None)
    rep = NormalNormal("b", Model([dist]))._replicated_structure(st, 3)
    assert rep.kind == ("diagonal" if kind == "identity" else kind)
    assert rep.narrow == (rep.diag is not False) and rep.diagonal_only == (not (rep.diag is False or rep.off is not None))
    assert (rep.kind == "dense") == (rep.diag is False and rep.band is None)
    dense = np.asarray(rep.matrix.toarray() if as_sparse else rep.matrix)
    assert np.array_equal(dense, 3.0 * M)
    if rep.narrow:
        assert np.array_equal(rep.diag, np.diag(3.0 * M)) and (rep.off is None or np.array_equal(rep.off, np.diag(3.0 * M, 1)))
    elif rep.kind == "band":
        assert np.array_equal(rep.band, 3.0 * st.band)


def test_identity_memo():
    """by_identity: a hit only for the very objects the entry was made from -- not for an equal object, not for an entry that
    sits under another object's key (an id handed out again after a collection), not when the second of two objects differs."""
    from openmcmc_amd.memo import by_identity

    made = []

    def make():
        made.append(len(made))
        return made[-1]

    memo, A, B = {}, np.arange(3.0), np.arange(3.0)
    assert by_identity(memo, make, A) == 0 and by_identity(memo, make, A) == 0 and made == [0]    # the same object: one call
    assert by_identity(memo, make, B) == 1 and by_identity(memo, make, A) == 0 and made == [0, 1]  # equal, another object
    # the entry made from A under the key of B: what a recycled id looks like
    only_b = {}
    by_identity(only_b, lambda: None, B)
    (key_b,) = only_b
    planted = {}
    by_identity(planted, lambda: "from A", A)
    (key_a,) = planted
    planted[key_b] = planted.pop(key_a)
    assert by_identity(planted, lambda: "from B", B) == "from B" and by_identity(planted, lambda: "again", B) == "from B"
    # two key objects: both must be the same
    two, A2, B2 = {}, np.arange(3.0), np.arange(3.0)
    assert by_identity(two, lambda: "A, B", A, B) == "A, B" and by_identity(two, lambda: "new", A, B) == "A, B"
    assert by_identity(two, lambda: "A, B2", A, B2) == "A, B2" and by_identity(two, lambda: "A2, B", A2, B) == "A2, B"
    (key_ab,) = [k for k, (objs, v) in two.items() if v == "A, B"]
    (key_ab2,) = [k for k, (objs, v) in two.items() if v == "A, B2"]
    two[key_ab2] = two[key_ab]  # first object right, second object another
    assert by_identity(two, lambda: "made again", A, B2) == "made again"
    assert by_identity(two, lambda: "none", A, None) == "none" and by_identity(two, lambda: "x", A, None) == "none"  # None is a key object too


def test_manifold_mala_route_names_the_route_sample_takes():
    """ManifoldMALA.route on one hand-built state per route: numpy arrays and ChainArrays over CPU tensors, no engine ("transform"
    uploads its statistics: tests/test_transform_gpu.py asserts it)."""
    import torch

    from openmcmc_amd.chains import ChainArray, ragged_from_lists
    from openmcmc_amd.distribution.location_scale import NullDistribution
    from openmcmc_amd.parameter import LinearCombinationWithTransform, MixtureParameterMatrix, MixtureParameterVector
    from openmcmc_amd.sampler.metropolis_hastings import ManifoldMALA

    C, p = 3, 4
    fixed = ChainArray(torch.zeros(C, p, 1, dtype=torch.float64))
    ragged = ragged_from_lists([[1.0], [2.0, 3.0], [4.0]], p, 0, "k", torch.device("cpu"))
    gauss = Model([Normal("beta", mean="m0", precision="P0")])
    state = {"beta": fixed, "m0": np.zeros((p, 1)), "P0": np.eye(p), "B": np.ones((6, p)), "y": np.ones((6, 1)), "P": sparse.identity(6).tocsc(),
             "tau": ChainArray(torch.ones(C, 1, 1, dtype=torch.float64)), "k": ChainArray(torch.tensor([1.0, 2.0, 1.0]).reshape(C, 1, 1)),
             "mu": np.zeros((2, 1)), "lam": np.ones((2, 1)), "alloc": np.zeros((p, 1), dtype=int)}
    assert ManifoldMALA("beta", gauss).route(state) == "white"
    assert ManifoldMALA("beta", gauss, whitened=False).route(state) == "products"
    lik = dict(mean=LinearCombination({"beta": "B"}), precision=ScaledMatrix("P", "tau"))
    mixture_prior = Normal("beta", mean=MixtureParameterVector("mu", "alloc"), precision=MixtureParameterMatrix("lam", "alloc"))
    regression = Model([Normal("y", **lik), Normal("beta", mean="m0", precision="P0")])
    # "diag": a ragged parameter whatever the model; the parameter's own mixture prior under nothing but null distributions
    assert ManifoldMALA("beta", regression).route({**state, "beta": ragged}) == "diag"
    assert ManifoldMALA("beta", Model([NullDistribution("y", **lik), mixture_prior])).route(state) == "diag"
    # ... and not a model with a likelihood that does depend on the parameter, nor a null likelihood under a plain prior
    assert ManifoldMALA("beta", regression).route(state) == "dense"
    assert ManifoldMALA("beta", Model([Normal("y", **lik), mixture_prior])).route(state) == "dense"
    assert ManifoldMALA("beta", Model([NullDistribution("y", **lik), Normal("beta", mean="m0", precision="P0")])).route(state) == "dense"
    moving = Normal("y", mean=LinearCombinationWithTransform(form={"beta": "B"}, transform={"beta": True}), precision=ScaledMatrix("P", "tau"))
    assert ManifoldMALA("beta", Model([moving, Normal("beta", mean="m0", precision="P0")]), fused=False).route(state) == "general"


@pytest.mark.parametrize("shape", [1e-3, 0.5, 1.0, 2.0, 1e6])
def test_gamma_log_p_by_observation_at_zero_matches_scipy(shape):
    """The torch branch of Gamma.log_p (per-replicate densities of a per-chain response, run here on CPU tensors): at x = 0
    +inf for shape < 1, log(rate) for shape 1, -inf above, as stats.gamma.logpdf."""
    import torch
    from scipy import stats

    from openmcmc_amd.chains import ChainArray

    x = np.array([[[0.0, 1.5, -0.0]], [[-1.0, 0.0, 1e-300]]])
    st = {"x": ChainArray(torch.tensor(x)), "a": np.array([[shape]]), "b": np.array([[2.0]])}
    got = Gamma("x", "a", "b").log_p(st, by_observation=True).numpy()
    ref = stats.gamma.logpdf(x[:, 0, :], shape, scale=0.5)
    inf = ~np.isfinite(ref)
    assert np.array_equal(got[inf], ref[inf])
    assert np.allclose(got[~inf], ref[~inf], rtol=1e-13, atol=0.0)
