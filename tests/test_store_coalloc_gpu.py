"""Co-allocation matrix and least-squares partition of the device store (omc_store_coalloc, omc_store_partition_score,
Engine.store_coalloc / store_partition_score) against the numpy restatement of coalloc_model.py.  Every result is an exact
integer: everything is held array_equal.  The int8 MFMA operand lane maps are not documented for gfx950; the structured
pattern below is their check -- no off-diagonal 16 x 16 sub-tile of its matrix is symmetric and no two contraction positions
agree, so a k-order mismatch between the operands or a transposed sub-tile cannot pass it."""

import numpy as np
import pytest
from coalloc_model import batches_of, canonical, coalloc, first_argmin, flags_of, scores

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 5, 64)
N_IDX = (1, 15, 16, 17, 127, 128, 129, 257)
SHAPES = ((1, 1), (5, 2), (37, 3), (700, 4))  # the last: 2800 pooled rows, several 256-row slices are joined


def engine(C):
    from openmcmc_amd.engine import Engine
    return Engine(C, seed=1)


def structured(n_iter, C, size, K):
    """label of element e at row r = it C + c: (r (e + 1) + e // 7) % K"""
    r = np.arange(n_iter * C, dtype=np.int64).reshape(n_iter, C, 1)
    e = np.arange(size, dtype=np.int64).reshape(1, 1, size)
    return ((r * (e + 1) + e // 7) % K).astype(np.float64)


def reference(x, K, index, pooled, per_label=False):
    """(counts, flags) stacked over the batches as the entry point lays them out"""
    Zs = batches_of(x, K, index, pooled)
    counts = np.stack([coalloc(Z, K, per_label) for Z in Zs])
    flags = np.stack([flags_of(Z) for Z in Zs])
    return (counts[0], flags[0]) if pooled else (counts, flags)


def reference_scores(x, K, index, pooled, counts):
    """(scores (n_iter, C), best (batches, 2)) from counts laid out as the entry point's"""
    n_iter, C = x.shape[:2]
    Zs = batches_of(x, K, index, pooled)
    cs = [counts] if pooled else list(counts)
    sc = [scores(Z, c, Z.shape[0]) for Z, c in zip(Zs, cs)]
    best = np.array([first_argmin(s) for s in sc], dtype=np.int64)
    return (sc[0].reshape(n_iter, C), best[0]) if pooled else (np.stack(sc, axis=1), best)


def check_case(eng, x, K, index, pooled):
    d = eng.to_device(x)
    counts, flags = eng.store_coalloc(d, K, index=index, pooled=pooled)
    ref_c, ref_f = reference(x, K, index, pooled)
    got = counts.cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, ref_c)
    assert np.array_equal(flags.cpu().numpy(), ref_f)
    assert np.array_equal(got, np.swapaxes(got, -1, -2))
    score, best = eng.store_partition_score(d, K, counts, index=index, pooled=pooled)
    ref_s, ref_b = reference_scores(x, K, index, pooled, ref_c)
    assert np.array_equal(score.cpu().numpy(), ref_s)
    assert np.array_equal(best.cpu().numpy(), ref_b)


# ------------------------------------------------------------------------------------------------- 1. tile and contraction edges
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n_idx", N_IDX)
def test_tile_and_contraction_edges(n_idx, shape):
    n_iter, C = shape
    a = N_IDX.index(n_idx) + SHAPES.index(shape)
    rng = np.random.default_rng(100 * n_idx + n_iter)
    eng = engine(C)
    # structured pattern with one K, random labels with another; one of them under an index, over a store wider than the selection
    # (shuffled, with repeats); both pooled and per chain
    for kind, K in (("structured", KS[a % 5]), ("random", KS[(a + 2) % 5])):
        with_index = (kind == "structured") == (a % 2 == 0)
        size = n_idx + 5 if with_index else n_idx
        x = structured(n_iter, C, size, K) if kind == "structured" else rng.integers(0, K, size=(n_iter, C, size)).astype(np.float64)
        index = None
        if with_index:
            index = rng.integers(0, size, size=n_idx)
            index[-1] = index[0]
        for pooled in (True, False):
            check_case(eng, x, K, index, pooled)
    eng.close()


@pytest.mark.parametrize("K", KS)
def test_every_label_count_on_the_structured_pattern(K):
    """n = 129 (two tiles: an off-diagonal one), 37 x 3 rows, no index: every K, the padded ones (3, 5) included"""
    eng = engine(3)
    x = structured(37, 3, 129, K)
    for pooled in (True, False):
        check_case(eng, x, K, None, pooled)
    eng.close()


# ------------------------------------------------------------------------------------------------- 2. the label rule
def test_label_rule():
    n_iter, C, size, K = 41, 2, 40, 5
    rng = np.random.default_rng(7)
    x = rng.integers(0, K, size=(n_iter, C, size)).astype(np.float64)
    specials = [np.nan, -0.0, 0.5, -1.0, float(K), K + 0.0, np.inf, -np.inf, 5e-324, K - 1 + 0.5, np.nextafter(1.0, 2.0)]
    for k, v in enumerate(specials * 9):
        x[rng.integers(0, n_iter), rng.integers(0, C), (3 * k) % size] = v
    x[:, :, 17] = np.nan          # an element that is always absent
    x[:, 1, 18] = -0.0            # label 0 throughout one chain
    eng = engine(C)
    d = eng.to_device(x)
    for pooled in (True, False):
        counts, flags = (t.cpu().numpy() for t in eng.store_coalloc(d, K, pooled=pooled))
        ref_c, ref_f = reference(x, K, None, pooled)
        assert np.array_equal(counts, ref_c) and np.array_equal(flags, ref_f)
        rows = n_iter * C if pooled else n_iter
        diag = np.diagonal(counts, axis1=-2, axis2=-1)
        assert np.array_equal(diag, rows - flags[..., 0] - flags[..., 1])  # a draw without a label does not match itself
        assert not counts[..., 17, :].any() and not counts[..., :, 17].any()
        assert flags[..., 1].sum() > 0 and flags[..., 0].sum() > rows
        check_case(eng, x, K, None, pooled)
    eng.close()


# ------------------------------------------------------------------------------------------------- 3. per_label
@pytest.mark.parametrize("K", (1, 3, 64))
def test_per_label(K):
    n_iter, C, size = 300, 3, 131
    rng = np.random.default_rng(K)
    x = rng.integers(0, K, size=(n_iter, C, size)).astype(np.float64)
    x[rng.random(x.shape) < 0.02] = np.nan
    index = rng.integers(0, size, size=70)
    eng = engine(C)
    d = eng.to_device(x)
    for pooled in (True, False):
        per, flags = eng.store_coalloc(d, K, index=index, pooled=pooled, per_label=True)
        plain, flags2 = eng.store_coalloc(d, K, index=index, pooled=pooled)
        per, plain = per.cpu().numpy(), plain.cpu().numpy()
        assert per.shape == plain.shape[:-2] + (K,) + plain.shape[-2:]
        assert np.array_equal(per.sum(axis=-3), plain) and np.array_equal(flags.cpu().numpy(), flags2.cpu().numpy())
        assert np.array_equal(per, reference(x, K, index, pooled, per_label=True)[0])
        assert np.array_equal(per, np.swapaxes(per, -1, -2))
        hist, _ = eng.store_histogram(d, np.arange(K + 1, dtype=np.float64), index=index, pooled=pooled)  # (.., n, K)
        assert np.array_equal(np.diagonal(per, axis1=-2, axis2=-1), np.swapaxes(hist.cpu().numpy(), -1, -2))
    eng.close()


# ------------------------------------------------------------------------------------------------- 4. symmetry, determinism
def test_symmetric_and_repeatable():
    n_iter, C, size, K = 700, 4, 257, 3
    x = np.random.default_rng(11).integers(0, K, size=(n_iter, C, size)).astype(np.float64)
    eng = engine(C)
    d = eng.to_device(x)
    for pooled in (True, False):
        for per_label in (False, True):
            a, _ = eng.store_coalloc(d, K, pooled=pooled, per_label=per_label)
            b, _ = eng.store_coalloc(d, K, pooled=pooled, per_label=per_label)
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.array_equal(a, b) and np.array_equal(a, np.swapaxes(a, -1, -2))
        counts, _ = eng.store_coalloc(d, K, pooled=pooled)
        s1, b1 = eng.store_partition_score(d, K, counts, pooled=pooled)
        s2, b2 = eng.store_partition_score(d, K, counts, pooled=pooled)
        assert np.array_equal(s1.cpu().numpy(), s2.cpu().numpy()) and np.array_equal(b1.cpu().numpy(), b2.cpu().numpy())
    eng.close()


# ------------------------------------------------------------------------------------------------- 5. the edges of the contract
def test_contract_edges():
    import torch

    from openmcmc_amd import _abi

    n_iter, C, size, K, POISON = 6, 2, 9, 3, -7
    x = np.random.default_rng(5).integers(0, K, size=(n_iter, C, size)).astype(np.float64)
    eng = engine(C)
    d = eng.to_device(x)
    idx = torch.tensor([0, 3, 3, 8], dtype=torch.int64, device=d.device)
    good_counts, _ = eng.store_coalloc(d, K)

    def poisoned(*shape):
        return torch.full(shape, POISON, dtype=torch.int64, device=d.device)

    def untouched(*ts):
        return all(bool((t == POISON).all()) for t in ts)

    def call(n_iter=n_iter, sz=size, index=None, n_idx=None, k=K):
        n = (size if index is None else index.numel()) if n_idx is None else n_idx
        ip = None if index is None else index.data_ptr()
        counts, flags = poisoned(size, size), poisoned(size, 2)
        st = _abi.lib.omc_store_coalloc(eng._ctx, n_iter, sz, d.data_ptr(), ip, n, k, 1, 0, counts.data_ptr(), flags.data_ptr())
        eng.synchronize()
        text = _abi.lib.omc_last_error().decode()
        score, best = poisoned(6, C), poisoned(2)
        st2 = _abi.lib.omc_store_partition_score(eng._ctx, n_iter, sz, d.data_ptr(), ip, n, k, 1, good_counts.data_ptr(),
                                                 score.data_ptr(), best.data_ptr())
        eng.synchronize()
        text2 = _abi.lib.omc_last_error().decode()
        return (st, text, untouched(counts, flags)), (st2, text2, untouched(score, best))

    bad_hi = torch.tensor([0, 3, size, 8], dtype=torch.int64, device=d.device)
    bad_lo = torch.tensor([0, -1, 3, 8], dtype=torch.int64, device=d.device)
    for kw, status, text_has in (({"index": bad_hi}, _abi.INVALID_ARG, "index outside"), ({"index": bad_lo}, _abi.INVALID_ARG, "index outside"),
                                 ({"k": 0}, _abi.INVALID_ARG, "n_labels"), ({"k": 65}, _abi.UNSUPPORTED, "n_labels"),
                                 ({"n_idx": size - 1}, _abi.INVALID_ARG, "n_idx"), ({"index": idx, "n_idx": 0}, _abi.INVALID_ARG, "n_idx"),
                                 ({"n_iter": 0}, _abi.INVALID_ARG, "n_iter"), ({"sz": 0}, _abi.INVALID_ARG, "size")):
        for st, text, clean in call(**kw):
            assert st == status and text_has in text and clean, (kw, st, text, clean)
    for st, _, clean in call(index=idx[:1].repeat(size)):  # a valid call writes
        assert st == _abi.OK and not clean
    # flags_out may be NULL
    counts = poisoned(size, size)
    assert _abi.lib.omc_store_coalloc(eng._ctx, n_iter, size, d.data_ptr(), None, size, K, 1, 0, counts.data_ptr(), None) == _abi.OK
    assert np.array_equal(counts.cpu().numpy(), good_counts.cpu().numpy())
    # the binding's own words
    with pytest.raises(ValueError, match="index outside"):
        eng.store_coalloc(d, K, index=[0, size])
    with pytest.raises(ValueError, match="n_labels"):
        eng.store_coalloc(d, 0)
    with pytest.raises(NotImplementedError):
        eng.store_coalloc(d, 65)
    with pytest.raises(TypeError, match="counts"):
        eng.store_partition_score(d, K, good_counts, pooled=False)
    eng.close()


# ------------------------------------------------------------------------------------------------- 6. the partition
def test_first_minimum_among_tied_rows():
    n_iter, C, size, K = 40, 3, 70, 3
    rng = np.random.default_rng(13)
    planted = rng.integers(0, K, size=size)
    x = np.broadcast_to(planted, (n_iter, C, size)).astype(np.float64).copy()
    noisy = rng.random((n_iter, C)) < 0.7
    noisy[2, 1] = noisy[2, 2] = noisy[9, 0] = False          # several rows are the planted draw itself: tied at the minimum
    noisy[0, :] = noisy[1, :] = noisy[2, 0] = True
    x[noisy] = rng.integers(0, K, size=(int(noisy.sum()), size))
    x[5] = x[20]                                           # duplicated rows away from the minimum
    eng = engine(C)
    d = eng.to_device(x)
    for pooled in (True, False):
        check_case(eng, x, K, None, pooled)
    counts, _ = eng.store_coalloc(d, K)
    score, best = (t.cpu().numpy() for t in eng.store_partition_score(d, K, counts))
    flat = score.reshape(-1)
    assert (flat == flat.min()).sum() >= 3 and best[0] == 2 * C + 1 == int(np.argmin(flat)) and best[1] == flat.min()
    eng.close()


def test_planted_clusters_under_label_switching():
    n_iter, C, size, K = 200, 4, 30, 3
    rng = np.random.default_rng(17)
    planted = np.repeat(np.arange(K), size // K)
    z = np.broadcast_to(planted, (n_iter, C, size)).copy()
    noise = rng.random(z.shape) < 0.10
    z[noise] = rng.integers(0, K, size=int(noise.sum()))
    # label switching: every chain names the clusters its own way, at random -- drawn again until two clusters share the name most
    # chains give them with a clear majority (a mode over the chains then cannot tell them apart, whatever the noise does)
    while True:
        perms = np.stack([rng.permutation(K) for _ in range(C)])
        votes = [np.bincount(perms[:, k], minlength=K) for k in range(K)]
        top = [int(v.argmax()) for v in votes]
        if len(set(top)) < K and all(np.sort(v)[-1] > np.sort(v)[-2] for v, t in zip(votes, top) if top.count(t) > 1):
            break
    x = np.stack([perms[c][z[:, c, :]] for c in range(C)], axis=1).astype(np.float64)
    eng = engine(C)
    d = eng.to_device(x)
    counts, _ = eng.store_coalloc(d, K)
    score, best = (t.cpu().numpy() for t in eng.store_partition_score(d, K, counts))
    ref_s, ref_b = reference_scores(x, K, None, True, counts.cpu().numpy())
    assert np.array_equal(score, ref_s) and np.array_equal(best, ref_b)
    it, c = divmod(int(best[0]), C)
    assert np.array_equal(canonical(x[it, c].astype(np.int64)), canonical(planted))
    # the element-wise mode of the raw labels is misled: it does not separate the three clusters
    mode = np.array([np.bincount(x[:, :, e].astype(np.int64).reshape(-1), minlength=K).argmax() for e in range(size)])
    assert not np.array_equal(canonical(mode), canonical(planted))
    eng.close()
