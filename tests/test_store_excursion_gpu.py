"""First failures of the device store (omc_store_first_failure, Engine.store_first_failure) against the numpy restatement of
tests/excursion_model.py (which tests/test_excursion_model_host.py ties to the definition).  h and r are integers: every comparison
is np.array_equal, for the automatic, the short and the long form (argument algo), with and without an index, for 1, 2, 3, 5 and 8
slots with different tables per slot, over the smallest shapes at which a form can go wrong: rows shorter than a wave, around one and two
waves' pairs, odd sizes (every second row 8 bytes off a 16-byte boundary), row counts around the 32 rows of a workgroup and of a
flush group, one and three chains."""

import numpy as np
import pytest
from excursion_model import first_failure_slots

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 1001]
SHAPES = [(1, 1), (2, 1), (63, 1), (65, 1), (257, 1), (1, 3), (21, 3), (86, 3)]  # (n_iter, C): R = 1, 2, 63, 65, 257, 3, 63, 258
ALGOS = (0, 1, 2)
SLOTS = (1, 2, 3, 5, 8)  # the instantiations keep 1, 2, 4 and 8 minima: 3 and 5 leave slots of a wider one unused
BOUNDS_LO = np.array([-np.inf, -np.inf, -1.0, -0.5, 0.0, 0.5, np.inf])
BOUNDS_HI = np.array([np.inf, np.inf, 1.0, 0.5, 0.0, -np.inf])


def engine(C):
    from openmcmc_amd.engine import Engine

    return Engine(C, seed=1)


def store_of(N, C, size, rng):
    """draws on a grid of halves, so that a draw equals a bound often; NaN, +inf and -inf draws; one row that agrees with every
    open side (all zeros would not: a row of 0.25) and one of NaN"""
    x = np.round(2 * rng.standard_normal((N * C, size))) / 2
    u = rng.random(x.shape)
    x[u < 0.04] = np.nan
    x[(u >= 0.04) & (u < 0.07)] = np.inf
    x[(u >= 0.07) & (u < 0.10)] = -np.inf
    x[rng.integers(0, N * C)] = 0.25
    if N * C > 2:
        x[rng.integers(0, N * C)] = np.nan
    return x.reshape(N, C, size)


def tables(L, n, rng):
    """(lo, hi, pos) (L, n): bounds from the grid of the draws and +-inf on either side; slot 0 the identity order, slot 1 the
    reverse, the others random permutations"""
    lo, hi = rng.choice(BOUNDS_LO, (L, n)), rng.choice(BOUNDS_HI, (L, n))
    pos = np.stack([np.arange(n) if l == 0 else np.arange(n)[::-1] if l == 1 else rng.permutation(n) for l in range(L)])
    return lo, hi, np.ascontiguousarray(pos)


def indices(size, rng):
    sub = rng.permutation(size)[: max(1, size // 2)]
    return [None, np.array([size // 2]), np.concatenate([sub, sub[:2], sub[:1]]), rng.integers(0, size, size + 7)]


def run(eng, d, lo, hi, pos, idx, algo):
    h, r = eng.store_first_failure(d, lo, hi, pos, index=idx, want_rows=True, algo=algo)
    return h.cpu().numpy(), r.cpu().numpy().reshape(r.shape[0], -1)


@pytest.mark.parametrize("size", SIZES)
def test_h_and_r_match_the_restatement(size):
    rng = np.random.default_rng(1000 + size)
    engines = {C: engine(C) for C in (1, 3)}
    for N, C in SHAPES:
        eng = engines[C]
        x = store_of(N, C, size, rng)
        d = eng.to_device(x)
        rows = x.reshape(N * C, size)
        for idx in indices(size, rng):
            n = size if idx is None else len(idx)
            for L in SLOTS:
                lo, hi, pos = tables(L, n, rng)
                want_h, want_r = first_failure_slots(rows, lo, hi, pos, idx)
                assert want_h.shape == (L, n + 1) and np.all(want_h.sum(axis=1) == N * C)
                for algo in ALGOS:
                    h, r = run(eng, d, lo, hi, pos, idx, algo)
                    what = (N, C, n, L, algo)
                    assert h.dtype == np.int64 and r.dtype == np.int32 and h.shape == want_h.shape and r.shape == want_r.shape, what
                    assert np.array_equal(r, want_r), what
                    assert np.array_equal(h, want_h), what
                h2 = eng.store_first_failure(d, lo, hi, pos, index=idx)  # a repeated call, without the rows
                assert h2[1] is None and np.array_equal(h2[0].cpu().numpy(), want_h)
    for eng in engines.values():
        eng.close()


def test_the_rules_one_by_one():
    """NaN fails; +-inf draws are values (a -inf draw agrees with lo = -inf only, a +inf draw with hi = +inf only); a draw on a
    bound fails; an element every row agrees at and one no row agrees at; the minimum is over pos[k], not over k"""
    inf, nan = np.inf, np.nan
    #                 k=0    1     2     3     4
    rows = np.array([[0.5, 2.0, -inf, inf, 1.0],
                     [0.5, 1.0, -inf, inf, nan],
                     [0.5, 3.0, 0.0, 0.0, 2.0],
                     [nan, 3.0, 0.0, 0.0, 2.0]])
    R, n = rows.shape
    eng = engine(1)
    d = eng.to_device(rows.reshape(R, 1, n))

    def call(lo, hi, pos, algo):
        h, r = run(eng, d, np.asarray(lo, dtype=float), np.asarray(hi, dtype=float), np.asarray(pos), None, algo)
        return h[0].tolist(), r[0].tolist()

    for algo in ALGOS:
        free = ([-inf] * n, [inf] * n)
        # no bound anywhere: only NaN draws fail -- row 1 at k = 4, row 3 at k = 0
        assert call(*free, [0, 1, 2, 3, 4], algo) == ([1, 0, 0, 0, 1, 2], [5, 4, 5, 0])
        # the reverse order: the same elements at other places
        assert call(*free, [4, 3, 2, 1, 0], algo) == ([1, 0, 0, 0, 1, 2], [5, 0, 5, 4])
        # strict bounds at k = 1: (1, 3) holds 2.0 only; the order puts k = 1 at place 2, k = 0 at place 3, k = 4 at place 0
        assert call([-inf, 1.0, -inf, -inf, -inf], [inf, 3.0, inf, inf, inf], [3, 2, 1, 4, 0], algo) == ([1, 0, 2, 0, 0, 1], [5, 0, 2, 2])
        # -inf draws at k = 2 against a finite lower bound fail, against lo = -inf with a finite upper bound they agree
        assert call([-inf, -inf, -1.0, -inf, -inf], [inf] * n, [1, 2, 0, 3, 4], algo)[1] == [0, 0, 5, 1]
        assert call([-inf] * n, [inf, inf, 0.0, inf, inf], [1, 2, 0, 3, 4], algo)[1] == [5, 4, 0, 0]
        # +inf draws at k = 3 likewise
        assert call([-inf] * n, [inf, inf, inf, 1.0, inf], [1, 2, 3, 0, 4], algo)[1] == [0, 0, 5, 1]
        assert call([-inf, -inf, -inf, 0.0, -inf], [inf] * n, [1, 2, 3, 0, 4], algo)[1] == [5, 4, 0, 0]
        # an infinite bound on the wrong side: nothing is above +inf or below -inf
        assert call([inf, -inf, -inf, -inf, -inf], [inf] * n, [0, 1, 2, 3, 4], algo)[0] == [R, 0, 0, 0, 0, 0]
        assert call([-inf] * n, [inf, inf, inf, -inf, inf], [4, 3, 2, 0, 1], algo)[0] == [R, 0, 0, 0, 0, 0]
    # every row agrees at every selected element: h[n] == R
    h, r = eng.store_first_failure(d, [-inf, 0.0], [inf, inf], [1, 0], index=[1, 1], want_rows=True)
    assert h.cpu().numpy().tolist() == [[0, 0, R]] and r.cpu().numpy().ravel().tolist() == [2] * R
    eng.close()


def test_a_row_beyond_the_lds_tile_takes_the_long_form_whatever_algo_says():
    N, C, size = 2, 3, 6200  # 49 600 bytes a row
    rng = np.random.default_rng(7)
    x = store_of(N, C, size, rng)
    lo, hi, pos = tables(2, size, rng)
    want_h, want_r = first_failure_slots(x.reshape(N * C, size), lo, hi, pos)
    eng = engine(C)
    d = eng.to_device(x)
    for algo in ALGOS:
        h, r = run(eng, d, lo, hi, pos, None, algo)
        assert np.array_equal(h, want_h) and np.array_equal(r, want_r), algo
    eng.close()


def test_short_form_workgroups_that_walk_several_tiles():
    """More tiles than the short form launches workgroups (eight per compute unit): a workgroup walks the tiles b, b + grid, ..,
    writing its LDS tile and its r values again and, with 3 slots, keeping h in LDS counters until its last tile (with 5 slots
    5 x 514 counters are more than it keeps: the atomics go to the output).  513 selected elements of rows of 3 make 64 lanes a row
    and 4 rows a tile; 24 577 rows are 6145 tiles, more than 8 x 768."""
    N, C, size, n = 24577, 1, 3, 513
    rng = np.random.default_rng(11)
    x = store_of(N, C, size, rng)
    idx = rng.integers(0, size, n)
    eng = engine(C)
    d = eng.to_device(x)
    for L in (3, 5):
        lo, hi, pos = tables(L, n, rng)
        # lower bounds from the grid of the draws, mostly far down: which places fail depends on the value, so r takes many values
        lo = np.where(rng.random((L, n)) < 0.8, -9.0, rng.choice(np.arange(-4.5, 0.5, 0.5), (L, n)))
        hi = np.full((L, n), np.inf)
        want_h, want_r = first_failure_slots(x.reshape(N, size), lo, hi, pos, idx)
        assert np.all(np.count_nonzero(want_h, axis=1) >= 6)
        for algo in (1, 2, 1):
            h, r = run(eng, d, lo, hi, pos, idx, algo)
            assert np.array_equal(r, want_r) and np.array_equal(h, want_h), (L, algo)
    eng.close()


def abi(eng, d, lo, hi, pos, h, r=None, idx=None, n_slots=1, algo=0, n_iter=None, size=None, n_idx=None, store=True):
    from openmcmc_amd import _abi

    N, _, sz = d.shape
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    st = _abi.lib.omc_store_first_failure(eng._ctx, N if n_iter is None else n_iter, sz if size is None else size, p(d) if store else None,
                                          p(idx), (sz if idx is None else idx.numel()) if n_idx is None else n_idx, n_slots, p(lo),
                                          p(hi), p(pos), algo, p(h), p(r))
    return st, _abi.lib.omc_last_error().decode()


def test_invalid_calls_say_why_and_write_nothing():
    import torch

    from openmcmc_amd import _abi

    N, C, size = 4, 3, 5
    eng = engine(C)
    d = eng.to_device(np.random.default_rng(23).standard_normal((N, C, size)))
    dev = d.device
    lo, hi = eng.full((8, size), -np.inf), eng.full((8, size), np.inf)
    pos = torch.arange(size, dtype=torch.int32, device=dev).repeat(8, 1).contiguous()
    h = torch.full((8, size + 1), -7, dtype=torch.int64, device=dev)
    r = torch.full((8, N, C), -7, dtype=torch.int32, device=dev)

    def untouched():
        eng.synchronize()
        return bool((h == -7).all()) and bool((r == -7).all())

    cases = [({"store": False}, "NULL"), ({"lo": None}, "NULL"), ({"hi": None}, "NULL"), ({"pos": None}, "NULL"), ({"h": None}, "NULL"),
             ({"n_iter": 0}, "n_iter"), ({"size": 0}, "size"), ({"n_idx": 0}, "n_idx"), ({"n_idx": size - 1}, "n_idx != size"),
             ({"n_slots": 0}, "n_slots"), ({"n_slots": 9}, "n_slots"), ({"algo": 3}, "algo"), ({"algo": -1}, "algo")]
    for kw, text_has in cases:
        args = {"lo": lo, "hi": hi, "pos": pos, "h": h, "r": r}
        args.update(kw)
        st, text = abi(eng, d, **args)
        assert st == _abi.INVALID_ARG and text_has in text and untouched(), (kw, text)
    for algo in ALGOS:
        for bad in ([0, 1, size], [-1, 2, 3]):
            idx = torch.as_tensor(bad, dtype=torch.int64, device=dev)
            st, text = abi(eng, d, lo, hi, pos, h, r, idx=idx, algo=algo)
            assert st == _abi.INVALID_ARG and "index outside" in text and untouched()
        for slot, k, v in ((0, 0, -1), (0, size - 1, size), (7, 2, size), (7, 4, -(2 ** 31))):
            bad_pos = pos.clone()
            bad_pos[slot, k] = v
            st, text = abi(eng, d, lo, hi, bad_pos, h, r, n_slots=8, algo=algo)
            assert st == _abi.INVALID_ARG and "pos entry outside" in text and untouched(), (slot, k, v)
        bad_pos = pos.clone()
        bad_pos[7, 2] = size  # beyond the slots of the call: not read
        assert abi(eng, d, lo, hi, bad_pos, h.clone(), None, n_slots=7, algo=algo)[0] == _abi.OK
    with pytest.raises(ValueError, match="index outside"):
        eng.store_first_failure(d, lo[0, :2], hi[0, :2], [0, 1], index=[0, size])
    with pytest.raises(ValueError, match=r"pos must lie in \[0, 5\)"):
        eng.store_first_failure(d, lo[0], hi[0], [0, 1, 2, 3, size])
    with pytest.raises(ValueError, match="must hold integers"):
        eng.store_first_failure(d, lo[0], hi[0], np.arange(size, dtype=float))
    with pytest.raises(ValueError, match="one value per selected element"):
        eng.store_first_failure(d, lo[0], hi[0], pos[0], index=[0, 1])
    with pytest.raises(ValueError, match="between 1 and 8 slots"):
        eng.store_first_failure(d, eng.full((9, size), 0.0), eng.full((9, size), 1.0), pos[:1].repeat(9, 1))
    # rows_out may be NULL; a pos that is no permutation gives what the definition gives
    st, _ = abi(eng, d, lo, hi, pos, h, None, n_slots=8)
    assert st == _abi.OK and h.cpu().numpy().tolist() == [[0] * size + [N * C]] * 8 and bool((r == -7).all())
    x = d.cpu().numpy().reshape(N * C, size)
    same_pos = np.full((1, size), 2)
    got = eng.store_first_failure(d, np.zeros(size), np.full(size, np.inf), same_pos)[0].cpu().numpy()
    assert np.array_equal(got, first_failure_slots(x, np.zeros((1, size)), np.full((1, size), np.inf), same_pos)[0])
    eng.close()
