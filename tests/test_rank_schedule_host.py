"""The bitonic network behind omc_store_ranks as host arithmetic (no GPU): the launch list omc_store_rank_schedule returns for a
column of S keys and a tile of T is replayed here in numpy, compare-exchange by compare-exchange as include/omcmc_hip.h words
it, and must sort.  The entry points walk the same list, so a stage or a stride missing from it shows here."""

import ctypes

import numpy as np
import pytest

CASES = [(1, 64), (63, 64), (64, 64), (65, 64), (200, 64), (4100, 64), (4100, 4096), (8193, 8192)]


def schedule(S, tile, cap=4096):
    from openmcmc_amd import _abi

    n = ctypes.c_int64(-1)
    out = (ctypes.c_int64 * (3 * cap))()
    status = _abi.lib.omc_store_rank_schedule(S, tile, out, cap, ctypes.byref(n))
    return status, n.value, [tuple(out[3 * i: 3 * i + 3]) for i in range(max(0, min(n.value, cap)))]


def compare_exchange(a, k, j):
    """stride j of stage k on the whole column: positions i (bit j clear) and i + j, ascending where bit k of i is clear"""
    i = np.arange(a.size)
    i = i[(i & j) == 0]
    lo, hi = np.minimum(a[i], a[i + j]), np.maximum(a[i], a[i + j])
    up = (i & k) == 0
    a[i], a[i + j] = np.where(up, lo, hi), np.where(up, hi, lo)


def replay(launches, a, T):
    """the launch list applied to a column a of P keys; every launch is checked against what its kind allows"""
    for kind, k, j in launches:
        if kind == 0:  # every tile: stages 2 .. k = T, all their strides
            assert k == T and j == T // 2
            kk = 2
            while kk <= k:
                jj = kk // 2
                while jj >= 1:
                    compare_exchange(a, kk, jj)
                    jj //= 2
                kk *= 2
        elif kind == 1:  # one stride that leaves the tile
            assert T <= j < k <= a.size
            compare_exchange(a, k, j)
        else:  # the strides inside the tile of a later stage
            assert kind == 2 and j == T // 2 and T < k <= a.size
            jj = j
            while jj >= 1:
                compare_exchange(a, k, jj)
                jj //= 2
    return a


def columns(S, P, rng):
    pad = np.uint64(0xFFFFFFFFFFFFFFFF)
    cols = [rng.integers(0, 2 ** 64, size=S, dtype=np.uint64, endpoint=False),
            rng.integers(0, 3, size=S, dtype=np.uint64),                       # many equal keys
            np.full(S, 7, dtype=np.uint64),                                    # all equal
            np.arange(S, dtype=np.uint64)[::-1].copy(),                        # descending
            (rng.integers(0, 2 ** 64, size=S, dtype=np.uint64, endpoint=False) >> np.uint64(60)) << np.uint64(60)]
    return [np.concatenate([c, np.full(P - S, pad, dtype=np.uint64)]) for c in cols]


@pytest.mark.parametrize("S,tile", CASES)
def test_schedule_sorts(S, tile):
    status, n, launches = schedule(S, tile)
    assert status == 0 and n == len(launches)
    P = 1
    while P < S:
        P *= 2
    T = min(tile, P)
    d = (P // T).bit_length() - 1
    if P == 1:
        assert launches == []
    else:
        kinds = [l[0] for l in launches]
        assert kinds.count(1) == d * (d + 1) // 2 and kinds.count(0) == 1 and kinds.count(2) == d and kinds[0] == 0
    rng = np.random.default_rng(S * 31 + tile)
    for col in columns(S, P, rng):
        got = replay(launches, col.copy(), T)
        assert np.array_equal(got, np.sort(col)), (S, tile)


def test_default_tile_is_8192():
    assert schedule(8193, 0) == schedule(8193, 8192)
    assert schedule(100000, 0)[2] == schedule(100000, 8192)[2]


def test_too_small_a_capacity_and_bad_arguments_are_rejected():
    from openmcmc_amd import _abi

    status, n, _ = schedule(4100, 64)
    assert status == _abi.OK and n > 1
    status2, n2, _ = schedule(4100, 64, cap=n - 1)
    assert status2 == _abi.INVALID_ARG and n2 == n  # the count is still reported
    assert schedule(4100, 64, cap=n)[0] == _abi.OK
    for tile in (1, 32, 63, 96, 16384, -64):
        assert schedule(100, tile)[0] == _abi.INVALID_ARG
    assert schedule(0, 64)[0] == _abi.INVALID_ARG
    out = (ctypes.c_int64 * 3)()
    assert _abi.lib.omc_store_rank_schedule(100, 64, out, 1, None) == _abi.INVALID_ARG
