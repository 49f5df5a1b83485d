"""The draw-index conventions of the library, laid out as Philox counters (the field map in omc_common.h): no two distinct
draws within the supported ranges may read the same counter.  CPU only: the counters come from tests/philox_model.py,
which the GPU tests hold to the device bit for bit (test_rng_gpu.py, test_mixture_ragged_kernels_gpu.py)."""

import itertools

import philox_model as pm

NS = 1 << 8            # samplers per sweep: positions < 2^8
T_MAX = 1 << 32        # sweeps
SUB_MAX = 16           # sub-stream field, bits 44-47 of the draw index
K_MAX = 255            # mixture components (omc_mixture_normal_gamma's limit)
CHAIN_MAX = 1 << 40    # global chain ids

# edge values of every field: both ends, the powers of two and their neighbours (a field that overlaps another shows up
# where one field's low bit meets the other's high bit)
T_VALS = sorted({0, 1, 2, 3, T_MAX - 1} | {v for j in (7, 8, 15, 16, 24, 31) for v in (2**j - 1, 2**j)})
POS_VALS = [0, 1, 2, 15, 16, 127, 128, NS - 1]
SUB_VALS = [0, 1, 2, 4, 8, SUB_MAX - 1]
COMP_VALS = [None, 0, 1, 2, 15, 16, 17, 127, 128, K_MAX - 1]
CHAIN_VALS = [0, 1, 2, 2**32 - 1, 2**32, 2**32 + 1, 2**39, CHAIN_MAX - 1]


def sweep_draw(t, pos):
    """Sampler draw of sweep t at position pos (sampler.py _draw_index; mcmc.py's fused sweep and its Gamma blocks)."""
    return t * NS + pos


def fused_run_draw(t0, t, gdraw):
    """omc_gmrf_run: sweep t of a run that starts at sweep t0 has rec.draw = draw_index0 + t * draws_per_sweep with
    draw_index0 = t0 * ns (mcmc.py), and its Gamma term k draws at rec.draw + gdraw[k], gdraw[k] = the block's position
    (omc_tridiag_args.h sweep_gamma_key)."""
    return (t0 * NS + t * NS) + gdraw


def prior_draw(pos):
    return (1 << 40) + pos  # mcmc.py: start values drawn from the prior


def with_sub(draw, sub):
    return draw + ((sub & 0xF) << 44)  # distribution.py Gamma.rvs, location_scale.py Normal columns


def draws():
    """(tuple, purpose, draw index, block range) of every convention over the edge values."""
    for purpose in pm.PURPOSE:
        comps = COMP_VALS if purpose == "gamma" else [None]
        blocks = pm.GAMMA_BLOCKS if purpose == "gamma" else 1 << 32
        kinds = [("sweep", t, pos) for t in T_VALS for pos in POS_VALS] + [("prior", None, pos) for pos in POS_VALS]
        for (kind, t, pos), sub, comp in itertools.product(kinds, SUB_VALS, comps):
            d = with_sub(sweep_draw(t, pos) if kind == "sweep" else prior_draw(pos), sub)
            b0 = 0 if comp is None else pm.mixture_component_block0(comp)
            yield (purpose, kind, t, pos, sub, comp), purpose, d, b0, blocks


def test_fused_run_draws_are_the_sampler_draws():
    for t0, t, pos in itertools.product([0, 1, 7, T_MAX // 2], [0, 1, 5], [1, 2, NS - 1]):
        assert fused_run_draw(t0, t, pos) == sweep_draw(t0 + t, pos)


def test_draw_index_fields_fit_48_bits():
    assert sweep_draw(T_MAX - 1, NS - 1) < 1 << 40
    assert with_sub(prior_draw(NS - 1), SUB_MAX - 1) < 1 << 48
    assert pm.mixture_component_block0(K_MAX - 1) + pm.GAMMA_BLOCKS <= 1 << 32


def test_no_two_draws_share_a_counter():
    """Every (purpose, kind, sweep, position, sub, component, chain) owns its counters: same (c1, c2, c3) words only with
    disjoint block ranges."""
    seen = {}
    n = 0
    for key, purpose, d, b0, nb in draws():
        for chain in CHAIN_VALS:
            c0, c1, c2, c3 = pm.counter(purpose, d, chain, b0)
            assert c0 == b0  # the block range does not wrap the 32-bit word
            seen.setdefault((c1, c2, c3), []).append((b0, b0 + nb, key + (chain,)))
            n += 1
    clashes = []
    for words, owners in seen.items():
        owners.sort(key=lambda o: o[:2])
        for (lo0, hi0, k0), (lo1, hi1, k1) in zip(owners, owners[1:]):
            if lo1 < hi0:
                clashes.append((k0, k1))
    assert n > 50000
    assert not clashes, f"{len(clashes)} pairs of draws share Philox counters, e.g. {clashes[:3]}"
