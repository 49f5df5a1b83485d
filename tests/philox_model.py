"""Host (NumPy) model of the device random streams in openmcmc_amd/csrc/omc_common.h.
Philox4x32-10 is integer arithmetic: the device words must match these bit for bit."""

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
PURPOSE = {"normal": 0, "gamma": 1, "uniform": 2, "raw": 3}


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint32) for v in (c0, c1, c2, c3))
    k0, k1 = np.uint32(k0), np.uint32(k1)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c0.astype(np.uint64)
            p1 = M1 * c2.astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK).astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0, k1 = np.uint32(k0 + W0), np.uint32(k1 + W1)
    return c0, c1, c2, c3


def rng_blocks(seed, draw_index, purpose, global_chain, blocks):
    """Words of blocks `blocks` (array) for one chain; layout of omc_rng_block()."""
    blocks = np.asarray(blocks, dtype=np.uint32)
    c1 = np.full(blocks.shape, draw_index & 0xFFFFFFFF, dtype=np.uint32)
    c2 = np.full(blocks.shape, global_chain & 0xFFFFFFFF, dtype=np.uint32)
    c3v = (PURPOSE[purpose] << 24) | (((global_chain >> 32) & 0xFF) << 16) | ((draw_index >> 32) & 0xFFFF)
    c3 = np.full(blocks.shape, c3v, dtype=np.uint32)
    return philox4x32_10(blocks, c1, c2, c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def u53(lo, hi):
    v = lo.astype(np.uint64) ^ (hi.astype(np.uint64) << np.uint64(21))
    return 2.0**-53 + v.astype(np.float64) * 2.0**-53


def unit_mantissa(lo, hi20src):
    """float64 in [1, 2): mantissa = top 20 bits of hi20src, then all of lo (omc_unit_mantissa)."""
    bits = (np.uint64(0x3FF) << np.uint64(52)) | ((hi20src.astype(np.uint64) >> np.uint64(12)) << np.uint64(32)) \
        | lo.astype(np.uint64)
    return bits.view(np.float64)


def normal_pairs(x, y, z, w):
    """Words of one Philox block -> two N(0,1) (omc_normal_pair): Box-Muller with the radius uniform
    u = 2 - m(x, y) in (0, 1], the angle t = (m(z, w) - 3/2) pi/2 in [-pi/4, pi/4), a reflection x -> -x on
    bit 11 of w and a swap of the two coordinates on bit 10."""
    x, y, z, w = (np.asarray(v, dtype=np.uint32) for v in (x, y, z, w))
    u = 2.0 - unit_mantissa(x, y)
    r = np.sqrt(np.maximum(-2.0 * np.log(u), 0.0))
    t = (unit_mantissa(z, w) - 1.5) * (np.pi / 2)
    sn, cs = np.sin(t), np.cos(t)
    cs = np.where((w >> np.uint32(11)) & np.uint32(1), -cs, cs)
    swap = ((w >> np.uint32(10)) & np.uint32(1)).astype(bool)
    return np.where(swap, cs, sn) * r, np.where(swap, sn, cs) * r


def normals(seed, draw_index, global_chain, n):
    """First n N(0,1) of the chain's 'normal' stream."""
    nb = (n + 1) // 2
    x, y, z, w = rng_blocks(seed, draw_index, "normal", global_chain, np.arange(nb))
    out = np.empty(2 * nb)
    out[0::2], out[1::2] = normal_pairs(x, y, z, w)
    return out[:n]


def uniforms(seed, draw_index, global_chain, n, sub=0):
    """First n elements of the chain's 'uniform' stream as omc_elem_uniform defines them: element e is half e & 1 of
    block sub + (e >> 1), through u53.  Integer arithmetic and one exact scaling: the device's values bit for bit."""
    nb = (n + 1) // 2
    x, y, z, w = rng_blocks(seed, draw_index, "uniform", global_chain, (sub + np.arange(nb, dtype=np.uint64)) & MASK)
    out = np.empty(2 * nb)
    out[0::2], out[1::2] = u53(x, y), u53(z, w)
    return out[:n]


# ---- counters and the gamma stream (omc_common.h: field map, omc_standard_gamma) ----------------------------------
GAMMA_BLOCKS = 513      # blocks one Gamma(a) draw may read: 0 (the a < 1 boost) and 1 + 2j, 2 + 2j for 256 attempts
COMPONENT_SHIFT = 24    # mixture component k of k_mixture_normal_gamma reads blocks from (k + 1) << COMPONENT_SHIFT


def counter(purpose, draw_index, global_chain, block=0):
    """(c0, c1, c2, c3) of omc_rng_block() as Python ints."""
    c3 = (PURPOSE[purpose] << 24) | (((global_chain >> 32) & 0xFF) << 16) | ((draw_index >> 32) & 0xFFFF)
    return block & 0xFFFFFFFF, draw_index & 0xFFFFFFFF, global_chain & 0xFFFFFFFF, c3


def mixture_component_block0(k):
    """First block of mixture component k's gamma draw (k_mixture_normal_gamma)."""
    return (int(k) + 1) << COMPONENT_SHIFT


def standard_gamma(seed, draw_index, global_chain, a, block0=0):
    """Gamma(a, 1) of omc_standard_gamma (Marsaglia & Tsang, the device's block order).  Libm-level differences from the
    device only: a candidate lying within an ulp of its acceptance bound could be decided the other way."""
    def block(b):
        return [np.uint32(v[0]) for v in rng_blocks(seed, draw_index, "gamma", global_chain, [block0 + b])]

    boost = 1.0
    if a < 1.0:
        x, y, _, _ = block(0)
        boost = np.exp(np.log(u53(np.array([x]), np.array([y]))[0]) / a)
        a += 1.0
    d = a - 1.0 / 3.0
    cst = 1.0 / np.sqrt(9.0 * d)
    for attempt in range(256):
        n0, n1 = normal_pairs(*block(1 + 2 * attempt))
        x, y, z, w = block(2 + 2 * attempt)
        uu = u53(np.array([x, z]), np.array([y, w]))
        for xn, u in ((float(n0), uu[0]), (float(n1), uu[1])):
            v = 1.0 + cst * xn
            if not v > 0.0:
                continue
            v = v * v * v
            x2 = xn * xn
            if u < 1.0 - 0.0331 * x2 * x2 or np.log(u) < 0.5 * x2 + d * ((1.0 - v) + np.log(v)):
                return boost * d * v
    return boost * d
