"""The blocked band kernel's LDS images and its choice of form, as host arithmetic (openmcmc_amd/csrc/omc_band_common.h built for
the host by tests/native/band_layout_host.hip): every region at least as large as k_band_blocked indexes it, for every bandwidth
and every instantiation; the bytes launched; and every form the selector returns inside that instantiation's limits.  The needs
are spelled out here, independently of the struct: a region shortened in the header (the ring of solutions one block short for
w < NB, the backward image larger than the forward one on a narrow 8-column form) fails this test without a GPU."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024
PAIRS = [(16, 256), (8, 256), (8, 512), (16, 512)]
L_FIELDS = ("w NB NT W1 WS WP PS FBS ring rring Ld P dv Us misc fwd_end WB xs ms Sx Sm Lb Part dump diag bwd_end bytes").split()


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("native") / "band_layout_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "openmcmc_amd", "csrc"), os.path.join(ROOT, "tests", "native", "band_layout_host.hip"),
                    "-o", exe], check=True)
    out = {"F": [], "M": [], "L": [], "S": []}
    for line in subprocess.run([exe], capture_output=True, check=True, text=True).stdout.splitlines():
        tag, *v = line.split()
        out[tag].append(tuple(int(x) for x in v))
    return out


def parent_blocked_lds(w, NB, NT):
    """The formula the host sized the allocation with before the layout struct (blocked_lds of omc_bandwide.hip), restated."""
    W1, WS, WP, PS = w + 1, w + NB, (w + 15) & ~15, NB + 1
    fwd = WS * W1 + WS + 2 * (WP * PS + NB * PS + 2 * NB) + 2 + 64 + 2
    qpc = (NT - 64) // NB // 4
    bwd = 2 * (w + 2 * NB) + 2 * NB + NB * PS + 4 * NB * qpc + 64 + NB
    return max(fwd, bwd) * 8


def in_order(regions, end):
    """regions: (name, offset, doubles the kernel indexes) in the order they are laid out; each ends before the next begins."""
    for (name, at, need), (_, nxt, _) in zip(regions, regions[1:] + [("end", end, 0)]):
        assert at >= 0 and need > 0 and at + need <= nxt, (name, at, need, nxt)


def test_every_shape_is_enumerated(records):
    assert sorted({(r[1], r[2]) for r in records["L"]}) == sorted(PAIRS)
    assert sorted({(f[0], f[1]) for f in records["F"]}) == sorted(PAIRS) and len(records["F"]) == 9
    assert sorted({r[0] for r in records["L"]}) == list(range(1, 129)) and len(records["L"]) == 128 * len(PAIRS)


def test_images_hold_what_the_kernel_indexes(records):
    (fail, zero, dump0, counter, misc_slots), = records["M"]
    # misc: the flag, the zero, one dump slot per lane of a wave and the counter are distinct slots inside it
    assert len({fail, zero, counter} | set(range(dump0, dump0 + 64))) == 67 and max(fail, zero, counter, dump0 + 63) < misc_slots
    for rec in records["L"]:
        l = dict(zip(L_FIELDS, rec))
        w, NB, NT = l["w"], l["NB"], l["NT"]
        assert l["W1"] == w + 1 and l["PS"] == NB + 1
        assert l["WS"] >= w + NB                              # the open columns: the block and the w behind it
        assert l["WP"] % 16 == 0 and w <= l["WP"] < w + 16    # panel rows in whole 16 x 16 tiles
        # ---- forward image.  A copy of the block column is Ld, P, dv, Us; the second copy lies FBS behind the first.
        copy = [("Ld", l["Ld"], NB * (NB + 1)), ("P", l["P"], l["WP"] * (NB + 1)), ("dv", l["dv"], NB), ("Us", l["Us"], NB)]
        in_order([("ring", l["ring"], (w + NB) * (w + 1)), ("rring", l["rring"], w + NB)] + copy
                 + [(n + "'", at + l["FBS"], need) for n, at, need in copy] + [("misc", l["misc"], misc_slots)], l["fwd_end"])
        assert l["ring"] == 0                                  # zero_at, dump_at, ld_at, dv_at count from the ring's first double
        assert l["rring"] == l["WS"] * l["W1"]                 # ring[slot * W1 + d], slot < WS, and the right-hand side as one more row
        assert l["P"] == l["Ld"] + NB * l["PS"]                # rows of the block column are read through Ld[row * PS + b], row < NB + w
        # ---- backward image
        qpc = (NT - 64) // NB // 4                             # quads of far threads per column
        assert qpc >= 1 and 4 * qpc * NB == NT - 64
        in_order([("xs", l["xs"], w + 2 * NB), ("ms", l["ms"], w + 2 * NB), ("Sx", l["Sx"], NB), ("Sm", l["Sm"], NB),
                  ("Lb", l["Lb"], NB * (NB + 1)), ("Part", l["Part"], 4 * NB * qpc), ("dump", l["dump"], 64), ("diag", l["diag"], NB)],
                 l["bwd_end"])
        assert l["WB"] >= w + 2 * NB and l["xs"] == 0 and l["ms"] == l["xs"] + l["WB"]  # (the two rings are cleared as one array)
        # ---- the allocation
        assert l["bytes"] >= 8 * max(l["fwd_end"], l["bwd_end"])
        assert l["bytes"] == parent_blocked_lds(w, NB, NT), (w, NB, NT)


def form_ok(w, form, limits, nbytes):
    NB, NT, _, _ = form
    wmax, wgs = limits[form]
    return (w <= wmax and -(-w // 16) <= NT // 64 and -(-(w + 1) // (64 - NB)) <= NT // 64
            and parent_blocked_lds(w, NB, NT) * wgs <= LDS_LIMIT and nbytes[(w, NB, NT)] * wgs <= LDS_LIMIT)


def test_selector_stays_inside_each_forms_limits(records):
    limits = {f[:4]: f[4:] for f in records["F"]}
    nbytes = {r[:3]: r[-1] for r in records["L"]}
    assert {(s[2], s[3]) for s in records["S"]} == {(c, f) for c in (256, 257, 768, 769, 1024) for f in (0, 4, 8, 16, 512)}
    assert {s[0] for s in records["S"]} >= set(range(1, 129)) and {s[1] for s in records["S"]} == {1, 2, 3, 4}
    for w, n_terms, n_chains, forced, *form in records["S"]:
        form = tuple(form)
        if form[0] == 0:  # none: outside the kernel's range, or nothing instantiated would do
            assert not (1 <= w <= 128) or not any(f[2] >= n_terms and form_ok(w, f, limits, nbytes) for f in limits), (w, n_terms, forced)
            continue
        assert 1 <= w <= 128 and form in limits, (w, n_terms, n_chains, forced, form)
        assert form[2] >= n_terms                                       # compiled for at least the terms of the model
        assert form_ok(w, form, limits, nbytes), (w, n_terms, n_chains, forced, form)
    # 16 columns per step stop where their image stops fitting, not at a number kept beside it
    wide = limits[(16, 512, 2, 1)][0]
    assert parent_blocked_lds(wide, 16, 512) <= LDS_LIMIT < parent_blocked_lds(wide + 1, 16, 512)
