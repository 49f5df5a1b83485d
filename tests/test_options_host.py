"""The option table (openmcmc_amd/csrc/omc_options.h) without a device: tests/native/options_host.hip applies probes to a
default-constructed context and prints every option's member after each.  Held to the frozen expectation of
tests/options_expect.py: the defaults, both ends of every range and every member of every set accepted, the nearest values outside
rejected with nothing changed, what run_reenter and the sweep clock's pair do besides, unknown names; and the table's names against
the sources that set options and against the documentation in include/omcmc_hip.h."""

import os
import re
import shutil
import subprocess

import pytest

import options_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("native") / "options_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "openmcmc_amd", "csrc"), os.path.join(ROOT, "tests", "native", "options_host.hip"),
                    "-o", out], check=True)
    return out


def run(exe, probes):
    """(table names, defaults {member: value}, [(status, {member: value})] per probe)"""
    text = "".join(f"{n} {v}\n" for n, v in probes)
    lines = subprocess.run([exe], input=text, capture_output=True, check=True, text=True).stdout.splitlines()
    rec = {t: [l.split()[1:] for l in lines if l.split()[0] == t] for t in "NRDP"}
    assert len(rec["N"]) == len(rec["R"]) == len(rec["D"]) == 1 and len(rec["P"]) == len(probes)
    members = rec["R"][0]
    as_dict = lambda v: dict(zip(members, (int(x) for x in v), strict=True))  # noqa: E731
    return rec["N"][0], as_dict(rec["D"][0]), [(int(p[0]), as_dict(p[1:])) for p in rec["P"]]


def follow(exe, probes):
    """every probe's status and every member afterwards, against the model"""
    _, first, got = run(exe, probes)
    state = E.defaults()
    assert first == state
    for (name, value), (status, after) in zip(probes, got, strict=True):
        if name == "!pos":
            state["sweep_times_pos"] = value
            want = E.OK
        else:
            before = dict(state)
            want = E.apply(state, name, value)
            if want != E.OK:
                assert state == before
        assert status == want, (name, value, status)
        assert after == state, (name, value, {k: (after[k], state[k]) for k in state if after[k] != state[k]})
    return state


def test_defaults(exe):
    names, first, _ = run(exe, [])
    assert sorted(names) == E.NAMES and len(set(names)) == len(names)
    assert first == E.defaults()
    for member, value in {"dev_cus": 256, "run_epoch": 1, "run_sweeps_per_launch": 32, "run_reenter": 2, "tridiag_newton_max": 4,
                          "dense_overlap": 1, "dense_blocked_min": 144, "mh_gemm_ksplit": 4, "band_seg_overlap": 192}.items():
        assert first[member] == value, member
    assert all(v == 0 for m, v in first.items() if m not in ("dev_cus", "run_epoch", "run_sweeps_per_launch", "run_reenter",
                                                            "tridiag_newton_max", "dense_overlap", "dense_blocked_min",
                                                            "mh_gemm_ksplit", "band_seg_overlap"))


def test_ranges_and_sets(exe):
    probes = E.plain_probes()
    for name, value in [("run_reenter", 3), ("tridiag_seg", 12), ("rank_tile", 96), ("rank_tile", 16384), ("band_seg_count", 1),
                        ("mh_gemm_ksplit", 3), ("dense_blocked_min", 0), ("dense_blocked_min", 32769)]:
        assert (name, value) in probes and value in E.PLAIN[name]["reject"]
    assert {n for n, _ in probes} == set(E.PLAIN)
    end = follow(exe, probes)
    want = E.defaults()
    want["run_reenter_force"] = 1
    assert end == want  # every option back at its default


def test_run_reenter_sets_force(exe):
    _, first, got = run(exe, [("run_reenter", 3), ("run_reenter", 2)])
    assert first["run_reenter_force"] == 0
    assert got[0][0] == E.INVALID_ARG and got[0][1]["run_reenter_force"] == 0  # a rejected value does not force
    assert got[1][0] == E.OK and got[1][1]["run_reenter_force"] == 1 and got[1][1]["run_reenter"] == 2


def test_pointers(exe):
    probes = [(n, v) for n in E.POINTERS for v in (0x7F0000001000, 0, -1, 0)]
    assert follow(exe, probes) == E.defaults()


def test_sweep_clock_cap_and_pointer(exe):
    a, b = 0x7F0000002000, 0x7F0000004000
    probes = []
    for p in E.clock_probes(a, b):  # the position stands at 5 before every probe: reset by the accepted ones, kept by the rejected
        probes += [("!pos", 5), p]
    _, _, got = run(exe, probes)
    by = dict(zip(range(len(probes)), got))
    idx = {i: p for i, p in enumerate(probes) if p[0] != "!pos"}
    seen = [(p, by[i][0], by[i][1]["sweep_times_ptr"], by[i][1]["sweep_times_cap"], by[i][1]["sweep_times_pos"]) for i, p in idx.items()]
    assert seen[0] == (("sweep_times_ptr", a), E.INVALID_ARG, 0, 0, 5)   # a pointer given at capacity 0
    assert seen[2] == (("sweep_times_cap", 63), E.INVALID_ARG, 0, 0, 5)  # a capacity of 63
    assert seen[7] == (("sweep_times_ptr", a), E.OK, a, 64, 0)           # a pointer given at capacity 64
    assert seen[11] == (("sweep_times_cap", 128), E.OK, 0, 128, 0)       # a change of capacity clears the pointer
    assert follow(exe, probes) == E.defaults()


def test_unknown_names(exe):
    probes = [(n, 1) for n in E.UNKNOWN]
    _, _, got = run(exe, probes)
    assert all(status == E.INVALID_ARG for status, _ in got)
    assert follow(exe, probes) == E.defaults()


def table_names(exe):
    return set(run(exe, [])[0])


def test_names_set_in_the_sources_are_in_the_table(exe):
    names = table_names(exe)
    files = [os.path.join(ROOT, "bench.py")]
    for top in ("openmcmc_amd", "tests", "benchmarks"):
        for d, _, fs in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(d, f) for f in fs if f.endswith((".py", ".sh", ".hip"))]
    used = {}
    for f in files:
        for m in re.finditer(r"""set_option\(\s*(?:[\w.]+\s*,\s*)?b?(["'])([\w ]*)\1""", open(f, encoding="utf-8").read()):
            used.setdefault(m.group(2), f)
    assert len(used) >= 20, sorted(used)  # the pattern still finds the calls
    unknown_on_purpose = set(E.UNKNOWN) | set(E.UNKNOWN_WITH_BLANKS)
    assert {n: f for n, f in used.items() if n not in names and n not in unknown_on_purpose} == {}


def test_names_of_the_table_are_documented(exe):
    header = open(os.path.join(ROOT, "include", "omcmc_hip.h"), encoding="utf-8").read()
    end = header.index("omc_status omc_ctx_set_option(")
    comment = header[header.rindex("/*", 0, end):end]
    missing = [n for n in sorted(table_names(exe)) if f'"{n}"' not in comment]
    assert missing == []
