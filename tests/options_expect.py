"""What omc_ctx_set_option accepts, frozen: every option's default, the values at the ends of its range (or every member of its
set), the nearest values outside, and what an accepted value leaves in the context.  Written from the documented behaviour, not
from the table of openmcmc_amd/csrc/omc_options.h, which tests/test_options_host.py (no device) and tests/test_options_gpu.py
(through Engine.set_option) hold to it."""

I64_MAX, I64_MIN = 2**63 - 1, -(2**63)
OK, INVALID_ARG = 0, 1
RING_MIN = 64


def _rng(default, lo, hi):
    return dict(default=default, accept=[lo, hi], reject=[lo - 1, hi + 1])


def _set(default, members, extra_reject=()):
    members = sorted(members)
    near = {m + d for m in members for d in (-1, 1)} | set(extra_reject)
    return dict(default=default, accept=members, reject=sorted(near - set(members)))


def _flag():  # any value, stored as value != 0
    return dict(default=0, accept=[0, 1, 2, -1, I64_MAX, I64_MIN], reject=[], store=lambda v: int(v != 0))


# the options whose rule is a range, a set or a flag; the sweep clock's pair and the pointers follow below
PLAIN = {
    "tridiag_algo": _rng(0, 0, 2),
    "tridiag_seg": _set(0, [0, 8, 10, 16, 20, 32], extra_reject=[12]),
    "run_sweeps_per_launch": _rng(32, 1, 32),
    "run_block_sweeps": _rng(0, 0, 32),
    "run_reenter": _rng(2, 0, 2),
    "tridiag_quad_skip": _rng(0, 0, 15),
    "tridiag_perturb_ppb": _rng(0, 0, 1_000_000_000),
    "tridiag_newton_max": _rng(4, 0, 64),
    "band_algo": _rng(0, 0, 3),
    "diag_algo": _rng(0, 0, 2),
    "hist_algo": _rng(0, 0, 1),
    "reduce_algo": _rng(0, 0, 2),
    "hist2d_algo": _rng(0, 0, 3),
    "rank_tile": _set(0, [0] + [2**k for k in range(6, 14)], extra_reject=[96, 16384, 32, -64]),
    "rank_chunk": dict(default=0, accept=[0, I64_MAX], reject=[-1, I64_MIN]),
    "autocorr_slice": dict(default=0, accept=[0, I64_MAX], reject=[-1, I64_MIN]),
    "band_seg_overlap": _rng(192, 8, 65536),
    "band_seg_count": dict(default=0, accept=[0, 2, 128], reject=[-1, 1, 129]),
    "band_blocked_threads": _set(0, [0, 4, 8, 16, 512]),
    "mh_gemm_ksplit": _set(4, [1, 2, 4]),
    "dense_blocked_min": _rng(144, 1, 32768),
    "dense_panel_old": _rng(0, 0, 1),
    "dense_overlap": _rng(1, 0, 1),
    "tridiag_generic": _flag(),
    "mh_use_rocblas": _flag(),
    "gram_use_rocblas": _flag(),
    "spectral_use_rocblas": _flag(),
    "dense_use_rocsolver": _flag(),
    # any value, stored as (int)value
    "debug_zero_z": dict(default=0, accept=[0, 1, -1, 2**31 - 1, -(2**31)], reject=[]),
}
POINTERS = ["stamps_ptr", "run_event_begin", "run_event_end"]  # any value, stored as the pointer or event; default 0
NAMES = sorted(list(PLAIN) + POINTERS + ["sweep_times_ptr", "sweep_times_cap"])
# members that are no option of their own
DEFAULTS_EXTRA = {"run_reenter_force": 0, "sweep_times_pos": 0, "dev_cus": 256, "run_epoch": 1}
COUNTERS = ["tridiag_join_fallbacks", "run_handoff_timeouts", "band_join_fallbacks", "band_join_retries", "wall_clock_khz",
            "reenter_abi_ok", "sweep_times_pos"]


def defaults():
    d = {n: PLAIN[n]["default"] for n in PLAIN}
    d.update({n: 0 for n in POINTERS + ["sweep_times_ptr", "sweep_times_cap"]})
    d.update(DEFAULTS_EXTRA)
    return d


def apply(state, name, value):
    """The documented effect of omc_ctx_set_option(name, value) on `state` (a dict as defaults() makes it): its status."""
    if name in PLAIN:
        o = PLAIN[name]
        if value in o["reject"]:
            return INVALID_ARG
        assert value in o["accept"] or value == o["default"], (name, value)  # the model knows the probed values only
        state[name] = o.get("store", lambda v: v)(value)
        if name == "run_reenter":
            state["run_reenter_force"] = 1
        return OK
    if name in POINTERS:
        state[name] = value
        return OK
    if name == "sweep_times_cap":
        if value != 0 and value < RING_MIN:
            return INVALID_ARG
        if value != state["sweep_times_cap"]:
            state["sweep_times_ptr"] = 0
        state["sweep_times_cap"] = value
        state["sweep_times_pos"] = 0
        return OK
    if name == "sweep_times_ptr":
        if value != 0 and state["sweep_times_cap"] < RING_MIN:
            return INVALID_ARG
        state["sweep_times_ptr"] = value
        state["sweep_times_pos"] = 0
        return OK
    return INVALID_ARG  # unknown name: nothing changed


def plain_probes():
    """(name, value) for every plain option: each accepted value, and after each of them every rejected one (so that "unchanged"
    is seen at more than the default), then the default again."""
    out = []
    for name, o in PLAIN.items():
        for r in o["reject"]:
            out.append((name, r))
        for a in o["accept"]:
            out.append((name, a))
            out.extend((name, r) for r in o["reject"])
        out.append((name, o["default"]))
    return out


def clock_probes(ptr_a, ptr_b):
    """The sweep clock's capacity and pointer (ptr_a, ptr_b: two non-zero addresses), ending with both off."""
    return [("sweep_times_ptr", ptr_a),   # at capacity 0: rejected
            ("sweep_times_ptr", 0),       # switching off is always accepted
            ("sweep_times_cap", 63), ("sweep_times_cap", 1), ("sweep_times_cap", -1),  # rejected
            ("sweep_times_ptr", ptr_a),   # still capacity 0
            ("sweep_times_cap", 64),
            ("sweep_times_ptr", ptr_a),   # accepted
            ("sweep_times_cap", 64),      # the same capacity keeps the pointer
            ("sweep_times_ptr", ptr_b),
            ("sweep_times_cap", 63),      # rejected: pointer and capacity stay
            ("sweep_times_cap", 128),     # a change of capacity clears the pointer
            ("sweep_times_ptr", ptr_a),
            ("sweep_times_cap", 0),       # ... also the change to 0
            ("sweep_times_ptr", ptr_b),   # rejected again
            ("sweep_times_ptr", 0)]


UNKNOWN = ["no_such_option", "tridiag_alg", "TRIDIAG_ALGO", "sweep_times_pos", "run_event_", "run_event_bogus"]
UNKNOWN_WITH_BLANKS = ["", "tridiag_algo ", " tridiag_algo"]  # not through the line-by-line probes of the host program
