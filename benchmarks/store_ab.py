#!/usr/bin/env python3
"""A/B timing of two builds of libomcmc_hip.so on the store-summary benchmarks at their default sizes.

    bash benchmarks/build_rev.sh HEAD~1 before
    python3 benchmarks/store_ab.py [--before build/ab/libomcmc_hip_before.so] [--rounds 5] [--out FILE] [script ...]

Per script (default: the fourteen benchmarks/store_*.py of the summaries) the two builds run alternately -- before, after, before,
after, ... -- one fresh process per run, the other build through OMC_HIP_LIB.  A case is every timing in milliseconds of the
script's JSON line that the library produces (host, numpy and torch routes are left out).  Per case: the median of either side and
the spread (max - min over the rounds) of the BEFORE side; the case passes when the median after is not above the median before
by more than that spread.  A run that fails ends everything.  Exit status 1 if a case does not pass.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ["store_covariance.py", "store_hdi.py", "store_rank_diagnostics.py", "store_histogram.py", "store_histogram2d.py",
           "store_derive.py", "store_summaries.py", "store_diagnostics.py", "store_autocorr.py", "store_project.py", "store_loo.py",
           "store_loo_expect.py", "store_ess.py", "store_kde.py"]
NOT_OURS = re.compile(r"host|numpy|torch|wall|mcmc_|(^|[/_ ])gram|scipy|arviz", re.I)


def cases(node, path="", not_ours=NOT_OURS):
    """{case: ms} of a script's JSON: numbers under keys ending in "ms", rows {"case": .., "ms": ..} under their label; the cases
    whose name matches `not_ours` are left out"""
    found = {}
    if isinstance(node, dict):
        if "case" in node and isinstance(node.get("ms"), (int, float)):
            return {f"{path}{node['case']}": float(node["ms"])}
        for k, v in node.items():
            if isinstance(v, (int, float)) and not isinstance(v, bool) and k.endswith("ms"):
                found[f"{path}{k}"] = float(v)
            elif isinstance(v, (dict, list)):
                found.update(cases(v, f"{path}{k}/", not_ours))
    elif isinstance(node, list):
        for i, v in enumerate(node):
            found.update(cases(v, path if isinstance(v, dict) and "case" in v else f"{path}{i}/", not_ours))
    return {k: v for k, v in found.items() if not not_ours.search(k)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", default="build/ab/libomcmc_hip_before.so")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("scripts", nargs="*", default=SCRIPTS)
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None

    def say(text):
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    failed = 0
    say(f"before = {args.before}, after = the in-tree build; {args.rounds} rounds per script, before and after alternately; ms")
    for script in args.scripts:
        ms = {"before": {}, "after": {}}
        for r in range(args.rounds):
            for side in ("before", "after"):
                env = dict(os.environ)
                env.pop("OMC_HIP_LIB", None)
                if side == "before":
                    env["OMC_HIP_LIB"] = os.path.join(ROOT, args.before)
                run = subprocess.run([sys.executable, os.path.join(ROOT, "benchmarks", script)], env=env, capture_output=True, text=True, timeout=600)
                lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
                if run.returncode != 0 or not lines:
                    say(f"{script} round {r} {side}: status {run.returncode}\n{run.stderr[-1500:]}")
                    return 2
                for k, v in cases(json.loads(lines[-1])).items():
                    ms[side].setdefault(k, []).append(v)
        say(f"{script}")
        say(f"  {'case':<100s} {'before':>10s} {'spread':>10s} {'after':>10s}  verdict")
        for k in ms["before"]:
            b, a = ms["before"][k], ms["after"].get(k, [])
            mb, ma, spread = statistics.median(b), statistics.median(a), max(b) - min(b)
            ok = ma <= mb + spread
            failed += not ok
            say(f"  {k[:100]:<100s} {mb:10.3f} {spread:10.3f} {ma:10.3f}  {'pass' if ok else 'FAIL'}")
    say(f"{failed} cases fail")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
