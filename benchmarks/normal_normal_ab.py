#!/usr/bin/env python3
"""Is the host layer of the NormalNormal models as fast in the working tree as in another revision of the Python package?

    mkdir -p build/ab/parent && git archive HEAD~1 openmcmc_amd tests benchmarks bench.py oracle | tar -x -C build/ab/parent
    python3 benchmarks/normal_normal_ab.py [--before build/ab/parent] [--rounds 5] [--out profiles/normal_normal_refactor_ab.txt]

These models are bound by host calls, so their time per sweep is what a change of sampler/sampler.py or mcmc.py can move.  Child
processes of the two trees alternate, one at a time, for `--rounds` rounds; both load the in-tree libomcmc_hip.so; every child
runs its own tree's copy of the script and prints its own milliseconds per sweep.  The bar: the working tree's median is no slower
than the other tree's median plus that tree's own spread (max - min over its rounds), the noise of this measurement on this box.
bench.py's default run (the headline) drives the C ABI directly and does not pass through this code: it is run once per tree at the
end, as a sanity check.  Exit status 1 if a line misses the bar, 2 if a child failed (nothing more is started then).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINES = [("bench.py --config cfg5 --no-cpu", ["bench.py", "--config", "cfg5", "--no-cpu"]),
         ("hierarchical_smoother.py", ["benchmarks/hierarchical_smoother.py"]),
         ("smoother_plus_regression.py", ["benchmarks/smoother_plus_regression.py"]),
         ("two_block_regression.py", ["benchmarks/two_block_regression.py"]),
         ("linreg_through_mcmc.py", ["benchmarks/linreg_through_mcmc.py"]),
         ("mixture_regression.py", ["benchmarks/mixture_regression.py"])]
HEADLINE = ["bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20", "--no-cpu"]


class ChildFailed(Exception):
    pass


def run(tree, command):
    """(the last JSON line of the child's output or None, its whole output)"""
    env = dict(os.environ, OMC_HIP_LIB=os.path.join(ROOT, "openmcmc_amd", "libomcmc_hip.so"))
    got = subprocess.run([sys.executable] + command, cwd=tree, env=env, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if got.returncode != 0:
        raise ChildFailed(f"{' '.join(command)} in {tree} ended with status {got.returncode}:\n{got.stdout[-2000:]}")
    last = None
    for line in got.stdout.splitlines():
        if line.startswith("{"):
            last = json.loads(line)
    return last, got.stdout


def ms_per_sweep(tree, command):
    last, text = run(tree, command)
    if last is not None:
        return float(last["ms_per_step"])
    return float(re.search(r"([0-9.]+) ms per sweep", text).group(1))


def figures(tree, command):
    """{name of a figure within the line ("" where it has one): ms} of one child"""
    return {"": ms_per_sweep(tree, command)}


def main(lines=LINES, figures=figures):
    """The alternating rounds and the table; another set of lines (benchmarks/mh_host_ab.py) passes its own and how to read them."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", default="build/ab/parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    trees = {"before": os.path.join(ROOT, args.before), "after": ROOT}
    ms = {}
    try:
        for r in range(args.rounds):
            for label, command in lines:
                for name, tree in trees.items():
                    for sub, value in figures(tree, command).items():
                        ms.setdefault((label + sub, name), []).append(value)
                        print(f"round {r + 1}: {label + sub:34s} {name:6s} {value:9.3f} ms per sweep", flush=True)
        headline = {name: run(tree, HEADLINE)[0] for name, tree in trees.items()}
    except (ChildFailed, subprocess.TimeoutExpired) as e:
        print(e)
        return 2
    rows = [f"before = {args.before}, after = the working tree, one library; ms per sweep, median [min, max] over {args.rounds} alternating rounds;",
            "bar: after's median <= before's median + before's spread (max - min)", "",
            f"{'line':34s} {'before':>28s} {'after':>28s} {'bar':>9s}  verdict"]
    missed = 0
    for label in dict.fromkeys(label for label, _ in ms):
        b, a = ms[label, "before"], ms[label, "after"]
        bar = statistics.median(b) + max(b) - min(b)
        ok = statistics.median(a) <= bar
        missed += not ok
        cell = lambda v: f"{statistics.median(v):9.3f} [{min(v):8.3f}, {max(v):8.3f}]"  # noqa: E731
        rows.append(f"{label:34s} {cell(b)} {cell(a)} {bar:9.3f}  {'no slower' if ok else 'SLOWER'}")
    rows += ["", f"headline (bench.py {' '.join(HEADLINE[1:])}, once per tree; not through this code): " +
             ", ".join(f"{name} {h['value']:.4g} {h['unit']} ({h['ms_per_step']:.3f} ms per step)" for name, h in headline.items())]
    print("\n".join(rows))
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(rows) + "\n")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
