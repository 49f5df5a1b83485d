#!/usr/bin/env python3
"""Is the host layer of the Metropolis-Hastings samplers (sampler/metropolis_hastings.py, sampler/reversible_jump.py and the fused-step
wrappers of engine.py) as fast in the working tree as in another revision of the Python package?

    mkdir -p build/ab/parent && git archive HEAD~1 openmcmc_amd tests benchmarks bench.py oracle | tar -x -C build/ab/parent
    python3 benchmarks/mh_host_ab.py [--before build/ab/parent] [--rounds 5] [--out profiles/mh_host_refactor_ab.txt]

The method, the runner and the table are those of benchmarks/normal_normal_ab.py: child processes of the two trees alternate, one at a
time and each under its own time limit, for `--rounds` rounds on one libomcmc_hip.so; the first child that fails ends the run.  Only the
lines are new, the ones this code bounds: cfg4 by blocks of steps and by single steps, cfg5, ManifoldMALA and RandomWalk through
MCMC.run_mcmc (one figure per sampler) and the transformed-parameter step (the fused and the launch-by-launch route per p).  The bar
per figure: the working tree's median is no slower than the other tree's median plus that tree's own spread (max - min over its
rounds).  The default headline does not pass through this code: once per tree at the end, as a sanity check.
"""
import json
import re
import sys

from normal_normal_ab import main, ms_per_sweep, run

LINES = [("bench.py --config cfg4 --no-cpu", ["bench.py", "--config", "cfg4", "--no-cpu"]),
         ("bench.py --config cfg4 --mala-single --no-cpu", ["bench.py", "--config", "cfg4", "--mala-single", "--no-cpu"]),
         ("bench.py --config cfg5 --no-cpu", ["bench.py", "--config", "cfg5", "--no-cpu"]),
         ("mala_through_mcmc.py", ["benchmarks/mala_through_mcmc.py"]),
         ("transform_mala.py", ["benchmarks/transform_mala.py"])]


def figures(tree, command):
    """{name of a figure within the line: ms} of one child: bench.py gives one, the two scripts one per sampler / route and size"""
    if command[0] == "bench.py":
        return {"": ms_per_sweep(tree, command)}
    text = run(tree, command)[1]
    if command[0].endswith("mala_through_mcmc.py"):
        return {f" {name}": float(ms) for name, ms in re.findall(r"^(\w+) d=\d+ C=\d+: ([0-9.]+) ms per step", text, re.M)}
    found = {}
    for rec in (json.loads(line) for line in text.splitlines() if line.startswith("{")):
        for route in ("fused", "general"):
            found[f" p={rec['p']} {route}"] = rec[f"{route}_us_per_step_median"] / 1e3
    return found


if __name__ == "__main__":
    sys.exit(main(LINES, figures))
