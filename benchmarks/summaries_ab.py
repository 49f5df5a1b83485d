#!/usr/bin/env python3
"""Are the posterior summaries of the device store (openmcmc_amd/summary on openmcmc_amd/engine_store.py) as fast in the working tree
as in another revision of the Python package?

    mkdir -p build/ab/parent && git archive HEAD~1 openmcmc_amd tests benchmarks bench.py oracle | tar -x -C build/ab/parent
    python3 benchmarks/summaries_ab.py [--before build/ab/parent] [--rounds 5] [--out profiles/summaries_refactor_ab.txt] [script.py ...]

The method, the runner and the table are those of benchmarks/normal_normal_ab.py, as in benchmarks/mh_host_ab.py: child processes of the
two trees alternate, one at a time and each under its own time limit, for `--rounds` rounds on one libomcmc_hip.so; the first child that
fails ends the run.  The kernels are the same library in both trees, so what can move is the Python time per call.  The lines are the six
store benchmarks that go through the moved code at their default sizes (all of them, or the ones named on the command line); a figure is
every timing in milliseconds of a script's JSON line that the package produces -- device-timed wrapper calls and the end-to-end wall clock
of the MCMC methods alike; the host, numpy, scipy and torch routes beside them are left out.  The bar per figure: the working tree's
median is no slower than the other tree's median plus that tree's own spread (max - min over its rounds).  The default headline does not
pass through this code: once per tree at the end, as a sanity check.
"""
import re
import sys

from normal_normal_ab import main, run
from store_ab import cases

SCRIPTS = ["store_histogram.py", "store_kde.py", "store_kde2d.py", "store_derive.py", "store_loo.py", "store_hdi.py"]
NOT_OURS = re.compile(r"host|numpy|torch|scipy|arviz", re.I)  # (store_ab.py's own pattern also drops the wall-clock figures: kept here)


def figures(tree, command):
    """{figure within the line: ms} of one child, by the reading of benchmarks/store_ab.py.  A figure's name must be the same in every
    round: what a row's label says in brackets (some hold a measured time) is left out, and rows of one name are numbered in order."""
    found = {}
    for k, v in cases(run(tree, command)[0], not_ours=NOT_OURS).items():
        name = ": " + re.sub(r"\s*\([^()]*\)", "", k)
        n = sum(f == name or f.startswith(name + " #") for f in found)
        found[f"{name} #{n + 1}" if n else name] = v
    return found


if __name__ == "__main__":
    named = [a for a in sys.argv[1:] if a.endswith(".py")]
    sys.argv[1:] = [a for a in sys.argv[1:] if not a.endswith(".py")]
    sys.exit(main([(s, ["benchmarks/" + s]) for s in (named or SCRIPTS)], figures))
