#!/usr/bin/env python3
"""Do two revisions of the Python package give the same bits in every posterior summary of the device store (the methods of
openmcmc_amd/summary that MCMC inherits, on the wrappers of openmcmc_amd/engine_store.py that Engine inherits)?

    mkdir -p build/ab/parent && git archive HEAD~1 openmcmc_amd tests benchmarks bench.py oracle | tar -x -C build/ab/parent
    python3 benchmarks/summaries_same_bits.py [--before build/ab/parent] [--out profiles/summaries_refactor_same_bits.txt]

The method is that of benchmarks/normal_normal_same_bits.py / mh_same_bits.py: one fresh child process per source tree, one after the
other, both on the in-tree libomcmc_hip.so; every array that comes back is saved and the two files are compared with
np.array_equal(equal_nan=True), integers exactly; an argument error is recorded as the exception's type and text and compared as well.
Each child builds MCMC.__new__(MCMC) over the two stores of benchmarks/store_same_bits.py, (5, 3, 17) and (130, 2, 33), with their NaN,
infinity and tie columns (entries "x" and "o", an allocation entry "z" of labels 0 .. 2 with NaN padding, and the 2-D entry "lp"), and
calls every public summary: pooled and per chain where both forms exist, without and with the unsorted 19-entry index; histogram,
histogram2d, kde and kde2d also over the finite columns alone (int bins without and with a range, arrays of edges, extend 0 and 0.1,
bounds, pool_elements); the entries that are kept under a name (derive, project with base=name, posterior_predictive, log_likelihood,
loo_weights) twice, the second time over the first; the model-based summaries on a Normal response of 7 observations with a
LinearCombination mean -- precision a stored scalar, a constant of the state, and a stored scalar times a diagonal matrix -- with
pointwise_work_bytes set so that the observations go in three chunks, the last one short.
Afterwards benchmarks/store_same_bits.py's own child (every Engine.store_* entry point) runs once in either tree on the same library
and its arrays are compared in the same way.  Exit status 1 if anything differs, 2 if a child failed.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ERRORS = (NotImplementedError, ValueError, TypeError, KeyError, IndexError, AttributeError)
M_OBS, P_COEF = 7, 4


def flatten(key, node, out):
    if isinstance(node, dict):
        for k, v in node.items():
            flatten(f"{key}.{k}", v, out)
    elif isinstance(node, (tuple, list)):
        for i, v in enumerate(node):
            flatten(f"{key}#{i}", v, out)
    elif node is None:
        out[key] = np.array("None")
    else:
        out[key] = node.cpu().numpy() if hasattr(node, "cpu") else np.asarray(node)


def summaries(M, put, size, index):
    """Every summary that needs no model, on the entries "x", "o", "z" and "lp" of M.store."""
    finite = np.arange(3, size)  # (column 0 holds a NaN, column 1 an infinity, column 2 ties)
    for iname, idx in (("all", None), ("index", index), ("finite", finite)):
        n = size if idx is None else len(idx)
        idy = None if idx is None else idx[::-1].copy()
        k = f"{{}}/{iname}"
        put(k.format("rank_diagnostics"), lambda: M.rank_diagnostics("x", index=idx))
        for method, prob in (("bulk", None), ("tail", None), ("mean", None), ("sd", None), ("quantile", 0.3), ("quantile", [0.1, 0.9]),
                             ("median", None), ("local", (0.1, 0.9)), ("local", [(0.0, 0.5), (0.5, 1.0)]), ("quantile", None),
                             ("local", 0.5), ("quantile", [[0.1]]), ("quantile", 1.5), ("nonsense", None)):
            put(k.format("ess") + f"/{method}/{prob}", lambda: M.ess("x", method=method, prob=prob, index=idx))
        for method, prob in (("mean", None), ("sd", None), ("quantile", 0.3), ("quantile", [0.1, 0.9]), ("median", None), ("quantile", []),
                             ("bulk", None)):
            put(k.format("mcse") + f"/{method}/{prob}", lambda: M.mcse("x", method=method, prob=prob, index=idx))
        put(k.format("summarize"), lambda: M.summarize("x", index=idx))
        for split in (False, True):
            put(k.format("ranks") + f"/split{split}", lambda: M.ranks("x", index=idx, split=split))
        put(k.format("simultaneous_band"), lambda: M.simultaneous_band("x", prob=0.9, index=idx))
        put(k.format("simultaneous_band") + "/prob1", lambda: M.simultaneous_band("x", prob=1.0, index=idx))
        w = np.linspace(-1.0, 1.0, n)
        for reduce, kw in (("sum", {}), ("sum", {"weights": w}), ("mean", {}), ("count", {}), ("min", {}), ("max", {}), ("argmin", {}),
                           ("argmax", {}), ("count_above", {"threshold": 0.25}), ("supnorm", {"center": w, "scale": 2.0}),
                           ("min", {"weights": w}), ("median", {})):
            for omit in (True, False):
                put(k.format("derive") + f"/{reduce}/{sorted(kw)}/omit{omit}", lambda: M.derive("x", reduce, index=idx, omit_nan=omit, **kw))
        for again in (0, 1):  # a named entry, made and made again
            put(k.format("derive") + f"/named{again}", lambda: (M.derive("x", "max", index=idx, name="d"), M.store["d"], M.summary("d")))
        W = np.random.default_rng(3).standard_normal((3, n))
        put(k.format("project"), lambda: M.project("x", W, index=idx, offset=[0.5, -0.5, 0.0]))
        put(k.format("project") + "/nan_kept", lambda: M.project("x", W[0], index=idx, omit_nan=False))
        put(k.format("project") + "/noise", lambda: M.project("x", W, index=idx, noise_precision="tau", replicate=2))
        for again in (0, 1):
            put(k.format("project") + f"/named{again}", lambda: (M.project("x", W, index=idx, name="f"), M.store["f"]))
            put(k.format("project") + f"/accumulated{again}", lambda: (M.project("o", W, index=idx, base="f", name="f"), M.store["f"]))
        put(k.format("project") + "/reads_itself", lambda: M.project("f", np.ones((3, 3)), base="f", name="f"))
        for pname, pooled in (("pooled", True), ("chain", False)):
            kp = k + f"/{pname}"
            for prob in (0.94, [0.5, 0.9], np.linspace(0.05, 0.95, 10), [], [[0.5]]):
                for omit in (True, False):
                    put(kp.format("hdi") + f"/{np.size(prob)}/omit{omit}", lambda: M.hdi("x", prob=prob, index=idx, pooled=pooled, omit_nan=omit))
            put(kp.format("autocorrelation"), lambda: M.autocorrelation("x", index=idx, pooled=pooled))
            put(kp.format("autocorrelation") + "/raw", lambda: M.autocorrelation("x", max_lag=2, index=idx, pooled=pooled, normalize=False))
            put(kp.format("covariance"), lambda: M.covariance("x", index=idx, pooled=pooled))
            put(kp.format("covariance") + "/cross", lambda: M.covariance("x", "o", index=idx, other_index=idy, pooled=pooled))
            put(kp.format("correlation"), lambda: M.correlation("x", "o", index=idx, other_index=idy, pooled=pooled))
            put(kp.format("exceedance"), lambda: M.exceedance("x", [0.5, -np.inf, 0.0, np.inf], index=idx, pooled=pooled))
            put(kp.format("exceedance") + "/nan", lambda: M.exceedance("x", [0.5, np.nan], index=idx, pooled=pooled))
            for per_label in (False, True):
                put(kp.format("coallocation") + f"/per_label{per_label}",
                    lambda: M.coallocation("z", n_labels=3, index=idx, pooled=pooled, per_label=per_label))
            put(kp.format("partition"), lambda: M.partition("z", n_labels=3, index=idx, pooled=pooled))
            put(kp.format("coallocation") + "/no_labels", lambda: M.coallocation("z", index=idx, pooled=pooled))
            put(kp.format("coallocation") + "/not_an_allocation", lambda: M.partition("x", n_labels=3, index=idx, pooled=pooled))
            put(kp.format("coallocation") + "/labels_0", lambda: M.coallocation("z", n_labels=0, index=idx, pooled=pooled))
            # the binned summaries: an infinite draw raises unless the columns are the finite ones
            edges = np.array([-4.0, -1.5, -1.0, -0.25, 0.0, 0.125, 1.0, 2.5, 6.0])
            per = edges[None, :] * (1.0 + 0.05 * np.arange(n)[:, None])
            for bname, bins, rng in (("int", 8, None), ("int_range", 8, (-2.0, 2.5)), ("int_point", 8, (1.0, 1.0)), ("shared", edges, None),
                                     ("per", per, None), ("range_reversed", 8, (2.0, 1.0)), ("range_inf", 8, (0.0, np.inf)),
                                     ("bins_0", 0, None), ("edges_nan", [0.0, np.nan], None), ("edges_down", [1.0, 0.0], None),
                                     ("edges_3d", np.zeros((1, 1, 3)), None)):
                for density in (False, True):
                    put(kp.format("histogram") + f"/{bname}/density{density}",
                        lambda: M.histogram("x", bins=bins, range=rng, index=idx, pooled=pooled, density=density))
                rng2 = None if rng is None else [rng, None]
                for pool in (False, True):
                    put(kp.format("histogram2d") + f"/{bname}/pool{pool}",
                        lambda: M.histogram2d("x", "o", index_x=idx, index_y=idy, bins=bins, range=rng2, pooled=pooled, pool_elements=pool))
                put(kp.format("histogram2d") + f"/{bname}/xy", lambda: M.histogram2d("x", index_x=idx, index_y=idy, bins=[bins, 5], range=rng2,
                                                                                        pooled=pooled, density=True))
                if n <= 256:
                    put(kp.format("occupancy") + f"/{bname}", lambda: M.occupancy("x", "o", index_x=idx, index_y=idy, bins=bins, range=rng2, pooled=pooled))
            put(kp.format("histogram2d") + "/range_of_three", lambda: M.histogram2d("x", index_x=idx, index_y=idy, range=[(0, 1)] * 3, pooled=pooled))
            for kname, kw in (("default", {}), ("extend0", {"extend": 0}), ("extend0.1_g64", {"extend": 0.1, "grid_len": 64}),
                              ("bounds", {"bounds": (-9.0, None)}), ("bounds_both", {"bounds": (-9.0, 9.0), "bw": "isj"}),
                              ("bounds_bad", {"bounds": (9.0, None)}), ("silverman", {"bw": "silverman", "bw_fct": 1.5}), ("given", {"bw": 0.3}),
                              ("given_vector", {"bw": np.linspace(0.2, 0.6, n)}), ("given_wrong", {"bw": [0.2, 0.3]}), ("grid_7", {"grid_len": 7}),
                              ("grid_8.5", {"grid_len": 8.5}), ("extend_neg", {"extend": -0.1}), ("extend_inf", {"extend": np.inf}),
                              ("rule_unknown", {"bw": "nonsense"})):
                put(kp.format("kde") + f"/{kname}", lambda: M.kde("x", index=idx, pooled=pooled, **kw))
            put(kp.format("mode"), lambda: M.mode("x", index=idx, pooled=pooled, grid_len=32))
            H = np.array([[0.3, 0.1], [0.1, 0.5]])
            for kname, kw in (("default", {"grid_len": 16}), ("extend0", {"grid_len": 16, "extend": 0}), ("grid_xy", {"grid_len": (8, 24)}),
                              ("pool", {"grid_len": 16, "pool_elements": True}), ("pool_extend0", {"grid_len": 16, "pool_elements": True, "extend": 0}),
                              ("marginal", {"grid_len": 16, "bw": "marginal"}), ("silverman", {"grid_len": 16, "bw": "silverman", "bw_fct": 0.7}),
                              ("given", {"grid_len": 16, "bw": H}), ("given_per_pair", {"grid_len": 16, "bw": np.broadcast_to(H, (n, 2, 2))}),
                              ("given_pool_per_pair", {"grid_len": 16, "bw": np.broadcast_to(H, (n, 2, 2)), "pool_elements": True}),
                              ("given_asymmetric", {"grid_len": 16, "bw": [[1.0, 0.2], [0.1, 1.0]]}), ("no_probs", {"grid_len": 16, "probs": None}),
                              ("probs_17", {"grid_len": 16, "probs": np.linspace(0.1, 0.9, 17)}), ("probs_1", {"grid_len": 16, "probs": 1.0}),
                              ("grid_7", {"grid_len": 7}), ("grid_257", {"grid_len": (16, 257)}), ("grid_8.5", {"grid_len": 8.5}),
                              ("extend_neg", {"grid_len": 16, "extend": -1}), ("bw_fct_0", {"grid_len": 16, "bw_fct": 0}),
                              ("rule_unknown", {"grid_len": 16, "bw": "isj"})):
                put(kp.format("kde2d") + f"/{kname}", lambda: M.kde2d("x", "o", index_x=idx, index_y=idy, pooled=pooled, **kw))
            put(kp.format("joint_mode"), lambda: M.joint_mode("x", index_x=idx, index_y=idy, pooled=pooled, grid_len=16))
            put(kp.format("density_region"), lambda: M.density_region("x", "o", idx, idy, prob=0.8, pooled=pooled, grid_len=16))
    for pname, pooled in (("pooled", True), ("chain", False)):
        put(f"summary/{pname}", lambda: M.summary("x", pooled=pooled))
        put(f"summary/lp/{pname}", lambda: M.summary("lp", pooled=pooled))
        for omit in (True, False):
            put(f"quantiles/{pname}/omit{omit}", lambda: M.quantiles("x", [0.05, 0.5, 0.95], pooled=pooled, omit_nan=omit))
        put(f"quantiles/lp/{pname}", lambda: M.quantiles("lp", 0.5, pooled=pooled))
    put("diagnostics", lambda: M.diagnostics("x"))
    put("diagnostics/lp", lambda: M.diagnostics("lp"))
    put("histogram/lp", lambda: M.histogram("lp", bins=4))
    put("kde/lp", lambda: M.kde("lp", grid_len=8))
    for what, call in (("derive", lambda: M.derive("x", "sum", name="o")), ("project", lambda: M.project("x", np.ones(size), name="o"))):
        put(f"{what}/name_of_the_run", call)


def model_based(M, put, variant):
    """The summaries of a Normal response "y" of M.model; "beta" and "tau" are entries of M.store"""
    for pointwise in (False, True):
        put(f"{variant}/waic/pointwise{pointwise}", lambda: M.waic("y", pointwise=pointwise))
        put(f"{variant}/loo/pointwise{pointwise}", lambda: M.loo("y", pointwise=pointwise, reff=0.7))
    put(f"{variant}/loo/reff_vector", lambda: M.loo("y", reff=np.linspace(0.5, 1.0, M_OBS)))
    put(f"{variant}/loo/reff_0", lambda: M.loo("y", reff=0.0))
    put(f"{variant}/posterior_predictive", lambda: M.posterior_predictive("y", replicate=1))
    put(f"{variant}/posterior_predictive/fitted", lambda: M.posterior_predictive("y", noise=False))
    put(f"{variant}/log_likelihood", lambda: M.log_likelihood("y"))
    put(f"{variant}/loo_weights", lambda: M.loo_weights("y"))
    for again in (0, 1):
        put(f"{variant}/posterior_predictive/named{again}", lambda: (M.posterior_predictive("y", name="y_rep"), M.store["y_rep"]))
        put(f"{variant}/log_likelihood/named{again}", lambda: (M.log_likelihood("y", name="ll"), M.store["ll"]))
        put(f"{variant}/loo_weights/named{again}", lambda: (M.loo_weights("y", name="lw", reff=0.7), M.store["lw"]))
    put(f"{variant}/loo_expectation", lambda: M.loo_expectation("y", "x", index=np.arange(3, 3 + M_OBS), threshold=0.1))
    put(f"{variant}/loo_expectation/entry", lambda: M.loo_expectation("y", "y_rep", threshold=np.linspace(-1.0, 1.0, M_OBS), reff=0.7))
    put(f"{variant}/loo_expectation/wrong_size", lambda: M.loo_expectation("y", "x"))
    put(f"{variant}/loo_expectation/index_2d", lambda: M.loo_expectation("y", "x", index=[[1]]))
    put(f"{variant}/loo_expectation/threshold_short", lambda: M.loo_expectation("y", "y_rep", threshold=[0.0, 1.0]))
    put(f"{variant}/loo_predictive", lambda: M.loo_predictive("y"))
    put(f"{variant}/loo_pit", lambda: M.loo_pit("y"))
    put(f"{variant}/loo_pit/y_rep", lambda: M.loo_pit("y", y_rep="y_rep"))
    for what, call in (("posterior_predictive", lambda: M.posterior_predictive("y", name="x")), ("log_likelihood", lambda: M.log_likelihood("y", name="x")),
                       ("loo_weights", lambda: M.loo_weights("y", name="x"))):
        put(f"{variant}/{what}/name_of_the_run", call)
    put(f"{variant}/derived_names", lambda: np.array(sorted(M._derived)))
    put(f"{variant}/no_such_response", lambda: M.waic("beta"))


def child(path, tree):
    sys.path.insert(0, os.path.join(ROOT, "benchmarks"))
    from store_same_bits import SHAPES, host_store  # (puts ROOT in front of sys.path: the tree goes in after it)

    sys.path.insert(0, tree)
    import openmcmc_amd
    from scipy import sparse

    from openmcmc_amd.distribution.location_scale import Normal
    from openmcmc_amd.engine import Engine
    from openmcmc_amd.mcmc import MCMC
    from openmcmc_amd.model import Model
    from openmcmc_amd.parameter import LinearCombination, ScaledMatrix

    assert os.path.dirname(os.path.dirname(os.path.abspath(openmcmc_amd.__file__))) == os.path.abspath(tree)
    out = {}
    for shape in SHAPES:
        n_iter, C, size = shape
        tag = "x".join(map(str, shape))

        def put(key, fn):
            try:
                flatten(f"{tag}/{key}", fn(), out)
            except HOST_ERRORS as e:  # (anything else, a device error above all, ends the child)
                out[f"{tag}/{key}|raised"] = np.array(f"{type(e).__name__}: {e}")

        rng = np.random.default_rng(11)
        index = np.concatenate([[2, 0, 1, size - 1, 2], rng.integers(0, size, 14)])
        z = rng.integers(0, 3, shape).astype(np.float64)
        z[0, 0, size - 1] = np.nan
        M = MCMC.__new__(MCMC)
        M.engine = eng = Engine(C, seed=1)
        M.store_ring, M._n_dev, M.n_iter, M.n_chains, M.model, M.state, M._derived = 0, n_iter, n_iter, C, None, {}, set()
        M.store = {"x": eng.to_device(host_store(shape, 5)), "o": eng.to_device(host_store(shape, 6)), "z": eng.to_device(z),
                   "lp": eng.to_device(rng.standard_normal((n_iter, C))), "tau": eng.to_device(rng.gamma(2.0, 1.0, (n_iter, C, 1))),
                   "beta": eng.to_device(rng.standard_normal((n_iter, C, P_COEF)))}
        summaries(M, put, size, index)
        M.state = {"A": rng.standard_normal((M_OBS, P_COEF)), "y": rng.standard_normal((M_OBS, 1)), "tau0": np.array([[1.5]]),
                   "W": sparse.diags(np.linspace(0.5, 2.0, M_OBS), format="csc"), "I": sparse.identity(M_OBS, format="csc"),
                   "T": sparse.diags([np.ones(M_OBS - 1), np.full(M_OBS, 2.0), np.ones(M_OBS - 1)], [-1, 0, 1], format="csc")}
        M.pointwise_work_bytes = 8 * n_iter * C * 3  # three observations per chunk: 3 + 3 + 1
        mean = LinearCombination(form={"beta": "A"})
        for variant, prec in (("stored", "tau"), ("constant", "tau0"), ("diagonal", ScaledMatrix(matrix="W", scalar="tau")),
                              ("identity_matrix", ScaledMatrix(matrix="I", scalar="tau")), ("not_diagonal", ScaledMatrix(matrix="T", scalar="tau"))):
            M.model = Model([Normal("y", mean=mean, precision=prec)])
            model_based(M, put, variant)
        M.model = Model([Normal("y", mean="beta", precision="tau")])  # the entry itself is the mean: P_COEF observations, one chunk
        M.state["y"] = rng.standard_normal((P_COEF, 1))
        for name, call in (("posterior_predictive", lambda: M.posterior_predictive("y")), ("log_likelihood", lambda: M.log_likelihood("y")),
                           ("loo", lambda: M.loo("y")), ("loo_weights", lambda: M.loo_weights("y")), ("loo_predictive", lambda: M.loo_predictive("y"))):
            put(f"identity_mean/{name}", call)
        M.store_ring, M.n_iter = 4, 2 * n_iter  # a ring that holds the last iterations only: every summary refuses
        for name, call in (("summary", lambda: M.summary("x")), ("kde2d", lambda: M.kde2d("x")), ("loo", lambda: M.loo("y")),
                           ("histogram", lambda: M.histogram("x"))):
            put(f"ring/{name}", call)
        eng.check_status()
        eng.close()
    np.savez(path, **out)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def children(trees, command, tmp, name):
    """{tree's label: {key: array}} of one child per tree, one after the other, on the in-tree library; None if one failed"""
    got = {}
    for label, tree in trees:
        env = dict(os.environ, OMC_HIP_LIB=os.path.join(ROOT, "openmcmc_amd", "libomcmc_hip.so"))
        path = os.path.join(tmp, f"{name}_{label}.npz")
        run = subprocess.run([sys.executable] + command(tree, path), env=env, timeout=900)
        if run.returncode != 0:
            print(f"the {name} child of the {label} tree ended with status {run.returncode}: nothing compared")
            return None
        with np.load(path) as z:
            got[label] = {k: z[k] for k in z.files}
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", default="build/ab/parent")
    ap.add_argument("--out")
    ap.add_argument("--child")
    ap.add_argument("--tree")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.tree)
    trees = (("before", os.path.join(ROOT, args.before)), ("after", ROOT))
    rows = [f"before = {args.before}, after = the working tree, one library; arrays compared with np.array_equal(equal_nan=True), integers "
            "exactly, exceptions as type and text"]
    n_bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        got = children(trees, lambda tree, path: [os.path.abspath(__file__), "--child", path, "--tree", tree], tmp, "summaries")
        entry = children(trees, lambda tree, path: [os.path.join(tree, "benchmarks", "store_same_bits.py"), "--child", path], tmp, "store_same_bits")
    if got is None or entry is None:
        return 2
    before, after = got["before"], got["after"]
    groups = {}
    for key in sorted(set(before) | set(after)):
        ok = key in before and key in after and same(before[key], after[key])
        shape, *parts = key.split("|")[0].split(".")[0].split("#")[0].split("/")
        model_based = parts[0] in ("stored", "constant", "diagonal", "identity_matrix", "not_diagonal", "identity_mean", "ring")
        method = "/".join(parts[:2]) if model_based else parts[0]
        groups.setdefault((method, shape), []).append((key, ok))
    for (method, shape), found in sorted(groups.items()):
        raised = [key for key, _ in found if key.endswith("|raised")]
        ok = all(ok for _, ok in found)
        n_bad += not ok
        rows.append(f"{method:44s} {shape:10s} {'equal' if ok else 'NOT EQUAL'}  ({sum(ok for _, ok in found)} of {len(found)} entries, "
                    f"{len(raised)} of them exceptions)")
        rows += [f"    NOT EQUAL: {key}" for key, ok in found if not ok]
    texts = sorted({str(after[k]) for k in after if k.endswith("|raised")})
    rows.append(f"{len(groups)} lines, {len(after)} entries ({sum(k.endswith('|raised') for k in after)} exceptions of {len(texts)} distinct "
                f"texts), {sum(a.size for a in after.values() if a.dtype.kind in 'fiub')} numbers, {n_bad} lines unequal")
    rows += ["", "the exceptions, raised alike by both trees:"] + [f"    {t}" for t in texts]
    before, after = entry["before"], entry["after"]
    bad = [key for key in sorted(set(before) | set(after)) if not (key in before and key in after and same(before[key], after[key]))]
    rows += ["", f"benchmarks/store_same_bits.py --child in either tree (every Engine.store_* entry point), one library: {len(after)} arrays, "
             f"{len(bad)} unequal"] + [f"    NOT EQUAL: {key}" for key in bad]
    print("\n".join(rows))
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(rows) + "\n")
    return 1 if n_bad or bad else 0


if __name__ == "__main__":
    sys.exit(main())
