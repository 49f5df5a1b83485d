"""omc_dense_spectral_sample with its three products on omc_dgemm_small (the default) against rocBLAS DGEMM (option
spectral_use_rocblas), alternating, device events around 50 draws, six rounds; the two routes' outputs compared.
One JSON line per shape; profiles/spectral_products_ab.txt keeps a run."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openmcmc_amd.engine import Engine  # noqa: E402

for p, C in ((1000, 256), (1000, 1024), (1000, 64), (64, 256), (200, 512)):
    rng = np.random.default_rng(p + C)
    A = rng.standard_normal((p, 2 * p))
    G = A @ A.T / (2 * p)
    eng = Engine(C, seed=1)
    dG = eng.to_device(0.5 * (G + G.T))
    V, ev = eng.dense_spectral_prepare(dG)
    terms = eng.dense_terms([{"mat": None, "scale": eng.full((C,), 0.01)},
                             {"mat": dG, "rhs": eng.to_device(rng.standard_normal(p)), "scale": eng.full((C,), 1.0)}], p)
    x, m = eng.empty(C, p), eng.empty(C, p)
    res = {}
    times = {0: [], 1: []}
    for rep in range(6):
        for flag in (0, 1):
            eng.set_option("spectral_use_rocblas", flag)
            for _ in range(3):
                eng.dense_spectral_sample(p, terms, 1, V, ev, x, draw_index=3, mean_out=m)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n = 50
            e0.record()
            for it in range(n):
                eng.dense_spectral_sample(p, terms, 1, V, ev, x, draw_index=3)
            e1.record()
            torch.cuda.synchronize()
            times[flag].append(e0.elapsed_time(e1) / n * 1e3)
            eng.dense_spectral_sample(p, terms, 1, V, ev, x, draw_index=3, mean_out=m)
            res[flag] = (x.cpu().numpy().copy(), m.cpu().numpy().copy())
    eng.check_status()
    rel = max(float(np.max(np.abs(res[0][k] - res[1][k])) / np.max(np.abs(res[1][k]))) for k in (0, 1))
    rec = {"p": p, "C": C, "own_us": sorted(times[0]), "rocblas_us": sorted(times[1]), "max_rel_diff": rel}
    print(json.dumps(rec), flush=True)
    eng.close()
