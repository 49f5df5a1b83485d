"""numpy restatement of omc_store_coalloc / omc_store_partition_score, written from the text of include/omcmc_hip.h.  Shared by
test_coalloc_model_host.py (which holds it to Python loops and exact fractions) and the GPU tests (which hold the kernels to it,
array_equal)."""

import numpy as np


def labels_of(store, K):
    """int64 labels of fp64 draws by the header's label rule: v carries label k iff v == k for an integer 0 <= k < K (-0.0 is 0);
    -1 for NaN (element absent), -2 for any other value (not a label)."""
    v = np.asarray(store, dtype=np.float64)
    out = np.full(v.shape, -2, dtype=np.int64)
    out[np.isnan(v)] = -1
    with np.errstate(invalid="ignore"):
        ok = (v >= 0) & (v < K) & (np.floor(v) == v)
    out[ok] = v[ok].astype(np.int64)
    return out


def flags_of(Z):
    """(n, 2) int64 {NaN draws, other non-label draws} of the columns of labels Z (rows, n)"""
    return np.stack([(Z == -1).sum(axis=0), (Z == -2).sum(axis=0)], axis=1).astype(np.int64)


def coalloc(Z, K, per_label=False, chunk=512):
    """counts of labels Z (rows, n), negative = carries no label and matches nothing: (n, n), entry (i, j) = rows with z_i == z_j;
    per_label: (K, n, n), entry (k, i, j) = rows with z_i == k and z_j == k.  The broadcast compare, in chunks of rows."""
    Z = np.asarray(Z, dtype=np.int64)
    n = Z.shape[1]
    out = np.zeros((K, n, n) if per_label else (n, n), dtype=np.int64)
    for a in range(0, Z.shape[0], chunk):
        z = Z[a:a + chunk]
        if per_label:
            for k in range(K):
                out[k] += ((z[:, :, None] == k) & (z[:, None, :] == k)).sum(axis=0)
        else:
            out += ((z[:, :, None] == z[:, None, :]) & (z[:, :, None] >= 0)).sum(axis=0)
    return out


def scores(Z, counts, R):
    """score of every row s of labels Z (rows, n) against counts (n, n) of a batch of R rows:
    sum over positions i < j of [z_i^s == z_j^s] (R - 2 counts_ij), in int64"""
    Z = np.asarray(Z, dtype=np.int64)
    W = np.triu(np.int64(R) - 2 * np.asarray(counts, dtype=np.int64), 1)
    out = np.zeros(Z.shape[0], dtype=np.int64)
    for s, z in enumerate(Z):
        same = (z[:, None] == z[None, :]) & (z[:, None] >= 0)
        out[s] = (W * same).sum(dtype=np.int64)
    return out


def first_argmin(v):
    """(index of the first minimum, the minimum) -- np.argmin's rule, spelled out"""
    best = 0
    for i in range(1, len(v)):
        if v[i] < v[best]:
            best = i
    return best, v[best]


def canonical(labels):
    """labels renamed 0, 1, .. in order of first appearance; a negative label (absent) gives -1"""
    out, seen = np.full(len(labels), -1, dtype=np.int64), {}
    for i, v in enumerate(labels):
        if v >= 0:
            out[i] = seen.setdefault(int(v), len(seen))
    return out


def batches_of(store, K, index=None, pooled=True):
    """[labels (rows, n) of every batch] of a store (n_iter, C, size): one batch of n_iter C rows (row it C + c) pooled, else the
    C chains' own rows"""
    x = np.asarray(store)
    if index is not None:
        x = x[:, :, np.asarray(index)]
    Z = labels_of(x, K)
    return [Z.reshape(-1, Z.shape[2])] if pooled else [Z[:, c, :] for c in range(Z.shape[1])]
