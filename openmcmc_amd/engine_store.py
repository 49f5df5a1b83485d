"""The store wrappers of the C ABI, which Engine inherits: the omc_store_* / omc_kde* entry points on device tensors and their layout queries."""

import ctypes as C
import functools

import numpy as np

from openmcmc_amd._abi import INVALID_ARG, check, lib


@functools.lru_cache(maxsize=None)
def _torch():
    import torch  # (on first use, and once, as in engine.py)
    return torch


def _ptr(t):
    """Device pointer of a tensor of any dtype (None passes through as NULL)."""
    return None if t is None else t.data_ptr()


class StoreOps:
    """Posterior summaries of a device store (n_iter, C, size), on the `_ctx`, `n_chains`, `device`, `empty`, `to_device` and `_p` of an Engine."""

    def _store_shape(self, store):
        """(n_iter, size) of a device store (n_iter, C, size)"""
        if store.dim() != 3 or store.shape[1] != self.n_chains or not store.is_contiguous():
            raise ValueError("store must be a contiguous (n_iter, C, size) tensor")
        return store.shape[0], store.shape[2]

    def store_moments(self, store, pooled=False):
        """(mean, var) of a device store (n_iter, C, size): per chain (C, size) or pooled (size,)."""
        n_iter, size = self._store_shape(store)
        shape = (size,) if pooled else (self.n_chains, size)
        mean, var = self.empty(*shape), self.empty(*shape)
        check(lib.omc_store_moments(self._ctx, n_iter, size, self._p(store), int(pooled), self._p(mean), self._p(var)))
        return mean, var

    def store_quantiles(self, store, q, pooled=False, omit_nan=True):
        """np.quantile (omit_nan=False) / np.nanquantile (True) of a device store (n_iter, C, size) along the iterations,
        default "linear" method: (len(q), C, size) per chain or (len(q), size) pooled over chains; computed on the device."""
        n_iter, size = self._store_shape(store)
        qs = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
        if qs.ndim != 1 or qs.size < 1:
            raise ValueError("q must be a scalar or a one-dimensional sequence")
        if not np.all((qs >= 0) & (qs <= 1)):
            raise ValueError("Quantiles must be in the range [0, 1]")  # np.quantile's own message
        out = self.empty(*((qs.size, size) if pooled else (qs.size, self.n_chains, size)))
        check(lib.omc_store_quantiles(self._ctx, n_iter, size, self._p(store), int(pooled), qs.size,
                                      qs.ctypes.data_as(C.POINTER(C.c_double)), int(bool(omit_nan)), self._p(out)))
        return out

    def store_rhat_ess(self, store):
        """Split R-hat and effective sample size of every element of a device store (n_iter, C, size), computed on the
        device (omc_store_rhat_ess): (rhat, ess, lags) as device tensors of shape (size,), lags int32 = the lags the
        element's Geyer sequence used.  n_iter >= 4."""
        n_iter, size = self._store_shape(store)
        if n_iter < 4:
            raise ValueError("split R-hat and ESS need at least 4 stored iterations")
        rhat, ess = self.empty(size), self.empty(size)
        lags = self.empty(size, dtype=_torch().int32)
        check(lib.omc_store_rhat_ess(self._ctx, n_iter, size, self._p(store), self._p(rhat), self._p(ess), lags.data_ptr()))
        return rhat, ess, lags

    @staticmethod
    def _check_text(st):
        """check() for an entry point that says which argument it refuses: INVALID_ARG raises ValueError with the library's text"""
        if st == INVALID_ARG:
            raise ValueError("libomcmc_hip: " + (lib.omc_last_error() or b"invalid argument").decode())
        check(st)

    def _int64(self, v, what, empty_ok=True):
        """device int64 tensor of a host array (uploaded synchronously) or a tensor of integers; empty_ok: an empty host
        sequence passes whatever its type, for the caller's own complaint about the shape"""
        torch = _torch()
        if isinstance(v, torch.Tensor):
            if v.is_floating_point() or v.dtype is torch.bool:
                raise ValueError(f"{what} must hold integers")
            return v.to(device=self.device, dtype=torch.int64).contiguous()
        arr = np.asarray(v)
        if (arr.size or not empty_ok) and arr.dtype.kind not in "iu":
            raise ValueError(f"{what} must hold integers")
        # (torch.tensor copies from the numpy array before it returns: no asynchronous read of a temporary)
        return torch.tensor(np.ascontiguousarray(arr, dtype=np.int64), dtype=torch.int64, device=self.device)

    def _f64(self, v):
        """contiguous device fp64 tensor of a host array (uploaded synchronously) or a tensor"""
        torch = _torch()
        if isinstance(v, torch.Tensor):
            return v.to(device=self.device, dtype=torch.float64).contiguous()
        # (torch.tensor copies from the numpy array before it returns: no asynchronous read of a temporary)
        return torch.tensor(np.ascontiguousarray(v, dtype=np.float64), dtype=torch.float64, device=self.device)

    def _store_index(self, index, size):
        """(device int64 tensor or None, number of selected elements) of an element selection of a store"""
        if index is None:
            return None, size
        idx = self._int64(index, "index")
        if idx.dim() != 1 or idx.numel() < 1:
            raise ValueError("index must be a non-empty one-dimensional sequence")
        return idx, idx.numel()

    def _selection(self, store, index):
        """(n_iter, size, device int64 tensor or None, number of selected elements) of a store and a selection of its elements"""
        n_iter, size = self._store_shape(store)
        return (n_iter, size) + self._store_index(index, size)

    def store_cov(self, store_a, store_b=None, index_a=None, index_b=None, pooled=True, correlation=False):
        """Covariance (correlation=True: correlation) matrix of the elements of a device store (n_iter, C, size_a), or of
        its elements against those of a second store (n_iter, C, size_b), computed on the device (omc_store_cov):
        (n_a, n_b) pooled over chains and iterations, else (C, n_a, n_b) per chain.  index_a / index_b (sequence, numpy or
        torch integers) select elements, in that order, repeats allowed; without store_b the matrix is that of a with
        itself and exactly symmetric (index_b is then not accepted).  NaN draws propagate as in np.cov."""
        n_iter, size_a = self._store_shape(store_a)
        n_iter_b, size_b = (n_iter, size_a) if store_b is None else self._store_shape(store_b)
        if store_b is None and index_b is not None:
            raise ValueError("index_b needs store_b")
        if n_iter_b != n_iter:
            raise ValueError("store_a and store_b must hold the same number of iterations")
        idx_a, n_a = self._store_index(index_a, size_a)
        idx_b, n_b = (None, n_a) if store_b is None else self._store_index(index_b, size_b)
        out = self.empty(*((n_a, n_b) if pooled else (self.n_chains, n_a, n_b)))
        check(lib.omc_store_cov(self._ctx, n_iter, size_a, self._p(store_a), _ptr(idx_a), n_a,
                                size_b, self._p(store_b), _ptr(idx_b), n_b,
                                int(bool(pooled)), int(bool(correlation)), self._p(out)))
        return out

    @staticmethod
    def hist_tile(n_bins, per_element=False):
        """(TE, RB) of omc_store_histogram at n_bins: a workgroup counts a tile of TE consecutive selected elements over slices
        of RB rows (openmcmc_amd/csrc/omc_hist_layout.h through omc_store_histogram_layout; needs no GPU)."""
        return tuple(StoreOps.hist_layout(n_bins, per_element)[:2])

    @staticmethod
    def hist_layout(n_bins, per_element=False):
        """The ten numbers of omc_store_histogram_layout: TE, RB, edge stride, counter stride, byte offsets of the edges, the
        counters and the outside counts, bytes launched, the budget, threads of a workgroup."""
        out = (C.c_int32 * 10)()
        check(lib.omc_store_histogram_layout(int(n_bins), int(bool(per_element)), out))
        return list(out)

    def store_minmax(self, store, index=None, pooled=True):
        """(min, max, count) of the non-NaN draws of every selected element of a device store (n_iter, C, size), on the device
        (omc_store_minmax): np.nanmin, np.nanmax and the number of non-NaN draws, shape (n_idx,) pooled over chains and
        iterations, else (C, n_idx); count is int64; an element without a non-NaN draw gives NaN, NaN, 0."""
        n_iter, size, idx, n = self._selection(store, index)
        shape = (n,) if pooled else (self.n_chains, n)
        mn, mx = self.empty(*shape), self.empty(*shape)
        cnt = self.empty(shape, dtype=_torch().int64)
        check(lib.omc_store_minmax(self._ctx, n_iter, size, self._p(store), _ptr(idx), n,
                                   int(bool(pooled)), self._p(mn), self._p(mx), cnt.data_ptr()))
        return mn, mx, cnt

    def store_histogram(self, store, edges, index=None, pooled=True):
        """(counts, outside) of a device store (n_iter, C, size), on the device (omc_store_histogram): counts int64
        (n_idx, n_bins) pooled, else (C, n_idx, n_bins) = np.histogram(draws of the element, bins=edges)[0]; outside int64
        (.., 3) = draws below edges[0], above edges[-1], NaN.  edges: 1-D (n_bins + 1,) shared by all elements or 2-D
        (n_idx, n_bins + 1) per element, a host array (uploaded synchronously) or a device tensor; non-decreasing, no NaN."""
        torch = _torch()
        n_iter, size, idx, n = self._selection(store, index)
        e = self._f64(edges)
        if e.dim() not in (1, 2) or (e.dim() == 2 and e.shape[0] != n):
            raise ValueError("edges must be (n_bins + 1,) or (number of selected elements, n_bins + 1)")
        n_bins = e.shape[-1] - 1
        if not 1 <= n_bins <= 1024:
            raise ValueError("between 1 and 1024 bins")
        lead = (n,) if pooled else (self.n_chains, n)
        counts = self.empty(lead + (n_bins,), dtype=torch.int64)
        outside = self.empty(lead + (3,), dtype=torch.int64)
        check(lib.omc_store_histogram(self._ctx, n_iter, size, self._p(store), _ptr(idx), n,
                                      int(bool(pooled)), n_bins, e.data_ptr(), int(e.dim() == 2), counts.data_ptr(), outside.data_ptr()))
        return counts, outside

    def _counts(self, counts, what, min_dim=0, shape=None):
        torch = _torch()
        if (not isinstance(counts, torch.Tensor) or counts.dtype is not torch.int64 or not counts.is_cuda or counts.dim() < min_dim
                or (shape is not None and tuple(counts.shape) != shape)):
            raise TypeError(f"counts must be an int64 ROCm tensor {what}")
        return counts.contiguous()

    def _column(self, v, what, lead, tail=()):
        v = self.to_device(v)
        if tuple(v.shape) != lead + tail:
            raise ValueError(f"{what} must have the leading shape of counts, {lead}" + (f", and {tail}" if tail else ""))
        return v

    @staticmethod
    def _kde2d_probs(probs):
        p = np.zeros(0) if probs is None else np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if p.ndim != 1 or p.size > 16 or not np.all((p > 0) & (p < 1)):
            raise ValueError("probs must be at most 16 shares of mass, each in (0, 1)")
        return p

    KDE_RULES = {"given": 0, "scott": 1, "silverman": 2, "isj": 3, "experimental": 4}

    @staticmethod
    def kde_layout(n_bins):
        """The eight numbers of omc_kde_layout: threads of a workgroup, byte offsets of the counts, A2, the quarter-wave cosines,
        the Gaussian table and the block sums, bytes launched, the budget (openmcmc_amd/csrc/omc_kde_layout.h; needs no GPU)."""
        out = (C.c_int32 * 8)()
        check(lib.omc_kde_layout(int(n_bins), out))
        return list(out)

    def kde_binned(self, counts, lo, hi, rule="experimental", bw=None, bw_fct=1.0, reflect=(False, False)):
        """Kernel density estimates from bin counts, on the device (omc_kde_binned): counts int64 (.., G), 8 <= G <= 1024, over G
        evenly spaced bins of [lo, hi] (lo, hi fp64 of the leading shape) -> (density (.., G) at the bin centres, bw, mode, flag
        int32), device tensors.  rule: "scott", "silverman", "isj" (improved Sheather-Jones), "experimental" (the mean of the last
        two, ArviZ's default) or "given" with bw, a tensor of the leading shape; every bandwidth is multiplied by bw_fct.
        reflect=(lower, upper): the grid starts / ends at a bound of the support and the mass beyond it is mirrored back.
        flag: 0 ok, 1 ISJ found no root and Silverman's bandwidth stands in, 2 degenerate (NaN outputs; the other columns are not
        affected).  The estimate is a function of (counts, lo, hi) alone: under a sharded run all-reduce the counts taken over
        the same edges and make one call -- that is the KDE of all ranks' chains.  Repeated calls are bit-equal."""
        if rule not in self.KDE_RULES:
            raise ValueError(f"rule must be one of {sorted(self.KDE_RULES)}")
        counts = self._counts(counts, "(.., G)", min_dim=1)
        lead, G = tuple(counts.shape[:-1]), counts.shape[-1]
        if not 8 <= G <= 1024:
            raise ValueError("between 8 and 1024 bins")
        n_cols = int(np.prod(lead, dtype=np.int64))
        if n_cols < 1:
            raise ValueError("no column")
        lo, hi = self._column(lo, "lo", lead), self._column(hi, "hi", lead)
        if (rule == "given") != (bw is not None):
            raise ValueError('bw goes with rule="given"')
        bw_in = None if bw is None else self._column(bw, "bw", lead)
        density, bw_out, mode = self.empty(lead + (G,)), self.empty(lead), self.empty(lead)
        flag = self.empty(lead, dtype=_torch().int32)
        check(lib.omc_kde_binned(self._ctx, n_cols, G, counts.data_ptr(), self._p(lo), self._p(hi), self.KDE_RULES[rule],
                                 self._p(bw_in), float(bw_fct), int(bool(reflect[0])) | 2 * int(bool(reflect[1])),
                                 self._p(density), self._p(bw_out), flag.data_ptr(), self._p(mode)))
        return density, bw_out, mode, flag

    KDE2D_RULES = {"given": 0, "scott": 1, "silverman": 1}

    @staticmethod
    def kde2d_layout(nx, ny):
        """The sixteen numbers of omc_kde2d_layout: TX, TY (output tile), RY (columns a lane owns), RB (rows of a count block),
        threads, tiles along x and y, stride of a count row, slots of a plane of weights, byte offsets of the counts, the rows'
        flags, the rows' masks and the weights, bytes of a wave's weights, bytes launched, the budget
        (openmcmc_amd/csrc/omc_kde2d_layout.h; needs no GPU)."""
        out = (C.c_int32 * 16)()
        check(lib.omc_kde2d_layout(int(nx), int(ny), out))
        return list(out)

    def kde2d_binned(self, counts, lo_x, hi_x, lo_y, hi_y, rule="scott", bw=None, bw_fct=1.0, probs=None):
        """Joint kernel density estimates from 2-D bin counts, on the device (omc_kde2d_binned): counts int64 (.., nx, ny),
        8 <= nx, ny <= 256, over evenly spaced bins of [lo_x, hi_x] x [lo_y, hi_y] (fp64 of the leading shape) -> (density
        (.., nx, ny) at the bin centres, bw (.., 3) = the kernel covariance (h_xx, h_xy, h_yy), mode (.., 2), level (.., n_probs),
        level_pos int64 (.., n_probs), flag int32), device tensors.  rule: "scott" or "silverman" (the same rule in two
        dimensions, H = N^(-1/3) S: what scipy.stats.gaussian_kde does) or "given" with bw, a tensor (.., 3); every H is
        multiplied by bw_fct^2.  probs: the shares of mass, each in (0, 1), at most 16, whose highest-density regions are wanted:
        {density >= level} holds that share; level_pos is the level's position among the densities in descending order.
        flag: 0 ok, 2 degenerate (NaN outputs, level_pos -1; the other grids are not affected).  The estimate is a function of
        (counts, grid) alone: under a sharded run all-reduce the counts taken over the same edges and make one call -- that is the
        KDE of all ranks' chains.  Repeated calls are bit-equal."""
        torch = _torch()
        if rule not in self.KDE2D_RULES:
            raise ValueError(f"rule must be one of {sorted(self.KDE2D_RULES)}")
        counts = self._counts(counts, "(.., nx, ny)", min_dim=2)
        lead, (nx, ny) = tuple(counts.shape[:-2]), counts.shape[-2:]
        if not (8 <= nx <= 256 and 8 <= ny <= 256):
            raise ValueError("between 8 and 256 bins per axis")
        n_grids = int(np.prod(lead, dtype=np.int64))
        if n_grids < 1:
            raise ValueError("no grid")
        ends = [self._column(v, what, lead) for v, what in ((lo_x, "lo_x"), (hi_x, "hi_x"), (lo_y, "lo_y"), (hi_y, "hi_y"))]
        if (rule == "given") != (bw is not None):
            raise ValueError('bw goes with rule="given"')
        bw_in = None if bw is None else self._column(bw, "bw", lead, (3,))
        p = self._kde2d_probs(probs)
        n_probs = int(p.size)
        probs_dev = self._f64(p) if n_probs else None
        density, bw_out, mode = self.empty(lead + (nx, ny)), self.empty(lead + (3,)), self.empty(lead + (2,))
        level = self.empty(lead + (n_probs,))
        level_pos = self.empty(lead + (n_probs,), dtype=torch.int64)
        flag = self.empty(lead, dtype=torch.int32)
        check(lib.omc_kde2d_binned(self._ctx, n_grids, nx, ny, counts.data_ptr(), *(self._p(v) for v in ends),
                                   self.KDE2D_RULES[rule], self._p(bw_in), float(bw_fct), n_probs, self._p(probs_dev),
                                   self._p(density), self._p(bw_out), self._p(mode), self._p(level) if n_probs else None,
                                   level_pos.data_ptr() if n_probs else None, flag.data_ptr()))
        return density, bw_out, mode, level, level_pos, flag

    @staticmethod
    def hist2d_tile(nx, ny, per_pair=False, pool_pairs=False):
        """(TE, RB) of omc_store_histogram2d at an nx x ny grid: a workgroup counts a tile of TE consecutive pairs (1 with
        pool_pairs: one grid for all pairs) over slices of RB rows (openmcmc_amd/csrc/omc_hist2d_layout.h through
        omc_store_histogram2d_layout; needs no GPU).  pool_pairs: False / 0 a grid per pair, True / 1 pooled pairs, 2 pooled
        pairs with the occupancy grid."""
        return tuple(StoreOps.hist2d_layout(nx, ny, per_pair, pool_pairs)[1:3])

    @staticmethod
    def hist2d_layout(nx, ny, per_pair=False, pool_pairs=False):
        """The fourteen numbers of omc_store_histogram2d_layout: form (0 LDS counters, 1 direct), TE, RB, strides of a pair's
        x and y edges and of its counters, byte offsets of the x edges, the y edges, the counters, the occupancy counters and
        the outside counts, bytes launched, the budget, threads of a workgroup."""
        out = (C.c_int32 * 14)()
        check(lib.omc_store_histogram2d_layout(int(nx), int(ny), int(bool(per_pair)), int(pool_pairs), out))
        return list(out)

    def store_histogram2d(self, store_x, store_y, edges_x, edges_y, index_x=None, index_y=None, pooled=True, pool_pairs=False,
                          occupancy=False):
        """(counts, outside[, occupied]) of pairs of elements of device stores (n_iter, C, size_x) and (n_iter, C, size_y) -- the
        same tensor or two --, on the device (omc_store_histogram2d).  Pair k is (element index_x[k] of store_x, element
        index_y[k] of store_y) of the same row; the two selections must be equally long.  counts int64 (n_pairs, nx, ny) pooled
        over chains and iterations, else (C, n_pairs, nx, ny) = np.histogram2d(x, y, bins=[edges_x, edges_y])[0] of the pair's
        draws; with pool_pairs all pairs are counted into one grid, (nx, ny) or (C, nx, ny).  outside int64 (.., 2) = pairs
        with a coordinate outside its edges, pairs with a NaN coordinate (left out, as in numpy).  occupancy=True (pool_pairs
        only, at most 256 pairs): occupied int64, the shape of counts = the rows (iteration, chain) in which the cell holds at
        least one of the row's pairs.  edges_x (nx + 1,), edges_y (ny + 1,) shared by all pairs, or (n_pairs, nx + 1) and
        (n_pairs, ny + 1) per pair (both or neither; not with pool_pairs); host arrays (uploaded synchronously) or device
        tensors; non-decreasing, no NaN."""
        torch = _torch()
        n_iter, size_x = self._store_shape(store_x)
        n_iter_y, size_y = self._store_shape(store_y)
        if n_iter_y != n_iter:
            raise ValueError("store_x and store_y must hold the same number of iterations")
        idx_x, n = self._store_index(index_x, size_x)
        idx_y, n_y = self._store_index(index_y, size_y)
        if n != n_y:
            raise ValueError(f"{n} elements of x against {n_y} of y: pairs need equally many")
        ex, ey = self._f64(edges_x), self._f64(edges_y)
        if ex.dim() != ey.dim() or ex.dim() not in (1, 2) or (ex.dim() == 2 and (ex.shape[0] != n or ey.shape[0] != n)):
            raise ValueError("edges must be (nx + 1,) and (ny + 1,), or (number of pairs, nx + 1) and (number of pairs, ny + 1)")
        if ex.dim() == 2 and pool_pairs:
            raise ValueError("pooled pairs share their edges")
        if occupancy and not pool_pairs:
            raise ValueError("occupancy is that of the pooled pairs: pool_pairs=True")
        nx, ny = ex.shape[-1] - 1, ey.shape[-1] - 1
        if not (1 <= nx <= 1024 and 1 <= ny <= 1024):
            raise ValueError("between 1 and 1024 bins per axis")
        lead = (() if pooled else (self.n_chains,)) + (() if pool_pairs else (n,))
        counts = self.empty(lead + (nx, ny), dtype=torch.int64)
        outside = self.empty(lead + (2,), dtype=torch.int64)
        occupied = self.empty(lead + (nx, ny), dtype=torch.int64) if occupancy else None
        check(lib.omc_store_histogram2d(self._ctx, n_iter, size_x, self._p(store_x), _ptr(idx_x),
                                        size_y, self._p(store_y), _ptr(idx_y), n, int(bool(pooled)),
                                        int(bool(pool_pairs)), nx, ex.data_ptr(), ny, ey.data_ptr(), int(ex.dim() == 2),
                                        counts.data_ptr(), outside.data_ptr(), _ptr(occupied)))
        return (counts, outside, occupied) if occupancy else (counts, outside)

    @staticmethod
    def _n_labels(n_labels):
        k = int(n_labels)
        if k != n_labels or k < 1:
            raise ValueError("n_labels must be an integer >= 1")
        if k > 64:
            raise NotImplementedError("at most 64 labels")
        return k

    def store_coalloc(self, store, n_labels, index=None, pooled=True, per_label=False):
        """(counts, flags) of the allocation vectors in a device store (n_iter, C, size) of fp64 labels 0 .. n_labels - 1, on the
        device (omc_store_coalloc).  counts int64 (n, n) pooled over chains and iterations, else (C, n, n): entry (i, j) = the
        rows in which elements i and j carry the same label -- (Z[:, :, None] == Z[:, None, :]).sum(0) of the gathered labels;
        with per_label (K, n, n) or (C, K, n, n): entry (k, i, j) = the rows with z_i == k and z_j == k.  flags int64 (.., n, 2) =
        NaN draws (element absent) and other draws that are no label in [0, n_labels), per element; such a draw matches
        nothing, not even itself.  Exactly symmetric; every entry an exact integer; at most 64 labels."""
        torch = _torch()
        n_iter, size, idx, n = self._selection(store, index)
        k = self._n_labels(n_labels)
        lead = () if pooled else (self.n_chains,)
        counts = self.empty(lead + ((k,) if per_label else ()) + (n, n), dtype=torch.int64)
        flags = self.empty(lead + (n, 2), dtype=torch.int64)
        self._check_text(lib.omc_store_coalloc(self._ctx, n_iter, size, self._p(store), _ptr(idx), n, k, int(bool(pooled)),
                                               int(bool(per_label)), counts.data_ptr(), flags.data_ptr()))
        return counts, flags

    def store_partition_score(self, store, n_labels, counts, index=None, pooled=True):
        """(score, best) of the stored states of the same selection against counts, the plain (per_label=False) result of
        store_coalloc for the same arguments, on the device (omc_store_partition_score).  score int64 (n_iter, C): of the state
        s of a batch of R rows, sum over i < j of [z_i == z_j] (R - 2 counts_ij) -- R times the squared distance of the
        state's co-membership matrix from counts / R, up to a constant; best int64 (2,) pooled, else (C, 2) = the row of the
        first minimum of the batch (it * C + c pooled, it per chain) and its score: Dahl's least-squares partition."""
        torch = _torch()
        n_iter, size, idx, n = self._selection(store, index)
        k = self._n_labels(n_labels)
        lead = () if pooled else (self.n_chains,)
        counts = self._counts(counts, lead + (n, n), shape=lead + (n, n))
        score = self.empty((n_iter, self.n_chains), dtype=torch.int64)
        best = self.empty(lead + (2,), dtype=torch.int64)
        self._check_text(lib.omc_store_partition_score(self._ctx, n_iter, size, self._p(store), _ptr(idx), n, k, int(bool(pooled)),
                                                       counts.data_ptr(), score.data_ptr(), best.data_ptr()))
        return score, best

    @staticmethod
    def rank_schedule(n_draws, tile=0):
        """The launches that sort columns of n_draws keys with LDS tiles of `tile` keys (0: the default 8192), as
        omc_store_rank_schedule lists them: [(kind, k, j), ...] (include/omcmc_hip.h; needs no GPU)."""
        n = C.c_int64(0)
        cap = 1024
        out = (C.c_int64 * (3 * cap))()
        check(lib.omc_store_rank_schedule(int(n_draws), int(tile), out, cap, C.byref(n)))
        return [tuple(out[3 * i: 3 * i + 3]) for i in range(n.value)]

    def store_ranks(self, store, index=None, split=False):
        """Average ranks of the draws of every selected element of a device store (n_iter, C, size), on the device
        (omc_store_ranks): a device tensor (n_iter, C, n_idx), scipy.stats.rankdata(method="average") of the element's
        n_iter * C draws, bit for bit.  split=True: ranks among the split draws (first and last n_iter // 2 iterations of
        every chain, n_iter >= 4), NaN in the dropped middle row of an odd n_iter.  An element with a NaN draw gives NaN."""
        n_iter, size, idx, n = self._selection(store, index)
        if n_iter < (4 if split else 1):
            raise ValueError("split ranks need at least 4 stored iterations")
        out = self.empty(n_iter, self.n_chains, n)
        check(lib.omc_store_ranks(self._ctx, n_iter, size, self._p(store), _ptr(idx), n,
                                  int(bool(split)), self._p(out)))
        return out

    def store_rank_diagnostics(self, store, index=None):
        """Rank-normalised split R-hat, bulk-ESS and tail-ESS (Vehtari et al. 2021) of every selected element of a device
        store (n_iter, C, size), on the device (omc_store_rank_diagnostics): (rhat, ess_bulk, ess_tail) as device tensors
        of shape (n_idx,).  n_iter >= 4; an element with a NaN or infinite draw gives NaN."""
        n_iter, size, idx, n = self._selection(store, index)
        if n_iter < 4:
            raise ValueError("rank-normalised R-hat and ESS need at least 4 stored iterations")
        rhat, bulk, tail = self.empty(n), self.empty(n), self.empty(n)
        check(lib.omc_store_rank_diagnostics(self._ctx, n_iter, size, self._p(store), _ptr(idx), n,
                                             self._p(rhat), self._p(bulk), self._p(tail)))
        return rhat, bulk, tail

    def store_ess_indicator(self, store, prob_lo, prob_hi, index=None, counts=0, algo=0):
        """Effective sample size of indicator series of every selected element of a device store (n_iter, C, size), on the
        device (omc_store_ess_indicator): ArviZ's ess(method="quantile") and ess(method="local").  prob_lo, prob_hi: equally long
        sequences; prob_lo[i] < 0 (or None for all) means no lower end, I = (x <= q_hi), else 0 <= lo <= hi <= 1 and
        I = (q_lo <= x <= q_hi), q the np.quantile of the element's split draws.  Returns (ess, lags, q[, counts]) as device
        tensors: ess fp64 (n_p, n_idx), lags int32 (n_p, n_idx), q fp64 (n_p, n_idx, 2) the thresholds (NaN: no lower end), and
        with counts = n_cnt > 0 the exact integers int64 (n_p, n_idx, 2 + 2 n_cnt) = Nn, Q, then the pairs A(t), H(t), t < n_cnt
        <= n_iter // 2 (include/omcmc_hip.h).  Intervals beyond 32 go in groups of 32.  algo: 0 auto, 1 bits in LDS, 2 bits in
        global memory -- same bits.  n_iter >= 4; an element with a NaN or infinite draw gives NaN."""
        torch = _torch()
        n_iter, size, idx, n = self._selection(store, index)
        if n_iter < 4:
            raise ValueError("the ESS of an indicator needs at least 4 stored iterations")
        hi = np.ascontiguousarray(np.atleast_1d(np.asarray(prob_hi, dtype=np.float64)))
        lo = np.full(hi.shape, -1.0) if prob_lo is None else np.ascontiguousarray(np.atleast_1d(np.asarray(prob_lo, dtype=np.float64)))
        if hi.ndim != 1 or hi.size < 1 or lo.shape != hi.shape:
            raise ValueError("prob_lo and prob_hi must be equally long non-empty one-dimensional sequences")
        n_cnt = int(counts)
        n_p = hi.size
        ess, q = self.empty(n_p, n), self.empty(n_p, n, 2)
        lags = self.empty((n_p, n), dtype=torch.int32)
        cnt = self.empty((n_p, n, 2 + 2 * n_cnt), dtype=torch.int64) if n_cnt > 0 else None
        dp = C.POINTER(C.c_double)
        for i in range(0, n_p, 32):  # at most 32 intervals per call of omc_store_ess_indicator
            m = min(32, n_p - i)
            check(lib.omc_store_ess_indicator(self._ctx, n_iter, size, self._p(store), _ptr(idx), n,
                                              lo[i: i + m].ctypes.data_as(dp), hi[i: i + m].ctypes.data_as(dp), m, int(algo),
                                              self._p(ess[i: i + m]), lags[i: i + m].data_ptr(), self._p(q[i: i + m]),
                                              cnt[i: i + m].data_ptr() if cnt is not None else None, n_cnt))
        return (ess, lags, q, cnt) if cnt is not None else (ess, lags, q)

    def store_order_stats(self, store, pos, index=None, split=True):
        """Order statistics of every selected element of a device store (n_iter, C, size) at given positions, on the device
        (omc_store_order_stats): a device tensor (n_idx, n_pos) = np.sort(column)[pos[e]], the column being the element's split
        draws (split=True: first and last n_iter // 2 iterations of every chain, n_iter >= 4) or all n_iter * C draws.  pos:
        integers (n_idx, n_pos), a host array or a device tensor; a position outside the column raises ValueError.  An element
        with a NaN draw gives NaN; a zero comes back as +0.0."""
        n_iter, size, idx, n = self._selection(store, index)
        if n_iter < (4 if split else 1):
            raise ValueError("split order statistics need at least 4 stored iterations")
        p = self._int64(pos, "pos", empty_ok=False)
        if p.dim() != 2 or p.shape[0] != n or p.shape[1] < 1:
            raise ValueError(f"pos must be (number of selected elements = {n}, n_pos), got shape {tuple(p.shape)}")
        out = self.empty(n, p.shape[1])
        check(lib.omc_store_order_stats(self._ctx, n_iter, size, self._p(store), _ptr(idx), n, int(bool(split)),
                                        p.data_ptr(), p.shape[1], self._p(out)))
        return out

    def store_hdi(self, store, prob, index=None, pooled=True, omit_nan=True):
        """Highest-density intervals of every selected element of a device store (n_iter, C, size), on the device
        (omc_store_hdi): (hdi, n_valid) as device tensors.  hdi is fp64 (n_prob, n_idx, 2) pooled over chains and iterations,
        else (n_prob, C, n_idx, 2) per chain, [..., 0] the lower and [..., 1] the upper limit of the shortest interval that
        holds floor(prob * n) + 1 of the column's n valid draws (ArviZ's unimodal hdi: both limits are stored draws);
        n_valid is int64 (n_idx,) or (C, n_idx), the draws that are not NaN.  prob: a number or a sequence of at most 8,
        each inside (0, 1); a scalar is one probability (n_prob = 1).  omit_nan leaves NaN draws out; without it a column
        with a NaN gives NaN.  A column with an infinite draw or without a valid draw gives NaN."""
        n_iter, size, idx, n = self._selection(store, index)
        probs = np.atleast_1d(np.asarray(prob, dtype=np.float64))
        if probs.ndim != 1 or not 1 <= probs.size <= 8:
            raise ValueError("prob must be a number or a sequence of 1 to 8 numbers")
        if not np.all((probs > 0) & (probs < 1)):
            raise ValueError("every prob must lie inside (0, 1)")
        lead = (probs.size,) if pooled else (probs.size, self.n_chains)
        out = self.empty(*lead, n, 2)
        cnt = self.empty(lead[1:] + (n,), dtype=_torch().int64)
        host = (C.c_double * probs.size)(*probs.tolist())
        check(lib.omc_store_hdi(self._ctx, n_iter, size, self._p(store), _ptr(idx), n, host, probs.size,
                                int(not pooled), int(bool(omit_nan)), self._p(out), cnt.data_ptr()))
        return out, cnt

    REDUCE_OPS = {"sum": 0, "min": 1, "max": 2, "argmin": 3, "argmax": 4, "count_above": 5, "supnorm": 6}

    def _reduce_vector(self, v, n, what):
        """device fp64 (n,) of a vector aligned with the selection: a host array or a device tensor, a scalar is broadcast"""
        if v is None:
            return None
        t = self._f64(v)
        if t.numel() == 1:
            t = t.reshape(1).expand(n)
        if t.dim() != 1 or t.shape[0] != n:
            raise ValueError(f"{what} must be a scalar or hold one value per selected element ({n}), got shape {tuple(t.shape)}")
        return t.contiguous()

    def store_reduce(self, store, op, index=None, omit_nan=True, a=None, b=None):
        """Per-draw reduction of a device store (n_iter, C, size) over the selected elements of every row, on the device
        (omc_store_reduce): (out, count) as device tensors (n_iter, C), fp64 and int64 -- shaped like log_post.  op, with x the
        element at selection position k: "sum" of a[k] * x (a=None: of x), "min" / "max" of x, "argmin" / "argmax" the position
        in the selection of the first smallest / largest x, "count_above" the number with x > a[k], "supnorm" the largest
        fabs(x - a[k]) / b[k].  count is the number of terms that are not NaN.  omit_nan leaves NaN terms out (np.nansum, np.nanmax,
        ...; a row without a term gives 0 for "sum" and "count_above", NaN otherwise); without it a NaN term makes the result NaN,
        "argmin" / "argmax" the position of the first NaN.  a, b: host arrays or device tensors with one value per SELECTED
        element, scalars are broadcast.  "sum" is within n_idx 2^-53 sum|terms| of the exact sum, everything else is exact."""
        n_iter, size, idx, n = self._selection(store, index)
        code = self.REDUCE_OPS.get(op)
        if code is None:
            raise ValueError(f"unknown reduction {op!r}: one of {', '.join(self.REDUCE_OPS)}")
        av, bv = self._reduce_vector(a, n, "a"), self._reduce_vector(b, n, "b")
        out = self.empty(n_iter, self.n_chains)
        cnt = self.empty((n_iter, self.n_chains), dtype=_torch().int64)
        self._check_text(lib.omc_store_reduce(
            self._ctx, n_iter, size, self._p(store), _ptr(idx), n, code, int(bool(omit_nan)), self._p(av), self._p(bv),
            self._p(out), cnt.data_ptr()))
        return out, cnt

    def store_first_failure(self, store, lo, hi, pos, index=None, want_rows=False, algo=0):
        """First failures of the stored states of a device store (n_iter, C, size) against per-element sides, on the device
        (omc_store_first_failure; one read of the store for all slots): (h, r) as device tensors.  lo, hi (fp64) and pos
        (integers, a permutation of 0 .. n_idx - 1 per slot) are (L, n_idx) tables of 1 <= L <= 8 slots, host arrays or device
        tensors; (n_idx,) vectors are one slot.  With x the element at selection position k, a row agrees at k iff x is not NaN,
        (lo[k] == -inf or x > lo[k]) and (hi[k] == +inf or x < hi[k]); its first failure is the smallest pos[k] among the positions
        it does not agree at, n_idx if it agrees everywhere.  h is int64 (L, n_idx + 1): h[l, j] = the rows, pooled over chains and
        iterations, whose first failure is j; r is int32 (L, n_iter, C), the first failures themselves, or None without
        want_rows.  algo: 0 automatic, 1 short rows staged in LDS, 2 a wave per row -- the same integers.  Exact: repeated calls
        are equal, and the h of several engines over the same tables (chains sharded over ranks) add."""
        torch = _torch()
        n_iter, size, idx, n = self._selection(store, index)
        lo_t, hi_t = self._f64(lo), self._f64(hi)
        pos_t = self._int64(pos, "pos", empty_ok=False)
        if lo_t.dim() == 1:
            lo_t = lo_t.unsqueeze(0)
        if hi_t.dim() == 1:
            hi_t = hi_t.unsqueeze(0)
        if pos_t.dim() == 1:
            pos_t = pos_t.unsqueeze(0)
        L = lo_t.shape[0]
        if lo_t.dim() != 2 or not (tuple(lo_t.shape) == tuple(hi_t.shape) == tuple(pos_t.shape) == (L, n)):
            raise ValueError(f"lo, hi and pos must be ({n},) or (L, {n}), one value per selected element and slot, all of one shape")
        if not 1 <= L <= 8:
            raise ValueError("between 1 and 8 slots")
        if int(pos_t.min()) < 0 or int(pos_t.max()) >= n:  # (before the cast to int32; the library checks its table again)
            raise ValueError(f"pos must lie in [0, {n})")
        pos_t = pos_t.to(torch.int32).contiguous()
        h = self.empty((L, n + 1), dtype=torch.int64)
        r = self.empty((L, n_iter, self.n_chains), dtype=torch.int32) if want_rows else None
        self._check_text(lib.omc_store_first_failure(
            self._ctx, n_iter, size, self._p(store), _ptr(idx), n, L, self._p(lo_t), self._p(hi_t), pos_t.data_ptr(), int(algo),
            h.data_ptr(), _ptr(r)))
        return h, r

    def store_autocorr(self, store, max_lag, index=None, pooled=True, normalize=True):
        """Autocorrelation of every selected element of a device store (n_iter, C, size), on the device (omc_store_autocorr):
        (acf, tau, window, mean) as device tensors.  acf is fp64 (n_idx, max_lag + 1) pooled -- the chains' autocovariances
        around their own means, averaged -- else (C, n_idx, max_lag + 1) per chain: g(t) = sum_i d_i d_{i+t} / n_iter of the
        centred draws, divided by g(0) with normalize.  tau, fp64 (n_idx,) or (C, n_idx), is the integrated autocorrelation
        time by Geyer's initial positive sequence, window (int32, same shape) the lags it used: a window that reaches
        max_lag means tau is a lower bound.  mean is fp64 (C, n_idx), the per-chain means the draws were centred on.
        0 <= max_lag <= n_iter - 1, n_iter >= 2.  A column with a NaN or infinite draw gives NaN; a column that never moved
        an autocovariance of 0, NaN once normalised, tau NaN and window 0."""
        n_iter, size, idx, n = self._selection(store, index)
        if n_iter < 2:
            raise ValueError("the autocorrelation needs at least 2 stored iterations")
        max_lag = int(max_lag)
        if not 0 <= max_lag <= n_iter - 1:
            raise ValueError(f"max_lag must lie in [0, n_iter - 1] = [0, {n_iter - 1}]")
        lead = () if pooled else (self.n_chains,)
        acf = self.empty(*lead, n, max_lag + 1)
        tau = self.empty(*lead, n)
        window = self.empty(lead + (n,), dtype=_torch().int32)
        mean = self.empty(self.n_chains, n)
        self._check_text(lib.omc_store_autocorr(
            self._ctx, n_iter, size, self._p(store), _ptr(idx), n, max_lag, int(not pooled), int(bool(normalize)), self._p(acf),
            self._p(tau), window.data_ptr(), self._p(mean)))
        return acf, tau, window, mean

    def store_project(self, store, W, index=None, offset=None, base=None, omit_nan=True, prec=None, z=None, replicate=0, out=None):
        """Linear maps of a device store (n_iter, C, size) over the selected elements of every row, on the device
        (omc_store_project): the device tensor (n_iter, C, m) with, for x the element at selection position k of row (it, c),
        out[it, c, j] = base[it, c, j] + offset[j] + sum_k W[j, k] * x[k] -- store2d[:, index] @ W.T.  W (m, n_idx) and offset (m,)
        are host arrays or device tensors; a 1-D W counts as one output, and the leading columns of a wider fp64 device matrix
        are read where they lie (ld_w = its row stride).  base, prec and z are device stores (n_iter, C, m) --
        prec (n_iter, C, 1) or (n_iter, C, m) -- of the same iterations.  With prec, z / sqrt(prec) is added: z the injected
        normals, else element j of the chain's normal stream at draw index (1 << 41) + it + (replicate << 44), replicate
        0 .. 15 -- the same numbers however the chains are sharded over engines.  omit_nan leaves NaN elements out (their terms
        are 0: np.nansum; a row with nothing left gives base + offset); without it IEEE rules hold as in numpy's matmul.  out: the
        tensor to write, which may be base itself (accumulate in place).  Within (n_idx + 2) 2^-53 (|base| + |offset| +
        sum|terms|) of the exact value; repeated calls, and the same rows in a store of fewer iterations or chains, are
        bit-equal."""
        torch = _torch()
        n_iter, size, idx, n = self._selection(store, index)
        if (isinstance(W, torch.Tensor) and W.is_cuda and W.dtype is torch.float64 and W.dim() == 2 and W.shape[0] > 1
                and W.stride(1) == 1 and W.stride(0) >= W.shape[1]):
            Wt = W  # rows of a wider device matrix are read where they lie (ld_w = the row stride)
        else:
            Wt = self.to_device(W)
        if Wt.dim() == 1:
            Wt = Wt.reshape(1, -1)
        if Wt.dim() != 2 or Wt.shape[0] < 1 or Wt.shape[1] != n:
            raise ValueError(f"W must be (m, {n}): one row per output, one column per selected element, got shape {tuple(Wt.shape)}")
        m = Wt.shape[0]
        off = None
        if offset is not None:
            off = self.to_device(offset).reshape(-1)
            if off.numel() != m:
                raise ValueError(f"offset must hold one value per output ({m})")
        sizes = {"base": (m,), "prec": (1, m), "z": (m,)}
        for what, t in (("base", base), ("prec", prec), ("z", z)):
            if t is None:
                continue
            n_it, sz = self._store_shape(t)
            if n_it != n_iter:
                raise ValueError(f"{what} holds {n_it} iterations, the store {n_iter}")
            if sz not in sizes[what]:
                raise ValueError(f"{what} must hold {' or '.join(str(s) for s in sizes[what])} values per draw, got {sz}")
        if z is not None and prec is None:
            raise ValueError("z needs prec")
        if out is None:
            out = self.empty(n_iter, self.n_chains, m)
        elif self._store_shape(out) != (n_iter, m):
            raise ValueError(f"out must be ({n_iter}, {self.n_chains}, {m})")
        elif out.data_ptr() == store.data_ptr():
            raise ValueError("out must not be the store the map reads (other rows of it are still being read)")
        replicate = int(replicate)
        if not 0 <= replicate <= 15:
            raise ValueError("replicate must lie in 0 .. 15")
        self._check_text(lib.omc_store_project(
            self._ctx, n_iter, size, self._p(store), _ptr(idx), n, m, self._p(Wt), Wt.stride(0), self._p(off), self._p(base),
            int(bool(omit_nan)), self._p(prec), 0 if prec is None else prec.shape[2], self._p(z), replicate, self._p(out)))
        return out

    def _loo_inputs(self, store, index, y, prec):
        """_loglik_inputs of store_psis / store_loo_expect, where y and prec are both None for an entry of log-likelihoods"""
        if (y is None) != (prec is None):
            raise ValueError("y and prec must be given together")
        if y is None:
            return self._selection(store, index) + (None, None)
        return self._loglik_inputs(store, y, prec, index)

    def _loglik_inputs(self, store, y, prec, index):
        """(n_iter, size, idx, n, y, prec) of the observation and precision arguments of store_loglik / store_psis"""
        n_iter, size, idx, n = self._selection(store, index)
        yv = self._reduce_vector(y.reshape(-1) if isinstance(y, _torch().Tensor) else np.asarray(y, dtype=np.float64).reshape(-1), n, "y")
        n_it, sz = self._store_shape(prec)
        if n_it != n_iter:
            raise ValueError(f"prec holds {n_it} iterations, the store {n_iter}")
        if sz not in (1, n):
            raise ValueError(f"prec must hold 1 or {n} values per draw, got {sz}")
        return n_iter, size, idx, n, yv, prec

    def store_loglik(self, store, y, prec, index=None, lse=True, mean=True, var=True, ll=False):
        """Column summaries of the pointwise Normal log-density of a device MEAN entry (n_iter, C, size), on the device
        (omc_store_loglik): (lse, mean, var, ll) as device tensors, None for what was not asked.  For the element x at selection
        position k of row (it, c), ll = 0.5 log(tau) - 0.5 log(2 pi) - 0.5 tau (y[k] - x)^2 with tau = prec[it, c, 0 or k]; lse (n_idx,) is
        log sum exp of ll over all n_iter * C >= 2 draws, mean and var (n_idx,) its mean and unbiased variance, ll the pointwise
        entry (n_iter, C, n_idx) in the store's layout.  y: host array or device tensor with one value per SELECTED element; prec:
        a device store (n_iter, C, 1) or (n_iter, C, n_idx).  A column with an ll that is not finite gives NaN in lse, mean and
        var.  One read of the entry; repeated calls are bit-equal."""
        n_iter, size, idx, n, yv, prec = self._loglik_inputs(store, y, prec, index)
        if not (lse or mean or var or ll):
            raise ValueError("nothing asked for: lse, mean, var and ll are all False")
        outs = [self.empty(n) if want else None for want in (lse, mean, var)]
        ll_out = self.empty(n_iter, self.n_chains, n) if ll else None
        self._check_text(lib.omc_store_loglik(
            self._ctx, n_iter, size, self._p(store), _ptr(idx), n, self._p(yv), self._p(prec), prec.shape[2], self._p(outs[0]),
            self._p(outs[1]), self._p(outs[2]), self._p(ll_out)))
        return outs[0], outs[1], outs[2], ll_out

    def store_psis(self, store, tail_max, index=None, y=None, prec=None):
        """Pareto-smoothed importance sampling leave-one-out of every selected column of a device store (n_iter, C, size), on the
        device (omc_store_psis): (elpd, k, tail) as device tensors (n_idx,), fp64, fp64 and int64 -- the PSIS-LOO expected log
        predictive density of the observation, the Pareto k of its importance ratios (+inf where the tail holds 4 draws or
        fewer) and the tail length used.  store holds pointwise log-likelihoods, or, with y and prec as in store_loglik, the mean
        entry from which they are computed on load (the same bits).  tail_max: a number or one per selected element, each in
        1 .. n_iter * C - 1.  A column with an ll that is not finite gives NaN, NaN and -1."""
        n_iter, size, idx, n, yv, prec = self._loo_inputs(store, index, y, prec)
        tm = self._tail_max(tail_max, n)
        elpd, k = self.empty(n), self.empty(n)
        tail = self.empty(n, dtype=_torch().int64)
        self._check_text(lib.omc_store_psis(
            self._ctx, n_iter, size, self._p(store), _ptr(idx), n, self._p(yv), self._p(prec),
            0 if prec is None else prec.shape[2], tm.data_ptr(), self._p(elpd), self._p(k), tail.data_ptr()))
        return elpd, k, tail

    def _tail_max(self, tail_max, n):
        """tail_max, a number or one per selected element, as a device int64 tensor (n,)"""
        tm = self._int64(tail_max.cpu().numpy() if isinstance(tail_max, _torch().Tensor) else tail_max, "tail_max").reshape(-1)
        if tm.numel() == 1:
            tm = tm.expand(n)
        if tm.shape[0] != n:
            raise ValueError(f"tail_max must be a number or hold one value per selected element ({n})")
        return tm.contiguous()

    def store_loo_expect(self, store, tail_max, index=None, y=None, prec=None, f="entry", values=None, values_index=None,
                         threshold=None, want=("mean", "var", "ess", "k", "tail"), lw=False):
        """PSIS-LOO expectations of every selected column of a device store (n_iter, C, size), on the device
        (omc_store_loo_expect): a dict of device tensors (n_idx,) for the names in want -- "mean", "var" (the leave-one-out
        weighted mean and population variance of a per-draw quantity f), "below" (the weighted share of draws with
        f <= threshold), "ess" (the effective sample size of the weights, W^2 / sum w^2), "invprec" (the weighted mean of
        1 / precision), "k" and "tail" (as store_psis, the same bits) -- and with lw=True "lw", the normalised smoothed log
        weights (n_iter, C, n_idx) in the store's layout, what az.psislw returns.  store, tail_max, index, y and prec as
        store_psis.  f: "entry" takes element values_index[k] (k itself without values_index) of the device entry values
        (n_iter, C, vsize); "mean" the mean entry's own element; "cdf" the Normal predictive distribution function at the
        observation (both need y and prec).  threshold: one value per selected element, required exactly with "below".
        Every draw has the smoothed weight of its position in the sorted column; tied tail draws share theirs evenly.  A
        column with an ll that is not finite gives NaN, -1 in tail and NaN down its lw column."""
        torch = _torch()
        kinds = {"entry": 0, "mean": 1, "cdf": 2}
        if f not in kinds:
            raise ValueError(f"unknown f {f!r}: one of {', '.join(kinds)}")
        names = ("mean", "var", "below", "ess", "invprec", "k", "tail")
        want = (want,) if isinstance(want, str) else tuple(want)
        for w in want:
            if w not in names:
                raise ValueError(f"unknown output {w!r}: one of {', '.join(names)}")
        if not want and not lw:
            raise ValueError("nothing asked for: want is empty and lw is False")
        n_iter, size, idx, n, yv, prec = self._loo_inputs(store, index, y, prec)
        vidx, vsize = None, 0
        if f == "entry":
            if values is None:
                raise ValueError('f="entry" needs values')
            n_it, vsize = self._store_shape(values)
            if n_it != n_iter:
                raise ValueError(f"values holds {n_it} iterations, the store {n_iter}")
            vidx, nv = self._store_index(values_index, vsize)
            if nv != n:
                raise ValueError(f"values selects {nv} elements, the store {n}")
        elif values is not None or values_index is not None:
            raise ValueError('values and values_index apply to f="entry" only')
        if ("below" in want) != (threshold is not None):
            raise ValueError('threshold and "below" must be given together')
        thr = None
        if threshold is not None:
            thr = self._reduce_vector(threshold.reshape(-1) if isinstance(threshold, torch.Tensor)
                                      else np.asarray(threshold, dtype=np.float64).reshape(-1), n, "threshold")
        tm = self._tail_max(tail_max, n)
        out = {w: (self.empty(n, dtype=torch.int64) if w == "tail" else self.empty(n)) for w in want}
        if lw:
            out["lw"] = self.empty(n_iter, self.n_chains, n)
        p = {w: (out[w].data_ptr() if w in out else None) for w in names + ("lw",)}
        self._check_text(lib.omc_store_loo_expect(
            self._ctx, n_iter, size, self._p(store), _ptr(idx), n, self._p(yv), self._p(prec),
            0 if prec is None else prec.shape[2], tm.data_ptr(), kinds[f], self._p(values), vsize, _ptr(vidx), self._p(thr),
            p["mean"], p["var"], p["below"], p["ess"], p["invprec"], p["k"], p["tail"], p["lw"]))
        return out

    def store_thin(self, store, every, first=0):
        """store[first::every] of a device store (n_iter, C, ...) as a packed device tensor (one launch)."""
        if store.dim() < 2 or store.shape[1] != self.n_chains or not store.is_contiguous():
            raise ValueError("store must be a contiguous (n_iter, C, ...) tensor")
        n_iter = store.shape[0]
        every, first = int(every), int(first)
        if every < 1 or not 0 <= first < n_iter:
            raise ValueError("every must be >= 1 and first inside the store")
        n_out = (n_iter - first + every - 1) // every
        size = int(np.prod(store.shape[2:])) if store.dim() > 2 else 1
        out = self.empty(*((n_out,) + tuple(store.shape[1:])))
        check(lib.omc_store_thin(self._ctx, n_iter, size, self._p(store), first, every, self._p(out), None))
        return out
