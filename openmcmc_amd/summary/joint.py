import numpy as np

from openmcmc_amd.distribution.distribution import Categorical
from openmcmc_amd.summary.base import SummaryBase
from openmcmc_amd.summary.ranges import auto_range, bin_edges, grid_lengths, linspace_edges, widen


class JointSummaries(SummaryBase):
    def covariance(self, key, other=None, index=None, other_index=None, pooled=True, correlation=False):
        """Posterior covariance matrix of the elements of store[key] -- np.cov of the stored draws -- or, with `other`, of
        its elements against those of store[other] (the off-diagonal block of np.cov of the stacked variables), computed on
        the device (no gather of the store): pooled over chains and iterations -> (n_a, n_b), else per chain ->
        (C, n_a, n_b).  index / other_index select elements (in that order, repeats allowed); a 2-D entry ("log_post") counts
        as one element.  An element with a NaN draw (the padding of variable-size parameters) gives NaN in its row and
        column; a single stored draw gives 0.  Under a sharded multi-GPU run this is the covariance over this rank's
        chains only."""
        self._whole_store_on_device("covariance")
        a = self._store_3d(key)
        b = None if other is None else self._store_3d(other)
        return self.engine.store_cov(a, b, index_a=index, index_b=other_index, pooled=pooled, correlation=correlation).cpu().numpy()

    def correlation(self, key, other=None, index=None, other_index=None, pooled=True):
        """Posterior correlation matrix -- np.corrcoef of the stored draws: `covariance` scaled by the standard deviations
        and clipped to [-1, 1]; an element that never moved gives NaN in its row and column."""
        return self.covariance(key, other=other, index=index, other_index=other_index, pooled=pooled, correlation=True)

    def _allocation_labels(self, key, n_labels):
        """K of the allocation entry store[key]: n_labels, or the last dimension of the prob of the model's Categorical on key"""
        if n_labels is not None:
            return self.engine._n_labels(n_labels)
        dist = self.model.get(key) if self.model is not None else None
        if not isinstance(dist, Categorical):
            raise ValueError(f"'{key}' is not the response of a Categorical of the model: give n_labels")
        return self.engine._n_labels(np.shape(dist.prob.predictor(self.state))[-1])

    def _coallocation(self, key, n_labels, index, pooled, per_label):
        t = self._store_3d(key)
        K = self._allocation_labels(key, n_labels)
        counts, flags = self.engine.store_coalloc(t, K, index=index, pooled=pooled, per_label=per_label)
        flags = flags.cpu().numpy()
        if flags[..., 1].any():
            per_element = flags[..., 1].reshape(-1, flags.shape[-2]).sum(axis=0)
            first = int(np.flatnonzero(per_element)[0])
            el = first if index is None else int(self.engine._store_index(index, t.shape[2])[0][first])
            raise ValueError(f"'{key}' is not an allocation in [0, {K}): element {el} holds {int(per_element[first])} draws that are "
                             f"neither an integer label below {K} nor NaN")
        return t, K, counts, flags

    def coallocation(self, key, n_labels=None, index=None, pooled=True, per_label=False):
        """Posterior similarity (co-clustering) matrix of the allocation vector store[key] -- labels 0 .. K - 1 as MixtureAllocation
        draws them -- computed on the device (no gather of the store): a dict of host arrays "prob" (n, n) = P(z_i = z_j), the
        share of the stored draws in which elements i and j carry the same label, "counts" (int64, prob = counts / rows),
        "absent" (n,) the NaN draws of every element (the padding of variable-size parameters; such a draw matches nothing, so
        the diagonal of counts is rows - absent) and "rows"; per chain (pooled=False) (C, n, n), (C, n) and rows = n_iter.
        per_label=True: (K, n, n) or (C, K, n, n), entry (k, i, j) = P(z_i = k and z_j = k) -- for spike-and-slab the joint
        inclusion probability of two coefficients; its diagonal is the marginal P(z_i = k) and its sum over k the plain form.
        The matrix does not change when the labels are permuted (label switching), which mean, quantiles or kde of a label do.
        n_labels defaults to the number of categories of the model's Categorical on key.  A draw that is neither NaN nor an
        integer in [0, K) raises ValueError.  index selects elements (in that order, repeats allowed).  Under a sharded
        multi-GPU run these are this rank's chains only; counts of several ranks can simply be added."""
        self._whole_store_on_device("coallocation")
        t, _, counts, flags = self._coallocation(key, n_labels, index, pooled, per_label)
        rows = t.shape[0] * (t.shape[1] if pooled else 1)
        counts = counts.cpu().numpy()
        return {"prob": counts / float(rows), "counts": counts, "absent": flags[..., 0], "rows": rows}

    def partition(self, key, n_labels=None, index=None, pooled=True):
        """Point estimate of the partition behind the allocation vector store[key]: the stored draw whose co-membership matrix
        is nearest (least squares) to the posterior similarity matrix of `coallocation` -- Dahl's (2006) least-squares
        clustering, the stored draw of least posterior expected Binder loss --, found on the device (no gather of the store).
        A dict of host arrays: "labels" int64 (n,) the draw, relabelled in order of first appearance (0, 1, ..), -1 for an
        absent (NaN) element; "iteration", "chain" where it is stored (the first of equals); "score" its score and "scores"
        (n_iter, C) int64 those of all stored draws, sum over i < j of [z_i = z_j] (rows - 2 counts_ij): rows times the squared
        distance up to a constant.  pooled=False: one estimate per chain against that chain's own matrix -- "labels" (C, n),
        "iteration" (C,), "chain" = 0 .. C - 1, "score" (C,).  Unlike the element-wise mode of the labels it is not misled by
        label switching.  n_labels, index and the ValueError as in `coallocation`.  Under a sharded multi-GPU run this is the
        estimate from this rank's chains only."""
        self._whole_store_on_device("partition")
        t, K, counts, _ = self._coallocation(key, n_labels, index, pooled, False)
        score, best = self.engine.store_partition_score(t, K, counts, index=index, pooled=pooled)
        best = best.cpu().numpy()
        C = t.shape[1]
        if pooled:
            it, ch = np.int64(best[0] // C), np.int64(best[0] % C)
            draws = t[int(it), int(ch)]
        else:
            it, ch = best[:, 0].copy(), np.arange(C, dtype=np.int64)
            draws = t[self.engine._int64(it, "iteration"), self.engine._int64(ch, "chain")]
        draws = draws.cpu().numpy()  # (size,) or (C, size): the chosen rows alone leave the device
        if index is not None:
            draws = draws[..., self.engine._store_index(index, t.shape[2])[0].cpu().numpy()]

        def canonical(z):
            out, seen = np.full(z.shape, -1, dtype=np.int64), {}
            for i, v in enumerate(z):
                if v == v:
                    out[i] = seen.setdefault(int(v), len(seen))
            return out

        labels = canonical(draws) if pooled else np.stack([canonical(z) for z in draws])
        return {"labels": labels, "iteration": it, "chain": ch, "score": best[..., 1].copy() if not pooled else np.int64(best[1]),
                "scores": score.cpu().numpy()}

    def _axis_edges(self, t, index, bins, rng, pool_elements):
        """Edges of one axis of histogram2d: (n + 1,) shared by all pairs or (n_pairs, n + 1), by np.histogramdd's rules"""
        messages = ("bins must be integers between 1 and 1024 or arrays of edges",
                    "bins must be integers, (n + 1,) edges or, without pool_elements, (n_pairs, n + 1) edges")
        return bin_edges(bins, rng, lambda: self._minmax(t, index), messages, pool=pool_elements)

    def _hist2d(self, key_x, key_y, index_x, index_y, bins, range, pooled, pool_elements, occupancy):
        tx = self._store_3d(key_x)
        ty = tx if key_y is None else self._store_3d(key_y)
        try:
            n_given = len(bins)
        except TypeError:
            n_given = 1
        if n_given != 2:  # (np.histogram2d: an int, or one array of edges for both axes)
            bins = [bins, bins]
        rngs = [None, None] if range is None else list(range)
        if len(rngs) != 2:
            raise ValueError("range must be [[xlo, xhi], [ylo, yhi]]")
        ex = self._axis_edges(tx, index_x, bins[0], rngs[0], pool_elements)
        ey = self._axis_edges(ty, index_y, bins[1], rngs[1], pool_elements)
        gx, gy = ex, ey
        if ex.ndim != ey.ndim:  # per-pair edges on one axis only: the other axis' edges for every pair
            n = max(ex.shape[0] if ex.ndim == 2 else 0, ey.shape[0] if ey.ndim == 2 else 0)
            gx = ex if ex.ndim == 2 else np.broadcast_to(ex, (n, ex.size))
            gy = ey if ey.ndim == 2 else np.broadcast_to(ey, (n, ey.size))
        out = self.engine.store_histogram2d(tx, ty, gx, gy, index_x=index_x, index_y=index_y, pooled=pooled,
                                            pool_pairs=pool_elements, occupancy=occupancy)
        return [v.cpu().numpy() for v in out], ex, ey, tx.shape[0] * (tx.shape[1] if pooled else 1)

    def histogram2d(self, key_x, key_y=None, index_x=None, index_y=None, bins=10, range=None, pooled=True, pool_elements=False,
                    density=False):
        """np.histogram2d of the stored draws of pairs of elements, counted on the device (one read of the selected columns, no
        gather): (hist, xedges, yedges) as host arrays.  Pair k is element index_x[k] of store[key_x] against element index_y[k]
        of store[key_y] in the same (iteration, chain) state (key_y=None: two elements of store[key_x]; index None: all elements;
        in that order, repeats allowed; a 2-D entry ("log_post") counts as one element; both sides equally many).  hist is
        (n_pairs, nx, ny) pooled over chains and iterations, else (C, n_pairs, nx, ny); with pool_elements=True all pairs are
        counted into one map, (nx, ny) or (C, nx, ny) -- the joint map of a variable-size parameter, locations against
        coefficients.  int64 counts, or with density=True fp64, divided in np.histogramdd's order (by the x widths, by the y
        widths, then by the sum), so that the densities are bit-equal to numpy's.
        bins, as numpy takes them: an int, (nx, ny), one array of edges for both axes, or [xedges, yedges]; an axis' edges are
        (n + 1,) shared by all pairs or (n_pairs, n + 1) per pair (not with pool_elements) and are returned as given.  An int
        axis with range=[[xlo, xhi], [ylo, yhi]] gets the shared edges np.linspace(lo, hi, n + 1); without a range (or with None
        in its place) every coordinate gets the edges numpy would give it, np.linspace over its own non-NaN minimum and maximum
        over ALL chains (widened by 0.5 either way when they are equal, (0, 1) without a draw; an infinite draw raises ValueError
        as in numpy) -- edges (n_pairs, n + 1), or with pool_elements (n + 1,) over all selected elements.
        A pair with a NaN coordinate (the padding of variable-size parameters) is left out.  Under a sharded multi-GPU run these
        are the counts of this rank's chains only; counts of several ranks over the same edges can simply be added."""
        self._whole_store_on_device("histogram2d")
        (counts, _), ex, ey, _ = self._hist2d(key_x, key_y, index_x, index_y, bins, range, pooled, pool_elements, False)
        hist = counts
        if density:  # (np.histogramdd's order of operations)
            s = counts.sum(axis=(-2, -1), keepdims=True).astype(np.float64)
            hist = counts.astype(np.float64) / np.diff(ex, axis=-1)[..., :, None] / np.diff(ey, axis=-1)[..., None, :]
            hist /= s
        return hist, ex, ey

    def occupancy(self, key_x, key_y=None, index_x=None, index_y=None, bins=10, range=None, pooled=True):
        """In what share of the stored states a cell of the (x, y) grid holds at least one of the selected pairs: (prob, xedges,
        yedges), prob fp64 (nx, ny) over all chains and iterations, else (C, nx, ny) -- per state np.histogram2d(...)[0] > 0,
        averaged over the states, counted on the device.  What a variable-size parameter has in place of marginals: where its
        components (knots, sources) lie, location against coefficient or x against y.  Pairs, bins and range as `histogram2d`
        with pool_elements=True (the elements always share their edges); at most 256 pairs; NaN-padded components are left
        out.  Under a sharded multi-GPU run: this rank's chains only; prob times the states adds across ranks over the same
        edges."""
        self._whole_store_on_device("occupancy")
        (_, _, occupied), ex, ey, rows = self._hist2d(key_x, key_y, index_x, index_y, bins, range, pooled, True, True)
        return occupied / rows, ex, ey

    def kde2d(self, key_x, key_y=None, index_x=None, index_y=None, pooled=True, grid_len=128, bw="scott", bw_fct=1.0, extend=0.1,
              probs=(0.5, 0.9), pool_elements=False):
        """Joint kernel density estimate of pairs of elements -- the surface, the contour levels and the joint mode of
        az.plot_pair(kind="kde") / az.plot_kde(x, y, hdi_probs=...) -- from one joint histogram pass over the store and a
        full-covariance binned Gaussian convolution on the device (no gather): a dict of host arrays "grid_x" (.., nx), "grid_y"
        (.., ny) (the bin centres), "density" (.., nx, ny), "bw" (.., 3) = the kernel covariance (h_xx, h_xy, h_yy), "mode" (.., 2),
        "probs", "levels" (.., n_probs), "flag" (int32), "n" (pairs counted) and "outside" (pairs left out: a NaN coordinate).
        Pairs are selected as in `histogram2d`: pair k is element index_x[k] of store[key_x] against element index_y[k] of
        store[key_y] in the same state (key_y=None: two elements of store[key_x]); the leading shape is (n_pairs,) pooled over
        chains and iterations, else (C, n_pairs); with pool_elements=True all pairs go into one density, () or (C,) -- the joint
        density of a NaN-padded variable-size parameter, locations against coefficients.  grid_len: an int or (nx, ny), each
        8..256.  The grid of a coordinate spans its minimum and maximum over ALL chains (with pool_elements: over all selected
        elements), widened by extend (max - min) either way; a coordinate that never moved is widened by 0.5 as in `kde` and
        leaves its pair with flag 2 under a rule.  The pairs are counted into the cells with the edges np.linspace(a, b, n + 1)
        (counts equal np.histogram2d); the density is the binned convolution at the bin centres, without reflection at bounds.
        bw: "scott" or "silverman" (one rule in two dimensions, H = N^(-1/3) S, S the covariance of the binned pairs: what
        scipy.stats.gaussian_kde and ArviZ use); "marginal", the product kernel H = diag(h_x^2, h_y^2), h the coordinate's own
        `kde(..., bw="experimental")` bandwidth on the marginal counts times N^(1/30) (the 1-D rate N^(-1/5) moved to the 2-D
        rate N^(-1/6)) -- the choice for the bimodal joints of mixture-prior and reversible-jump models, which Scott's rule
        oversmooths; or a symmetric 2 x 2 matrix, or (n_pairs, 2, 2).  Every H is multiplied by bw_fct^2.  "levels": for every
        prob the density level whose region {density >= level} is the highest-density region holding that share of the mass
        (ArviZ's _find_hdi_contours); "mode": the grid point of the largest density, the lowest flat index of equal ones.
        flag: 0 ok; 1 ("marginal") the Sheather-Jones equation of a coordinate had no root and Silverman's bandwidth stands in; 2
        degenerate (fewer than two pairs, non-empty rows or columns, a singular or nearly singular H; density, bw, mode and levels
        are NaN).  An infinite draw raises ValueError as in `histogram2d`.  Under a sharded multi-GPU run this covers this rank's
        chains only; the estimate is a function of the counts and the grid alone, so counts of several ranks over the same edges
        can be added and handed to `engine.kde2d_binned`, which gives the estimate of all ranks' chains."""
        self._whole_store_on_device("kde2d")
        tx = self._store_3d(key_x)
        ty = tx if key_y is None else self._store_3d(key_y)
        try:
            nx, ny = grid_len
        except TypeError:
            nx = ny = grid_len
        nx, ny = grid_lengths((nx, ny), 256, "grid_len must be an integer or (nx, ny), each between 8 and 256", extend)
        # every argument is judged before the store is read
        if not (np.ndim(bw_fct) == 0 and bw_fct > 0 and np.isfinite(bw_fct)):
            raise ValueError("bw_fct must be a finite positive number")
        p = self.engine._kde2d_probs(probs)
        H = None
        if not isinstance(bw, str):
            H = np.asarray(bw, dtype=np.float64)
            n_sel = tx.shape[2] if index_x is None else len(index_x)
            if H.shape not in ((2, 2), (n_sel, 2, 2)) or (H.ndim == 3 and pool_elements):
                raise ValueError("bw must be a rule's name, a 2 x 2 matrix or, without pool_elements, an (n_pairs, 2, 2) array")
            if not np.array_equal(H[..., 0, 1], H[..., 1, 0]):
                raise ValueError("bw must be symmetric")
        elif bw not in ("scott", "silverman", "marginal"):
            raise ValueError('bw must be "scott", "silverman", "marginal" or a symmetric 2 x 2 matrix')

        ends, edges = [], []  # (a, b) and the edges of x, then of y: per pair, or one for all with pool_elements
        for t, index, n in ((tx, index_x, nx), (ty, index_y, ny)):
            a, b = widen(*auto_range(*self._minmax(t, index), pool=pool_elements), extend=extend)
            e = linspace_edges(a, b, n)
            ends += [a[0], b[0]] if pool_elements else [a, b]
            edges.append(e[0] if pool_elements else e)
        ex, ey = edges
        counts, outside = self.engine.store_histogram2d(tx, ty, ex, ey, index_x=index_x, index_y=index_y, pooled=pooled,
                                                        pool_pairs=pool_elements)
        lead = tuple(counts.shape[:-2])
        # (device tensors of the leading shape, () with pooled elements, which a host array would not keep)
        ends = [self.engine.to_device(np.array(np.broadcast_to(v, lead))).reshape(lead) for v in ends]
        rule, given, flag1 = bw, None, None
        if isinstance(bw, str) and bw == "marginal":
            n_pairs = counts.sum(dim=(-2, -1)).double()
            _, hx, _, fx = self.engine.kde_binned(counts.sum(dim=-1), ends[0], ends[1], rule="experimental")
            _, hy, _, fy = self.engine.kde_binned(counts.sum(dim=-2), ends[2], ends[3], rule="experimental")
            up = n_pairs ** (1.0 / 30.0)
            hx, hy = hx * up, hy * up
            given = self.engine.full(lead + (3,), 0.0)
            given[..., 0], given[..., 2] = hx * hx, hy * hy
            rule, flag1 = "given", ((fx == 1) | (fy == 1)).cpu().numpy()
        elif H is not None:
            rule = "given"
            given = np.array(np.broadcast_to(np.stack([H[..., 0, 0], H[..., 0, 1], H[..., 1, 1]], axis=-1), lead + (3,)))
        density, h, mode, level, _, flag = self.engine.kde2d_binned(counts, *ends, rule=rule, bw=given, bw_fct=bw_fct, probs=p)
        flag = flag.cpu().numpy()
        if flag1 is not None:
            flag = np.where((flag == 0) & flag1, np.int32(1), flag).astype(np.int32)
        gx, gy = 0.5 * (ex[..., :-1] + ex[..., 1:]), 0.5 * (ey[..., :-1] + ey[..., 1:])
        return {"grid_x": np.ascontiguousarray(np.broadcast_to(gx, lead + (nx,))),
                "grid_y": np.ascontiguousarray(np.broadcast_to(gy, lead + (ny,))), "density": density.cpu().numpy(),
                "bw": h.cpu().numpy(), "mode": mode.cpu().numpy(), "probs": p, "levels": level.cpu().numpy(), "flag": flag,
                "n": counts.sum(dim=(-2, -1)).cpu().numpy(), "outside": outside.sum(dim=-1).cpu().numpy()}

    def joint_mode(self, key_x, key_y=None, index_x=None, index_y=None, pooled=True, **kde2d_args):
        """Joint posterior mode of pairs of elements: the grid point of the largest joint kernel density estimate,
        kde2d(key_x, key_y, index_x, index_y, pooled, **kde2d_args)["mode"], (.., 2).  The pair of marginal `mode`s is no joint
        mode: a ridge or a second cluster moves a marginal's peak to where the joint density has none."""
        return self.kde2d(key_x, key_y, index_x, index_y, pooled, **kde2d_args)["mode"]

    def density_region(self, key_x, key_y=None, index_x=None, index_y=None, prob=0.9, pooled=True, **kde2d_args):
        """The highest-density region of pairs of elements that holds the share `prob` of the mass: (mask, grid_x, grid_y), mask
        bool (.., nx, ny) = density >= level of kde2d(..., probs=(prob,)) -- the cells inside az.plot_kde's contour at
        hdi_probs=[prob]; all False for a degenerate pair (flag 2)."""
        out = self.kde2d(key_x, key_y, index_x, index_y, pooled, probs=(prob,), **kde2d_args)
        with np.errstate(invalid="ignore"):
            mask = out["density"] >= out["levels"][..., 0, None, None]
        return mask, out["grid_x"], out["grid_y"]
