class SummaryBase:
    """A summary reads these attributes of its object and no others, so `MCMC.__new__(MCMC)` with them set is all it needs: `engine`,
    `store` ({key: device tensor (n_iter, C[, size])}), `state`, `model` (or None), `n_iter`, `n_chains`, `store_ring`, `_n_dev` (the
    iteration slabs on the device) and `_derived` (the names of the entries that summaries made)."""

    def _whole_store_on_device(self, what):
        if self.store_ring and self._n_dev != self.n_iter:
            raise ValueError(f"{what} reduces the device store, and with store_ring the device holds the last {self._n_dev} of "
                             f"{self.n_iter} iterations only: reduce the drained store (host_store) instead")

    def _store_3d(self, key):
        t = self.store[key]
        return (t.unsqueeze(-1) if t.dim() == 2 else t.reshape(t.shape[0], t.shape[1], -1)).contiguous()

    def _minmax(self, t, index):
        return [v.cpu().numpy() for v in self.engine.store_minmax(t, index=index, pooled=True)]

    def _claim(self, name, what):
        """`what` is about to be kept under `name` (None: under none): an entry a summary made may be made again, one of the run not"""
        if name is not None and name in self.store and name not in self._derived:
            raise ValueError(f"{name!r} is a store entry of the run: choose another name for {what}")

    def _keep(self, name, tensor):
        self.store[name] = tensor
        self._derived.add(name)
