"""The methods that moved out of MCMC (to openmcmc_amd/summary) and out of Engine (to openmcmc_amd/engine_store.py) are still attributes
of MCMC and of Engine, with the signatures they had before the move and a docstring wherever they had one: the two tables below were
printed from the classes before the move (name, str(inspect.signature), whether inspect.getdoc was non-empty).  No Engine is created."""

import inspect

import pytest

MCMC = [
    ('_whole_store_on_device', '(self, what)', False),
    ('summary', '(self, key, pooled=True)', True),
    ('quantiles', '(self, key, q, pooled=True, omit_nan=True)', True),
    ('diagnostics', '(self, key)', True),
    ('rank_diagnostics', '(self, key, index=None)', True),
    ('_selected_columns', '(self, key, index)', True),
    ('_column_chunks', '(self, t, cols, n)', True),
    ('_mean_sd_ess', '(self, key, index, squared)', True),
    ('_probs', '(prob, method)', True),
    ('ess', "(self, key, method='bulk', prob=None, index=None)", True),
    ('mcse', "(self, key, method='mean', prob=None, index=None)", True),
    ('summarize', '(self, key, index=None, hdi_prob=0.94)', True),
    ('ranks', '(self, key, index=None, split=False)', True),
    ('hdi', '(self, key, prob=0.94, index=None, pooled=True, omit_nan=True)', True),
    ('derive', '(self, key, reduce, index=None, weights=None, threshold=None, center=None, scale=None, omit_nan=True, name=None)', True),
    ('project', '(self, key, matrix, index=None, offset=None, base=None, omit_nan=True, name=None, noise_precision=None, replicate=0)', True),
    ('_predictive_precision', "(self, dist, m, what='posterior_predictive')", True),
    ('_normal_response', '(self, response, what)', True),
    ('posterior_predictive', '(self, response, name=None, replicate=0, noise=True)', True),
    ('_pointwise_chunks', '(self, response, what)', True),
    ('log_likelihood', '(self, response, name=None)', True),
    ('waic', '(self, response, pointwise=False)', True),
    ('loo', '(self, response, pointwise=False, reff=1.0)', True),
    ('_loo_tail_max', '(self, reff, m)', True),
    ('_loo_expect', '(self, what, response, reff, f, want, values=None, index=None, threshold=None, lw=False)', True),
    ('loo_expectation', '(self, response, values, index=None, threshold=None, reff=1.0)', True),
    ('loo_predictive', '(self, response, reff=1.0)', True),
    ('loo_pit', '(self, response, y_rep=None, reff=1.0)', True),
    ('loo_weights', '(self, response, name=None, reff=1.0)', True),
    ('simultaneous_band', '(self, key, prob=0.95, index=None)', True),
    ('autocorrelation', '(self, key, max_lag=None, index=None, pooled=True, normalize=True)', True),
    ('_store_3d', '(self, key)', False),
    ('covariance', '(self, key, other=None, index=None, other_index=None, pooled=True, correlation=False)', True),
    ('correlation', '(self, key, other=None, index=None, other_index=None, pooled=True)', True),
    ('_allocation_labels', '(self, key, n_labels)', True),
    ('_coallocation', '(self, key, n_labels, index, pooled, per_label)', False),
    ('coallocation', '(self, key, n_labels=None, index=None, pooled=True, per_label=False)', True),
    ('partition', '(self, key, n_labels=None, index=None, pooled=True)', True),
    ('histogram', '(self, key, bins=10, range=None, index=None, pooled=True, density=False)', True),
    ('kde', "(self, key, index=None, pooled=True, grid_len=512, bw='experimental', bw_fct=1.0, extend=0.1, bounds=None)", True),
    ('mode', '(self, key, index=None, pooled=True, **kde_args)', True),
    ('exceedance', '(self, key, thresholds, index=None, pooled=True)', True),
    ('_axis_edges', '(self, t, index, bins, rng, pool_elements)', True),
    ('_hist2d', '(self, key_x, key_y, index_x, index_y, bins, range, pooled, pool_elements, occupancy)', False),
    ('histogram2d', '(self, key_x, key_y=None, index_x=None, index_y=None, bins=10, range=None, pooled=True, pool_elements=False, density=False)', True),
    ('occupancy', '(self, key_x, key_y=None, index_x=None, index_y=None, bins=10, range=None, pooled=True)', True),
    ('kde2d', "(self, key_x, key_y=None, index_x=None, index_y=None, pooled=True, grid_len=128, bw='scott', bw_fct=1.0, extend=0.1, probs=(0.5, 0.9), pool_elements=False)", True),
    ('joint_mode', '(self, key_x, key_y=None, index_x=None, index_y=None, pooled=True, **kde2d_args)', True),
    ('density_region', '(self, key_x, key_y=None, index_x=None, index_y=None, prob=0.9, pooled=True, **kde2d_args)', True),
]
ENGINE = [
    ('_store_shape', '(self, store)', True),
    ('store_moments', '(self, store, pooled=False)', True),
    ('store_quantiles', '(self, store, q, pooled=False, omit_nan=True)', True),
    ('store_rhat_ess', '(self, store)', True),
    ('_check_text', '(st)', True),
    ('_int64', '(self, v, what, empty_ok=True)', True),
    ('_f64', '(self, v)', True),
    ('_store_index', '(self, index, size)', True),
    ('_selection', '(self, store, index)', True),
    ('store_cov', '(self, store_a, store_b=None, index_a=None, index_b=None, pooled=True, correlation=False)', True),
    ('hist_tile', '(n_bins, per_element=False)', True),
    ('hist_layout', '(n_bins, per_element=False)', True),
    ('store_minmax', '(self, store, index=None, pooled=True)', True),
    ('store_histogram', '(self, store, edges, index=None, pooled=True)', True),
    ('kde_layout', '(n_bins)', True),
    ('kde_binned', "(self, counts, lo, hi, rule='experimental', bw=None, bw_fct=1.0, reflect=(False, False))", True),
    ('kde2d_layout', '(nx, ny)', True),
    ('kde2d_binned', "(self, counts, lo_x, hi_x, lo_y, hi_y, rule='scott', bw=None, bw_fct=1.0, probs=None)", True),
    ('hist2d_tile', '(nx, ny, per_pair=False, pool_pairs=False)', True),
    ('hist2d_layout', '(nx, ny, per_pair=False, pool_pairs=False)', True),
    ('store_histogram2d', '(self, store_x, store_y, edges_x, edges_y, index_x=None, index_y=None, pooled=True, pool_pairs=False, occupancy=False)', True),
    ('_n_labels', '(n_labels)', False),
    ('store_coalloc', '(self, store, n_labels, index=None, pooled=True, per_label=False)', True),
    ('store_partition_score', '(self, store, n_labels, counts, index=None, pooled=True)', True),
    ('rank_schedule', '(n_draws, tile=0)', True),
    ('store_ranks', '(self, store, index=None, split=False)', True),
    ('store_rank_diagnostics', '(self, store, index=None)', True),
    ('store_ess_indicator', '(self, store, prob_lo, prob_hi, index=None, counts=0, algo=0)', True),
    ('store_order_stats', '(self, store, pos, index=None, split=True)', True),
    ('store_hdi', '(self, store, prob, index=None, pooled=True, omit_nan=True)', True),
    ('_reduce_vector', '(self, v, n, what)', True),
    ('store_reduce', '(self, store, op, index=None, omit_nan=True, a=None, b=None)', True),
    ('store_autocorr', '(self, store, max_lag, index=None, pooled=True, normalize=True)', True),
    ('store_project', '(self, store, W, index=None, offset=None, base=None, omit_nan=True, prec=None, z=None, replicate=0, out=None)', True),
    ('_loo_inputs', '(self, store, index, y, prec)', True),
    ('_loglik_inputs', '(self, store, y, prec, index)', True),
    ('store_loglik', '(self, store, y, prec, index=None, lse=True, mean=True, var=True, ll=False)', True),
    ('store_psis', '(self, store, tail_max, index=None, y=None, prec=None)', True),
    ('_tail_max', '(self, tail_max, n)', True),
    ('store_loo_expect', "(self, store, tail_max, index=None, y=None, prec=None, f='entry', values=None, values_index=None, threshold=None, want=('mean', 'var', 'ess', 'k', 'tail'), lw=False)", True),
    ('store_thin', '(self, store, every, first=0)', True),
]


def classes():
    from openmcmc_amd.engine import Engine
    from openmcmc_amd.mcmc import MCMC

    return {"MCMC": MCMC, "Engine": Engine}


@pytest.mark.parametrize("owner, name, signature, documented",
                         [("MCMC",) + row for row in MCMC] + [("Engine",) + row for row in ENGINE])
def test_the_method_is_where_it_was(owner, name, signature, documented):
    fn = getattr(classes()[owner], name)
    assert str(inspect.signature(fn)) == signature
    assert fn.__name__ == name
    if documented:
        assert inspect.getdoc(fn)


def test_tables_and_constants_are_where_they_were():
    c = classes()
    assert c["Engine"].KDE_RULES == {"given": 0, "scott": 1, "silverman": 2, "isj": 3, "experimental": 4}
    assert c["Engine"].KDE2D_RULES == {"given": 0, "scott": 1, "silverman": 1}
    assert c["Engine"].REDUCE_OPS == {"sum": 0, "min": 1, "max": 2, "argmin": 3, "argmax": 4, "count_above": 5, "supnorm": 6}
    assert c["MCMC"].pointwise_work_bytes == 1 << 30


def test_mcmc_no_longer_defines_a_summary_and_engine_no_store_wrapper():
    c = classes()
    assert not {name for name, _, _ in MCMC} & set(vars(c["MCMC"]))
    assert not {name for name, _, _ in ENGINE} & set(vars(c["Engine"]))


def test_the_summaries_are_a_plain_class():
    import dataclasses

    from openmcmc_amd.summary import StoreSummaries

    assert issubclass(classes()["MCMC"], StoreSummaries)
    for cls in StoreSummaries.__mro__[:-1]:
        assert not dataclasses.is_dataclass(cls) and "__init__" not in vars(cls) and not vars(cls).get("__annotations__")
    fields = [f.name for f in dataclasses.fields(classes()["MCMC"])]
    assert fields == ["state", "samplers", "model", "n_burn", "n_iter", "n_thin", "n_chains", "seed", "device", "chain_id_offset", "fuse",
                      "engine", "store_ring", "sink", "store"]


def test_every_recorded_write_still_wraps_a_method_of_its_name():
    from openmcmc_amd import engine

    for name in engine._WRITES:
        assert getattr(engine.Engine, name).__name__ == name
        assert name in vars(engine.Engine)  # (the recording wrapper is set on Engine itself)
