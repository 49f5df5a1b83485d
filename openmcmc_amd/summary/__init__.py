"""Posterior summaries of the device store, which MCMC inherits: of one entry (marginal), several elements (joint), a response (predictive), the field at all elements at once (excursion)."""

from openmcmc_amd.summary.excursion import ExcursionSummaries
from openmcmc_amd.summary.joint import JointSummaries
from openmcmc_amd.summary.marginal import MarginalSummaries
from openmcmc_amd.summary.predictive import PredictiveSummaries


class StoreSummaries(MarginalSummaries, JointSummaries, PredictiveSummaries, ExcursionSummaries):
    """Every summary of the store, on the attributes base.SummaryBase lists."""
