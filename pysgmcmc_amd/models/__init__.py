"""Models driven by the SG-MCMC update path. Exports what ``pysgmcmc/models/__init__.py:2-13`` exports except ``BaseModel`` (the
abstract model interface of ``models/base_model.py`` is outside the sampler path; its two normalisation
helpers live in ``bayesian_neural_network``), and, beyond the reference, ``posterior_predictive`` and ``heldout_score``: the
predictive moments of device traces, and their score against held-out targets, each in one device call."""
from pysgmcmc_amd.models.bayesian_neural_network import (
    BayesianNeuralNetwork,
    log_variance_prior_log_like,
    weight_prior_log_like,
)
from pysgmcmc_amd.models.predictive import posterior_predictive
from pysgmcmc_amd.models.scoring import HeldOutScore, heldout_score

__all__ = ("BayesianNeuralNetwork", "log_variance_prior_log_like", "weight_prior_log_like", "posterior_predictive",
           "heldout_score", "HeldOutScore")
