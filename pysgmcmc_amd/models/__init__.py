"""Models driven by the SG-MCMC update path. Exports what ``pysgmcmc/models/__init__.py:2-13`` exports except ``BaseModel`` (the
abstract model interface of ``models/base_model.py`` is outside the sampler path; its two normalisation
helpers live in ``bayesian_neural_network``), and, beyond the reference, ``posterior_predictive``, ``heldout_score`` and
``predictive_gradients``: the predictive moments of device traces, their score against held-out targets, and their gradients
with respect to the inputs, each in one device call; and ``BNNParticleCost`` / ``bnn_particles``: the BNN cost on flat particles for
particle samplers, whose costs and parameter gradients come from one kernel launch; and ``bnn_posterior_scores``: the
posterior's score at every row of a trace from that kernel, for ``diagnostics.stein``; and ``loo_score``: PSIS-LOO of device
traces on their training set (K13's pointwise log densities through ``diagnostics.psis_loo``); and ``calibration_score``: PIT,
central-interval coverage and CRPS of device traces against held-out targets (K11's means through ``diagnostics.calibration``)."""
from pysgmcmc_amd.models.bayesian_neural_network import (
    BayesianNeuralNetwork,
    log_variance_prior_log_like,
    weight_prior_log_like,
)
from pysgmcmc_amd.models.particles import BNNParticleCost, bnn_particles
from pysgmcmc_amd.models.predictive import PredictiveGradients, posterior_predictive, predictive_gradients
from pysgmcmc_amd.models.scores import bnn_posterior_scores
from pysgmcmc_amd.models.scoring import HeldOutScore, calibration_score, heldout_score, loo_score

__all__ = ("BayesianNeuralNetwork", "log_variance_prior_log_like", "weight_prior_log_like", "posterior_predictive",
           "heldout_score", "HeldOutScore", "predictive_gradients", "PredictiveGradients", "BNNParticleCost",
           "bnn_particles", "bnn_posterior_scores", "loo_score", "calibration_score")
