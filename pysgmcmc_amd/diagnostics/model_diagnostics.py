"""Diagnostics on models: the held-out score of a sampled BNN ensemble, on the host in numpy float64.

The reference's module of this name is a placeholder (``pysgmcmc/diagnostics/model_diagnostics.py``: "Add diagnostics on
models here (e.g. mean squared error of bnn etc.)"). These functions are the host statement of what K13
(``kernels.bnn_score``, ``include/sgmcmc_hip_score.h``) computes on the device: the same formulas, with numpy's own
summation. They take the ``(S, N)`` means of ``S`` sampled networks at ``N`` test rows, their ``(S,)`` log-variances and the
``(N,)`` targets, all in the units the networks work in.
"""
import numpy as np

__all__ = ["pointwise_log_likelihood", "log_pointwise_predictive_density", "waic", "ensemble_rmse"]

LOG_2PI = 1.8378770664093453


def pointwise_log_likelihood(means, log_var, y):
    """``(S, N)``: the Gaussian log density of ``y[r]`` under network ``s``, ``-0.5 * (log 2 pi + log_var_s) -
    (y[r] - means[s][r])^2 * 0.5 / (exp(log_var_s) + 1e-16)`` (the reference's density, ``bayesian_neural_network.py:368``)."""
    means = np.asarray(means, dtype=np.float64)
    log_var = np.asarray(log_var, dtype=np.float64).reshape(-1, 1)
    y = np.asarray(y, dtype=np.float64).reshape(1, -1)
    if means.ndim != 2 or log_var.shape[0] != means.shape[0] or y.shape[1] != means.shape[1]:
        raise ValueError("pointwise_log_likelihood: means (S, N), log_var (S,) and y (N,) do not fit: %s, %s, %s" % (
            means.shape, log_var.shape[:1], y.shape[1:]))
    a = -0.5 * (LOG_2PI + log_var)
    b = 0.5 / (np.exp(log_var) + 1e-16)
    d = y - means
    return a - (d * d) * b


def log_pointwise_predictive_density(loglik):
    """``(N,)``: ``log mean_s exp(loglik[s][r])``, shifted by the row's maximum so that it stays finite however small
    the densities are."""
    loglik = np.asarray(loglik, dtype=np.float64)
    top = loglik.max(axis=0)
    return (top + np.log(np.exp(loglik - top).sum(axis=0))) - np.log(float(loglik.shape[0]))


def waic(loglik):
    """``(lppd, p_waic, elpd_waic, row_lppd, row_pwaic)``: ``row_pwaic[r]`` is the sample variance over the networks of
    ``loglik[:, r]`` (0 for one network), ``lppd`` the MEAN of ``row_lppd``, ``p_waic`` the sum of ``row_pwaic`` and
    ``elpd_waic = sum(row_lppd) - p_waic`` (Watanabe 2010; Gelman, Hwang and Vehtari 2014, eq. 12)."""
    loglik = np.asarray(loglik, dtype=np.float64)
    S = loglik.shape[0]
    row_lppd = log_pointwise_predictive_density(loglik)
    if S > 1:
        row_pwaic = ((loglik - loglik.mean(axis=0)) ** 2).sum(axis=0) / (S - 1)
    else:
        row_pwaic = np.zeros(loglik.shape[1])
    p_waic = row_pwaic.sum()
    return row_lppd.mean(), p_waic, row_lppd.sum() - p_waic, row_lppd, row_pwaic


def ensemble_rmse(means, y):
    """Root mean squared error of the ensemble mean ``means.mean(axis=0)`` against ``y``."""
    means = np.asarray(means, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    return float(np.sqrt(((means.mean(axis=0) - y) ** 2).mean()))
