"""Held-out score of a small tanh-MLP BNN from device-resident traces, in one device call.

The reference leaves model diagnostics open (``pysgmcmc/diagnostics/model_diagnostics.py`` is a placeholder). Here the
samples stay where ``FusedBNNChains.collect`` / ``DeviceTrace.record`` left them: ``heldout_score`` hands the trace and the
held-out targets to K13 (``kernels.bnn_score``, ``include/sgmcmc_hip_score.h``), which runs K11's forward pass and reduces
the pointwise Gaussian log densities over the samples and the rows in float64 on the device. Nothing here waits for the
host. ``diagnostics.model_diagnostics`` states the same quantities in numpy on the host.
"""
import collections

import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd.models.predictive import _trace_arguments

__all__ = ["HeldOutScore", "heldout_score", "loo_score", "calibration_score"]

HeldOutScore = collections.namedtuple("HeldOutScore", ["lppd", "p_waic", "elpd_waic", "rmse", "row_lppd", "row_pwaic",
                                                       "ens_mean", "ens_var", "sample_loglik", "loglik"])
HeldOutScore.__doc__ = """What :func:`heldout_score` returns, all device tensors; the scalars are 0-d float64.

``lppd``: the mean over the rows of ``row_lppd``. ``p_waic``: the sum of ``row_pwaic``. ``elpd_waic``: ``sum(row_lppd) -
p_waic``. ``rmse``: of the ensemble mean against ``y``. ``row_lppd``, ``row_pwaic``, ``ens_mean``, ``ens_var``: float64
``(N,)``. ``sample_loglik``: float64 ``(S,)`` or None. ``loglik``: float64 ``(S, N)`` or None."""


def heldout_score(traces, X, y, layer_sizes, pointwise=False, per_sample=False):
    """Score of the networks sampled in ``traces`` against the held-out targets ``y`` at the rows of ``X``.

    ``traces``, ``X``, ``layer_sizes``: what :func:`~pysgmcmc_amd.models.posterior_predictive` accepts, refused alike. ``y``:
    ``(N,)`` device tensor of the traces' dtype, in the units the networks work in (normalised like the training targets).
    With ``S`` sampled networks, ``l[s][r]`` the Gaussian log density of ``y[r]`` under network ``s`` (mean: its output,
    variance: ``exp(log_var_s) + 1e-16``):

    * ``row_lppd[r] = log mean_s exp(l[s][r])``, evaluated with the row's maximum taken out; ``lppd`` is its mean over the rows
    * ``row_pwaic[r]`` = the sample variance over ``s`` of ``l[s][r]`` (0 for one sample); ``p_waic`` is its sum
    * ``elpd_waic = sum(row_lppd) - p_waic``; ``rmse = sqrt(mean((ens_mean - y)^2))``
    * ``pointwise=True`` also returns ``loglik`` ``(S, N)``; ``per_sample=True`` ``sample_loglik[s] = sum_r l[s][r]``

    Returns a :class:`HeldOutScore` of device tensors without host synchronisation. Allocates its outputs (and the ``(S, N)``
    means the reductions read) and nothing else."""
    chains, sizes, first, S, N = _trace_arguments("heldout_score", traces, X, layer_sizes, y)
    if N == 0:
        raise ValueError("heldout_score: X holds no rows, so there is nothing to score")
    dev, f64 = first.device, torch.float64
    means = torch.empty(S, N, dtype=first.dtype, device=dev)
    row_lppd, row_pwaic, ens_mean, ens_var = (torch.empty(N, dtype=f64, device=dev) for _ in range(4))
    loglik = torch.empty(S, N, dtype=f64, device=dev) if pointwise else None
    sample_loglik = torch.empty(S, dtype=f64, device=dev) if per_sample else None
    summary = torch.empty(3, dtype=f64, device=dev)
    kernels.bnn_score(chains, sizes, X, y, means, row_lppd, row_pwaic, ens_mean, ens_var, loglik=loglik,
                      sample_loglik=sample_loglik, summary=summary)
    return HeldOutScore(lppd=summary[0] / N, p_waic=summary[1], elpd_waic=summary[0] - summary[1],
                        rmse=torch.sqrt(summary[2] / N), row_lppd=row_lppd, row_pwaic=row_pwaic, ens_mean=ens_mean,
                        ens_var=ens_var, sample_loglik=sample_loglik, loglik=loglik)


def _strided_draws(traces, limit):
    """``(traces, k)``: ``traces`` as they are when they hold at most ``limit`` samples in all, else every ``k``-th sample of
    every chain, ``k`` the smallest that fits, as one matrix of rows (``FusedBNNChains.stein_discrepancy`` strides alike)."""
    from pysgmcmc_amd.diagnostics.device_trace import _chain_matrices
    if torch.is_tensor(traces) and traces.dim() == 3:
        mats = list(traces.unbind(0))
    else:
        mats = _chain_matrices(traces)
    m, n = len(mats), int(mats[0].shape[0])
    if m * n <= limit:
        return traces, 1
    if m > limit:
        raise ValueError("loo_score: %d chains, the limit is %d draws in all" % (m, limit))
    k = 1
    while m * len(range(0, n, k)) > limit:
        k += 1
    return torch.cat([x[::k] for x in mats], dim=0), k


def loo_score(traces, X, y, layer_sizes, r_eff=1.0, weights=False):
    """Pareto-smoothed importance-sampling leave-one-out of the networks sampled in ``traces`` on the observations
    ``(X, y)`` they were trained on: K13 (:func:`heldout_score` with ``pointwise=True``) leaves the pointwise log densities
    on the device and K19 (``diagnostics.psis_loo``) turns every observation's column into ``elpd_loo``, ``p_loo`` and the
    Pareto shape ``khat`` that says whether the estimate can be trusted (``khat > 0.7``: it cannot).

    ``traces``, ``X``, ``y``, ``layer_sizes``: what :func:`heldout_score` takes, particle matrices included. ``r_eff``: the
    relative efficiency of the draws (1 for independent ones). More than ``kernels.psis_max_draws()`` draws in all are strided
    evenly (every ``k``-th sample of every chain, ``k`` the smallest that fits); the result's ``thinning`` is that ``k``.
    Returns a ``diagnostics.PsisLoo`` of device tensors; nothing waits for the host."""
    from pysgmcmc_amd.diagnostics.psis import psis_loo
    traces, k = _strided_draws(traces, kernels.psis_max_draws())
    score = heldout_score(traces, X, y, layer_sizes, pointwise=True)
    return psis_loo(score.loglik, r_eff=r_eff, weights=weights)._replace(thinning=k)


def calibration_score(traces, X, y, layer_sizes, levels=(0.5, 0.8, 0.9, 0.95), n_bins=10):
    """Calibration of the networks sampled in ``traces`` against the held-out targets ``y`` at the rows of ``X``: K11's
    forward pass (``kernels.bnn_predict``) leaves every network's output on the device, the variance of network ``s``'s
    Gaussian is ``exp((double)log_var_s) + 1e-16`` from the last parameter of its sample row, and K20
    (``diagnostics.calibration``) turns every row's mixture into the probability integral transform of its target and the
    closed-form CRPS, and counts the coverage of the central ``levels`` and the PIT histogram of ``n_bins`` bins.

    ``traces``, ``X``, ``y``, ``layer_sizes``: what :func:`heldout_score` takes, particle matrices included. More than
    ``kernels.calib_max_draws()`` draws in all are strided evenly (every ``k``-th sample of every chain, ``k`` the smallest
    that fits); the result's ``thinning`` is that ``k``. Returns a ``diagnostics.Calibration`` of device tensors, in the units
    the networks work in; nothing waits for the host."""
    from pysgmcmc_amd.diagnostics.calibration import calibration
    traces, k = _strided_draws(traces, kernels.calib_max_draws())
    chains, sizes, first, S, N = _trace_arguments("calibration_score", traces, X, layer_sizes, y)
    if N == 0:
        raise ValueError("calibration_score: X holds no rows, so there is nothing to score")
    means = torch.empty(S, N, dtype=first.dtype, device=first.device)
    kernels.bnn_predict(chains, sizes, X, means)
    last = kernels._bnn_n_params(sizes) - 1
    mats = [chains] if torch.is_tensor(chains) else chains
    log_var = torch.cat([x[..., last].reshape(-1) for x in mats])
    var = torch.exp(log_var.double()) + 1e-16
    return calibration(means, var, y, levels=levels, n_bins=n_bins)._replace(thinning=k)
