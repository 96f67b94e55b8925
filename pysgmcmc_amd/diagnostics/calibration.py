"""Calibration of a kept ensemble's posterior predictive: PIT, central-interval coverage and CRPS; the host statement, in numpy.

The predictive of row ``r`` is the equal-weight mixture of the ``S`` Gaussians ``N(means[s][r], var[s])``. The probability
integral transform ``pit[r] = F_r(y[r])`` is uniform when the predictive is calibrated; the coverage of the central ``level``
interval is the share of rows with ``|pit - 1/2| <= level / 2``; the continuous ranked probability score rewards sharpness and
calibration together, in the units of ``y``, and has an exact closed form for a mixture of Gaussians (Grimit et al. 2006;
``crps_mixnorm`` of R's scoringRules) that holds a sum over all ``S^2`` pairs of draws.

``mixture_calibration_host`` states in numpy float64 what kernel K20 (``include/sgmcmc_hip_calib.h``) computes on the device,
operation by operation and with the same order of every sum, so the two differ only through ``erf``, ``erfc`` and ``exp``
(``torch.erf`` / ``torch.erfc`` on CPU float64 tensors here, numpy's ``exp``); the counts of ``summary`` are exact.

This module needs no GPU and no native library to import. ``calibration`` at its end is the device route.
"""
import collections

import numpy as np

from pysgmcmc_amd.diagnostics.psis import fixed_sum

__all__ = ["SQRT2", "INV_SQRTPI", "MAX_DRAWS", "MAX_LEVELS", "MAX_BINS", "abs_moment", "mixture_calibration_host",
           "summary_of", "Calibration", "calibration_of_summary", "calibration"]

SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
INV_SQRTPI = float.fromhex("0x1.20dd750429b6dp-1")
MAX_DRAWS = 4096                                          # SGMCMC_CALIB_MAX_DRAWS
MAX_LEVELS = 16                                           # SGMCMC_CALIB_MAX_LEVELS
MAX_BINS = 64                                             # SGMCMC_CALIB_MAX_BINS


def _erf(u):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64))).numpy()


def _erfc(u):
    import torch
    return torch.erfc(torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64))).numpy()


def abs_moment(d, c):
    """``A(d, c) = E|N(d, c^2)|``, as the header writes it: ``e = c SQRT2; u = d / e; e (u erf(u) + exp(-(u u)) INV_SQRTPI)``."""
    with np.errstate(all="ignore"):
        e = np.asarray(c, dtype=np.float64) * SQRT2
        u = np.asarray(d, dtype=np.float64) / e
        return e * (u * _erf(u) + np.exp(-(u * u)) * INV_SQRTPI)


def summary_of(pit, crps, levels=(), n_bins=0):
    """``summary`` of the header from ``pit`` and ``crps``: ``{the fixed-order sum of crps, the rows holding a NaN, the rows
    inside each central interval, the rows in each PIT bin}``, float64 ``(2 + len(levels) + n_bins,)``."""
    pit, crps = np.asarray(pit, dtype=np.float64), np.asarray(crps, dtype=np.float64)
    bad = np.isnan(pit) | np.isnan(crps)
    good = pit[~bad]
    out = [fixed_sum(crps) if crps.shape[0] else 0.0, float(bad.sum())]
    for level in levels:
        level = np.float64(level)
        out.append(float(((0.5 - 0.5 * level <= good) & (good <= 0.5 + 0.5 * level)).sum()))
    if n_bins > 0:
        b = np.minimum(n_bins - 1, np.floor(good * np.float64(n_bins)).astype(np.int64))
        out.extend(float((b == k).sum()) for k in range(n_bins))
    return np.array(out, dtype=np.float64)


def mixture_calibration_host(means, var, y, levels=(), n_bins=0):
    """PIT and CRPS of every target ``y[r]`` under the mixture of the ``S`` Gaussians ``N(means[s][r], var[s])``.

    ``means``: ``(S, n_rows)``; ``var``: ``(S,)``; ``y``: ``(n_rows,)``; ``levels``: numbers in (0, 1); ``n_bins``: 0 .. 64.
    Returns a dict of float64 arrays: ``pit`` and ``crps`` ``(n_rows,)`` and ``summary`` ``(2 + len(levels) + n_bins,)`` as
    the header states them. Non-finite inputs are not checked and propagate into their own row."""
    mu = np.asarray(means, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if mu.ndim != 2:
        raise ValueError("mixture_calibration: means must be (S, n_rows), got %s" % (tuple(mu.shape),))
    S, n_rows = mu.shape
    if S < 1 or S > MAX_DRAWS:
        raise ValueError("mixture_calibration: S = %d draws, must be 1 .. %d" % (S, MAX_DRAWS))
    levels = [float(v) for v in levels]
    if len(levels) > MAX_LEVELS:
        raise ValueError("mixture_calibration: n_levels = %d, must be 0 .. %d" % (len(levels), MAX_LEVELS))
    if n_bins < 0 or n_bins > MAX_BINS:
        raise ValueError("mixture_calibration: n_bins = %d, must be 0 .. %d" % (n_bins, MAX_BINS))
    for k, v in enumerate(levels):
        if not (0.0 < v < 1.0):
            raise ValueError("mixture_calibration: levels[%d] = %g, must lie in (0, 1)" % (k, v))
    if var.shape[0] != S or y.shape[0] != n_rows:
        raise ValueError("mixture_calibration: var must hold S = %d values and y n_rows = %d" % (S, n_rows))
    dS = np.float64(S)
    with np.errstate(all="ignore"):
        sd = np.sqrt(var)
        d = y[None, :] - mu                               # (S, n_rows)
        P = fixed_sum(0.5 * _erfc(-((d / sd[:, None]) / SQRT2)), axis=0)
        T = fixed_sum(abs_moment(d, sd[:, None]), axis=0)
        Dg = fixed_sum(np.sqrt(var + var) * (SQRT2 * INV_SQRTPI))
        # the pairs t < s in the order (s, t ascending); c is the same for every row
        si, ti = np.tril_indices(S, -1)
        c = np.sqrt(var[si] + var[ti])
        G = np.empty(n_rows)
        terms = np.zeros((S, S))
        for r in range(n_rows):
            col = np.ascontiguousarray(mu[:, r])
            terms[si, ti] = abs_moment(col[si] - col[ti], c)
            # np.cumsum adds one by one (np.sum does not); the zeros behind the diagonal change nothing
            g = np.cumsum(terms, axis=1)[:, -1]
            G[r] = fixed_sum(g)
        pit = P / dS
        crps = T / dS - ((G + G) + Dg) / (2.0 * dS * dS)
    return dict(pit=pit, crps=crps, summary=summary_of(pit, crps, levels, n_bins))


Calibration = collections.namedtuple("Calibration", ["pit", "crps", "mean_crps", "levels", "coverage", "calibration_error",
                                                     "pit_hist", "n_bad", "thinning"], defaults=(1,))
Calibration.__doc__ = """What :func:`calibration` returns, all device tensors; the scalars are 0-d float64.

``pit``, ``crps``: float64 ``(N,)``, the probability integral transform and the CRPS of every target. ``mean_crps``: the
fixed-order sum of ``crps`` divided by ``N``. ``levels``: the central levels asked for; ``coverage[k]``: the share of the rows
that hold no NaN whose ``pit`` lies in ``[1/2 - levels[k] / 2, 1/2 + levels[k] / 2]``; ``calibration_error``: the mean over the
levels of ``|coverage - levels|``. ``pit_hist``: the number of rows in each of the ``n_bins`` equal bins of ``[0, 1]`` (``pit =
1`` in the last). ``n_bad``: the number of rows whose ``pit`` or ``crps`` is NaN, which are in no interval and no bin.
``thinning``: the stride with which the draws were taken (1: all of them)."""


def calibration_of_summary(pit, crps, summary, levels):
    """A :class:`Calibration` from K20's outputs; ``xp`` ops only, so device tensors stay on the device (and numpy arrays
    give numpy fields: the host route of ``BayesianNeuralNetwork.calibration``)."""
    n_levels, N = len(levels), int(pit.shape[0])
    counts = summary[2:2 + n_levels]
    if isinstance(summary, np.ndarray):
        lv = np.asarray(levels, dtype=np.float64)
    else:
        import torch
        lv = torch.tensor([float(v) for v in levels], dtype=summary.dtype, device=summary.device)
    coverage = counts / (N - summary[1])
    return Calibration(pit=pit, crps=crps, mean_crps=summary[0] / N, levels=lv, coverage=coverage,
                       calibration_error=abs(coverage - lv).mean(), pit_hist=summary[2 + n_levels:], n_bad=summary[1])


def calibration(means, var, y, levels=(0.5, 0.8, 0.9, 0.95), n_bins=10):
    """Calibration of the ``(S, N)`` device tensor ``means`` with the float64 ``(S,)`` variances ``var`` against the targets
    ``y (N,)`` by kernel K20 (``kernels.mixture_calibration``): a :class:`Calibration` of device tensors. Nothing waits for
    the host; there is no CPU route (``mixture_calibration_host`` is the host statement)."""
    import torch

    from pysgmcmc_amd import kernels
    if not torch.is_tensor(means) or means.dim() != 2:
        raise ValueError("calibration: means must be an (S, N) device tensor")
    if int(means.shape[1]) == 0:
        raise ValueError("calibration: means holds no rows")
    levels = tuple(float(v) for v in levels)
    summary = torch.empty(2 + len(levels) + int(n_bins), dtype=torch.float64, device=means.device)
    pit, crps = kernels.mixture_calibration(means, var, y, levels, n_bins, summary=summary)
    return calibration_of_summary(pit, crps, summary, levels)
