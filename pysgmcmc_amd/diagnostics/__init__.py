"""Diagnostics: toy targets, trace containers and cross-chain statistics (same exports as
``pysgmcmc/diagnostics/__init__.py:1-9``), plus the device-resident trace, the all-parameter effective sample size, the
all-parameter R-hat and ESS of many chains, their rank-normalised forms (``rank``), the kernel Stein discrepancy of traces
and particle sets and greedy Stein thinning by it (``stein``), Pareto-smoothed importance-sampling leave-one-out of
pointwise log densities (``psis``), and the calibration of a kept ensemble's predictive: PIT, coverage and CRPS
(``calibration``, the device route; ``mixture_calibration_host``, the numpy statement)."""
from pysgmcmc_amd.diagnostics import psis, rank, stein
from pysgmcmc_amd.diagnostics.calibration import Calibration, calibration, mixture_calibration_host
from pysgmcmc_amd.diagnostics.device_trace import (DeviceTrace, chain_diagnostics_all, effective_n_all,
                                                    effective_sample_sizes_of, gelman_rubin_all, rank_diagnostics_all)
from pysgmcmc_amd.diagnostics.psis import PsisLoo, gpd_fit, psis_loo, psis_loo_host
from pysgmcmc_amd.diagnostics.rank import RankDiagnostics, rank_diagnostics, rank_normalized_chains
from pysgmcmc_amd.diagnostics.sample_chains import PYSGMCMCTrace, pymc3_multitrace
from pysgmcmc_amd.diagnostics.sampler_diagnostics import effective_sample_sizes, gelman_rubin
from pysgmcmc_amd.diagnostics.stein import (SteinDiscrepancy, SteinThinning, kernel_stein_discrepancy, stein_kernel_matrix,
                                             stein_thinning, stein_thinning_indices)

__all__ = ("PYSGMCMCTrace", "pymc3_multitrace", "effective_sample_sizes", "gelman_rubin",
           "DeviceTrace", "effective_n_all", "effective_sample_sizes_of", "chain_diagnostics_all", "gelman_rubin_all",
           "rank", "rank_diagnostics_all", "rank_diagnostics", "rank_normalized_chains", "RankDiagnostics",
           "stein", "SteinDiscrepancy", "kernel_stein_discrepancy", "stein_kernel_matrix",
           "SteinThinning", "stein_thinning", "stein_thinning_indices",
           "psis", "PsisLoo", "psis_loo", "psis_loo_host", "gpd_fit",
           "Calibration", "calibration", "mixture_calibration_host")
