"""Diagnostics: toy targets, trace containers and cross-chain statistics (same exports as
``pysgmcmc/diagnostics/__init__.py:1-9``), plus the device-resident trace and the all-parameter effective sample size."""
from pysgmcmc_amd.diagnostics.device_trace import DeviceTrace, effective_n_all, effective_sample_sizes_of
from pysgmcmc_amd.diagnostics.sample_chains import PYSGMCMCTrace, pymc3_multitrace
from pysgmcmc_amd.diagnostics.sampler_diagnostics import effective_sample_sizes, gelman_rubin

__all__ = ("PYSGMCMCTrace", "pymc3_multitrace", "effective_sample_sizes", "gelman_rubin",
           "DeviceTrace", "effective_n_all", "effective_sample_sizes_of")
