"""256 SGHMC chains of the reference's default BNN advanced together (one workgroup per chain), then the
Gelman-Rubin statistic and the effective sample size of EVERY parameter across ALL of them in one more launch -- the job
`pysgmcmc/diagnostics/sample_chains.py` and `sampler_diagnostics.py` do chain after chain and dimension after dimension."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import time

import numpy as np
import torch

from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains

rng = np.random.RandomState(1)
X = rng.rand(100, 1)
y = np.sinc(X * 10 - 5).sum(axis=1)
chains = FusedBNNChains.for_dataset(X, y, n_chains=256, burn_in_steps=1000, seed=7)
t0 = time.perf_counter()
chains.steps(5000)                                       # burn-in and mixing
# [256 chains, 50 snapshots, 5252 parameters], written by ONE launch of 5000 steps that keeps every 100th theta itself
snaps = chains.collect(50, every=100)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print("%d chains x %d steps in %.2f s = %.2f M samples/s"
      % (chains.n_chains, chains.n_iterations, dt, chains.n_chains * chains.n_iterations / dt / 1e6))
# R-hat and ESS of all 5252 parameters over all 256 chains, on the device. R-hat of single weights is a stern judge (the
# weight-space symmetries of an MLP keep chains apart that predict alike); the last parameter is the noise log-variance.
rhat, ess = chains.diagnose(snaps)
print("R-hat of %d parameters over %d chains: max %.3f, median %.3f; of the noise log-variance: %.3f"
      % (rhat.numel(), chains.n_chains, float(rhat.max()), float(rhat.median()), float(rhat[-1])))
print("effective sample size: median %d of %d kept samples" % (int(ess.median()), snaps.shape[0] * snaps.shape[1]))
