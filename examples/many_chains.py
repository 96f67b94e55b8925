"""256 SGHMC chains of the reference's default BNN advanced together (one workgroup per chain), then the
Gelman-Rubin statistic and the effective sample size of EVERY parameter across ALL of them in one more launch -- the job
`pysgmcmc/diagnostics/sample_chains.py` and `sampler_diagnostics.py` do chain after chain and dimension after dimension --
and the score of the 12 800 kept networks on a held-out fifth of the data (lppd, WAIC, RMSE) in one more device call."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import time

import numpy as np
import torch

from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains

rng = np.random.RandomState(1)
X_all = rng.rand(125, 1)
y_all = np.sinc(X_all * 10 - 5).sum(axis=1)
X, y, X_held, y_held = X_all[:100], y_all[:100], X_all[100:], y_all[100:]      # a fifth is held out
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
# The held-out score of all 256 x 50 kept networks, from the device trace: K11's forward pass and float64 reductions in a
# fixed order, nothing copied to the host but the four numbers printed here. p_waic is the sum over the points of the
# variance of the log density between the networks: where the chains have not mixed (R-hat above) it is large.
score = chains.score(X_held, y_held, snaps)
print("held-out score of %d networks on %d points: lppd %.4f per point, elpd_waic %.3f (p_waic %.3f), RMSE %.4f"
      % (snaps.shape[0] * snaps.shape[1], len(y_held), float(score.lppd), float(score.elpd_waic), float(score.p_waic),
         float(score.rmse)))
