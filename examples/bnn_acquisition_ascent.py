"""The inner loop of Bayesian optimisation on the device: 16 SGHMC chains of the reference's default BNN on sinc, their kept
networks in a device trace, then a batch of candidate points climbs the lower confidence bound mean - kappa * sqrt(var) by
gradient ascent, every step one call of `chains.predictive_gradients` (the predictive moments AND their derivatives with
respect to the inputs). No parameter, prediction or gradient is copied to the host; only the two printed numbers are."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains

rng = np.random.RandomState(1)
X = rng.rand(100, 1)
y = np.sinc(X * 10 - 5).sum(axis=1)
chains = FusedBNNChains.for_dataset(X, y, n_chains=16, burn_in_steps=1000, seed=7)
chains.steps(5000)                                       # burn-in and mixing
trace = chains.collect(20, every=100)                    # [16 chains, 20 snapshots, 5252 parameters]

kappa, rate, floor = 1.0, 0.002, 1e-12        # sinc(10 x - 5) has slopes up to 13: a step moves a candidate by < 0.03
x = torch.linspace(0.05, 0.95, 32, device=trace.device, dtype=trace.dtype).reshape(-1, 1)     # 32 candidate points


def acquisition(x):
    """mean - kappa * sd at every candidate and its derivative with respect to the candidate, float64 on the device."""
    p = chains.predictive_gradients(x, trace)
    sd = torch.sqrt(p.var + floor)
    return p.mean - kappa * sd, p.dmean - kappa * p.dvar / (2.0 * sd)[:, None]


start, _ = acquisition(x)
for _ in range(40):
    _, slope = acquisition(x)
    x = (x + rate * slope.to(x.dtype)).clamp_(0.0, 1.0)
end, _ = acquisition(x)
print("lower confidence bound of %d candidates over %d networks: best %.4f -> %.4f, mean %.4f -> %.4f after 40 ascent steps"
      % (x.shape[0], trace.shape[0] * trace.shape[1], float(start.max()), float(end.max()), float(start.mean()),
         float(end.mean())))
