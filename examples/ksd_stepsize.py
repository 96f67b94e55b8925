"""Kernel Stein discrepancy against the stepsize: what R-hat and ESS do not see.

Four SGHMC chains of the reference's default BNN (3 x 50 tanh units) on sinc run at three stepsizes on the whole-step kernel.
R-hat and the effective sample size measure mixing; the kernel Stein discrepancy (`diagnostics.stein`, kernel K16) measures
the distance of the samples to the posterior itself, bias of the stationary distribution included, from the samples and the
posterior's score at each of them (`models.bnn_posterior_scores`, kernel K15, no autograd). One line per stepsize puts the
three next to each other; collect -> diagnose -> discrepancy runs without a parameter leaving the device. The last line is
the same number for the particles of a short SVGD run (`examples/svgd_bnn.py`): traces and particle sets are comparable by
it. With the defaults the chains, which start from different nets, are far from having met (R-hat well above 1): raise
--samples and --every for a comparison of stepsizes that means something.

    python examples/ksd_stepsize.py [--samples N] [--every K] [--svgd-steps S]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from pysgmcmc_amd import diagnostics, models
from pysgmcmc_amd.data_batches import Placeholder, generate_batches
from pysgmcmc_amd.samplers import SVGDSampler
from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule

device, dtype = torch.device("cuda:0"), torch.float32
parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
parser.add_argument("--samples", type=int, default=200, help="kept samples per chain (default 200)")
parser.add_argument("--every", type=int, default=50, help="steps between kept samples (default 50)")
parser.add_argument("--svgd-steps", type=int, default=1000, help="steps of the SVGD run (default 1000)")
args = parser.parse_args()
layer_sizes, n_chains = [1, 50, 50, 50, 1], 4

rng = np.random.RandomState(1)
X = rng.rand(100, 1)
y = np.sinc(X * 10 - 5).sum(axis=1)

print("%d chains x %d samples, every %d-th step; IMQ kernel, c = 1, beta = -1/2" % (n_chains, args.samples, args.every))
print("%10s %10s %10s %12s %12s" % ("stepsize", "max R-hat", "mean ESS", "KSD", "U-statistic"))
for stepsize in (1e-3, 1e-2, 5e-2):
    chains = FusedBNNChains.for_dataset(X, y, n_chains, seed=0, dtype=dtype, device=device, stepsize=stepsize,
                                        burn_in_steps=2000)
    chains.steps(3000)                                           # burn-in, nothing kept
    trace = chains.collect(args.samples, every=args.every)
    rhat, ess = chains.diagnose(trace)
    ksd = chains.stein_discrepancy(trace)
    print("%10g %10.3f %10.1f %12.5g %12.5g%s" % (
        stepsize, float(rhat[torch.isfinite(rhat)].max()), float(ess.double().mean()), float(ksd.ksd), float(ksd.u_statistic),
        "" if ksd.thinning == 1 else "   (every %d-th kept sample)" % ksd.thinning))

x_in, y_in = Placeholder(dtype=dtype, device=device), Placeholder(dtype=dtype, device=device)
cost = models.BNNParticleCost(layer_sizes, x_in, y_in, batch_size=20, n_examples=X.shape[0])
sampler = SVGDSampler(models.bnn_particles(64, 1, seed=0, dtype=dtype, device=device), cost,
                      batch_generator=generate_batches(X, y, x_in, y_in, batch_size=20, seed=1),
                      stepsize_schedule=ConstantStepsizeSchedule(5e-3), session=device, dtype=dtype)
sampler.sample_format = "view"
for _ in range(args.svgd_steps):
    next(sampler)
particles = sampler.particles.detach()                           # (64, P) at the sampler's row pitch: read in place
X_dev = torch.as_tensor(X, dtype=dtype, device=device)
y_dev = torch.as_tensor(y, dtype=dtype, device=device)
scores = models.bnn_posterior_scores(particles, layer_sizes, X_dev, y_dev)
ksd = diagnostics.kernel_stein_discrepancy(particles, scores)
print("SVGD, 64 particles, %d steps: KSD %.5g, U-statistic %.5g" % (args.svgd_steps, float(ksd.ksd), float(ksd.u_statistic)))
