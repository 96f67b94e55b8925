"""Stein variational gradient descent on the reference's default BNN (3 x 50 tanh units) on sinc, without autograd: the costs
and the parameter gradients of all particles come from one launch of kernel K15 per step (`BNNParticleCost`), the update from
the SVGD kernels. The particle matrix `sampler.particles` is an (n, P) device matrix of flat parameter rows, which is what
`models.posterior_predictive` and `models.heldout_score` read: particles -> predict -> score never leaves the device, and no
parameter is copied to the host; only the printed numbers are.

    python examples/svgd_bnn.py [--particles N] [--steps K]

Up to 128 particles step on the register-resident SVGD kernels, 129 .. 1024 (e.g. ``--particles 512``) on the tiled ones."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from pysgmcmc_amd import models
from pysgmcmc_amd.data_batches import Placeholder, generate_batches
from pysgmcmc_amd.samplers import SVGDSampler
from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule

device, dtype = torch.device("cuda:0"), torch.float32
parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
parser.add_argument("--particles", type=int, default=16, help="number of particles, 1 .. 1024 (default 16)")
parser.add_argument("--steps", type=int, default=3000, help="number of SVGD steps (default 3000)")
args = parser.parse_args()
layer_sizes, n_particles, n_steps = [1, 50, 50, 50, 1], args.particles, args.steps

rng = np.random.RandomState(1)
X = rng.rand(100, 1)
y = np.sinc(X * 10 - 5).sum(axis=1)
X_test = torch.linspace(0.0, 1.0, 200, device=device, dtype=dtype).reshape(-1, 1)
y_test = torch.sinc(X_test * 10 - 5).sum(dim=1)

x_in, y_in = Placeholder(dtype=dtype, device=device), Placeholder(dtype=dtype, device=device)
cost = models.BNNParticleCost(layer_sizes, x_in, y_in, batch_size=20, n_examples=X.shape[0])
sampler = SVGDSampler(models.bnn_particles(n_particles, 1, seed=0, dtype=dtype, device=device), cost,
                      batch_generator=generate_batches(X, y, x_in, y_in, batch_size=20, seed=1),
                      stepsize_schedule=ConstantStepsizeSchedule(5e-3), session=device, dtype=dtype)
sampler.sample_format = "view"               # samples and costs stay on the device
sampler.use_hip_graph = True                 # K15 replayed from a graph, the SVGD update launched behind it


def heldout():
    particles = sampler.particles.detach()[None]         # (1 chain, n rows, P), row pitch 5312: read in place
    score = models.heldout_score(particles, X_test, y_test, layer_sizes)
    mean, var = models.posterior_predictive(particles, X_test, layer_sizes)
    return float(score.rmse), float(score.lppd), float(var.mean())


before = heldout()
for _ in range(n_steps):
    next(sampler)
after = heldout()
print("SVGD, %d particles of the %d-parameter net, %d steps on the kernel route (%s)" % (
    n_particles, sampler.particle_dim, n_steps, "K15" if sampler._particle_costs is not None else "autograd"))
print("held-out RMSE %.4f -> %.4f, log pointwise predictive density %.3f -> %.3f, mean predictive variance of the particles "
      "%.2e -> %.2e" % (before[0], after[0], before[1], after[1], before[2], after[2]))
