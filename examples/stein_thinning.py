"""A small ensemble by Stein thinning instead of every k-th sample.

Four SGHMC chains of the reference's default BNN (3 x 50 tanh units) on sinc run on the whole-step kernel and keep a device
trace. An acquisition loop, or anything that predicts at many points, wants a handful of nets, not the whole trace. The usual
answer is every k-th row; greedy Stein thinning (`diagnostics.stein_thinning`, kernel K17) instead picks the rows that keep
the kernel Stein discrepancy of the picked set smallest, from the Stein kernel matrix K16 has computed anyway. The flow is
collect -> stein_discrepancy -> thin to 16 nets -> predict with the thinned nets and with every k-th net; no parameter leaves
the device along it. Printed: the KSD of the trace, of the thinned and of the strided ensemble, and both RMSEs on held-out
points.

    python examples/stein_thinning.py [--samples N] [--every K] [--nets M]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains

device, dtype = torch.device("cuda:0"), torch.float32
parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
parser.add_argument("--samples", type=int, default=200, help="kept samples per chain (default 200)")
parser.add_argument("--every", type=int, default=50, help="steps between kept samples (default 50)")
parser.add_argument("--nets", type=int, default=16, help="size of the ensemble (default 16)")
args = parser.parse_args()
n_chains = 4

rng = np.random.RandomState(1)
X = rng.rand(100, 1)
y = np.sinc(X * 10 - 5).sum(axis=1)
X_test = np.linspace(0.0, 1.0, 200)[:, None]
y_test = torch.as_tensor(np.sinc(X_test * 10 - 5).sum(axis=1), dtype=torch.float64, device=device)

chains = FusedBNNChains.for_dataset(X, y, n_chains, seed=0, dtype=dtype, device=device, stepsize=1e-2, burn_in_steps=2000)
chains.steps(3000)                                               # burn-in, nothing kept
trace = chains.collect(args.samples, every=args.every)
whole = chains.stein_discrepancy(trace)
ensemble, thinned = chains.thin(trace, args.nets)

rows = trace.reshape(-1, trace.shape[2])
stride = rows.shape[0] // args.nets
strided = rows[::stride][:args.nets]
ksd_strided = chains.stein_discrepancy(strided)


def rmse(nets):
    mean, _ = chains.predict(X_test, nets)
    return float(torch.sqrt(torch.mean((mean.double().reshape(-1) - y_test) ** 2)))


print("%d chains x %d samples, every %d-th step; IMQ kernel, c = 1, beta = -1/2" % (n_chains, args.samples, args.every))
print("%-34s %12s %12s" % ("", "KSD", "test RMSE"))
print("%-34s %12.5g %12.5g" % ("the whole trace (%d nets)" % rows.shape[0], float(whole.ksd), rmse(trace)))
print("%-34s %12.5g %12.5g" % ("Stein thinning, %d nets" % args.nets, float(thinned.ksd_path[-1]), rmse(ensemble)))
print("%-34s %12.5g %12.5g" % ("every %d-th row, %d nets" % (stride, args.nets), float(ksd_strided.ksd), rmse(strided)))
print("picked rows (chain, sample): %s" % ", ".join(
    "(%d, %d)" % divmod(int(i), args.samples) for i in thinned.indices.tolist()))
