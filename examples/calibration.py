"""Can the error bars of a BNN ensemble be believed? PIT, central-interval coverage and CRPS of held-out points.

SGHMC chains of the default BNN on the reference's sinc problem are collected into a device trace; the trace, the held-out
inputs and their targets go through K11 (every network's output at every point) and K20 (the probability integral transform
of every target under the mixture of the networks' Gaussians, and the exact CRPS of that mixture). A calibrated predictive
has a flat PIT histogram and covers the central 50 / 80 / 90 / 95 % intervals that often; an overconfident one piles the PIT
at both ends and covers less. Nothing but the printed figures leaves the device.

    python examples/calibration.py [training points] [held-out points] [chains] [kept samples per chain] [keep every]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains

args = sys.argv[1:]
n_train = int(args[0]) if len(args) > 0 else 200
n_test = int(args[1]) if len(args) > 1 else 500
n_chains = int(args[2]) if len(args) > 2 else 4
n_kept = int(args[3]) if len(args) > 3 else 250
keep_every = int(args[4]) if len(args) > 4 else 40
dev = torch.device("cuda:0")

rng = np.random.RandomState(1)
X = rng.uniform(-3.0, 3.0, size=(n_train, 1))
y = np.sinc(X[:, 0]) + 0.05 * rng.randn(n_train)
X_test = rng.uniform(-3.0, 3.0, size=(n_test, 1))
y_test = np.sinc(X_test[:, 0]) + 0.05 * rng.randn(n_test)

chains = FusedBNNChains.for_dataset(X, y, n_chains, seed=2, device=dev, burn_in_steps=5000)
chains.steps(10000)                                                       # burn-in and some way beyond it
trace = chains.collect(n_kept, every=keep_every)
cal = chains.calibration(X_test, y_test, trace)
score = chains.score(X_test, y_test, trace)

print("%d held-out points, %d chains x %d draws (every %d-th of them)" % (n_test, n_chains, n_kept, cal.thinning))
print("  mean CRPS %.5f   RMSE of the ensemble mean %.5f   rows holding a NaN %d" % (
    float(cal.mean_crps), float(score.rmse), int(cal.n_bad)))
print("  central interval   coverage")
for level, cover in zip(cal.levels.tolist(), cal.coverage.tolist()):
    print("  %14.0f %%   %7.3f" % (100.0 * level, cover))
print("  calibration error (mean |coverage - level|) %.4f" % float(cal.calibration_error))
hist = cal.pit_hist.tolist()
print("  PIT histogram (%d bins; a calibrated predictive puts %.0f in each):" % (len(hist), n_test / float(len(hist))))
for b, count in enumerate(hist):
    print("  [%.1f, %.1f%s %5d %s" % (b / float(len(hist)), (b + 1) / float(len(hist)), "]" if b == len(hist) - 1 else ")",
                                     int(count), "#" * int(round(40.0 * count / max(hist)))))
