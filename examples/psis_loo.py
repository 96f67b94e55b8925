"""WAIC and PSIS-LOO side by side on a BNN that fits a few hundred points, once on clean data and once with a planted outlier.

At the defaults the chains are short and still drifting, so every observation's log density varies strongly over the draws:
p_waic and p_loo come out far above the number of points and khat says of EVERY row that these draws do not support a
leave-one-out estimate (the diagnosis WAIC cannot give). The planted outlier stands out all the same: its khat is an order
of magnitude above the others', and WAIC's figure for it is fifty times LOO's.

Two groups of SGHMC chains on the reference's sinc problem; the second group's data set has one target moved far off the
curve. Each group is collected, scored (K13: lppd and the WAIC penalty) and cross-validated (K13's pointwise log densities
through K19: elpd_loo, p_loo and the Pareto shape khat of every observation) on the device. An influential observation is
exactly where WAIC fails silently; PSIS-LOO says so itself: the rows whose khat exceeds 0.7 are the ones whose leave-one-out
density cannot be trusted from these draws (Vehtari, Gelman, Gabry 2017).

    python examples/psis_loo.py [points] [chains] [kept samples per chain] [keep every] [outlier size]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains

args = sys.argv[1:]
n_points = int(args[0]) if len(args) > 0 else 200
n_chains = int(args[1]) if len(args) > 1 else 2
n_kept = int(args[2]) if len(args) > 2 else 250
keep_every = int(args[3]) if len(args) > 3 else 40
outlier = float(args[4]) if len(args) > 4 else 3.0
dev = torch.device("cuda:0")

rng = np.random.RandomState(1)
X = rng.uniform(-3.0, 3.0, size=(n_points, 1))
y_clean = np.sinc(X[:, 0]) + 0.05 * rng.randn(n_points)
y_planted = y_clean.copy()
y_planted[0] += outlier

for name, y in (("clean", y_clean), ("one planted outlier (row 0, moved by %+g)" % outlier, y_planted)):
    chains = FusedBNNChains.for_dataset(X, y, n_chains, seed=2, device=dev, burn_in_steps=5000)
    chains.steps(10000)                                                   # burn-in and some way beyond it
    trace = chains.collect(n_kept, every=keep_every)
    waic = chains.score(X, y, trace)
    loo = chains.loo(X, y, trace)
    khat = loo.khat.cpu().numpy()
    print("%s: %d points, %d chains x %d draws" % (name, n_points, n_chains, n_kept))
    print("  lppd %9.3f   p_waic %7.3f   elpd_waic %9.3f" % (float(waic.lppd) * n_points, float(waic.p_waic),
                                                            float(waic.elpd_waic)))
    print("  lppd %9.3f   p_loo  %7.3f   elpd_loo  %9.3f   (se %.3f)" % (float(loo.lppd), float(loo.p_loo),
                                                                         float(loo.elpd_loo), float(loo.se)))
    bad = np.flatnonzero(khat > 0.7)
    print("  khat: largest %.3f, %d of %d rows above 0.7%s" % (khat.max(), int(loo.n_bad), n_points,
                                                              ": rows %s%s" % (", ".join(str(r) for r in bad[:12]),
                                                                               " ..." if bad.size > 12 else "")
                                                              if bad.size else ""))
    for r in bad[:12]:
        print("    row %d: x = %+.3f, y = %+.3f, khat = %.3f, elpd_loo = %.3f against WAIC's %.3f" % (
            r, X[r, 0], y[r], khat[r], float(loo.row_elpd[r]), float(waic.row_lppd[r] - waic.row_pwaic[r])))
