"""Chains that agree in location and differ in scale: the classic Gelman-Rubin statistic passes them, the rank-normalised
split R-hat (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) does not.

16 relativistic SGHMC chains on the reference's three-mode Gaussian mixture (modes at -5, 0, 5; symmetric about 0), all
started at the middle mode. Eight run at the reference's stepsize and are thinned until their kept draws are nearly
independent draws from all three modes. Eight run at a stepsize so small that they have not left the neighbourhood of
their starting point when the run ends: the common SG-MCMC failure of a chain stuck at a small stepsize. All sixteen chains
have mean 0, so the classic R-hat, which compares means, sees nothing; the rank-normalised folded draws see the difference in
scale. Each group is ONE launch of the toy-chain kernel, each diagnosis a device call: K12 for the classic pair, K18 + K12
for the rank-normalised one.

    python examples/rank_diagnostics.py [fast stepsize] [slow stepsize] [kept samples] [keep every, fast] [keep every, slow]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from pysgmcmc_amd import diagnostics
from pysgmcmc_amd.diagnostics.objective_functions import gmm2_log_likelihood, to_negative_log_likelihood
from pysgmcmc_amd.samplers import RelativisticSGHMCSampler
from pysgmcmc_amd.samplers.builtin_target_chains import BuiltinTargetChains
from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule

args = sys.argv[1:]
eps_fast = float(args[0]) if len(args) > 0 else 1.51
eps_slow = float(args[1]) if len(args) > 1 else 0.0005
n_kept = int(args[2]) if len(args) > 2 else 500
keep_fast = int(args[3]) if len(args) > 3 else 2000
keep_slow = int(args[4]) if len(args) > 4 else 2
dev = torch.device("cuda:0")


def group(eps, seeds, keep_every):
    samplers = [RelativisticSGHMCSampler(params=[torch.tensor(0.0, dtype=torch.float32, device=dev)],
                                         cost_fun=to_negative_log_likelihood(gmm2_log_likelihood),
                                         stepsize_schedule=ConstantStepsizeSchedule(eps), session=dev, dtype=torch.float32,
                                         seed=seed) for seed in seeds]
    kept = BuiltinTargetChains(samplers).run(n_kept * keep_every, keep_every=keep_every)       # (kept, chain, 1)
    return kept.permute(1, 0, 2)


fast, slow = group(eps_fast, range(1, 9), keep_fast), group(eps_slow, range(9, 17), keep_slow)
trace = torch.cat([fast, slow]).contiguous()                 # (16 chains, n_kept, 1 parameter)
for name, g, eps, keep in (("fast", fast, eps_fast, keep_fast), ("slow", slow, eps_slow, keep_slow)):
    means = g[:, :, 0].mean(dim=1)
    print("8 %s chains at stepsize %g, every %d-th draw kept: chain means %+.3f .. %+.3f, pooled sd %.3f" % (
        name, eps, keep, float(means.min()), float(means.max()), float(g.std())))
rhat, ess = diagnostics.chain_diagnostics_all(trace)
d = diagnostics.rank_diagnostics_all(trace, details=True)
print("classic R-hat          %.4f   (ESS %d of %d draws)" % (float(rhat[0]), int(ess[0]), trace.shape[0] * trace.shape[1]))
print("rank-normalised R-hat  %.4f   (bulk %.4f, folded %.4f)" % (float(d.rhat_rank[0]), float(d.rhat_bulk[0]),
                                                                   float(d.rhat_folded[0])))
print("bulk ESS %d, tail ESS %d (lower tail %d, upper tail %d)" % (int(d.ess_bulk[0]), int(d.ess_tail[0]),
                                                                     int(d.ess_tail_lo[0]), int(d.ess_tail_hi[0])))
print("at the usual threshold of 1.01 the classic statistic %s and the rank-normalised one %s" % (
    "passes" if float(rhat[0]) < 1.01 else "fails", "fails" if float(d.rhat_rank[0]) > 1.01 else "passes"))
