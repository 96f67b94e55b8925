"""Times ``models.heldout_score`` (K13, include/sgmcmc_hip_score.h) on a (256, 50, 5252) f32 trace of the default 3 x 50 net
at N = 37, 1 000 and 10 000 held-out rows, against the same quantities from what the project offered before K13:
``posterior_predictive(..., return_individual_predictions=True)`` followed by float64 torch expressions on the device.
Medians of 21 runs after a warm-up call, device events on the stream. The share of each launch is taken by difference
between calls that hold one launch more (forward alone; + rows; + per-sample sums; + totals), alternated in one loop.
The record is profiles/bnn_score.txt.

    python tools/gpu/bnn_score_measure.py [output file]
"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from pysgmcmc_amd import kernels
from pysgmcmc_amd.models import heldout_score, posterior_predictive
from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else open(os.devnull, "w")
def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True); out.write(line + "\n"); out.flush()

dev = torch.device("cuda:0")
sizes, P, m, n = [1, 50, 50, 50, 1], 5252, 256, 50
S, dt, f64 = m * n, torch.float32, torch.float64
say("device", torch.cuda.get_device_name(0), "torch", torch.__version__)
say("trace (%d, %d, %d) %s = %d sampled networks" % (m, n, P, dt, S))

g = torch.Generator(device="cpu").manual_seed(7)
base = torch.cat([p.reshape(-1) for p in init_mlp_params(1, seed=5)])
trace = base[None, None, :] + 0.1 * torch.randn(m, n, P, generator=g, dtype=f64)
trace[:, :, -1] = np.log(1e-2) + 0.5 * torch.rand(m, n, generator=g, dtype=f64)
trace = trace.to(dt).to(dev)

def timed(fns, runs=21):
    """Median, min, max in ms of every function of ``fns``, alternated run by run."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize(); ts[k].append(a.elapsed_time(b))
    return [(statistics.median(t), min(t), max(t)) for t in ts]

def torch_score(X, y):
    """The same quantities from the posterior predictive's (S, N) matrix by float64 torch expressions on the device."""
    f, noise = posterior_predictive(trace, X, sizes, return_individual_predictions=True)
    lv = trace[:, :, -1].reshape(-1, 1).double()
    d = y.double()[None, :] - f.double()
    ll = -0.5 * (1.8378770664093453 + lv) - d * d * (0.5 / (torch.exp(lv) + 1e-16))
    row_lppd = torch.logsumexp(ll, dim=0) - float(np.log(S))
    row_pwaic = ll.var(dim=0, unbiased=True)
    ens_mean = f.double().mean(dim=0)
    rmse = torch.sqrt(((ens_mean - y.double()) ** 2).mean())
    return row_lppd.mean(), row_pwaic.sum(), row_lppd.sum() - row_pwaic.sum(), rmse, row_lppd, row_pwaic

for N in (37, 1000, 10000):
    rng = np.random.RandomState(N)
    X = torch.as_tensor(rng.uniform(-1, 1, size=(N, 1)), dtype=dt, device=dev)
    y = torch.as_tensor(np.sinc(X.cpu().numpy()[:, 0]) + 0.05 * rng.randn(N), dtype=dt, device=dev)
    means = torch.empty(S, N, dtype=dt, device=dev)
    rows = [torch.empty(N, dtype=f64, device=dev) for _ in range(4)]
    sl, sm = torch.empty(S, dtype=f64, device=dev), torch.empty(3, dtype=f64, device=dev)
    ll = torch.empty(S, N, dtype=f64, device=dev)
    say("---- N = %d held-out rows (means %.1f MB, loglik %.1f MB)" % (N, S * N * 4 / 1e6, S * N * 8 / 1e6))
    names = ["forward alone (kernels.bnn_predict, means only)", "forward + rows (kernels.bnn_score, no optional output)",
             "forward + rows + totals (summary)", "forward + rows + per-sample sums + totals",
             "forward + rows storing loglik + per-sample sums + totals",
             "models.heldout_score (allocations, forward + rows + totals, torch scalars)",
             "posterior_predictive(individual) + float64 torch expressions"]
    fns = [lambda: kernels.bnn_predict(trace, sizes, X, means),
           lambda: kernels.bnn_score(trace, sizes, X, y, means, *rows),
           lambda: kernels.bnn_score(trace, sizes, X, y, means, *rows, summary=sm),
           lambda: kernels.bnn_score(trace, sizes, X, y, means, *rows, sample_loglik=sl, summary=sm),
           lambda: kernels.bnn_score(trace, sizes, X, y, means, *rows, loglik=ll, sample_loglik=sl, summary=sm),
           lambda: heldout_score(trace, X, y, sizes),
           lambda: torch_score(X, y)]
    res = timed(fns)
    for name, (med, lo, hi) in zip(names, res):
        say("%-78s median %8.3f ms  [%.3f .. %.3f]" % (name, med, lo, hi))
    fwd, row, tot, smp = res[0][0], res[1][0] - res[0][0], res[2][0] - res[1][0], res[3][0] - res[2][0]
    whole = res[3][0]
    say("shares of the four-launch call by difference: forward %.1f %%, rows %.1f %%, per-sample sums %.1f %%, totals %.1f %%" % (
        100 * fwd / whole, 100 * row / whole, 100 * smp / whole, 100 * tot / whole))
    got, want = heldout_score(trace, X, y, sizes), torch_score(X, y)
    say("heldout_score against the torch expressions: lppd %.9f / %.9f, p_waic %.6f / %.6f, rmse %.9f / %.9f, "
        "max |row_lppd difference| %.3e" % (float(got.lppd), float(want[0]), float(got.p_waic), float(want[1]),
                                            float(got.rmse), float(want[3]), float((got.row_lppd - want[4]).abs().max())))
    del means, ll
    torch.cuda.empty_cache()
say("done")
