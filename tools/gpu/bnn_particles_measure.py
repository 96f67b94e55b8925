"""Times kernel K15 (``kernels.bnn_particles_cost_grad``, include/sgmcmc_hip_particles.h) and ``SVGDSampler`` on it against
the same sampler on torch autograd (``cost.use_hip_kernel = False``: the vmap route, which is what a sampler took before the
kernel existed), on the default net [1, 50, 50, 50, 1] at batch 20 with 16 and 128 particles in f32 and f64:
  (a) K15 alone; (b) one ``next(sampler)`` on the K15 route; (c) the same with ``use_hip_kernel = False``;
(b) and (c) in eager stepping and with ``use_hip_graph = True``. Device events on the stream around blocks of 20 calls,
medians of 11 blocks after a warm-up block, (b) and (c) alternating block by block. The record is profiles/bnn_particles.txt.

    python tools/gpu/bnn_particles_measure.py [output file]
"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from pysgmcmc_amd import kernels
from pysgmcmc_amd.data_batches import Placeholder, generate_batches
from pysgmcmc_amd.models import BNNParticleCost, bnn_particles
from pysgmcmc_amd.samplers import SVGDSampler
from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else open(os.devnull, "w")
def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True); out.write(line + "\n"); out.flush()

dev = torch.device("cuda:0")
sizes, B, P, CALLS, BLOCKS = [1, 50, 50, 50, 1], 20, 5252, 20, 11
say("device", torch.cuda.get_device_name(0), "torch", torch.__version__)
say("net", sizes, "batch", B, "LDS bytes f32", kernels.bnn_particles_lds_bytes(sizes, B, torch.float32), "f64",
    kernels.bnn_particles_lds_bytes(sizes, B, torch.float64))
rng = np.random.RandomState(1)
X = rng.rand(100, 1)
y = np.sinc(X * 10 - 5).sum(axis=1)

def block(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS                      # us per call

def median_of(fns):
    """us per call of each fn: a warm-up block each, then BLOCKS blocks each, the fns taking turns"""
    for fn in fns:
        block(fn)
    ts = [[] for _ in fns]
    for _ in range(BLOCKS):
        for k, fn in enumerate(fns):
            ts[k].append(block(fn))
    return [(statistics.median(t), min(t), max(t)) for t in ts]

def sampler(n, dt, kernel, graph):
    xp, yp = Placeholder(dtype=dt, device=dev), Placeholder(dtype=dt, device=dev)
    cost = BNNParticleCost(sizes, xp, yp, batch_size=B, n_examples=100)
    cost.use_hip_kernel = kernel
    s = SVGDSampler(bnn_particles(n, 1, seed=3, dtype=dt, device=dev), cost, batch_generator=generate_batches(X, y, xp, yp, B, seed=1),
                    stepsize_schedule=ConstantStepsizeSchedule(1e-3), session=dev, dtype=dt)
    s.sample_format, s.use_hip_graph = "view", graph
    return s

for dt in (torch.float32, torch.float64):
    for n in (16, 128):
        say("---- %d particles, %s" % (n, dt))
        theta = torch.stack(bnn_particles(n, 1, seed=3, dtype=dt, device=dev)).reshape(-1)
        grad, costs = torch.empty_like(theta), torch.empty(n, dtype=dt, device=dev)
        Xb, yb = torch.tensor(X[:B], dtype=dt, device=dev), torch.tensor(y[:B], dtype=dt, device=dev)
        (med, lo, hi), = median_of([lambda: kernels.bnn_particles_cost_grad(theta, n, P, sizes, Xb, yb, grad, P, costs, B, 100, 1.0,
                                                                           1e-6, 0.01)])
        say("(a) K15 alone:                                   median %8.1f us (min %.1f, max %.1f) per call" % (med, lo, hi))
        for graph in (False, True):
            b, c = sampler(n, dt, True, graph), sampler(n, dt, False, graph)
            mode = "use_hip_graph=True" if graph else "eager             "
            try:
                next(c)
            except Exception as exc:                             # e.g. a cost that cannot be recorded into a graph
                (mb, lb, hb), = median_of([lambda: next(b)])
                say("(b) next(sampler), K15 route,      %s: median %8.1f us (min %.1f, max %.1f) per step" % (mode, mb, lb, hb))
                say("(c) next(sampler), autograd,        %s: NOT MEASURED, the step raised %s: %s" % (
                    mode, type(exc).__name__, str(exc).splitlines()[0]))
                continue
            (mb, lb, hb), (mc, lc, hc) = median_of([lambda: next(b), lambda: next(c)])
            route = "vmap" if c._vmapped else "loop"
            say("(b) next(sampler), K15 route,      %s: median %8.1f us (min %.1f, max %.1f) per step" % (mode, mb, lb, hb))
            say("(c) next(sampler), autograd (%s), %s: median %8.1f us (min %.1f, max %.1f) per step   (c)/(b) = %.2f" % (
                route, mode, mc, lc, hc, mc / mb))
            assert b._particle_costs is not None and c._particle_costs is None
            del b, c
        torch.cuda.empty_cache()
say("done")
