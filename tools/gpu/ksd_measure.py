"""K16 (kernels.ksd) against the torch statement of the same thing, and K15's chunked score time: the figures of
profiles/ksd.txt.

    python tools/gpu/ksd_measure.py [output file]

Event-timed medians, the two routes interleaved in one process after a warm-up of every shape. The torch statement is three
library products plus the element-wise passes in the case's dtype (IMQ, c = 1, beta = -1/2): what a user would write."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch

from pysgmcmc_amd import kernels, models

DEV = torch.device("cuda:0")
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(line=""):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def torch_statement(x, s):
    """V of the IMQ Stein kernel by library products; every n x n pass is a torch op in x's dtype"""
    n, d = x.shape
    xc = x - x.mean(dim=0, keepdim=True)
    A, B, C = xc @ xc.T, s @ s.T, s @ xc.T
    dA, dC = A.diagonal(), C.diagonal()
    r2 = torch.clamp(dA[:, None] + dA[None, :] - 2.0 * A, min=0.0)
    t = (C + C.T) - (dC[:, None] + dC[None, :])
    u = 1.0 + r2
    phi = torch.rsqrt(u)
    d1 = -0.5 * phi / u
    d2 = -1.5 * d1 / u
    kp = phi * B + 2.0 * d1 * t - 2.0 * d * d1 - 4.0 * d2 * r2
    return kp.double().sum() / (float(n) * n)


def median_ms(fns, reps):
    """medians of the event-timed calls of each function, the functions alternating"""
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in times], [float(np.min(t)) for t in times]


say("K16, kernels.ksd (IMQ, c = 1, beta = -1/2, row sums and stats, no matrix) against the torch statement (three library")
say("products and the element-wise passes in the same dtype); event-timed medians (minima) in ms, alternating, %s" %
    torch.cuda.get_device_name(0))
say("%6s %6s %8s %18s %18s %10s %12s" % ("n", "dim", "dtype", "K16", "torch", "K16/torch", "rel diff V"))
for n, d in ((1024, 5253), (4096, 5253)):
    for dt in (torch.float32, torch.float64):
        g = torch.Generator(device="cpu").manual_seed(n + d)
        x = (0.3 + torch.randn(n, d, generator=g, dtype=torch.float64) / d ** 0.5).to(dt).to(DEV)
        s = torch.randn(n, d, generator=g, dtype=torch.float64).to(dt).to(DEV)
        ws = kernels.ksd_workspace(n, x)
        rows = torch.empty(n, dtype=torch.float64, device=DEV)
        stats = torch.empty(4, dtype=torch.float64, device=DEV)
        box = {}

        def k16():
            kernels.ksd(x, s, ws, row_sums=rows, stats=stats)

        def lib():
            box["v"] = torch_statement(x, s)

        for _ in range(3):
            k16()
            lib()
        torch.cuda.synchronize()
        (m_k, m_t), (lo_k, lo_t) = median_ms([k16, lib], 15)
        rel = abs(float(stats[0]) - float(box["v"])) / abs(float(box["v"]))
        say("%6d %6d %8s %9.3f (%6.3f) %9.3f (%6.3f) %10.2f %12.2e" % (n, d, str(dt)[6:], m_k, lo_k, m_t, lo_t, m_k / m_t, rel))
        del x, s, ws

say()
say("models.bnn_posterior_scores (K15, one launch per chunk of data rows) for a 4096-row trace of the default net at N = 100")
layer_sizes = [1, 50, 50, 50, 1]
rng = np.random.RandomState(1)
X = rng.rand(100, 1)
y = np.sinc(X * 10 - 5).sum(axis=1)
for dt in (torch.float32, torch.float64):
    theta = torch.stack(models.bnn_particles(8, 1, seed=0, dtype=dt, device=DEV)).repeat(512, 1)
    theta += 0.01 * torch.randn(theta.shape, dtype=dt, device=DEV)
    Xd, yd = torch.as_tensor(X, dtype=dt, device=DEV), torch.as_tensor(y, dtype=dt, device=DEV)
    res = torch.empty_like(theta)
    from pysgmcmc_amd.models.scores import bnn_scores_chunk_rows
    chunk = bnn_scores_chunk_rows(layer_sizes, 100, dt)

    def scores():
        models.bnn_posterior_scores(theta, layer_sizes, Xd, yd, out=res)

    for _ in range(2):
        scores()
    torch.cuda.synchronize()
    (m,), (lo,) = median_ms([scores], 7)
    say("%8s: %d rows x %d parameters, chunks of %d data rows (%d launches): %.3f ms (min %.3f)" % (
        str(dt)[6:], theta.shape[0], theta.shape[1], chunk, -(-100 // chunk), m, lo))
