"""K17 (kernels.stein_thin) against the torch statement of the same loop: the figures of profiles/stein_thin.txt.

    python tools/gpu/stein_thin_measure.py [output file]

Event-timed medians, the two routes interleaved in one process after a warm-up of every shape. The torch statement is what a
user would write on the device: per pick an argmin, an index by the device-side result and the addition of that row, in
double, with the path kept on the device (no host synchronisation inside the loop, as in K17)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch

from pysgmcmc_amd import kernels

DEV = torch.device("cuda:0")
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(line=""):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def torch_statement(K, m, indices, path):
    """the greedy loop in torch ops on the device: three or four launches and a device-side index per pick"""
    h = 0.5 * K.diagonal().double()
    acc = torch.zeros_like(h)
    S = torch.zeros((), dtype=torch.float64, device=K.device)
    for t in range(1, m + 1):
        obj = acc + h
        j = torch.argmin(obj)
        S = S + 2.0 * obj[j]
        indices[t - 1] = j
        path[t - 1] = S / (float(t) * float(t))
        acc = acc + K[j].double()
    return indices, path


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


say("K17, kernels.stein_thin (one launch, one workgroup) against the torch statement of the same loop (argmin, index, add per")
say("pick, in double on the device); event-timed medians (minima) in ms, alternating, %s" % torch.cuda.get_device_name(0))
say("%6s %6s %8s %18s %20s %10s %12s" % ("n", "m", "dtype", "K17", "torch", "torch/K17", "same picks"))
n = 4096
for dt in (torch.float32, torch.float64):
    g = torch.Generator(device="cpu").manual_seed(n)
    G = torch.randn(n, 8, generator=g, dtype=torch.float64)
    K = G @ G.T + torch.diag(0.5 + 1.5 * torch.rand(n, generator=g, dtype=torch.float64))
    K = K.to(dt)
    K = (torch.triu(K) + torch.triu(K, 1).T).to(DEV)
    for m, reps in ((64, 15), (4096, 5)):
        idx_k = torch.empty(m, dtype=torch.int32, device=DEV)
        idx_t = torch.empty(m, dtype=torch.int64, device=DEV)
        path_k, path_t = (torch.empty(m, dtype=torch.float64, device=DEV) for _ in range(2))

        def k17():
            kernels.stein_thin(K, m, indices=idx_k, path=path_k)

        def lib():
            torch_statement(K, m, idx_t, path_t)

        for _ in range(2):
            k17()
            lib()
        torch.cuda.synchronize()
        (m_k, m_t), (lo_k, lo_t) = median_ms([k17, lib], reps)
        same = bool(torch.equal(idx_k.long(), idx_t))
        say("%6d %6d %8s %9.3f (%6.3f) %10.3f (%8.3f) %10.1f %12s" % (n, m, str(dt)[6:], m_k, lo_k, m_t, lo_t, m_t / m_k, same))
        say("%31s %.2f us a pick" % ("", 1e3 * m_k / m))
    del K
