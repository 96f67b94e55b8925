"""K20 (kernels.mixture_calibration) against a torch statement of the same sums, and models.calibration_score as a whole:
the timing figures of profiles/calibration.txt. (The two measured bounds in that file come from
tests/test_calibration_gpu.py, which prints every difference before it asserts.)

    python tools/gpu/calibration_measure.py [output file]

Event-timed medians of the repetitions after a warm-up of every shape, the routes alternating in one process, every
repetition on a fresh input drawn on the device outside the timed region. The torch statement is what a user would write on
the device: the PIT as the mean of the draws' normal CDFs, the first CRPS term as a mean over the draws, and the pair term as
the mean of A over the whole S x S matrix of pairs (diagonal included, both triangles), in double, chunked over the rows so
that the (S, S, chunk) temporary stays within CHUNK_BYTES."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from pysgmcmc_amd import kernels, models

DEV = torch.device("cuda:0")
REPS, REPS_LARGE = 21, 5                                  # REPS_LARGE where S * S * n_rows exceeds LARGE pair terms
LARGE = 2e9
CHUNK_BYTES = 1 << 30
LEVELS, N_BINS = (0.5, 0.8, 0.9, 0.95), 10
SQRT2, INV_SQRTPI = math.sqrt(2.0), 1.0 / math.sqrt(math.pi)
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(line=""):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def expected_abs(d, c):
    e = c * SQRT2
    u = d / e
    return e * (u * torch.erf(u) + torch.exp(-(u * u)) * INV_SQRTPI)


def torch_statement(args):
    """(pit, crps, coverage counts, histogram) of the (S, R) means in torch ops, in double."""
    means, var, y = args
    S, R = means.shape
    mu, yy = means.double(), y.double()
    sd = torch.sqrt(var)[:, None]
    d = yy[None, :] - mu
    pit = (0.5 * torch.erfc(-(d / sd) / SQRT2)).mean(dim=0)
    first = expected_abs(d, sd).mean(dim=0)
    c = torch.sqrt(var[:, None] + var[None, :])[:, :, None]
    rows = max(1, CHUNK_BYTES // (8 * S * S))
    pair = torch.empty(R, dtype=torch.float64, device=means.device)
    for lo in range(0, R, rows):
        m = mu[:, lo:lo + rows]
        pair[lo:lo + rows] = expected_abs(m[:, None, :] - m[None, :, :], c).sum(dim=(0, 1))
    crps = first - pair / (2.0 * S * S)
    half = torch.tensor(LEVELS, dtype=torch.float64, device=means.device)[:, None] * 0.5
    counts = ((pit[None, :] - 0.5).abs() <= half).sum(dim=1)
    hist = torch.bincount((pit * N_BINS).floor().long().clamp(max=N_BINS - 1), minlength=N_BINS)
    return pit, crps, counts, hist


def fresh(S, R, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    trend = torch.sin(torch.linspace(0.0, 3.0, R, device=DEV))
    means = (trend[None, :] + 0.4 * torch.randn(S, R, generator=g, device=DEV)).to(dtype)
    var = torch.exp(0.75 * torch.randn(S, generator=g, dtype=torch.float64, device=DEV) - 1.5)
    y = (trend + 0.5 * torch.randn(R, generator=g, device=DEV)).to(dtype)
    return means, var, y


def median_ms(make, fns, reps):
    """fns alternate; every repetition of every route gets make(seed) afresh, drawn before the start event."""
    times = [[] for _ in fns]
    for rep in range(reps):
        for k, fn in enumerate(fns):
            arg = make(1000 * rep + k)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(arg)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in times], [float(np.min(t)) for t in times]


say("K20, kernels.mixture_calibration (one launch, one workgroup per row, plus the 256-lane summary) with 4 levels and 10 bins,")
say("float32 means, against the torch statement of the same sums (the dense S x S pair matrix in double on the device, chunked")
say("over the rows to %d MiB a temporary); event-timed medians (minima) in ms of %d repetitions (%d where S * S * n_rows > %.0e)," % (
    CHUNK_BYTES >> 20, REPS, REPS_LARGE, LARGE))
say("alternating, a fresh input per repetition, %s" % torch.cuda.get_device_name(0))
say("%6s %7s %5s %20s %22s %10s   %s" % ("S", "n_rows", "reps", "K20", "torch", "torch/K20", "agreement of the two"))
for S in (512, 2048, 4096):
    for R in (100, 5000):
        reps = REPS_LARGE if float(S) * S * R > LARGE else REPS
        pit, crps = (torch.empty(R, dtype=torch.float64, device=DEV) for _ in range(2))
        summary = torch.empty(2 + len(LEVELS) + N_BINS, dtype=torch.float64, device=DEV)

        def k20(args):
            kernels.mixture_calibration(args[0], args[1], args[2], LEVELS, N_BINS, pit, crps, summary)

        make = lambda seed: fresh(S, R, seed)
        args = make(7)
        for _ in range(2):
            k20(args)
            t = torch_statement(args)
        torch.cuda.synchronize()
        d_pit = float((t[0] - pit).abs().max())
        d_crps = float((t[1] - crps).abs().max())
        same_counts = bool(torch.equal(t[2].double(), summary[2:2 + len(LEVELS)]) and torch.equal(t[3].double(), summary[-N_BINS:]))
        del t, args
        (m_k, m_t), (lo_k, lo_t) = median_ms(make, [k20, torch_statement], reps)
        say("%6d %7d %5d %10.3f (%7.3f) %11.3f (%8.3f) %10.2f   counts equal %s, max |d pit| %.2g, max |d crps| %.2g" % (
            S, R, reps, m_k, lo_k, m_t, lo_t, m_t / m_k, same_counts, d_pit, d_crps))
        del pit, crps, summary
        torch.cuda.empty_cache()

say()
say("models.calibration_score as a whole (K11's forward pass, the variances, K20 and its summary, the allocations), float32")
say("traces of the [1, 50, 50, 50, 1] net drawn afresh per repetition; medians (minima) in ms:")
say("%6s %7s %5s %20s" % ("S", "n_rows", "reps", "calibration_score"))
sizes = [1, 50, 50, 50, 1]
P = kernels._bnn_n_params(sizes)
for S in (512, 2048, 4096):
    for R in (100, 5000):
        reps = REPS_LARGE if float(S) * S * R > LARGE else REPS
        g = torch.Generator(device=DEV).manual_seed(S + R)
        X = torch.rand(R, 1, generator=g, device=DEV) * 6.0 - 3.0
        y = torch.sinc(X[:, 0]) + 0.05 * torch.randn(R, generator=g, device=DEV)

        def make(seed):
            gg = torch.Generator(device=DEV).manual_seed(seed)
            return 0.2 * torch.randn(S, P, generator=gg, device=DEV)

        def whole(trace):
            return models.calibration_score(trace, X, y, sizes)

        for _ in range(2):
            whole(make(3))
        torch.cuda.synchronize()
        (m_w,), (lo_w,) = median_ms(make, [whole], reps)
        say("%6d %7d %5d %10.3f (%7.3f)" % (S, R, reps, m_w, lo_w))
        torch.cuda.empty_cache()
