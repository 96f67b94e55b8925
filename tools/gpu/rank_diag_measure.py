"""K18 (kernels.rank_normalize) and diagnostics.rank_diagnostics_all against a torch statement of the same transform, and the
two measured bounds of tests/test_rank_diag_gpu.py: the figures of profiles/rank_diag.txt.

    python tools/gpu/rank_diag_measure.py [output file]

Event-timed medians of repeated launches after a warm-up of every shape, the routes alternating in one process. The torch
statement is what a user would write on the device: a transpose copy of the split trace to (P, N), torch.sort along the
pooled axis, tie runs by cummax / cummin, torch.special.ndtri, a scatter back to draw order, the same for |x - median|, the
two tail indicators, and the copy into the (2 m, n / 2, 4 P) layout K12 reads."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from pysgmcmc_amd import diagnostics, kernels
from pysgmcmc_amd.diagnostics import rank

import rank_cases as C

DEV = torch.device("cuda:0")
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(line=""):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def _scores(v, N):
    """normal scores of the average ranks of the rows of v (P, N), in draw order"""
    s, idx = torch.sort(v, dim=1)
    pos = torch.arange(N, device=v.device).expand_as(s)
    start = torch.ones_like(s, dtype=torch.bool)
    start[:, 1:] = s[:, 1:] != s[:, :-1]
    end = torch.ones_like(start)
    end[:, :-1] = start[:, 1:]
    first = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), dim=1).values
    last = torch.flip(torch.cummin(torch.flip(torch.where(end, pos, torch.full_like(pos, N)), [1]), dim=1).values, [1])
    p = ((first + last + 2).double() - 0.75) / (2.0 * N + 0.5)
    z = torch.empty_like(s)
    z.scatter_(1, idx, torch.special.ndtri(p))
    return z, s


def torch_statement(x, buf):
    m, n, P = x.shape
    half = n // 2
    N = 2 * m * half
    split = torch.stack([x[:, :half], x[:, n - half:]], dim=1).reshape(2 * m, half, P)
    v = split.permute(2, 0, 1).reshape(P, N).double()
    z, s = _scores(v, N)
    med = (s[:, N // 2 - 1] + s[:, N // 2]) * 0.5
    zf, _ = _scores((v - med[:, None]).abs(), N)
    lo = (v <= s[:, (N - 1) // 20, None]).double()
    hi = (v >= s[:, (19 * (N - 1) + 19) // 20, None]).double()
    for k, a in enumerate((zf, z, lo, hi)):
        buf[:, :, k * P:(k + 1) * P] = a.reshape(P, 2 * m, half).permute(1, 2, 0)
    return buf


def median_ms(fns, reps):
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


say("K18, kernels.rank_normalize (one launch, one workgroup per column), the whole diagnostics.rank_diagnostics_all (K18 + two")
say("K12 launches) and the torch statement of K18's transform (sort, tie runs, ndtri, scatter; in double on the device);")
say("event-timed medians (minima) in ms, alternating, P = 5253, %s" % torch.cuda.get_device_name(0))
say("%6s %5s %5s %8s %18s %18s %20s %10s %10s" % ("N", "m", "n", "dtype", "K18", "rank_diag_all", "torch", "torch/K18", "tails same"))
P = 5253
for m, n in ((4, 128), (16, 256), (32, 256)):
    N = 2 * m * (n // 2)
    for dt in (torch.float32, torch.float64):
        g = torch.Generator(device="cpu").manual_seed(N)
        x = torch.randn(m, n, P, generator=g, dtype=torch.float64).to(dt).to(DEV)
        buf_k = torch.empty(2 * m, n // 2, 4 * P, dtype=torch.float64, device=DEV)
        buf_t = torch.empty_like(buf_k)
        blocks = [buf_k[:, :, k * P:(k + 1) * P] for k in range(4)]

        def k18():
            kernels.rank_normalize(x, z=blocks[1], z_folded=blocks[0], tail_lo=blocks[2], tail_hi=blocks[3])

        def whole():
            diagnostics.rank_diagnostics_all(x)

        def lib():
            torch_statement(x, buf_t)

        for _ in range(2):
            k18()
            whole()
            lib()
        torch.cuda.synchronize()
        (m_k, m_w, m_t), (lo_k, lo_w, lo_t) = median_ms([k18, whole, lib], 7)
        same = bool(torch.equal(buf_k[:, :, 2 * P:], buf_t[:, :, 2 * P:]))
        zdiff = float((buf_k[:, :, :2 * P] - buf_t[:, :, :2 * P]).abs().max())
        say("%6d %5d %5d %8s %9.3f (%6.3f) %9.3f (%6.3f) %10.3f (%8.3f) %10.2f %10s   max |z - torch z| %.2g" % (
            N, m, n, str(dt)[6:], m_k, lo_k, m_w, lo_w, m_t, lo_t, m_t / m_k, same, zdiff))
        del x, buf_k, buf_t, blocks
        torch.cuda.empty_cache()

say()
say("Largest ulp distance between K18's z and the host table (statistics.NormalDist().inv_cdf, AS241) over ALL 2 N - 1")
say("possible arguments; 0 on the central branch by construction, the tail branches go through the device's log and sqrt:")
worst = 0
for m, n in ((2, 4096), (1, 64)):
    xa = C.all_rank2_trace(m, n)
    N = m * n
    r2 = C.pooled_rank2(xa)[0].ravel()
    table = rank.z_of_rank2(N)
    for dt in (torch.float32, torch.float64):
        z = torch.empty(2 * m, n // 2, 3, dtype=torch.float64, device=DEV)
        kernels.rank_normalize(torch.as_tensor(xa, device=DEV).to(dt), z=z)
        dist = C.ulp_distance(z.cpu().numpy().ravel(), table[r2])
        mid = C.central(r2, N)
        worst = max(worst, int(dist.max()))
        say("  N = %5d %8s: %d ulp over %d arguments (central branch %d ulp, %d of the arguments)" % (
            N, str(dt)[6:], int(dist.max()), np.unique(r2).size, int(dist[mid].max()), int(np.unique(r2[mid]).size)))
say("  TAIL_ULP_MEASURED = %d" % worst)

say()
say("Largest relative difference of rank_diagnostics_all's R-hats and raw ESS values to the host statement")
say("rank.rank_diagnostics at the largest test case, 64 chains x 128 draws x 20 columns (N = 8192):")
xa = C.ar_chains(64, 128, 20, seed=64)
h = rank.rank_diagnostics(xa)
worst = 0.0
for dt in (torch.float32, torch.float64):
    d = diagnostics.rank_diagnostics_all(torch.as_tensor(xa, device=DEV).to(dt), details=True)
    for name in ("rhat_rank", "rhat_bulk", "rhat_folded", "raw_bulk", "raw_tail_lo", "raw_tail_hi"):
        a, b = getattr(d, name).cpu().numpy(), getattr(h, name)
        rel = float(np.max(np.abs(a - b) / np.abs(b)))
        worst = max(worst, rel)
        say("  %8s %12s: %.3g" % (str(dt)[6:], name, rel))
say("  REL_MEASURED = %.3g" % worst)
