"""K19 (kernels.psis_loo) against a torch statement of the same transform, and models.loo_score as a whole: the timing
figures of profiles/psis_loo.txt. (The three measured bounds in that file come from tests/test_psis_loo_gpu.py, which
prints every difference before it asserts.)

    python tools/gpu/psis_loo_measure.py [output file]

Event-timed medians of REPS repetitions after a warm-up of every shape, the routes alternating in one process, every
repetition on a fresh input drawn on the device outside the timed region. The torch statement is what a user would write on
the device: a transposed copy, a batched sort of the whole matrix, the last M sorted values as a masked tail, the grid fit
as a loop of G passes over every tail, the smoothed tail scattered back to draw order, and torch.logsumexp."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from pysgmcmc_amd import kernels, models
from pysgmcmc_amd.diagnostics import psis

DEV = torch.device("cuda:0")
REPS = 21
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(line=""):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def torch_statement(ll, r_eff=1.0):
    """(elpd_loo, khat, n_tail, row_lppd, lwn) of the (S, R) matrix ll in torch ops, in double."""
    S, R = ll.shape
    M = psis.tail_length(S, r_eff)
    l = ll.t().contiguous()                                               # (R, S)
    lr = -l
    lw = lr - lr.max(dim=1, keepdim=True).values
    s, idx = torch.sort(lw, dim=1, stable=True)
    cut = s[:, S - M - 1].clamp(min=psis.LOG_DBL_MIN)[:, None]
    tail = s[:, S - M:]
    mask = tail > cut                                                     # the tail sits at the end of the M values
    n = mask.sum(dim=1)
    dn = n.double().clamp(min=1.0)
    ec = torch.exp(cut)
    x = torch.where(mask, torch.exp(tail) - ec, torch.zeros_like(tail))
    G = 30.0 + torch.floor(torch.sqrt(dn))
    q = (M - n + torch.floor(dn / 4.0 + 0.5).long() - 1).clamp(0, M - 1)
    xq3 = 3.0 * x.gather(1, q[:, None])[:, 0]
    xinv = 1.0 / x[:, -1]
    g_max = 30 + int(math.isqrt(M))
    bs, Ls = [], []
    for j in range(1, g_max + 1):
        b = (1.0 - torch.sqrt(G / (j - 0.5))) / xq3 + xinv
        k = torch.log1p(-b[:, None] * x).sum(dim=1) / dn                  # x = 0 outside the tail adds log1p(0) = 0
        L = dn * (torch.log(-(b / k)) - k - 1.0)
        bs.append(b)
        Ls.append(torch.where(G >= j, L, torch.full_like(L, -math.inf)))
    b, L = torch.stack(bs, dim=1), torch.stack(Ls, dim=1)                 # (R, g_max)
    w = 1.0 / torch.exp(L[:, None, :] - L[:, :, None]).sum(dim=2)
    w = torch.where(w < 10.0 * np.finfo(np.float64).eps, torch.zeros_like(w), w)
    w = torch.where(torch.isfinite(L), w, torch.zeros_like(w))
    w = w / w.sum(dim=1, keepdim=True)
    bb = (b * w).sum(dim=1)
    kk = torch.log1p(-bb[:, None] * x).sum(dim=1) / dn
    sigma = -kk / bb
    khat = (dn * kk + 5.0) / (dn + 10.0)
    p = (torch.arange(M, device=ll.device)[None, :] - (M - n)[:, None] + 0.5) / dn[:, None]
    p = p.clamp(min=0.0)
    y = sigma[:, None] * torch.expm1(-khat[:, None] * torch.log1p(-p)) / khat[:, None]
    smooth = (n > 4) & torch.isfinite(khat)
    s = s.clone()
    s[:, S - M:] = torch.where(mask & smooth[:, None], torch.log(y + ec), tail)
    s.clamp_(max=0.0)
    lw = torch.empty_like(s).scatter_(1, idx, s)
    lwn = lw - torch.logsumexp(lw, dim=1, keepdim=True)
    elpd = torch.logsumexp(lwn + l, dim=1)
    lppd = torch.logsumexp(l, dim=1) - math.log(S)
    khat = torch.where(n > 4, khat, torch.full_like(khat, math.inf))
    return elpd, khat, n, lppd, lwn.t()


def fresh_loglik(S, R, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    mu = 0.3 + 0.4 * torch.randn(S, 1, generator=g, dtype=torch.float64, device=DEV)
    y = torch.randn(1, R, generator=g, dtype=torch.float64, device=DEV)
    return -0.5 * math.log(2.0 * math.pi) - 0.5 * (y - mu) ** 2


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


say("K19, kernels.psis_loo (one launch, one workgroup per observation column, plus the 256-lane totals) with row_lppd,")
say("log_weights and summary on, against the torch statement of the same transform (batched sort, masked tail, the grid")
say("loop; in double on the device); event-timed medians (minima) of %d repetitions in ms, alternating, a fresh input per" % REPS)
say("repetition, r_eff = 1, %s" % torch.cuda.get_device_name(0))
say("%6s %7s %5s %18s %20s %10s   %s" % ("S", "n_rows", "M", "K19", "torch", "torch/K19", "agreement of the two"))
for S in (512, 4096, 8192):
    for R in (100, 5000):
        elpd, khat = (torch.empty(R, dtype=torch.float64, device=DEV) for _ in range(2))
        row_lppd = torch.empty(R, dtype=torch.float64, device=DEV)
        n_tail = torch.empty(R, dtype=torch.int32, device=DEV)
        logw = torch.empty(S, R, dtype=torch.float64, device=DEV)
        summary = torch.empty(4, dtype=torch.float64, device=DEV)

        def k19(ll):
            kernels.psis_loo(ll, 1.0, elpd, khat, n_tail, row_lppd, logw, summary)

        def lib(ll):
            return torch_statement(ll)

        make = lambda seed: fresh_loglik(S, R, seed)
        ll = make(7)
        for _ in range(2):
            k19(ll)
            t = lib(ll)
        torch.cuda.synchronize()
        same_tail = bool(torch.equal(t[2].to(torch.int32), n_tail))
        d_khat = float((t[1] - khat).abs().max())
        d_elpd = float((t[0] - elpd).abs().max())
        del t, ll
        (m_k, m_t), (lo_k, lo_t) = median_ms(make, [k19, lib], REPS)
        say("%6d %7d %5d %9.3f (%6.3f) %10.3f (%8.3f) %10.2f   n_tail equal %s, max |d khat| %.2g, max |d elpd_loo| %.2g" % (
            S, R, psis.tail_length(S), m_k, lo_k, m_t, lo_t, m_t / m_k, same_tail, d_khat, d_elpd))
        del elpd, khat, row_lppd, n_tail, logw, summary
        torch.cuda.empty_cache()

say()
say("models.loo_score as a whole (K11 + K13 with loglik, then K19 and its totals, the allocations and the standard error),")
say("float32 traces of the [1, 50, 50, 50, 1] net drawn afresh per repetition; medians (minima) of %d repetitions in ms:" % REPS)
say("%6s %7s %18s" % ("S", "n_rows", "loo_score"))
sizes = [1, 50, 50, 50, 1]
P = kernels._bnn_n_params(sizes)
for S in (512, 4096, 8192):
    for R in (100, 5000):
        g = torch.Generator(device=DEV).manual_seed(S + R)
        X = torch.rand(R, 1, generator=g, device=DEV) * 6.0 - 3.0
        y = torch.sinc(X[:, 0]) + 0.05 * torch.randn(R, generator=g, device=DEV)

        def make(seed):
            gg = torch.Generator(device=DEV).manual_seed(seed)
            return 0.2 * torch.randn(S, P, generator=gg, device=DEV)

        def whole(trace):
            return models.loo_score(trace, X, y, sizes)

        for _ in range(2):
            whole(make(3))
        torch.cuda.synchronize()
        (m_w,), (lo_w,) = median_ms(make, [whole], REPS)
        say("%6d %7d %9.3f (%6.3f)" % (S, R, m_w, lo_w))
        torch.cuda.empty_cache()
