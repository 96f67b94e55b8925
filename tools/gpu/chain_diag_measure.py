"""Times ``kernels.chain_diag`` (K12, include/sgmcmc_hip_chains.h) -- the full diagnosis and the R-hat-only launch, `waves`
auto and 1 -- on AR(1) traces shaped like ``examples/many_chains.py``'s, (256, 50, 5252) and (64, 50, 5252) in f32, against
what the package had for the same numbers before: ``gelman_rubin_from_chains`` on the whole trace (torch ops on a float64
copy), K10 (``effective_n_all``) at 64 chains, and at 256 chains the column loop of the scalar ``effective_n``, timed over
256 columns and SCALED to 5252. Medians of 11 runs after a warm-up call: device events on the stream for the device calls,
a host clock around the column loop (every call of it reads its result back). The record is profiles/chain_diagnostics.txt.

    python tools/gpu/chain_diag_measure.py [output file]
"""
import os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from pysgmcmc_amd import kernels
from pysgmcmc_amd.diagnostics import effective_n_all
from pysgmcmc_amd.diagnostics.sampler_diagnostics import effective_n, gelman_rubin_from_chains

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else open(os.devnull, "w")
def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True); out.write(line + "\n"); out.flush()

dev = torch.device("cuda:0")
P, n = 5252, 50
say("device", torch.cuda.get_device_name(0), "torch", torch.__version__)

def trace(m):
    """AR(1) columns with phi drawn from {0, .5, .9, .97}, a per-chain shift in a third of them, lognormal scales."""
    g = torch.Generator(device=dev).manual_seed(7)
    phi = torch.tensor([0.0, 0.5, 0.9, 0.97], device=dev)[torch.randint(0, 4, (P,), generator=g, device=dev)]
    e = torch.randn(m, n, P, generator=g, device=dev)
    x = torch.empty_like(e)
    x[:, 0] = e[:, 0]
    for i in range(1, n):
        x[:, i] = phi * x[:, i - 1] + torch.sqrt(1 - phi * phi) * e[:, i]
    shift = (torch.rand(P, generator=g, device=dev) < 0.33) * torch.randn(m, 1, P, generator=g, device=dev) * 2.0
    return ((x + shift) * torch.exp(2.0 * torch.randn(P, generator=g, device=dev))).float().contiguous()

def events(fn, runs=11):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b))
    return "median %8.3f ms   [%.3f .. %.3f]" % (statistics.median(ts), min(ts), max(ts))

for m in (256, 64):
    t = trace(m)
    rhat = torch.empty(P, dtype=torch.float64, device=dev)
    ess = torch.empty(P, dtype=torch.int64, device=dev)
    raw = torch.empty(P, dtype=torch.float64, device=dev)
    stop = torch.empty(P, dtype=torch.int32, device=dev)
    kernels.chain_diag(t, rhat, ess, raw, stop)
    lags = stop.double()
    say("---- (%d, %d, %d) f32, %.0f MB; stop lag min %d median %d mean %.1f max %d; rhat median %.3f max %.2f; ess median %d"
        % (m, n, P, t.numel() * 4 / 1e6, int(stop.min()), int(stop.median()), float(lags.mean()), int(stop.max()),
           float(rhat.median()), float(rhat.max()), int(ess.median())))
    for waves in (None, 1, 2, 4, 8, 16):
        if waves is not None and waves > (m + 15) // 16:
            continue
        say("K12 full (rhat, ess, raw, stop_lag), waves %-4s events: %s" % (waves or "auto", events(lambda: kernels.chain_diag(t, rhat, ess, raw, stop, waves=waves))))
    for waves in (None, 1):
        say("K12 R-hat only,                      waves %-4s events: %s" % (waves or "auto", events(lambda: kernels.chain_diag(t, rhat, waves=waves))))
    say("gelman_rubin_from_chains, whole trace (torch, f64 copy), events: %s" % events(lambda: gelman_rubin_from_chains(t)))
    ref = gelman_rubin_from_chains(t)
    say("   max relative R-hat difference to it: %.3g" % float(((rhat - ref).abs() / ref).max()))
    if m <= 64:
        say("K10 effective_n_all (ess, raw, stop_lag), events:               %s" % events(lambda: effective_n_all(t, details=True)))
        e10 = effective_n_all(t)
        say("   columns whose ess differs from K10's (other summation order beyond 16 chains): %d of %d" % (int((e10 != ess).sum()), P))
    else:
        cols = 256
        effective_n(t[:, :, 0]); torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            loop = [effective_n(t[:, :, j]) for j in range(cols)]
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        say("column loop of effective_n over %d columns, host clock: median %.1f ms of 3 -> SCALED to %d columns: %.0f ms"
            % (cols, med * 1e3, P, med * 1e3 * P / cols))
        say("   columns of those %d whose ess differs from K12's: %d" % (cols, sum(int(a != int(b)) for a, b in zip(loop, ess[:cols].cpu()))))
    del t
    torch.cuda.empty_cache()
say("done")
