"""Times the many-particle SVGD path (``kernels.svgd_many_step``, include/sgmcmc_hip_svgd_many.h) at dim 5252 (pitch 5312)
with 129, 256, 512 and 1024 particles in f32 and f64:
  (a) the step entry alone, and its kernel-matrix stage alone (``svgd_many_kernel`` without kernel gradients: every launch
      but UPDATE, plus the copy of K); the difference is the UPDATE launch;
  (b) one ``next(sampler)`` on the K15 route (``BNNParticleCost``), eager and with ``use_hip_graph = True``;
  (c) the same step written as torch expressions on the device -- ``cdist``, sort-median, two matmuls and the tail -- which is
      what a user would write without these kernels;
  (d) one large-dim row: 256 x 1 000 003 in f32, (a) and (c);
  (e) the bar units the kernels reach at the cases of tests/svgd_many_cases.py (the oracle runs on the host: a minute);
  (f) the cases of tests/svgd_many_exact_cases.py: whether the median of every lattice cloud is the oracle's bit for bit, and
      the bar units at the small-n and translated cases (seconds; ``--exact-only`` runs nothing else).
Device events on the stream around blocks of calls, medians of 9 blocks after a warm-up block, (a) and (c) alternating block
by block. The record is profiles/svgd_many.txt.

    python tools/gpu/svgd_many_measure.py [output file] [--no-units] [--exact-only]
"""
import math, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from pysgmcmc_amd import kernels
from pysgmcmc_amd.data_batches import Placeholder, generate_batches
from pysgmcmc_amd.models import BNNParticleCost, bnn_particles
from pysgmcmc_amd.samplers import SVGDSampler
from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
out = open(argv[0], "w") if argv else open(os.devnull, "w")
def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True); out.write(line + "\n"); out.flush()

dev = torch.device("cuda:0")
sizes, B, P, PITCH, BLOCKS = [1, 50, 50, 50, 1], 20, 5252, 5312, 9
EPS, ALPHA, FUDGE = 1e-3, 0.9, 1e-6
say("device", torch.cuda.get_device_name(0), "torch", torch.__version__)
rng = np.random.RandomState(1)
X = rng.rand(100, 1)
y = np.sinc(X * 10 - 5).sum(axis=1)

def block(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls                      # us per call

def median_of(fns, calls=10):
    for fn in fns:
        block(fn, calls)
    ts = [[] for _ in fns]
    for _ in range(BLOCKS):
        for k, fn in enumerate(fns):
            ts[k].append(block(fn, calls))
    return [(statistics.median(t), min(t), max(t)) for t in ts]

def torch_step(x, g, h, n, sign):
    """svgd.py:118-181 as torch expressions on [n, d] device tensors, in place on x and h"""
    D = torch.cdist(x, x) ** 2
    flat = D.flatten().sort().values
    N = n * n
    med = flat[N // 2] if N % 2 else 0.5 * (flat[N // 2 - 1] + flat[N // 2])
    h2 = 0.5 * med / math.log(n + 1.0)
    K = torch.exp(-D / h2 / 2)
    kg = (-(K @ x) + x * K.sum(dim=1, keepdim=True)) / h2
    gt = (K @ g + sign * kg) / n
    h.mul_(ALPHA).add_((1 - ALPHA) * gt * gt)
    x.sub_(EPS * gt / (FUDGE + h.sqrt()))

def sampler(n, dt, graph):
    xp, yp = Placeholder(dtype=dt, device=dev), Placeholder(dtype=dt, device=dev)
    cost = BNNParticleCost(sizes, xp, yp, batch_size=B, n_examples=100)
    s = SVGDSampler(bnn_particles(n, 1, seed=3, dtype=dt, device=dev), cost, batch_generator=generate_batches(X, y, xp, yp, B, seed=1),
                    stepsize_schedule=ConstantStepsizeSchedule(EPS), session=dev, dtype=dt)
    s.sample_format, s.use_hip_graph = "view", graph
    return s

def state(n, d, ld, dt):
    x = torch.zeros(n * ld, dtype=dt, device=dev)
    x.view(n, ld)[:, :d] = 0.3 + torch.randn(n, d, dtype=dt, device=dev) / math.sqrt(d)
    g = torch.randn(n * ld, dtype=dt, device=dev)
    h = torch.rand(n * ld, dtype=dt, device=dev) * 0.95 + 0.05
    return x, g, h

def entry_rows(n, d, ld, dt, calls):
    x, g, h = state(n, d, ld, dt)
    xt, gt_, ht = (t.view(n, ld)[:, :d].contiguous() for t in (x, g, h))
    ws = kernels.svgd_many_workspace(n, x)
    step = lambda: kernels.svgd_many_step(x, g, h, n, d, EPS, ALPHA, FUDGE, ws, ld=ld, repulsion_sign=-1)
    kmat = lambda: kernels.svgd_many_kernel(x, n, d, ws, ld=ld, kernel_gradients=False)
    ref = lambda: torch_step(xt, gt_, ht, n, -1.0)
    (ma, la, ha), (mk, lk, hk), (mc, lc, hc) = median_of([step, kmat, ref], calls)
    plan = kernels.svgd_many_plan(n, d, x)
    say("    launches:", " ".join("%s[%d]" % (kernels.SVGD_MANY_IDS[l.id], l.grid) for l in plan))
    say("(a) step entry:                    median %9.1f us (min %.1f, max %.1f); kernel-matrix stage %9.1f us (%.0f %%), "
        "UPDATE launch by difference %9.1f us (%.0f %%)" % (ma, la, ha, mk, 100 * mk / ma, ma - mk, 100 * (ma - mk) / ma))
    say("(c) torch restatement:             median %9.1f us (min %.1f, max %.1f)   (c)/(a) = %.2f" % (mc, lc, hc, mc / ma))
    assert torch.isfinite(x).all() and torch.isfinite(xt).all()

TIMINGS = "--exact-only" not in sys.argv
for dt in (torch.float32, torch.float64) if TIMINGS else ():
    for n in (129, 256, 512, 1024):
        say("---- %d particles x %d (pitch %d), %s" % (n, P, PITCH, dt))
        entry_rows(n, P, PITCH, dt, 10)
        for graph in (False, True):
            s = sampler(n, dt, graph)
            (mb, lb, hb), = median_of([lambda: next(s)])
            assert s._particle_costs is not None
            say("(b) next(sampler), K15 route, %s: median %9.1f us (min %.1f, max %.1f) per step" % (
                "use_hip_graph=True" if graph else "eager             ", mb, lb, hb))
            del s
        torch.cuda.empty_cache()
if TIMINGS:
    say("---- 256 particles x 1 000 003 (pitch 1 000 003), torch.float32")
    entry_rows(256, 1_000_003, 1_000_003, torch.float32, 3)
    torch.cuda.empty_cache()

if TIMINGS and "--no-units" not in sys.argv:
    import svgd_many_cases as M
    import test_svgd_tile_walk_gpu as W
    say("---- units of the displacement bar at c = 1 (X, H) reached by the kernels; c = %.2f (f32), %.2f (f64)" % (M.C[M.F32], M.C[M.F64]))
    for dtype in (M.F32, M.F64):
        for n, d in list(M.TABLE) + M.walk_cases(dtype) + M.phase_cases(dtype):
            row = []
            for sign in (1, -1):
                ref = M.step_reference(M.Case(n, d, dtype, sign))
                x, g, h = (torch.from_numpy(a.copy()).to(dev).reshape(-1) for a in (ref.X, ref.G, ref.H))
                ws = kernels.svgd_many_workspace(n, x)
                kernels.svgd_many_step(x, g, h, n, d, M.EPS, M.ALPHA, M.FUDGE, ws, repulsion_sign=sign)
                row += list(W.bar_units(ref, dtype, x.cpu().numpy().reshape(n, d).astype(np.float64),
                                        h.cpu().numpy().reshape(n, d).astype(np.float64)))
            Xk, K_ref, _, h_ref, _ = M.kernel_reference(n, d, dtype)
            xk = torch.from_numpy(Xk.copy()).to(dev)
            K, _, bw = kernels.svgd_many_kernel(xk.reshape(-1), n, d, kernels.svgd_many_workspace(n, xk), kernel_gradients=False)
            tol = M.TOL[dtype]
            useK = float(np.max(np.abs(K.cpu().numpy() - K_ref) / (tol["atol"] + tol["rtol"] * np.abs(K_ref))))
            say("%-8s %4d x %-5d  sign +1: %6.3f %6.3f   sign -1: %6.3f %6.3f   K uses %.3f of its bar, h %.3f" % (
                np.dtype(dtype).name, n, d, row[0], row[1], row[2], row[3], useK, abs(float(bw[1]) - h_ref) / h_ref / tol["rtol"]))
if "--no-units" not in sys.argv:
    import svgd_many_cases as M
    import svgd_many_exact_cases as E
    import test_svgd_tile_walk_gpu as W
    to_dev = lambda a: torch.from_numpy(np.array(a)).to(dev)

    def k_use(K, bw, K_ref, h_ref, dtype):
        tol = M.TOL[dtype]
        return (float(np.max(np.abs(K.cpu().numpy() - K_ref) / (tol["atol"] + tol["rtol"] * np.abs(K_ref)))),
                abs(float(bw[1]) - h_ref) / h_ref / tol["rtol"])

    def step_units(ref, n, d, dtype, sign):
        x, g, h = (to_dev(a).reshape(-1) for a in (ref.X, ref.G, ref.H))
        kernels.svgd_many_step(x, g, h, n, d, M.EPS, M.ALPHA, M.FUDGE, kernels.svgd_many_workspace(n, x), repulsion_sign=sign)
        return list(W.bar_units(ref, dtype, x.cpu().numpy().reshape(n, d).astype(np.float64),
                                h.cpu().numpy().reshape(n, d).astype(np.float64)))

    say("---- lattice clouds: the median against the oracle in the case's own dtype, in keys (0: the same bits)")
    for dtype in (M.F32, M.F64):
        for family, n, d in E.LATTICE:
            ref = E.exact_reference(family, n, d, dtype)
            x = to_dev(ref.X)
            K, _, bw = kernels.svgd_many_kernel(x.reshape(-1), n, d, kernels.svgd_many_workspace(n, x), kernel_gradients=False)
            off = int(E.keys(bw.cpu().numpy()[:1])[0]) - int(E.keys(np.asarray(ref.med, dtype).reshape(1))[0])
            f = E.select_facts(ref.D)
            say("%-8s %-8s %4d x %-4d median %-22r %+d keys from the oracle's; %3d distinct keys, count_le - mid = %-6d  "
                "K uses %.3f of its bar, h %.3f" % ((np.dtype(dtype).name, family, n, d, float(bw[0]), off, f.distinct,
                                                     f.count_le - f.mid) + k_use(K, bw, ref.K, ref.h, dtype)))
    say("---- 2 .. 127 particles and translated clouds: units of the displacement bar at c = 1 (X, H)")
    for dtype in (M.F32, M.F64):
        for kind, cases in (("small", E.SMALL), ("translated", E.TRANSLATED)):
            for n, d in cases:
                row = []
                for sign in (1, -1):
                    ref = (M.step_reference(M.Case(n, d, dtype, sign)) if kind == "small"
                           else E.translated_step_reference(n, d, dtype, sign))
                    row += step_units(ref, n, d, dtype, sign)
                Xk, K_ref, _, h_ref, _ = (M.kernel_reference if kind == "small" else E.translated_kernel_reference)(n, d, dtype)
                xk = to_dev(Xk)
                K, _, bw = kernels.svgd_many_kernel(xk.reshape(-1), n, d, kernels.svgd_many_workspace(n, xk), kernel_gradients=False)
                say("%-8s %-10s %4d x %-4d sign +1: %6.3f %6.3f   sign -1: %6.3f %6.3f   K uses %.3f of its bar, h %.3f" % (
                    (np.dtype(dtype).name, kind, n, d, row[0], row[1], row[2], row[3]) + k_use(K, bw, K_ref, h_ref, dtype)))
say("done")
