"""GPU tests of the public sampler API (reference surface) on the HIP path.

Parity bar: with injected noise and the SAME gradients the arena state equals the
oracle bit for bit; with autograd (fp32 GPU) gradients the trajectory tracks the fp64
oracle trajectory within rtol 1e-4 / atol 1e-5 over 100 steps; with
Philox noise chains are seed-reproducible (the reference's own criterion) and sample the
right stationary law.
"""
import os
from itertools import islice

import numpy as np
import pytest
import torch

from pysgmcmc_amd.diagnostics.objective_functions import (
    banana_log_likelihood, gmm1_log_likelihood, gmm2d_log_likelihood, to_negative_log_likelihood)
from pysgmcmc_amd.samplers import RelativisticSGHMCSampler, SGHMCSampler, SGLDSampler
from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TARGETS = {
    "gmm1": (gmm1_log_likelihood, lambda dt: [torch.tensor(0., dtype=dt)]),
    "banana": (banana_log_likelihood, lambda dt: [torch.tensor(0., dtype=dt), torch.tensor(6., dtype=dt)]),
}
CTORS = {"sghmc": SGHMCSampler, "sgld": SGLDSampler, "rsghmc": RelativisticSGHMCSampler}


def _golden_cases():
    d = np.load(os.path.join(GOLDEN, "trajectories.npz"))
    return [str(k) for k in d["cases"]]


@pytest.mark.parametrize("key", _golden_cases())
def test_golden_trajectories_through_sampler_api(gpu, key):
    """All 56 committed trajectories (3 samplers x gmm1/banana x f32/f64 x eps x burn-in)."""
    d = np.load(os.path.join(GOLDEN, "trajectories.npz"))
    sampler, target, dtname, eps, burn = key.split("|")
    dt = torch.float32 if dtname == "float32" else torch.float64
    fn, make = TARGETS[target]
    kw = {} if sampler == "rsghmc" else {"burn_in_steps": int(burn)}
    s = CTORS[sampler](params=make(dt), cost_fun=to_negative_log_likelihood(fn), session=gpu,
                       stepsize_schedule=ConstantStepsizeSchedule(float(eps)), dtype=dt, seed=0, **kw)
    if sampler == "rsghmc":
        s.arena.row("p").copy_(torch.from_numpy(d[key + "|p0"]).to(gpu))
    xi = torch.from_numpy(d[key + "|xi"]).to(gpu)
    s.noise_source = lambda step, n: xi[step]
    want_theta, want_cost = d[key + "|theta"], d[key + "|cost"]
    rtol, atol = (1e-4, 1e-5) if dt == torch.float32 else (1e-9, 1e-12)
    for t, (sample, cost) in enumerate(islice(s, want_theta.shape[0])):
        got = np.array([float(v) for v in sample]) if isinstance(sample, list) else np.array([float(sample)])
        if not np.isfinite(want_theta[t]).all():
            break                                   # eps = 0.1 cases may leave the basin; compared up to there
        assert np.allclose(got, want_theta[t], rtol=rtol, atol=atol), (key, t, got, want_theta[t])
        assert np.isclose(float(cost), want_cost[t], rtol=max(rtol, 1e-5), atol=1e-4 if dt == torch.float32 else 1e-9)


@pytest.mark.parametrize("dtname", ["float32", "float64"])
def test_bnn_golden_trajectory(gpu, dtname):
    """12 SGHMC steps of the 5 252-parameter sinc BNN: seed-matched minibatch windows, fused
    analytic cost path on the GPU, injected noise. Compared with the committed trajectory
    (fp64 CPU gradients): f32 within 2e-4 relative to max|theta|, f64 within 1e-9."""
    from pysgmcmc_amd.data_batches import Placeholder, generate_batches
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost
    d = np.load(os.path.join(GOLDEN, "bnn_trajectory.npz"))
    dt = torch.float32 if dtname == "float32" else torch.float64
    shapes = [(1, 50), (50,), (50, 50), (50,), (50, 50), (50,), (50, 1), (1,), (1, 1)]
    theta0 = d["theta0"]
    params, off = [], 0
    for shp in shapes:
        k = int(np.prod(shp))
        params.append(torch.tensor(theta0[off:off + k].reshape(shp), dtype=dt, device=gpu))
        off += k
    xp, yp = Placeholder(dtype=dt, device=gpu), Placeholder(dtype=dt, device=gpu)
    # fused + prior folded into the update kernel / fused + prior in the GEMM epilogue / plain autograd
    for fused, fold in ((True, True), (True, False), (False, False)):
        ps = [p.clone() for p in params]
        cost = BNNCost(xp, yp, batch_size=20, n_examples=100, fold_prior=fold)
        cost_fun = cost if fused else (lambda p, *_: cost(p))
        s = SGHMCSampler(params=ps, cost_fun=cost_fun,
                         batch_generator=generate_batches(d["X"], d["y"], xp, yp, batch_size=20, seed=1),
                         stepsize_schedule=ConstantStepsizeSchedule(0.01), burn_in_steps=6, mdecay=0.05,
                         scale_grad=100.0, session=gpu, dtype=dt, seed=0)
        s.sample_format = "view"
        nrng = np.random.default_rng(4321)
        xis = [nrng.normal(size=theta0.size).astype(dtname) for _ in range(12)]
        s.noise_source = lambda step, n: torch.from_numpy(xis[step]).to(gpu)
        want = d[dtname + "|theta"]
        tol = 2e-4 if dt == torch.float32 else 1e-9
        for t in range(12):
            theta_prev = s.arena.row("theta").cpu().numpy().astype(np.float64)
            _, c = next(s)
            got = s.arena.row("theta").cpu().numpy()
            assert np.abs(got - want[t]).max() <= tol * np.abs(want[t]).max(), (fused, fold, t)
            assert np.isclose(float(c), d[dtname + "|cost"][t], rtol=1e-4 if dt == torch.float32 else 1e-9)
            assert (s._grad_decay > 0) == (fused and fold)
            full_grad = s.arena.row("grad").cpu().numpy() + s._grad_decay * theta_prev
            gerr = np.abs(full_grad - d[dtname + "|grad"][t]).max()
            assert gerr <= (2e-4 if dt == torch.float32 else 1e-10) * np.abs(d[dtname + "|grad"][t]).max()


@pytest.mark.parametrize("name", ["sghmc", "sgld", "rsghmc"])
@pytest.mark.parametrize("target", ["gmm1", "banana"])
def test_seed_reproducibility_philox(gpu, name, target):
    """The reference's sampler test (tests/samplers/sampler_testing.py:29-59) on the HIP path."""
    fn, make = TARGETS[target]
    # like the reference's test the seed and the chain length are arbitrary; drawn from a SEEDED generator so that
    # a red run can be reproduced
    import zlib
    rng = np.random.RandomState(zlib.crc32(("%s|%s" % (name, target)).encode()))
    seed = int(rng.randint(0, 2 ** 31 - 1))
    n_samples = int(rng.randint(1, 100))

    def fresh_chain(sd):
        s = CTORS[name](params=make(torch.float32), cost_fun=to_negative_log_likelihood(fn), seed=sd,
                        session=gpu, dtype=torch.float32)
        return list(islice(s, n_samples))
    c1, c2, c3 = fresh_chain(seed), fresh_chain(seed), fresh_chain(seed + 1)
    for (s1, k1), (s2, k2) in zip(c1, c2):
        assert np.allclose(k1, k2) and np.allclose(s1, s2)
        assert np.array_equal(np.asarray(s1), np.asarray(s2))
    assert not np.array_equal(np.asarray(c1[-1][0]), np.asarray(c3[-1][0]))
    assert all(np.isfinite(np.asarray(s)).all() for s, _ in c1)


def test_stationary_distribution_standard_normal(gpu):
    """SGHMC and SGLD (frozen preconditioner after a 200-step burn-in) on U(x) = x^2/2 over 4096
    independent coordinates sample N(0, ~1): pooled variance within 8 % (the discretisation bias of
    SGLD at h = eps*minv is 1/(1-h/2) ~ 1.03), |mean| small, kurtosis ~ 3 -- a statistical check the
    reference never had. (With burn_in_steps=0 the reference's perpetual adaptation makes the step
    state-dependent and inflates the variance to ~1.8; that is the algorithm, not the kernel: the
    CPU oracle gives the same 1.8066.)"""
    n = 4096
    for ctor, kw, steps in ((SGHMCSampler, dict(mdecay=0.05), 3000), (SGLDSampler, {}, 6000)):
        x = torch.zeros(n, dtype=torch.float32, device=gpu)
        s = ctor(params=[x], cost_fun=lambda p: 0.5 * (p[0] ** 2).sum(), burn_in_steps=200,
                 stepsize_schedule=ConstantStepsizeSchedule(0.05), session=gpu, dtype=torch.float32, seed=3, **kw)
        s.sample_format = "view"
        acc, acc2, acc4, cnt = 0.0, 0.0, 0.0, 0
        for t, (sample, _) in enumerate(islice(s, steps)):
            if t >= steps // 3 and t % 20 == 0:
                v = sample.double()
                acc += v.mean().item(); acc2 += (v ** 2).mean().item(); acc4 += (v ** 4).mean().item(); cnt += 1
        mean, var, m4 = acc / cnt, acc2 / cnt, acc4 / cnt
        assert abs(mean) < 0.05, (ctor.__name__, mean)
        assert abs(var - 1.0) < 0.08, (ctor.__name__, var)
        assert abs(m4 / var ** 2 - 3.0) < 0.3, (ctor.__name__, m4)


def test_config0_sgld_2d_gaussian_mixture(gpu):
    """BASELINE.json configs[0]: SGLD on the 2-D Gaussian mixture (modes (-5,0), (0,0), (5,0), unit
    variance), reference defaults (A=1, scale_grad=1, burn_in_steps=3000, eps=0.01), fp32, seed 1,
    10 000 steps. Mode hopping is slow at this stepsize, so the assertions are on what is stable:
    finite, confined, and unit-scale spread around the nearest mode in both coordinates."""
    x = torch.tensor([0.0, 0.0], dtype=torch.float32)
    s = SGLDSampler(params=[x], cost_fun=to_negative_log_likelihood(gmm2d_log_likelihood), session=gpu,
                    dtype=torch.float32, seed=1)
    s.sample_format = "view"
    xs = torch.stack([smp.clone() for smp, _ in islice(s, 10000)])[3000:].double().cpu()
    assert not s.is_burning_in and torch.isfinite(xs).all()
    assert xs[:, 0].abs().max().item() < 10.0 and xs[:, 1].abs().max().item() < 6.0
    centers = torch.tensor([-5.0, 0.0, 5.0], dtype=torch.float64)
    resid = xs[:, 0:1] - centers[None, :]
    nearest = resid.gather(1, resid.abs().argmin(dim=1, keepdim=True)).squeeze(1)
    assert 0.5 < nearest.var().item() < 1.5
    assert 0.6 < xs[:, 1].var().item() < 1.7


def test_minv_summary_and_device_counter(gpu):
    from pysgmcmc_amd import kernels
    x = torch.randn(10000, device=gpu)
    s = SGHMCSampler(params=[x], cost_fun=lambda p: (p[0] ** 4).sum(), burn_in_steps=20, session=gpu,
                     dtype=torch.float32, seed=0)
    list(islice(s, 25))
    summ = s.minv_summary
    mv = np.concatenate([m.ravel() for m in s.minv]).astype(np.float64)
    assert np.isclose(summ["mean"], mv.mean(), rtol=1e-6) and summ["min"] == mv.min() and summ["max"] == mv.max()
    # device-resident step counter: step=5 by value == step=2 + counter 3
    a = torch.empty(1001, device=gpu)
    b = torch.empty(1001, device=gpu)
    ctr = torch.zeros(1, dtype=torch.int64, device=gpu)
    kernels.counter_add(ctr, 3)
    kernels.philox_normal(a, 9, 5)
    kernels.philox_normal(b, 9, 2, step_dev=ctr)
    assert torch.equal(a, b) and int(ctr.item()) == 3


def test_hip_graph_capture_of_update_kernel(gpu):
    """The launch is legal under stream capture; replays advance the noise via the device counter."""
    from pysgmcmc_amd import kernels
    n = 100000
    theta = torch.zeros(n, device=gpu)
    V = torch.zeros(n, device=gpu)
    grad = torch.zeros(n, device=gpu)
    minv = torch.ones(n, device=gpu)
    ctr = torch.zeros(1, dtype=torch.int64, device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        kernels.sghmc_step(theta, V, grad, None, None, None, minv, None, 0.01, 1.0, 0.05, False, seed=4, step=0,
                           step_dev=ctr)
    torch.cuda.current_stream().wait_stream(side)
    theta.zero_(); V.zero_()
    from pysgmcmc_amd.samplers.base_classes import graph_capture
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        kernels.sghmc_step(theta, V, grad, None, None, None, minv, None, 0.01, 1.0, 0.05, False, seed=4, step=0,
                           step_dev=ctr)
        kernels.counter_add(ctr, 1)
    th2, V2 = torch.zeros(n, device=gpu), torch.zeros(n, device=gpu)
    for t in range(3):
        g.replay()
        kernels.sghmc_step(th2, V2, grad, None, None, None, minv, None, 0.01, 1.0, 0.05, False, seed=4, step=t)
    torch.cuda.synchronize()
    assert int(ctr.item()) == 3
    assert torch.equal(theta, th2) and torch.equal(V, V2)


def test_hip_graph_mode_equals_eager(gpu):
    """use_hip_graph: one captured graph per (eps, phase) replayed each step gives the SAME chain as
    eager stepping (Philox step comes from the device counter), across the burn-in -> frozen switch,
    and the fused-statistics weight-prior value equals the recomputed one."""
    from pysgmcmc_amd.data_batches import Placeholder, generate_batches
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
    rng = np.random.RandomState(0)
    X, y = rng.rand(200, 3), rng.rand(200)

    def chain(graph):
        xp, yp = Placeholder(dtype=torch.float32, device=gpu), Placeholder(dtype=torch.float32, device=gpu)
        params = init_mlp_params(3, hidden=(32, 32), seed=5, dtype=torch.float32, device=gpu)
        s = SGHMCSampler(params=params, cost_fun=BNNCost(xp, yp, batch_size=16, n_examples=200),
                         batch_generator=generate_batches(X, y, xp, yp, batch_size=16, seed=2),
                         stepsize_schedule=ConstantStepsizeSchedule(0.01), burn_in_steps=5, scale_grad=200.0,
                         session=gpu, dtype=torch.float32, seed=9)
        s.sample_format = "view"
        s.use_hip_graph = graph
        costs = [float(c) for _, c in islice(s, 12)]
        return s, costs
    eager, ce = chain(False)
    split, cs = chain(True)                                           # cost graph + direct update launch
    graph, cg = chain("full")                                         # everything in the graph
    assert len(split._graphs) == 1
    assert len(graph._graphs) == 2                                    # burn-in graph + frozen graph
    for other in (split, graph):
        assert torch.equal(eager.arena.row("theta"), other.arena.row("theta"))
        assert torch.equal(eager.arena.row("V"), other.arena.row("V"))
    assert np.allclose(ce, cg, rtol=1e-6) and np.allclose(ce, cs, rtol=1e-6)
    assert graph.n_iterations == 12 and int(graph._step_ctr.item()) == 12
    st = graph.stats
    assert np.isclose(st["theta_sq"], (graph.arena.row("theta").double() ** 2).sum().item(), rtol=5e-7)
    assert np.isclose(st["momentum_sq"], (graph.arena.row("V").double() ** 2).sum().item(), rtol=5e-7)


def test_full_graph_mode_follows_a_stepsize_schedule_through_the_device_scalars(gpu):
    """``use_hip_graph = "full"`` captures the update too. A captured launch replays its arguments, so the
    stepsize-derived scalars live in a device block (``StepOpts.scalars_dev``) that a 1-thread launch refreshes when the
    schedule moves: a SCHEDULED stepsize (BurnInRampStepsizeSchedule, configs[4]) replays ONE graph per phase, the
    user's ``use_hip_graph`` attribute is never touched, the chain equals the eager chain bit for bit and the stepsizes
    are the schedule's."""
    from pysgmcmc_amd.data_batches import Placeholder, generate_batches
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
    from pysgmcmc_amd.stepsize_schedules import BurnInRampStepsizeSchedule
    rng = np.random.RandomState(0)
    X, y = rng.rand(200, 3), rng.rand(200)

    def chain(ctor, graph, **kw):
        xp, yp = Placeholder(dtype=torch.float32, device=gpu), Placeholder(dtype=torch.float32, device=gpu)
        params = init_mlp_params(3, hidden=(32, 32), seed=5, dtype=torch.float32, device=gpu)
        s = ctor(params=params, cost_fun=BNNCost(xp, yp, batch_size=16, n_examples=200),
                 batch_generator=generate_batches(X, y, xp, yp, batch_size=16, seed=2),
                 stepsize_schedule=BurnInRampStepsizeSchedule(1e-4, 1e-2, burn_in_steps=10),
                 session=gpu, dtype=torch.float32, seed=9, **kw)
        s.sample_format = "view"
        s.use_hip_graph = graph
        eps = []
        for _ in range(16):
            next(s)
            eps.append(float(s.epsilon))
        return s, eps
    for ctor, kw, rows, n_graphs in ((SGLDSampler, dict(burn_in_steps=10, scale_grad=200.0), ("theta", "minv"), 2),
                                     (SGHMCSampler, dict(burn_in_steps=10, scale_grad=200.0), ("theta", "V", "minv"), 2),
                                     (RelativisticSGHMCSampler, {}, ("theta", "p"), 1)):
        eager, e0 = chain(ctor, False, **kw)
        full, e1 = chain(ctor, "full", **kw)
        assert e0 == e1 and len(set(e0[:11])) == 11 and e0[10] == e0[-1] == 1e-2      # ramp, then constant
        assert full.use_hip_graph == "full" and len(full._graphs) == n_graphs         # one graph per phase, attribute untouched
        for row in rows:
            assert torch.equal(eager.arena.row(row), full.arena.row(row)), (ctor.__name__, row)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_bnn_cost_path_hip_equals_autograd(gpu, dt):
    """The MI355X cost path (GEMMs + loss-head + tanh-backward kernels writing into the arena)
    against plain autograd of the same NLL: cost, every gradient tensor, mse."""
    from pysgmcmc_amd.data_batches import Placeholder
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
    torch.manual_seed(0)
    for hidden, B, D in (((50, 50, 50), 20, 1), ((64, 32), 33, 5), ((128,), 256, 17)):
        params = init_mlp_params(D, hidden=hidden, seed=1, dtype=dt, device=gpu)
        for p in params[1::2]:
            p.normal_()
        xp = Placeholder().feed(torch.randn(B, D, dtype=dt, device=gpu))
        yp = Placeholder().feed(torch.randn(B, 1, dtype=dt, device=gpu))
        for fold in (False, True):
            c = BNNCost(xp, yp, batch_size=20, n_examples=1000, fold_prior=fold)
            ps = [p.clone().requires_grad_(True) for p in params]
            cost = c(ps)
            mse_ref = float(c.last_mse)
            grads = torch.autograd.grad(cost, ps)
            gv = [torch.full_like(p, float("nan")) for p in params]
            sumsq = sum((p.double() ** 2).sum() for p in params)
            for ts in (None, sumsq):
                cost2 = c.cost_and_grad(params, gv, theta_sumsq=ts)
                assert (c.grad_theta_coef > 0) == fold
                tol = 2e-5 if dt == torch.float32 else 1e-11
                assert abs(float(cost2) - float(cost.detach())) <= tol * abs(float(cost.detach()))
                assert abs(float(c.last_mse) - mse_ref) <= tol * mse_ref
                for a, b, p in zip(grads, gv, params):
                    full = b + c.grad_theta_coef * p           # the term the update kernel adds when folded
                    assert float((a - full).abs().max()) <= tol * float(a.abs().max()) + (1e-9 if dt == torch.float32 else 1e-15)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_bias_tanh_kernels(gpu, dt):
    """``bias_tanh`` (hidden-layer activation after a plain forward GEMM) and ``tanh_rowdot(bias=)`` against torch, for row
    pitches with and without 16-byte accesses; ``tanh_rowdot`` without a bias is unchanged."""
    from pysgmcmc_amd import kernels
    g = torch.Generator(device=gpu).manual_seed(3)
    tol = 1e-6 if dt == torch.float32 else 1e-14
    for rows, cols in ((256, 2048), (7, 50), (1, 4), (33, 130)):
        a = torch.randn(rows, cols, device=gpu, dtype=dt, generator=g)
        b = torch.randn(cols, device=gpu, dtype=dt, generator=g)
        w = torch.randn(cols, device=gpu, dtype=dt, generator=g)
        ref = torch.tanh(a + b)
        out = kernels.bias_tanh(a.clone(), b)
        assert (out - ref).abs().max().item() <= tol
        h, dot = a.clone(), torch.empty(rows, device=gpu, dtype=dt)
        kernels.tanh_rowdot(h, w, dot, bias=b)
        assert torch.equal(h, out)                                   # the same arithmetic in both kernels
        assert (dot - ref @ w).abs().max().item() <= 50 * tol * cols ** 0.5
        h2, dot2 = a.clone(), torch.empty(rows, device=gpu, dtype=dt)
        kernels.tanh_rowdot(h2, w, dot2)
        assert (h2 - torch.tanh(a)).abs().max().item() <= tol
    with pytest.raises(ValueError):
        kernels.bias_tanh(torch.zeros(4, 8, device=gpu, dtype=dt), torch.zeros(7, device=gpu, dtype=dt))


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_fused_head_launch_equals_separate_kernels(gpu, dt):
    """The loss head folded into the last layer's backward launch (the plan of ``BNNCost`` whenever the previous step kernel's
    sum(theta^2) records are at hand; slices from the rowdot launch) against the separate head + backward kernels (the plan
    without them): every gradient bit-equal, cost / mse to the last bits (sum(theta^2) is added in another order), for batches
    smaller and larger than the 16 slices and ragged widths."""
    from pysgmcmc_amd import kernels
    from pysgmcmc_amd.data_batches import Placeholder
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
    torch.manual_seed(1)
    for hidden, B, D in (((50, 50, 50), 20, 1), ((2048, 2048), 256, 784), ((70,), 5, 3), ((33, 17), 300, 4)):
        params = init_mlp_params(D, hidden=hidden, seed=2, dtype=dt, device=gpu)
        for p in params[1::2]:
            p.normal_()
        n = sum(p.numel() for p in params)
        # a statistics workspace like the one a step kernel leaves: many partials
        flat = torch.cat([p.reshape(-1) for p in params])
        st = kernels.StepStats(n, gpu)
        zeros = torch.zeros_like(flat)
        kernels.rsghmc_step(flat.clone(), zeros.clone(), zeros, 0.0, 1.0, 1.0, 0.0, 0.0, xi=zeros, stats=st)   # theta' = theta
        xp = Placeholder().feed(torch.randn(B, D, dtype=dt, device=gpu))
        yp = Placeholder().feed(torch.randn(B, 1, dtype=dt, device=gpu))
        for fold in (False, True):
            outs = []
            for fuse in (False, True):
                c = BNNCost(xp, yp, batch_size=20, n_examples=1000, fold_prior=fold)
                c.fused_layers = False       # (the fused last hidden layer needs the fused head: it would change the products between the two)
                gv = [torch.full_like(p, float("nan")) for p in params]
                cost = c.cost_and_grad(params, gv, theta_sumsq_partials=st.workspace if fuse else None)
                assert c.plan_summary(params, gv, st.workspace if fuse else None)["head"] == ("head+last_layer_backward" if fuse else "head")
                outs.append((float(cost), float(c.last_mse), [g.clone() for g in gv]))
            (c0, m0, g0), (c1, m1, g1) = outs
            rel = 1e-6 if dt == torch.float32 else 1e-14
            assert abs(c0 - c1) <= rel * abs(c0) and abs(m0 - m1) <= rel * abs(m0), (hidden, B, fold, c0, c1)
            for a, b in zip(g0, g1):
                assert torch.isfinite(b).all() and torch.equal(a, b), (hidden, B, fold)


def test_checkpoint_resume_with_minibatches_and_schedule(gpu):
    """A BNN chain with a minibatch generator and a stepsize ramp, checkpointed across the burn-in -> frozen switch and
    resumed in a FRESH sampler: same windows, same stepsizes, same Philox stream -> bit-equal chain (eager and graph)."""
    from pysgmcmc_amd.data_batches import Placeholder, generate_batches
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
    from pysgmcmc_amd.stepsize_schedules import BurnInRampStepsizeSchedule
    rng = np.random.RandomState(0)
    X, y = rng.rand(300, 4), rng.rand(300)

    def chain(graph):
        xp, yp = Placeholder(dtype=torch.float32, device=gpu), Placeholder(dtype=torch.float32, device=gpu)
        params = init_mlp_params(4, hidden=(32, 32), seed=5, dtype=torch.float32, device=gpu)
        s = SGLDSampler(params=params, cost_fun=BNNCost(xp, yp, batch_size=16, n_examples=300),
                        batch_generator=generate_batches(X, y, xp, yp, batch_size=16, seed=2),
                        stepsize_schedule=BurnInRampStepsizeSchedule(1e-4, 1e-2, burn_in_steps=9), burn_in_steps=9,
                        scale_grad=300.0, session=gpu, dtype=torch.float32, seed=9)
        s.sample_format = "view"
        s.use_hip_graph = graph
        return s
    for graph in (False, True):
        full = chain(graph)
        costs = [float(next(full)[1]) for _ in range(20)]
        a = chain(graph)
        for _ in range(6):
            next(a)
        ckpt = a.state_dict()
        assert "batch_generator" in ckpt and ckpt["stepsize_schedule"] == {"t": 6}
        b = chain(graph)
        b.load_state_dict(ckpt)
        resumed = [float(next(b)[1]) for _ in range(14)]
        assert resumed == costs[6:], (graph, resumed[:3], costs[6:9])
        for row in ("theta", "minv", "tau"):
            assert torch.equal(b.arena.row(row), full.arena.row(row)), (graph, row)
        assert b.n_iterations == 20 and not b.is_burning_in


def test_update_kernel_timer_through_the_sampler(gpu):
    """pysgmcmc_amd.profiling.UpdateKernelTimer attached to a sampler: one kernel-timestamp pair per update launch in
    eager and cost-graph stepping, none while disabled; the chain is unchanged by the instrumentation."""
    from pysgmcmc_amd.profiling import UpdateKernelTimer

    def chain(graph, timed, every=1):
        s = SGHMCSampler(params=[torch.zeros(500_000, device=gpu)], cost_fun=lambda p: 0.5 * (p[0] ** 2).sum(),
                         burn_in_steps=3, session=gpu, dtype=torch.float32, seed=4)
        s.sample_format = "view"
        s.use_hip_graph = graph
        t = UpdateKernelTimer(reserve=4, bracket=True)
        t.sample_every = every
        s.kernel_timer = t
        for _ in range(3):
            next(s)                                   # not enabled yet: nothing recorded
        assert not t.kevents
        t.enabled = timed
        for _ in range(7):
            next(s)
        torch.cuda.synchronize()
        return s, t
    ref, _ = chain(False, False)
    for graph in (False, True):
        s, t = chain(graph, True)
        us, steps, br = t.kernel_us(), t.step_us(), t.bracket_us()
        assert us.shape == (7,) and steps.shape == (6,) and br.shape == (7,)
        assert np.all(us > 1.0) and np.all(us < 500.0) and np.all(steps >= us[1:] * 0.99)
        assert torch.equal(s.arena.row("theta"), ref.arena.row("theta"))
    # sample_every = 3: only the launches of steps 3, 6, 9 of the enabled steps 3 .. 9 carry events (a timed launch costs device time)
    s, t = chain(True, True, every=3)
    assert [tag[0] for tag in t.tags] == [3, 6, 9] and t.kernel_us().shape == (3,)
    assert torch.equal(s.arena.row("theta"), ref.arena.row("theta"))
    assert UpdateKernelTimer.empty_bracket_us(20) >= 0.0


def test_concurrent_chains_on_one_gpu_equal_the_chains_alone(gpu):
    """``ConcurrentChains``: independent chains on their own streams (own hipGraphs), enqueued round-robin, compute exactly
    what they compute one after the other -- eager and graph stepping, through the burn-in switch."""
    from pysgmcmc_amd.data_batches import Placeholder, generate_batches
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
    from pysgmcmc_amd.samplers import ConcurrentChains
    from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule
    rng = np.random.RandomState(0)
    X, y = rng.rand(500, 12), rng.rand(500)

    def chain(k, graph):
        xp, yp = Placeholder(dtype=torch.float32, device=gpu), Placeholder(dtype=torch.float32, device=gpu)
        params = init_mlp_params(12, hidden=(64, 128, 64), seed=10 + k, dtype=torch.float32, device=gpu)
        s = SGHMCSampler(params=params, cost_fun=BNNCost(xp, yp, batch_size=32, n_examples=500),
                         batch_generator=generate_batches(X, y, xp, yp, batch_size=32, seed=k),
                         stepsize_schedule=ConstantStepsizeSchedule(0.01), burn_in_steps=5, scale_grad=500.0, session=gpu,
                         dtype=torch.float32, seed=20 + k)
        s.sample_format = "view"
        s.use_hip_graph = graph
        return s
    for graph in (False, True):
        alone = [chain(k, graph) for k in range(3)]
        costs_alone = [[float(next(s)[1]) for _ in range(14)] for s in alone]
        group = ConcurrentChains([chain(k, graph) for k in range(3)])
        costs = [[] for _ in range(3)]
        for i in range(14):
            results = next(group)
            if i % 3 == 0:
                group.join()                  # the cost is a view of the chain's buffer: read it before the next step
                for k, (_, cost) in enumerate(results):
                    costs[k].append((i, float(cost)))
        group.join()
        torch.cuda.synchronize()
        assert len(group) == 3 and len({st.cuda_stream for st in group.streams}) == 3
        for k in range(3):
            assert costs[k] == [(i, costs_alone[k][i]) for i in range(0, 14, 3)]
            for row in ("theta", "V", "minv"):
                assert torch.equal(group.samplers[k].arena.row(row), alone[k].arena.row(row)), (graph, k, row)
    with pytest.raises(ValueError):
        ConcurrentChains([])


def test_concurrent_chains_of_different_sampler_classes(gpu):
    """Chains of different samplers and dtypes (SGHMC f32 graph, SGLD f64 eager, relativistic SGHMC f32 full-graph) stepped as
    one ``ConcurrentChains`` group equal the chains alone; ``steps()`` = fork + run + join."""
    from pysgmcmc_amd.samplers import ConcurrentChains, RelativisticSGHMCSampler, SGLDSampler

    def make():
        cost = lambda p: 0.5 * (p[0] ** 2).sum() + 0.25 * (p[0] ** 4).sum()
        a = SGHMCSampler(params=[torch.linspace(-1, 1, 5003, device=gpu)], cost_fun=cost, burn_in_steps=6, session=gpu,
                         dtype=torch.float32, seed=1)
        b = SGLDSampler(params=[torch.linspace(-2, 2, 777, device=gpu, dtype=torch.float64)], cost_fun=cost, burn_in_steps=4,
                        session=gpu, dtype=torch.float64, seed=2)
        c = RelativisticSGHMCSampler(params=[torch.linspace(-1, 1, 1024, device=gpu)], cost_fun=cost, session=gpu,
                                     dtype=torch.float32, seed=3)
        for s, mode in ((a, True), (b, False), (c, "full")):
            s.sample_format = "view"
            s.use_hip_graph = mode
        return [a, b, c]
    alone = make()
    for s in alone:
        for _ in range(15):
            next(s)
    group = ConcurrentChains(make())
    group.steps(7)
    snapshot = [s.arena.row("theta").clone() for s in group.samplers]        # on the caller's stream, after the join
    group.steps(8)                                                            # fork: the chains wait for the clones
    torch.cuda.synchronize()
    for s, ref, snap in zip(group.samplers, alone, snapshot):
        assert torch.equal(s.arena.row("theta"), ref.arena.row("theta")) and s.n_iterations == 15
        assert not torch.equal(snap, s.arena.row("theta")) and torch.isfinite(snap).all()


def test_rhat_of_chains_that_share_a_gpu(gpu):
    """``RhatExchange.start([moments, ...])`` with no process group: R-hat over the local chains (fused Welford moments of
    ``ConcurrentChains``) equals the formula on the chains' explicit samples."""
    from pysgmcmc_amd.diagnostics.sampler_diagnostics import ChainMoments, RhatExchange, gelman_rubin_from_chains
    from pysgmcmc_amd.samplers import ConcurrentChains
    n = 1001
    chains = [SGHMCSampler(params=[torch.full((n,), 2.0 * k - 2.0, device=gpu)], cost_fun=lambda p: 0.5 * (p[0] ** 2).sum(),
                           burn_in_steps=30, session=gpu, dtype=torch.float32, seed=40 + k) for k in range(3)]
    moments = [ChainMoments(n, gpu) for _ in chains]
    for s in chains:
        s.sample_format = "view"
        s.use_hip_graph = True
    group = ConcurrentChains(chains)
    group.run(60)
    for s, m in zip(chains, moments):
        s.attach_moments(m, every=2)
    kept = [[] for _ in chains]
    for i in range(120):
        next(group)
        if i % 2 == 1:                                     # the steps whose update launch folded theta' into the moments
            for k, (s, st) in enumerate(zip(chains, group.streams)):
                with torch.cuda.stream(st):
                    kept[k].append(s.arena.row("theta").clone())
    group.join()
    assert all(m.count == 60 for m in moments)
    ex = RhatExchange(n, gpu, mode="allreduce")
    ex.start(moments)
    rhat, summ = ex.finish(with_summary=True)
    want = gelman_rubin_from_chains(torch.stack([torch.stack(c) for c in kept]))
    assert torch.allclose(rhat.double().cpu(), want.cpu(), rtol=2e-4) and np.isclose(summ["max"], want.max().item(), rtol=2e-4)
    with pytest.raises(RuntimeError):
        ex.start(moments[0])                               # one chain, no process group: no R-hat


def test_draw_noise_sample_api(gpu):
    s = SGHMCSampler(params=[torch.zeros(3, 2)], cost_fun=lambda p: (p[0] ** 2).sum(), session=gpu,
                     dtype=torch.float32, seed=4)
    z = s._draw_noise_sample(sigma=2.0, shape=(1000, 1))
    z2 = s._draw_noise_sample(sigma=2.0, shape=(1000, 1))
    assert z.shape == (1000, 1) and torch.equal(z, z2) and abs(z.std().item() - 2.0) < 0.2


def test_checkpoint_resume_and_numpy_format_on_gpu(gpu):
    """state_dict/load_state_dict resume a Philox chain bit-exactly (the reference cannot checkpoint);
    the default "numpy" sample format returns host copies that do not alias the arena."""
    mk = lambda: SGHMCSampler(params=[torch.zeros(1000), torch.ones(7, 3)],
                              cost_fun=lambda p: (p[0] ** 2).sum() + ((p[1] - 1) ** 4).sum(),
                              session=gpu, dtype=torch.float32, seed=21, burn_in_steps=6)
    s = mk()
    out = list(islice(s, 9))
    assert isinstance(out[-1][0][0], np.ndarray) and out[-1][0][1].shape == (7, 3)
    keep = out[-1][0][0].copy()
    state = s.state_dict()
    tail = [smp for smp, _ in islice(s, 5)]
    assert np.array_equal(keep, out[-1][0][0])                      # earlier samples are untouched copies
    s2 = mk()
    s2.load_state_dict(state)
    tail2 = [smp for smp, _ in islice(s2, 5)]
    for a, b in zip(tail, tail2):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert s2.n_iterations == 14 and not s2.is_burning_in


def test_materialize_r_and_relativistic_on_gpu(gpu, oracle):
    """`materialize_r` writes the reference's R_i = 1/(tau+1) variable too; the relativistic sampler
    draws its initial momenta from the relativistic law (seeded) and steps finitely."""
    x = torch.randn(5000, device=gpu)
    s = SGHMCSampler(params=[x], cost_fun=lambda p: 0.5 * (p[0] ** 2).sum(), session=gpu, dtype=torch.float32,
                     seed=2, burn_in_steps=50)
    s.materialize_r = True
    s.sample_format = "view"
    tau_before = None
    for _ in range(10):
        tau_before = s.arena.row("tau").clone()
        next(s)
    r = s.arena._rows["r"]
    assert torch.equal(r, 1.0 / (tau_before + 1.0))
    rs = [RelativisticSGHMCSampler(params=[torch.zeros(200000)], cost_fun=lambda p: 0.5 * (p[0] ** 2).sum(),
                                   session=gpu, dtype=torch.float32, seed=sd) for sd in (5, 5, 6)]
    p0 = [r_.arena.row("p").clone() for r_ in rs]
    assert torch.equal(p0[0], p0[1]) and not torch.equal(p0[0], p0[2])
    assert abs(p0[0].double().std().item() - 1.6430) < 0.02 and abs(p0[0].double().mean().item()) < 0.02
    rs[0].sample_format = "view"
    smp = [v for v, _ in islice(rs[0], 20)][-1]
    assert torch.isfinite(smp).all() and smp.abs().max().item() < 1.0


def test_torch_module_parameters_autograd_path(gpu):
    """Drop-in use from PyTorch: the parameters of an nn.Module are adopted into the arena (the module keeps
    working, its tensors alias theta), the cost is an ordinary autograd graph; chains are seed-reproducible
    and the posterior samples fit the data."""
    torch.manual_seed(0)
    X = torch.linspace(-1, 1, 64, device=gpu).reshape(-1, 1)
    Y = 2.0 * X - 0.5

    def run(seed):
        torch.manual_seed(1)
        net = torch.nn.Sequential(torch.nn.Linear(1, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1)).to(gpu)
        params = list(net.parameters())
        cost = lambda p: 0.5 * ((net(X) - Y) ** 2).sum() / 0.01 + 0.5 * sum((q ** 2).sum() for q in p)
        s = SGHMCSampler(params=params, cost_fun=cost, session=gpu, dtype=torch.float32, seed=seed,
                         burn_in_steps=300, stepsize_schedule=ConstantStepsizeSchedule(0.003), mdecay=0.05)
        s.sample_format = "view"
        for p, v in zip(params, s.arena.views("theta")):
            assert p.data_ptr() == v.data_ptr()                       # module tensors alias the arena
        costs = [float(c) for _, c in islice(s, 1500)]
        with torch.no_grad():
            mse = float(((net(X) - Y) ** 2).mean())
        return costs, mse, s.arena.row("theta").clone()
    c1, mse1, th1 = run(3)
    c2, mse2, th2 = run(3)
    assert torch.equal(th1, th2) and c1 == c2
    assert np.mean(c1[-200:]) < 0.05 * c1[0] and mse1 < 0.05


def test_numpy_format_large_chain_uses_fresh_host_buffers(gpu):
    """> 1 MiB chains copy through page-locked buffers: each sample owns its buffer (kept samples are never
    overwritten by later steps) and equals the device state at that step."""
    x = torch.zeros(600_000, device=gpu)
    s = SGHMCSampler(params=[x], cost_fun=lambda p: 0.5 * (p[0] ** 2).sum(), session=gpu, dtype=torch.float32,
                     seed=8, burn_in_steps=2)
    kept, snaps = [], []
    for sample, _ in islice(s, 5):
        kept.append(sample)
        snaps.append(s.arena.row("theta").cpu().numpy().copy())
    for a, b in zip(kept, snaps):
        assert isinstance(a, np.ndarray) and np.array_equal(a, b)
    assert not np.array_equal(kept[0], kept[-1])


@pytest.mark.parametrize("graph", [False, True])
def test_window_prefetch_in_the_update_launch_gives_the_same_chain(gpu, graph):
    """Round 6: the NEXT step's minibatch window is gathered by THIS step's update launch (``prefetch_windows``, the default)
    instead of by a launch of its own at the start of the next step -- same windows (the generator's draws, one step early), same
    chain bit for bit, in eager and in graph stepping; a step called with a feed_dict in between, whole-step kernel launches after
    ``next()`` and a checkpoint taken while a window is pending all see the generator's sequence unchanged."""
    from pysgmcmc_amd.data_batches import Placeholder, generate_batches
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
    rng = np.random.RandomState(0)
    X, y = rng.rand(300, 4), rng.rand(300)

    def chain(prefetch):
        xp, yp = Placeholder(dtype=torch.float32, device=gpu), Placeholder(dtype=torch.float32, device=gpu)
        params = init_mlp_params(4, hidden=(32, 32), seed=5, dtype=torch.float32, device=gpu)
        s = SGHMCSampler(params=params, cost_fun=BNNCost(xp, yp, batch_size=16, n_examples=300),
                         batch_generator=generate_batches(X, y, xp, yp, batch_size=16, seed=2),
                         stepsize_schedule=ConstantStepsizeSchedule(1e-2), burn_in_steps=5,
                         scale_grad=300.0, session=gpu, dtype=torch.float32, seed=9)
        s.sample_format, s.use_hip_graph, s.prefetch_windows = "view", graph, prefetch
        return s, xp, yp
    runs = {}
    for prefetch in (False, True):
        s, xp, yp = chain(prefetch)
        costs = [float(next(s)[1]) for _ in range(8)]
        assert (s._pending_window is not None) == prefetch            # a window is waiting in the feed buffers
        if prefetch:
            assert s._pending_window[1] is True
        # a step given a feed_dict (which the generator's batch overrides, pysgmcmc/samplers/base_classes.py:287-291: the pending
        # window must be taken, not a fresh draw): the generator's sequence goes on unchanged
        xe = torch.full((16, 4), 0.25, device=gpu)
        ye = torch.full((16, 1), 0.5, device=gpu)
        costs.append(float(s.__next__({xp: xe, yp: ye})[1]))
        costs += [float(next(s)[1]) for _ in range(4)]
        ckpt = s.state_dict()
        assert ("pending_window" in ckpt) == prefetch
        costs += [float(next(s)[1]) for _ in range(3)]
        if s.fused_bnn_available():
            costs += [float(c) for c in s.fused_bnn_steps(4)]
            costs += [float(next(s)[1]) for _ in range(2)]
        # ... and on to a path that does not feed through the static buffers at all (torch restatement of the cost, eager): the
        # window drawn ahead is still the next batch
        s.use_hip_graph, s.cost_fun.use_hip_kernels = False, False
        costs += [float(next(s)[1]) for _ in range(2)]
        assert s._pending_window is None
        theta = s.arena.row("theta").clone()
        # resume from the checkpoint in a fresh sampler
        r, _, _ = chain(prefetch)
        r.load_state_dict(ckpt)
        resumed = [float(next(r)[1]) for _ in range(3)]
        runs[prefetch] = (costs, theta, resumed)
        assert resumed == costs[13:16], (prefetch, resumed, costs[13:16])
    assert runs[True][0] == runs[False][0]
    assert torch.equal(runs[True][1], runs[False][1])
