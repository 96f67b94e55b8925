"""Kernel K15 (csrc/sgmcmc_bnn_particles.hip, include/sgmcmc_hip_particles.h) on the GPU: the cost and the parameter gradient
of every particle of a small tanh-MLP BNN in one launch, and ``SVGDSampler`` on it.

The weight and bias gradients are pinned to the whole-step kernel K8 bit for bit (one K8 step from the same point on the same
window leaves its gradient in its ``grad`` row), the ``log_var`` element and the cost to K8 within the rounding of one cast,
the prior term to its statement in numpy, everything to the float64 oracle within the project's bar for K8, and the results
to the layout: they depend on the particle and the minibatch alone."""
import numpy as np
import pytest
import torch

from pysgmcmc_amd import kernels, models
from pysgmcmc_amd.data_batches import Placeholder, generate_batches
from pysgmcmc_amd.models import BNNParticleCost, bnn_particles
from pysgmcmc_amd.samplers import SVGDSampler
from pysgmcmc_amd.samplers.base_classes import graph_capture
from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule

pytestmark = pytest.mark.gpu

DEFAULT = [1, 50, 50, 50, 1]
F32, F64 = torch.float32, torch.float64
N_DATA = 160
# (net, batch, dtypes): the default net (45 584 B of LDS in f32; 91 008 B in f64, which is already above the 64 KiB opt-in);
# every scalar path; mixed parity; no hidden layer; B * D0 above the workgroup; the f32 ceiling of the default net (162 704 B;
# in f64 it fits up to batch 49). The loop forms, LDS edges and grids beyond these: tests/test_bnn_particles_forms_gpu.py
CASES = [(DEFAULT, 20, (F32, F64)), ([3, 5, 7, 1], 3, (F32, F64)), ([2, 4, 3, 1], 5, (F32, F64)), ([4, 1], 1, (F32, F64)),
         ([4, 1], 2, (F32, F64)), ([30, 6, 1], 20, (F32, F64)), (DEFAULT, 116, (F32,))]
CASE_PARAMS = [pytest.param(sizes, B, dt, id="%s-B%d-%s" % ("x".join(map(str, sizes)), B, str(dt)[-2:]))
               for sizes, B, dts in CASES for dt in dts]
CONST = dict(n_examples=N_DATA, prior_mean=1e-6, prior_var=0.01)


def _n_params(sizes):
    return sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1


def _data(sizes, dt, gpu):
    rng = np.random.RandomState(sizes[0] * 7 + len(sizes))
    X = rng.uniform(-1.0, 1.0, size=(N_DATA, sizes[0]))
    y = np.sinc(X * 2.0).sum(axis=1) + 0.05 * rng.randn(N_DATA)
    return torch.tensor(X, dtype=dt, device=gpu).contiguous(), torch.tensor(y, dtype=dt, device=gpu).contiguous()


def _particles(sizes, n, dt, gpu, seed=0):
    """(n, P) contiguous: initial nets with every bias drawn too, so that no gradient element is trivially zero"""
    rng = np.random.RandomState(seed + 13 * len(sizes))
    rows = torch.stack(bnn_particles(n, sizes[0], hidden=sizes[1:-1], seed=seed + 1, dtype=F64)).numpy()
    rows = rows + 0.1 * rng.randn(*rows.shape)
    rows[:, -1] = -1.0 + 0.3 * rng.randn(n)                                      # log_var
    return torch.tensor(rows, dtype=dt, device=gpu).contiguous()


def _k15(theta, sizes, Xb, yb, B, n=None, ld=None, add_prior=True, wdecay=1.0, ld_grad=None, grad=None, costs=None):
    P = _n_params(sizes)
    n = theta.shape[0] if n is None else n
    ld = (theta.stride(0) if theta.dim() == 2 else P) if ld is None else ld
    ld_grad = P if ld_grad is None else ld_grad
    flat = theta.reshape(-1) if theta.dim() == 2 and theta.is_contiguous() else theta
    if grad is None:
        grad = torch.full(((n - 1) * ld_grad + P,), float("nan"), dtype=theta.dtype, device=theta.device)
    if costs is None:
        costs = torch.full((n,), float("nan"), dtype=theta.dtype, device=theta.device)
    kernels.bnn_particles_cost_grad(flat, n, ld, sizes, Xb, yb, grad, ld_grad, costs, B, wdecay=wdecay, add_prior=add_prior,
                                    **CONST)
    return grad, costs


def _k8(theta0, sizes, X, y, start, B, wdecay=1.0):
    """K8's gradient row and cost at theta0 on the window [start, start + B): one step of the whole-step kernel."""
    P, dt, dev = theta0.numel(), theta0.dtype, theta0.device
    rows = {k: torch.zeros(P, dtype=dt, device=dev) for k in ("V", "grad")}
    rows.update({k: torch.ones(P, dtype=dt, device=dev) for k in ("tau", "g", "v_hat", "minv")})
    theta = theta0.clone()
    cost = torch.empty(1, dtype=dt, device=dev)
    starts = torch.tensor([start], dtype=torch.int32, device=dev)
    kernels.bnn_fused_sghmc_steps(theta, rows["V"], rows["grad"], rows["tau"], rows["g"], rows["v_hat"], rows["minv"], sizes,
                                  X, y, starts, B, B, N_DATA, wdecay, 1e-6, 0.01, 0.01, float(N_DATA), 0.05, 0, 1, 6, 0, cost)
    return rows["grad"], cost


# ---- 1: weight and bias gradients are K8's, bit for bit ---------------------------------------------------------------------

@pytest.mark.parametrize("sizes, B, dt", CASE_PARAMS)
def test_weight_and_bias_gradients_are_the_whole_step_kernel_s_bits(gpu, sizes, B, dt):
    X, y = _data(sizes, dt, gpu)
    theta = _particles(sizes, 2, dt, gpu)
    P = _n_params(sizes)
    for p, start in ((0, 7), (1, N_DATA - B)):
        want, _ = _k8(theta[p], sizes, X, y, start, B)
        got, _ = _k15(theta[p:p + 1], sizes, X[start:start + B], y[start:start + B], B, add_prior=False)
        assert torch.isfinite(got).all() and float(got[:P - 1].abs().max()) > 0.0
        assert torch.equal(got[:P - 1], want[:P - 1]), (p, int((got[:P - 1] != want[:P - 1]).sum()))


# ---- 2: the log_var element and the cost against K8 ---------------------------------------------------------------------------

@pytest.mark.parametrize("sizes, dt", [([3, 5, 7, 1], F32), ([3, 5, 7, 1], F64), (DEFAULT, F32)])
def test_log_var_gradient_and_cost_are_k8_s_within_one_cast(gpu, sizes, dt):
    B = 65                                                                       # the head's sum spans two waves
    X, y = _data(sizes, dt, gpu)
    theta = _particles(sizes, 3, dt, gpu, seed=4)
    P = _n_params(sizes)
    for p, start in ((0, 0), (1, 31), (2, N_DATA - B)):
        want_g, want_c = _k8(theta[p], sizes, X, y, start, B)
        got_g, got_c = _k15(theta[p:p + 1], sizes, X[start:start + B], y[start:start + B], B, add_prior=False)
        assert torch.equal(got_g[:P - 1], want_g[:P - 1])
        for what, got, want in (("d/dlog_var", got_g[P - 1], want_g[P - 1]), ("cost", got_c[0], want_c[0])):
            got, want = got.cpu().numpy(), want.cpu().numpy()
            print("%s %s particle %d: K15 %r K8 %r" % (what, dt, p, got, want))
            if dt == F32:                                                        # two double sums in another order, one cast
                assert abs(got - want) <= np.spacing(np.float32(max(abs(got), abs(want)))), (what, got, want)
            else:
                assert abs(got - want) <= 1e-13 * abs(want), (what, got, want)


# ---- 3: the prior term -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("wdecay", [1.0, 0.0])
def test_the_prior_term_is_one_multiply_and_one_add(gpu, dt, wdecay):
    for sizes, B in ((DEFAULT, 20), ([3, 5, 7, 1], 3)):
        X, y = _data(sizes, dt, gpu)
        theta = _particles(sizes, 3, dt, gpu, seed=2)
        P = _n_params(sizes)
        raw, c_raw = _k15(theta, sizes, X[5:5 + B], y[5:5 + B], B, add_prior=False, wdecay=wdecay)
        full, c_full = _k15(theta, sizes, X[5:5 + B], y[5:5 + B], B, add_prior=True, wdecay=wdecay)
        real = np.float32 if dt == F32 else np.float64
        coef = real(wdecay / ((float(P) + (2.0 * 1e-16 + 1e-16)) * float(N_DATA)))
        th, r = theta.cpu().numpy().reshape(-1), raw.cpu().numpy()
        prod = coef * th
        want = r + prod if wdecay else r
        assert prod.dtype == real and want.dtype == real
        assert np.array_equal(full.cpu().numpy(), want)
        assert (wdecay == 0.0) == np.array_equal(full.cpu().numpy(), r)
        assert torch.equal(c_raw, c_full)                                        # the cost carries its weight prior either way


# ---- 4: against the float64 oracle -------------------------------------------------------------------------------------------

def _split(row, sizes):
    out, at = [], 0
    for l in range(len(sizes) - 1):
        out.append(row[at:at + sizes[l] * sizes[l + 1]].reshape(sizes[l], sizes[l + 1]))
        at += sizes[l] * sizes[l + 1]
        out.append(row[at:at + sizes[l + 1]])
        at += sizes[l + 1]
    out.append(row[at:at + 1].reshape(1, 1))
    return out


@pytest.mark.parametrize("sizes, B, dt", CASE_PARAMS)
def test_gradients_stay_within_the_project_s_bar_of_the_float64_oracle(gpu, oracle, sizes, B, dt):
    """The bar K8 meets against its golden trajectory: 2e-4 (f32) / 1e-9 (f64) of max|g|."""
    X, y = _data(sizes, dt, gpu)
    theta = _particles(sizes, 3, dt, gpu, seed=6)
    start = 11
    got, costs = _k15(theta, sizes, X[start:start + B], y[start:start + B], B)
    got, costs = got.cpu().numpy().astype(np.float64).reshape(3, -1), costs.cpu().numpy().astype(np.float64)
    Xb = X[start:start + B].cpu().numpy().astype(np.float64)
    yb = y[start:start + B].cpu().numpy().astype(np.float64).reshape(-1, 1)
    tol = 2e-4 if dt == F32 else 1e-9
    for p in range(3):
        c64, g64 = oracle.bnn_cost_and_grad(_split(theta[p].cpu().numpy().astype(np.float64), sizes), Xb, yb, B, N_DATA)
        g64 = np.concatenate([np.asarray(g).reshape(-1) for g in g64])
        dev = np.abs(got[p] - g64).max() / np.abs(g64).max()
        print("%s B=%d %s particle %d: max|g - g64| / max|g64| = %.3e, cost %.9g vs %.9g" % (sizes, B, dt, p, dev, costs[p], c64))
        assert dev <= tol, dev
        assert abs(costs[p] - c64) <= (1e-5 if dt == F32 else 1e-12) * abs(c64)


# ---- 5: the results do not depend on the layout ---------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [F32, F64])
def test_results_depend_on_the_particle_and_the_minibatch_alone(gpu, dt):
    sizes, B = [3, 5, 7, 1], 5
    P = _n_params(sizes)
    assert P == 71                                                               # odd: rows at ld = P are unaligned
    X, y = _data(sizes, dt, gpu)
    Xb, yb = X[9:9 + B], y[9:9 + B]
    theta = _particles(sizes, 130, dt, gpu, seed=8)
    # every particle on its own: the reference rows
    ref_g = torch.stack([_k15(theta[p:p + 1], sizes, Xb, yb, B)[0] for p in range(130)])
    ref_c = torch.cat([_k15(theta[p:p + 1], sizes, Xb, yb, B)[1] for p in (0, 1, 2, 15, 64, 129)])
    assert torch.isfinite(ref_g).all() and not torch.equal(ref_g[0], ref_g[1])
    for n in (1, 3, 16, 130):
        g, c = _k15(theta[:n], sizes, Xb, yb, B)
        assert torch.equal(g.reshape(n, P), ref_g[:n]), n
        if n == 130:
            assert torch.equal(c[[0, 1, 2, 15, 64, 129]], ref_c)
    # ld = P against the next multiple of 64; ld_grad another pitch again; gaps of grad keep their sentinel, guard rows
    # before and behind grad and costs stay untouched
    n, ld, ld_grad = 16, 128, 96
    wide = torch.full((n, ld), 1e30, dtype=dt, device=gpu)
    wide[:, :P] = theta[:n]
    guard = 3 * ld_grad
    gbuf = torch.full((guard + n * ld_grad + guard,), -7.5, dtype=dt, device=gpu)
    cbuf = torch.full((8 + n + 8,), -7.5, dtype=dt, device=gpu)
    kernels.bnn_particles_cost_grad(wide.reshape(-1), n, ld, sizes, Xb, yb, gbuf[guard:guard + n * ld_grad], ld_grad,
                                    cbuf[8:8 + n], B, **CONST, wdecay=1.0)
    rows = gbuf[guard:guard + n * ld_grad].reshape(n, ld_grad)
    assert torch.equal(rows[:, :P], ref_g[:n])
    assert bool((rows[:, P:] == -7.5).all()) and bool((gbuf[:guard] == -7.5).all()) and bool((gbuf[-guard:] == -7.5).all())
    assert bool((cbuf[:8] == -7.5).all()) and bool((cbuf[-8:] == -7.5).all())
    full_c = _k15(theta[:n], sizes, Xb, yb, B)[1]
    assert torch.equal(cbuf[8:8 + n], full_c)
    # the minibatch as a view of a [B, D0 + 4] buffer
    ext = torch.full((B, sizes[0] + 4), 1e30, dtype=dt, device=gpu)
    ext[:, :sizes[0]] = Xb
    view = ext[:, :sizes[0]]
    assert view.stride(0) == sizes[0] + 4 and not view.is_contiguous()
    g, c = _k15(theta[:n], sizes, view, yb, B)
    assert torch.equal(g.reshape(n, P), ref_g[:n]) and torch.equal(c, full_c)
    # a particle matrix that starts one element off a 16-byte boundary (4 bytes in f32, 8 in f64)
    off = torch.empty(n * P + 5, dtype=dt, device=gpu)
    assert off.data_ptr() % 16 == 0
    shifted = off[1:1 + n * P]
    shifted.copy_(theta[:n].reshape(-1))
    assert shifted.data_ptr() % 16 == theta.element_size()
    gs = torch.full((n * P + 5,), -7.5, dtype=dt, device=gpu)
    cs = torch.empty(n, dtype=dt, device=gpu)
    kernels.bnn_particles_cost_grad(shifted, n, P, sizes, Xb, yb, gs[3:3 + n * P], P, cs, B, **CONST, wdecay=1.0)
    assert torch.equal(gs[3:3 + n * P].reshape(n, P), ref_g[:n]) and torch.equal(cs, full_c)
    assert bool((gs[:3] == -7.5).all()) and bool((gs[3 + n * P:] == -7.5).all())


# ---- 6: the sampler ------------------------------------------------------------------------------------------------------

def _sinc():
    rng = np.random.RandomState(1)
    X = rng.rand(100, 1)
    return X, np.sinc(X * 10 - 5).sum(axis=1)


def _svgd(gpu, dt, n=8, kernel=True, graph=False, eps=1e-3):
    X, y = _sinc()
    xp, yp = Placeholder(dtype=dt, device=gpu), Placeholder(dtype=dt, device=gpu)
    cost = BNNParticleCost(DEFAULT, xp, yp, batch_size=20, n_examples=100)
    cost.use_hip_kernel = kernel
    s = SVGDSampler(bnn_particles(n, 1, seed=3, dtype=dt, device=gpu), cost, batch_generator=generate_batches(X, y, xp, yp, 20, seed=1),
                    stepsize_schedule=ConstantStepsizeSchedule(eps), session=gpu, dtype=dt)
    s.sample_format, s.use_hip_graph = "view", graph
    return s, cost


@pytest.mark.parametrize("dt", [F32, F64])
def test_the_sampler_s_gradient_row_is_the_kernel_s(gpu, dt, monkeypatch):
    s, cost = _svgd(gpu, dt)
    theta0 = s.arena.row("theta").clone()
    # (d) no autograd on this route
    def no_autograd(*a, **k):
        raise AssertionError("torch.autograd.grad was called on the K15 route")
    monkeypatch.setattr(torch.autograd, "grad", no_autograd)
    _, costs = next(s)
    monkeypatch.undo()
    assert not s.particles.requires_grad and s._vmapped is None
    Xb, yb = cost.x_placeholder.value, cost.y_placeholder.value
    pitch = s.particle_pitch
    assert pitch == 5312 and s.particle_dim == 5252
    grad = torch.zeros_like(theta0)
    want = torch.empty(8, dtype=dt, device=gpu)
    kernels.bnn_particles_cost_grad(theta0, 8, pitch, DEFAULT, Xb, yb, grad, pitch, want, 20, 100, 1.0, 1e-6, 0.01, add_prior=True)
    got = s.arena.row("grad")
    for p in range(8):
        assert torch.equal(got[p * pitch:p * pitch + 5252], grad[p * pitch:p * pitch + 5252]), p
    assert torch.equal(costs.reshape(-1), want) and s._grad_decay == 0.0
    assert not torch.equal(s.arena.row("theta"), theta0)                         # and the step was taken


@pytest.mark.parametrize("dt", [F32, F64])
def test_five_steps_track_the_autograd_route(gpu, dt):
    """Same particles, same windows: the kernel's dot products in k order against autograd's GEMMs. The bar is the one the
    whole-step kernel and the GEMM path meet after 14 steps. Stepsize 1e-3: SVGD's AdaGrad normalisation moves every element
    by about the stepsize per step, so five steps move the weights (0.14 in size at 50 inputs) by a few per cent."""
    a, _ = _svgd(gpu, dt, kernel=True)
    b, cost_b = _svgd(gpu, dt, kernel=False)
    for _ in range(5):
        _, ca = next(a)
        _, cb = next(b)
    assert a._particle_costs is not None and b._particle_costs is None
    ta, tb = a.particles, b.particles.detach()
    dev = float((ta - tb).abs().max()) / float(tb.abs().max())
    print("%s: max|dtheta| / max|theta| after 5 steps = %.3e; last costs differ by %.3e" % (
        dt, dev, float((ca.reshape(-1) - cb.reshape(-1)).abs().max())))
    assert dev <= (2e-4 if dt == F32 else 1e-9), dev
    assert torch.allclose(ca.reshape(-1), cb.reshape(-1).to(ca.dtype), rtol=1e-4 if dt == F32 else 1e-9)


@pytest.mark.parametrize("dt", [F32, F64])
def test_eager_graph_and_full_graph_stepping_are_one_trajectory(gpu, dt):
    runs = {}
    for mode in (False, True, "full"):
        s, _ = _svgd(gpu, dt, graph=mode)
        costs = []
        for _ in range(6):
            _, c = next(s)
            costs.append(c.reshape(-1).clone())
        runs[mode] = (s.particles.clone(), torch.stack(costs), s)
    assert runs[True][2]._graphs and runs["full"][2]._graphs and not runs[False][2]._graphs
    assert not runs["full"][2]._full_graph_disabled
    for mode in (True, "full"):
        assert torch.equal(runs[mode][0], runs[False][0]), mode
        assert torch.equal(runs[mode][1], runs[False][1]), mode
    assert not torch.equal(runs[False][1][0], runs[False][1][5])


# ---- 7: under stream capture ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [F32, F64])
def test_a_captured_launch_replays_the_eager_bits(gpu, dt):
    sizes, B, n = DEFAULT, 20, 5
    P = _n_params(sizes)
    X, y = _data(sizes, dt, gpu)
    theta = _particles(sizes, n, dt, gpu, seed=10)
    Xb, yb = X[3:3 + B].clone(), y[3:3 + B].clone()
    want_g, want_c = _k15(theta, sizes, Xb, yb, B)
    grad = torch.zeros(n * P, dtype=dt, device=gpu)
    costs = torch.zeros(n, dtype=dt, device=gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, capture_error_mode="thread_local"):
        _k15(theta, sizes, Xb, yb, B, grad=grad, costs=costs)
    for _ in range(2):
        grad.zero_()
        costs.zero_()
        graph.replay()
        assert torch.equal(grad, want_g) and torch.equal(costs, want_c)
    # a replay reads what the buffers hold then
    Xb.copy_(X[40:40 + B])
    yb.copy_(y[40:40 + B])
    graph.replay()
    again_g, again_c = _k15(theta, sizes, X[40:40 + B], y[40:40 + B], B)
    assert torch.equal(grad, again_g) and torch.equal(costs, again_c) and not torch.equal(again_g, want_g)


# ---- 8: downstream ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [F32, F64])
def test_the_pitched_particle_matrix_goes_straight_into_the_predictive(gpu, dt):
    s, _ = _svgd(gpu, dt)
    next(s)
    parts = s.particles.detach()
    assert parts.shape == (8, 5252) and parts.stride() == (5312, 1)
    X, y = _sinc()
    Xt = torch.tensor(X, dtype=dt, device=gpu)
    yt = torch.tensor(y, dtype=dt, device=gpu)
    mean, var = models.posterior_predictive(parts[None], Xt, DEFAULT)
    mean_c, var_c = models.posterior_predictive(parts.contiguous()[None], Xt, DEFAULT)
    assert torch.equal(mean, mean_c) and torch.equal(var, var_c) and torch.isfinite(mean).all()
    score = models.heldout_score(parts[None], Xt, yt, DEFAULT)
    score_c = models.heldout_score(parts.contiguous()[None], Xt, yt, DEFAULT)
    assert torch.equal(score.row_lppd, score_c.row_lppd) and torch.equal(score.rmse, score_c.rmse)
