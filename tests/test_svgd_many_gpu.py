"""The many-particle SVGD path (include/sgmcmc_hip_svgd_many.h, csrc/sgmcmc_svgd_many.hip) on the GPU: kernel matrix and
single step at every case of ``svgd_many_cases.py`` against the oracle, both layouts with canaries where the Gram grid walks,
the two paths side by side at 64 and 128 particles, duplicated particles, bit reproducibility, and ``SVGDSampler`` above 128
particles in its three stepping modes.

Bars. K and the bandwidth words: ``TOL`` of test_svgd_gpu.py against the f64 oracle. Steps: the displacement bar of
test_svgd_tile_walk_gpu.py with c = 8 x the oracle's own worst error over the table (svgd_many_cases.C: 8 x 3.912 in f32,
8 x 4.484 in f64), then the sweep's looser bars. Measured on an MI355X, units of the bar at c = 1 (X, H), the worst case of
each dtype: f32 17.8, 0.65 at (1024, 65, -1) against c = 31.3; f64 7.5, 0.50 at (1024, 65, -1) against c = 35.9 (the
matrix cores add the 1024 terms of a row of K G in one chain; numpy adds them blockwise); H at most 1.6 (f32, 1024 x 3). Every
case is in profiles/svgd_many.txt."""
import numpy as np
import pytest
import torch

from oracle import sgmcmc_oracle as O
from pysgmcmc_amd import kernels, models
from pysgmcmc_amd.data_batches import Placeholder, generate_batches
from pysgmcmc_amd.models import BNNParticleCost, bnn_particles
from pysgmcmc_amd.samplers import SVGDSampler
from pysgmcmc_amd.samplers.base_classes import graph_capture
from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule

import svgd_many_cases as M
import test_svgd_tile_walk_gpu as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = M.F32, M.F64
CANARY, TAIL = 7.0, 256
DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]


def _cases(dtype):
    return list(M.TABLE) + M.walk_cases(dtype) + M.phase_cases(dtype)


CASE_PARAMS = [pytest.param(n, d, dt, id="%dx%d-%s" % (n, d, np.dtype(dt).name)) for dt in (F32, F64) for n, d in _cases(dt)]
LAYOUT_PARAMS = [pytest.param(n, d, dt, id="%dx%d-%s" % (n, d, np.dtype(dt).name))
                 for dt in (F32, F64) for n, d in M.walk_cases(dt) + [(161, 257)] + M.phase_cases(dt)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                     # a copy: the shared references are read-only


def _check_kernel(what, X, K, kg, bw, K_ref, kg_ref, h_ref, med_ref, dtype):
    tol = M.TOL[dtype]
    rel = np.abs(K - K_ref) / (tol["atol"] + tol["rtol"] * np.abs(K_ref))
    print("%s: K uses %.3f of its bar, h %.3f of its" % (what, rel.max(), abs(bw[1] - h_ref) / h_ref / tol["rtol"]))
    np.testing.assert_allclose(bw[0], med_ref, rtol=tol["rtol"], err_msg=what)
    np.testing.assert_allclose(bw[1], h_ref, rtol=tol["rtol"], err_msg=what)
    np.testing.assert_allclose(bw[2], h_ref * h_ref, rtol=2 * tol["rtol"], err_msg=what)
    np.testing.assert_allclose(K, K_ref, err_msg=what, **tol)
    assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1), what                   # exact structure
    if kg is not None:
        # kernel gradients: a difference of two O(|x| * rowsum) sums, tolerance relative to that scale (test_svgd_gpu.py)
        scale = np.abs(X).max() * K_ref.sum(axis=1).max() / (h_ref * h_ref)
        np.testing.assert_allclose(kg, kg_ref, rtol=tol["rtol"], atol=tol["rtol"] * scale * 4, err_msg=what)


def _check_step(what, ref, dtype, x_new, h_new):
    x_new, h_new = x_new.astype(np.float64), h_new.astype(np.float64)
    ux, uh = W.bar_units(ref, dtype, x_new, h_new)
    print("%s: %.3f (X), %.3f (H) units of the bar at c = 1; c = %g" % (what, ux, uh, M.C[dtype]))
    bar_x, bar_h = W.step_bars(ref, dtype, M.C[dtype])
    ex = np.abs((x_new - ref.X.astype(np.float64)) - ref.disp) / bar_x
    eh = np.abs(h_new - ref.Hn) / bar_h
    assert ex.max() <= 1.0, "%s: displacement %.2f x its bar at %r" % (what, ex.max(), np.unravel_index(ex.argmax(), ex.shape))
    assert eh.max() <= 1.0, "%s: H %.2f x its bar at %r" % (what, eh.max(), np.unravel_index(eh.argmax(), eh.shape))
    rtol = M.SWEEP_RTOL[dtype]
    np.testing.assert_allclose(x_new, ref.Xn, rtol=rtol, atol=rtol, err_msg=what)
    np.testing.assert_allclose(h_new, ref.Hn, rtol=10 * rtol, atol=1e-2 * rtol, err_msg=what)


@pytest.mark.parametrize("n,d,dtype", CASE_PARAMS)
def test_kernel_matrix_matches_the_oracle(n, d, dtype):
    X, K_ref, kg_ref, h_ref, med_ref = M.kernel_reference(n, d, dtype)
    x = _dev(X)
    ws = kernels.svgd_many_workspace(n, x)
    ws.fill_(float("nan"))                                            # a partial that is read but never written shows
    K, kg, bw = kernels.svgd_many_kernel(x.reshape(-1), n, d, ws)
    torch.cuda.synchronize()
    assert torch.equal(x, _dev(X))
    _check_kernel("K %d x %d %s" % (n, d, np.dtype(dtype).name), X, K.cpu().numpy(), kg.cpu().numpy(), bw.cpu().numpy(),
                  K_ref, kg_ref, h_ref, med_ref, dtype)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("n,d,dtype", CASE_PARAMS)
def test_single_step_matches_the_oracle(n, d, dtype, sign):
    ref = M.step_reference(M.Case(n, d, dtype, sign))
    x, g, h = (_dev(a).reshape(-1) for a in (ref.X, ref.G, ref.H))
    ws = kernels.svgd_many_workspace(n, x)
    ws.fill_(float("nan"))
    kernels.svgd_many_step(x, g, h, n, d, M.EPS, M.ALPHA, M.FUDGE, ws, repulsion_sign=sign)
    torch.cuda.synchronize()
    assert torch.equal(g, _dev(ref.G).reshape(-1))
    _check_step("step %d x %d %s sign %+d" % (n, d, np.dtype(dtype).name, sign), ref, dtype,
                x.cpu().numpy().reshape(n, d), h.cpu().numpy().reshape(n, d))


# ---- layouts ---------------------------------------------------------------------------------------------------------------

def _layout(dim, layout):
    """(row pitch, base offset in elements): 16-byte aligned rows, or pitch = dim (odd) from a base shifted by one element"""
    if layout == "aligned":
        return (dim // 4 + 1) * 4, 0
    return dim, 1


def _buffer(a, ld, offset):
    n, d = a.shape
    buf = torch.full((offset + n * ld + TAIL,), CANARY, dtype=_dev(a[:1, :1]).dtype, device=DEV)
    view = buf[offset:]
    view[:n * ld].view(n, ld)[:, :d] = _dev(a)
    return buf, view


def _rows(host, n, d, ld, offset):
    return host[offset:offset + n * ld].reshape(n, ld)[:, :d]


def _canary_intact(host, n, d, ld, offset):
    keep = np.ones(host.shape[0], bool)
    for i in range(n):
        keep[offset + i * ld:offset + i * ld + d] = False
    return bool(np.all(host[keep] == CANARY))


@pytest.mark.parametrize("n,d,dtype", LAYOUT_PARAMS)
def test_bits_do_not_depend_on_pitch_alignment_or_the_run(n, d, dtype):
    """Kernel matrix, kernel gradients and one step in a 16-byte-aligned pitched layout and in an element-aligned one, each
    twice: one set of bits, canaries around every row intact, and those bits within the bars."""
    X, K_ref, kg_ref, h_ref, med_ref = M.kernel_reference(n, d, dtype)
    ref = M.step_reference(M.Case(n, d, dtype, -1))
    assert d % 2 == 1
    outs = []
    for layout in ("aligned", "element", "aligned", "element"):
        ld, offset = _layout(d, layout)
        bk, xk = _buffer(X, ld, offset)
        ws = kernels.svgd_many_workspace(n, xk)
        ws.fill_(float("nan"))
        f = getattr(kernels.lib(), "sgmcmc_svgd_many_kernel_" + ("f32" if dtype == F32 else "f64"))
        K = torch.empty((n, n), dtype=xk.dtype, device=DEV)
        bw = torch.empty(3, dtype=xk.dtype, device=DEV)
        bg, kg = _buffer(np.full((n, d), CANARY, dtype), ld, offset)                # kernel gradients at the same pitch
        rc = f(xk.data_ptr(), n, d, ld, ws.data_ptr(), K.data_ptr(), kg.data_ptr(), ld, bw.data_ptr(),
               torch.cuda.current_stream().cuda_stream)
        assert rc == 0, kernels.lib().sgmcmc_last_error()
        (bx, x), (_, g), (bh, h) = (_buffer(a, ld, offset) for a in (ref.X, ref.G, ref.H))
        ws.fill_(float("nan"))
        kernels.svgd_many_step(x, g, h, n, d, M.EPS, M.ALPHA, M.FUDGE, ws, ld=ld, repulsion_sign=-1)
        torch.cuda.synchronize()
        hk, hg, hx, hh = (b.cpu().numpy() for b in (bk, bg, bx, bh))
        what = "%d x %d %s [%s, pitch %d]" % (n, d, np.dtype(dtype).name, layout, ld)
        assert _canary_intact(hk, n, d, ld, offset) and np.array_equal(_rows(hk, n, d, ld, offset), X), what + ": X written"
        for name, host in (("kernel gradients", hg), ("X", hx), ("H", hh)):
            assert _canary_intact(host, n, d, ld, offset), "%s: %s written outside its rows" % (what, name)
        outs.append((K.cpu().numpy(), bw.cpu().numpy(), _rows(hg, n, d, ld, offset).copy(), _rows(hx, n, d, ld, offset).copy(),
                     _rows(hh, n, d, ld, offset).copy()))
        del bk, xk, bg, kg, bx, x, g, bh, h, ws
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b), "%d x %d: bits differ between layouts or runs" % (n, d)
    K, bw, kg, x_new, h_new = outs[0]
    _check_kernel("K %d x %d" % (n, d), X, K, kg, bw, K_ref, kg_ref, h_ref, med_ref, dtype)
    _check_step("step %d x %d" % (n, d), ref, dtype, x_new, h_new)


# ---- the two paths meet at the boundary -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", [(64, 33), (128, 257)])
def test_both_paths_agree_where_both_run(n, d, dtype):
    X, K_ref, kg_ref, h_ref, med_ref = M.kernel_reference(n, d, dtype)
    x = _dev(X).reshape(-1)
    ws_old, ws_new = kernels.svgd_workspace(n, x), kernels.svgd_many_workspace(n, x)
    old = [t.cpu().numpy() for t in kernels.svgd_kernel(x, n, d, ws_old)]
    new = [t.cpu().numpy() for t in kernels.svgd_many_kernel(x, n, d, ws_new)]
    tol = M.TOL[dtype]
    for (K, kg, bw), name in ((old, "register-resident"), (new, "tiled")):
        _check_kernel("%s K %d x %d" % (name, n, d), X, K, kg, bw, K_ref, kg_ref, h_ref, med_ref, dtype)
    np.testing.assert_allclose(new[0], old[0], **tol)
    np.testing.assert_allclose(new[2][:2], old[2][:2], rtol=tol["rtol"])
    np.testing.assert_allclose(new[2][2], old[2][2], rtol=2 * tol["rtol"])
    scale = np.abs(X).max() * K_ref.sum(axis=1).max() / (h_ref * h_ref)
    np.testing.assert_allclose(new[1], old[1], rtol=tol["rtol"], atol=tol["rtol"] * scale * 4)
    for sign in (1, -1):
        ref = M.step_reference(M.Case(n, d, dtype, sign))
        got = {}
        for name, step, ws in (("register-resident", kernels.svgd_step, ws_old), ("tiled", kernels.svgd_many_step, ws_new)):
            xs, g, h = (_dev(a).reshape(-1) for a in (ref.X, ref.G, ref.H))
            step(xs, g, h, n, d, M.EPS, M.ALPHA, M.FUDGE, ws, repulsion_sign=sign)
            got[name] = (xs.cpu().numpy().reshape(n, d), h.cpu().numpy().reshape(n, d))
            _check_step("%s step %d x %d sign %+d" % (name, n, d, sign), ref, dtype, *got[name])
        bar_x, bar_h = W.step_bars(ref, dtype, M.C[dtype])
        (xa, ha), (xb, hb) = got["register-resident"], got["tiled"]
        assert np.all(np.abs(xa.astype(np.float64) - xb) <= bar_x) and np.all(np.abs(ha.astype(np.float64) - hb) <= bar_h)


# ---- median among ties, reproducibility ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicated_particles_median_and_unit_kernel(dtype):
    base = M.cloud(65, 40, dtype, seed=5)
    X = np.concatenate([base, base], axis=0)                                       # 130 particles: even count, 260 zeros
    x = _dev(X)
    ws = kernels.svgd_many_workspace(130, x)
    K, _, bw = kernels.svgd_many_kernel(x.reshape(-1), 130, 40, ws, kernel_gradients=False)
    _, _, _, D_ref = O.svgd_kernel(X.astype(np.float64))
    np.testing.assert_allclose(bw[0].item(), O.svgd_median(D_ref), rtol=1e-5)
    K = K.cpu().numpy()
    np.testing.assert_allclose(K[np.arange(65), np.arange(65) + 65], 1.0, atol=2e-6)
    assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1)


def test_two_steps_are_bit_reproducible_at_a_multi_workgroup_size():
    n, d = 257, 20_000
    X = M.cloud(n, d, F32, seed=9)
    outs = []
    for _ in range(2):
        x = _dev(X).reshape(-1)
        g = (0.5 * x).contiguous()
        h = torch.zeros_like(x)
        ws = kernels.svgd_many_workspace(n, x)
        for _ in range(2):
            kernels.svgd_many_step(x, g, h, n, d, 0.1, 0.9, 1e-6, ws, repulsion_sign=-1)
        outs.append((x.cpu().numpy(), h.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.all(np.isfinite(outs[0][0])) and not np.array_equal(outs[0][0], X.reshape(-1))


# ---- the raw entry under stream capture ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_captured_step_replays_the_eager_bits(dtype):
    n, d = 130, 70                                                                 # even count: all eleven launches
    ref = M.step_reference(M.Case(n, d, dtype, -1))
    x, g, h = (_dev(a).reshape(-1) for a in (ref.X, ref.G, ref.H))
    ws = kernels.svgd_many_workspace(n, x)
    kernels.svgd_many_step(x, g, h, n, d, M.EPS, M.ALPHA, M.FUDGE, ws, repulsion_sign=-1)
    want_x, want_h = x.clone(), h.clone()
    x.copy_(_dev(ref.X).reshape(-1))
    h.copy_(_dev(ref.H).reshape(-1))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, capture_error_mode="thread_local"):
        kernels.svgd_many_step(x, g, h, n, d, M.EPS, M.ALPHA, M.FUDGE, ws, repulsion_sign=-1)
    for _ in range(2):
        x.copy_(_dev(ref.X).reshape(-1))
        h.copy_(_dev(ref.H).reshape(-1))
        ws.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(x, want_x) and torch.equal(h, want_h)


# ---- the sampler -----------------------------------------------------------------------------------------------------------

def test_200_particles_fit_a_gaussian():
    """The 50-particle test of test_svgd_gpu.py with 200 particles. The f64 oracle gives mean (1.010, -2.000) and std
    (1.013, 1.951) after these 600 steps."""
    from pysgmcmc_amd.sampling import Sampler
    rng = np.random.RandomState(0)
    x0 = rng.normal(size=(200, 2)) * 0.1 + 3.0
    mu = torch.tensor([1.0, -2.0], device=DEV)
    var = torch.tensor([1.0, 4.0], device=DEV)

    def cost(p):
        return 0.5 * ((p - mu) ** 2 / var).sum()

    s = Sampler.get_sampler(Sampler.SVGD, particles=[torch.tensor(r, device=DEV) for r in x0], cost_fun=cost,
                            dtype=torch.float32)
    s.sample_format = "device"
    for _ in range(600):
        sample, costs = next(s)
    P = torch.stack(sample).cpu().numpy()
    assert costs.shape == (200,)
    print("mean %r std %r" % (P.mean(axis=0), P.std(axis=0)))
    np.testing.assert_allclose(P.mean(axis=0), [1.0, -2.0], atol=0.15)
    np.testing.assert_allclose(P.std(axis=0), [1.0, 2.0], rtol=0.3)
    K, kg = s.svgd_kernel()
    K_ref, _, _, _ = O.svgd_kernel(P.astype(np.float64))
    np.testing.assert_allclose(K.cpu().numpy(), K_ref, rtol=1e-4, atol=1e-5)
    K2, _ = s.svgd_kernel(torch.stack(sample))                                     # a contiguous user tensor, ld = d
    assert torch.equal(K2, K)


def _quadratic(n, d=3, seed=4):
    x0 = np.random.RandomState(seed).normal(size=(n, d))
    cost = lambda P: 0.5 * (P ** 2).sum(dim=1)
    cost.batched = True
    return [torch.tensor(r, device=DEV) for r in x0], cost


def test_129_particles_step_and_1025_are_refused_with_both_limits():
    particles, cost = _quadratic(129)
    s = SVGDSampler(particles=particles, cost_fun=cost, dtype=torch.float32)
    s.sample_format = "device"
    before = s.particles.detach().clone()
    sample, costs = next(s)
    assert costs.shape == (129,) and len(sample) == 129
    now = s.particles.detach()
    assert torch.isfinite(now).all() and not torch.equal(now, before)
    particles, cost = _quadratic(1025)
    s = SVGDSampler(particles=particles, cost_fun=cost, dtype=torch.float32)
    with pytest.raises(ValueError, match=r"1024.*128|128.*1024"):
        next(s)
    with pytest.raises(ValueError, match=r"1024.*128|128.*1024"):
        s.svgd_kernel(torch.zeros(1025, 3, device=DEV))


DEFAULT = [1, 50, 50, 50, 1]


def _sinc():
    rng = np.random.RandomState(1)
    X = rng.rand(100, 1)
    return X, np.sinc(X * 10 - 5).sum(axis=1)


def _svgd_bnn(dt, n=257, graph=False, eps=1e-3):
    X, y = _sinc()
    xp, yp = Placeholder(dtype=dt, device=DEV), Placeholder(dtype=dt, device=DEV)
    cost = BNNParticleCost(DEFAULT, xp, yp, batch_size=20, n_examples=100)
    s = SVGDSampler(bnn_particles(n, 1, seed=3, dtype=dt, device=DEV), cost,
                    batch_generator=generate_batches(X, y, xp, yp, 20, seed=1),
                    stepsize_schedule=ConstantStepsizeSchedule(eps), session=torch.device(DEV), dtype=dt)
    s.sample_format, s.use_hip_graph = "view", graph
    return s


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_257_bnn_particles_step_alike_in_all_three_modes_without_autograd(dt, monkeypatch):
    def no_autograd(*a, **k):
        raise AssertionError("torch.autograd.grad was called on the K15 route")
    monkeypatch.setattr(torch.autograd, "grad", no_autograd)
    runs = {}
    for mode in (False, True, "full"):
        s = _svgd_bnn(dt, graph=mode)
        costs = []
        for _ in range(5):
            _, c = next(s)
            costs.append(c.reshape(-1).clone())
        runs[mode] = (s.particles.detach().clone(), torch.stack(costs), s)
    monkeypatch.undo()
    eager = runs[False][2]
    assert eager._particle_costs is not None and not eager.particles.requires_grad
    assert eager.n_particles == 257 and eager._ws().numel() * eager._ws().element_size() == \
        kernels.lib().sgmcmc_svgd_many_workspace_bytes(257, eager._ws().element_size())
    assert runs[True][2]._graphs and runs["full"][2]._graphs and not eager._graphs
    assert not runs["full"][2]._full_graph_disabled
    for mode in (True, "full"):
        assert torch.equal(runs[mode][0], runs[False][0]), mode
        assert torch.equal(runs[mode][1], runs[False][1]), mode
    assert torch.isfinite(runs[False][0]).all() and not torch.equal(runs[False][1][0], runs[False][1][4])
    # the pitched particle matrix goes into the predictive and the held-out score in place
    parts = eager.particles.detach()
    assert parts.shape == (257, 5252) and parts.stride() == (5312, 1)
    X, y = _sinc()
    Xt, yt = torch.tensor(X, dtype=dt, device=DEV), torch.tensor(y, dtype=dt, device=DEV)
    mean, var = models.posterior_predictive(parts[None], Xt, DEFAULT)
    mean_c, var_c = models.posterior_predictive(parts.contiguous()[None], Xt, DEFAULT)
    assert torch.equal(mean, mean_c) and torch.equal(var, var_c) and torch.isfinite(mean).all()
    score = models.heldout_score(parts[None], Xt, yt, DEFAULT)
    score_c = models.heldout_score(parts.contiguous()[None], Xt, yt, DEFAULT)
    assert torch.equal(score.row_lppd, score_c.row_lppd) and torch.equal(score.rmse, score_c.rmse)
