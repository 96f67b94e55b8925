"""Kernel K15 (csrc/sgmcmc_bnn_particles.hip) on the GPU at the rows of tests/particles_cases.py: every loop form, several trips
of every strided loop at 512 lanes, every remainder of the unrolled loops, L = 1 and L = 8, the LDS edges (the opt-in, the
ceilings, exactly 160 KiB) and a grid larger than the chip. That the rows reach all of this is asserted without a GPU in
tests/test_bnn_particles_cases.py.

a. bits      weight and bias gradients with ``add_prior=False`` equal the whole-step kernel K8's gradient row bit for bit at
             every row (K8 takes them all; it runs 1024 lanes, so its trip counts differ wherever a loop takes several).
b. values    gW_l and gb_l of every layer, d / d log_var and the cost against the truth (the statements in the next wider
             precision with numpy products): |got - truth| <= 4 * E + 4 * u_T * max|truth over the block|, E the largest error of
             ``particles_cases.kernel_order`` in the row's own dtype against the same truth over all particles of the row and the
             whole of the layer. The factor 4 is the project's allowance for the vendor's tanh and exp against numpy's. K8 and K15
             share ``forward_tile``, so (a) does not see an error there; this does. The whole-gradient bar of
             tests/test_bnn_particles_gpu.py holds at every row as well. Measured: profiles/bnn_particles_forms.txt.
c. launch    a particle has the bits of a launch of that particle alone whatever n (2, 3, 300), ld, ld_grad, ldx and the
             alignment of its row; canaries stay in the gaps of ``grad`` and around ``grad`` and ``cost_out``.
d. refusals  one batch past each ceiling: SGMCMC_EINVAL with the 160 KiB text, nothing written; the ceiling then runs.
e. guard     log_var -50 (the 1e-16 carries the division), -30 and 30: finite and within (b); a NaN particle among healthy ones.
f. capture   the opt-in above 64 KiB inside a captured graph at exactly 160 KiB, one row per dtype.

Outputs start as a canary and are checked after the run. The references are computed once per row and shared.

What no test of the VALUES can see (tried by hand, profiles/bnn_particles_forms.txt): a pair loop on an odd weight offset (the LDS
replays the misaligned access: cycles, not bits) and a strided loop that strides by less than the workgroup (equal values
written again). tests/test_bnn_particles_cases.py reads those conditions and strides from the source instead."""
import numpy as np
import pytest
import torch

import particles_cases as K
from pysgmcmc_amd import _lib, kernels

pytestmark = pytest.mark.gpu

TORCH = {K.F32: torch.float32, K.F64: torch.float64}
CASES = [pytest.param(sizes, B, dt, id=name) for (sizes, B, dt), name in zip(K.CASES, K.CASE_IDS)]
CANARY = -7.5
GUARD = 64
OLD_BAR = {K.F32: (2e-4, 1e-5), K.F64: (1e-9, 1e-12)}         # tests/test_bnn_particles_gpu.py: gradient, cost
REFUSED = r"code -1\): bnn_particles_cost_grad: .*160 KiB"


def _id(sizes, B, dt):
    return "%s-B%d-%s" % ("x".join(map(str, sizes)), B, K.NAME[dt])


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d/%d elements differ, first at %s" % (what, len(bad), g.size, bad[0]))


def _dev(gpu, *arrays):
    return [torch.from_numpy(np.array(a)).to(gpu) for a in arrays]


def _k15(theta, sizes, X, y, c, add_prior=True, ld=None, ld_grad=None, shift=0, grad_shift=0):
    """One launch on the rows of ``theta`` (n, P) laid out at pitch ``ld`` from element ``shift`` of a 16-byte aligned buffer
    whose every other element is 1e30; ``grad`` at pitch ``ld_grad`` from element ``grad_shift`` behind a guard. Returns
    (grad (n, P), costs (n,)) after checking that every written element is finite and that the canaries in the gaps of
    ``grad``, in front of and behind ``grad`` and ``cost_out`` are intact."""
    n, P = int(theta.shape[0]), int(theta.shape[1])
    dt, dev = theta.dtype, theta.device
    ld = P if ld is None else ld
    ld_grad = P if ld_grad is None else ld_grad
    span, gspan = (n - 1) * ld + P, (n - 1) * ld_grad + P
    tbuf = torch.full((shift + span + 8,), 1e30, dtype=dt, device=dev)
    assert tbuf.data_ptr() % 16 == 0
    torch.as_strided(tbuf, (n, P), (ld, 1), shift).copy_(theta)
    gbuf = torch.full((GUARD + grad_shift + gspan + GUARD,), CANARY, dtype=dt, device=dev)
    cbuf = torch.full((8 + n + 8,), CANARY, dtype=dt, device=dev)
    lo = GUARD + grad_shift
    kernels.bnn_particles_cost_grad(tbuf[shift:shift + span], n, ld, sizes, X, y, gbuf[lo:lo + gspan], ld_grad, cbuf[8:8 + n],
                                    c["batch_size"], c["n_examples"], c["wdecay"], c["prior_mean"], c["prior_var"],
                                    add_prior=add_prior)
    grad = torch.as_strided(gbuf, (n, P), (ld_grad, 1), lo).clone()
    costs = cbuf[8:8 + n].clone()
    assert bool((gbuf[:lo] == CANARY).all()) and bool((gbuf[lo + gspan:] == CANARY).all()), "grad's guards"
    if ld_grad > P and n > 1:
        gaps = torch.as_strided(gbuf, (n - 1, ld_grad - P), (ld_grad, 1), lo + P)
        assert bool((gaps == CANARY).all()), "the gaps of grad"
    assert bool((cbuf[:8] == CANARY).all()) and bool((cbuf[8 + n:] == CANARY).all()), "cost_out's guards"
    return grad, costs


def _written(grad, costs, what):
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(costs).all()), what
    assert not bool((grad == CANARY).any()) and not bool((costs == CANARY).any()), what


def _k8(theta0, sizes, X, y, B, c):
    """K8's gradient row and cost at ``theta0`` on the minibatch: one step of the whole-step kernel whose window starts at the
    batch's rows, behind a few rows the window must not read."""
    P, dt, dev = theta0.numel(), theta0.dtype, theta0.device
    lead = min(B, 7)
    X_all = torch.cat([X.flip(0)[:lead] + 0.5, X]).contiguous()
    y_all = torch.cat([y.flip(0)[:lead] - 0.5, y]).contiguous()
    rows = {k: torch.zeros(P, dtype=dt, device=dev) for k in ("V", "grad")}
    rows.update({k: torch.ones(P, dtype=dt, device=dev) for k in ("tau", "g", "v_hat", "minv")})
    theta = theta0.clone()
    cost = torch.empty(1, dtype=dt, device=dev)
    starts = torch.tensor([lead], dtype=torch.int32, device=dev)
    kernels.bnn_fused_sghmc_steps(theta, rows["V"], rows["grad"], rows["tau"], rows["g"], rows["v_hat"], rows["minv"], sizes,
                                  X_all, y_all, starts, B, c["batch_size"], c["n_examples"], c["wdecay"], c["prior_mean"],
                                  c["prior_var"], 0.01, float(K.N_EXAMPLES), 0.05, 0, 1, 6, 0, cost)
    return rows["grad"], cost


def _check_values(case, grad, costs, what, particles=None):
    """(b): every block of every particle within its bound of the truth, and the old whole-gradient bar. Returns the per-block
    figures [(name, E, the kernel's largest error, the smallest bound)] over the particles."""
    w = K.wide(case.dtype)
    got_g, got_c = grad.cpu().numpy().astype(w), costs.cpu().numpy().astype(w)
    particles = range(case.theta.shape[0]) if particles is None else particles
    figures = {}
    failures = []
    for p in particles:
        for name, where, E, bound in K.bounds(case, p):
            err = float(np.abs(got_g[p, where] - case.truth_grad[p, where]).max()) if where is not None else float(
                abs(got_c[p] - case.truth_cost[p]))
            old = figures.get(name, (E, 0.0, float("inf")))
            figures[name] = (E, max(old[1], err), min(old[2], bound))
            if not err <= bound:
                failures.append((what, p, name, err, bound, E))
        bar_g, bar_c = OLD_BAR[case.dtype]
        dev = float(np.abs(got_g[p] - case.truth_grad[p]).max() / np.abs(case.truth_grad[p]).max())
        assert dev <= bar_g, (what, p, dev)
        assert abs(got_c[p] - case.truth_cost[p]) <= bar_c * abs(case.truth_cost[p]), (what, p)
    order = [name for name, _, _, _ in K.bounds(case, 0)]
    table = [(name,) + figures[name] for name in order]
    print("\nK15 forms %s lds %d B: %s" % (what, K.lds_bytes(case.sizes, case.B, K.ESIZE[case.dtype]), "; ".join(
        "%s E %.2e err %.2e bound %.2e" % row for row in table)))
    assert not failures, failures
    return table


# ---- a. bits against K8 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes, B, dt", CASES)
def test_weight_and_bias_gradients_are_k8_s_bits_at_every_row(gpu, sizes, B, dt):
    case = K.case(sizes, B, dt)
    assert K.k8_takes(sizes, B, dt)                       # the table records that K8 takes every row: none is passed over
    theta, X, y = _dev(gpu, case.theta, case.X, case.y)
    P = case.P
    for p in (0, K.N_PARTICLES - 1):
        want, want_cost = _k8(theta[p], sizes, X, y, B, case.consts)
        got, got_cost = _k15(theta[p:p + 1], sizes, X, y, case.consts, add_prior=False)
        _written(got, got_cost, (sizes, B, p))
        assert float(got[0, :P - 1].abs().max()) > 0.0
        _same_bits(got[0, :P - 1], want[:P - 1], "%s particle %d against K8" % (_id(sizes, B, dt), p))
        # the cost and d / d log_var: two double sums in another order in front of one cast
        for what, a, b in (("d/dlog_var", got[0, P - 1], want[P - 1]), ("cost", got_cost[0], want_cost[0])):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            if dt == K.F32:
                assert abs(a - b) <= np.spacing(np.float32(max(abs(a), abs(b)))), (what, a, b)
            else:
                assert abs(a - b) <= 1e-13 * abs(b), (what, a, b)
    print("\nK15 forms %s: K8 took the row, %d weight and bias gradients equal bit for bit" % (_id(sizes, B, dt), P - 1))


# ---- b. values against the truth, per layer block ----------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes, B, dt", CASES)
def test_every_layer_block_is_within_four_times_the_reference_s_own_error(gpu, sizes, B, dt):
    case = K.case(sizes, B, dt)
    theta, X, y = _dev(gpu, case.theta, case.X, case.y)
    grad, costs = _k15(theta, sizes, X, y, case.consts)
    _written(grad, costs, (sizes, B))
    _check_values(case, grad, costs, _id(sizes, B, dt))


# ---- c. one set of bits whatever the launch -----------------------------------------------------------------------------------------

N_BIG = 300
PROBES = (0, 1, 2, 149, 255, 256, 299)


@pytest.mark.parametrize("sizes, B, dt", [pytest.param(*c, id=_id(*c)) for c in K.LAUNCH_CASES])
def test_a_particle_has_the_bits_of_its_own_launch_whatever_the_layout(gpu, sizes, B, dt):
    P, c = K.C.n_params(sizes), K.consts(B)
    theta, X, y = _dev(gpu, *K.make_data(sizes, B, dt, n=N_BIG, seed=1))
    alone = [_k15(theta[p:p + 1], sizes, X, y, c) for p in PROBES]
    alone_g, alone_c = torch.cat([a[0] for a in alone]), torch.cat([a[1] for a in alone])
    _written(alone_g, alone_c, "alone")
    assert not torch.equal(alone_g[0], alone_g[1])
    for n in (2, 3):
        g, cst = _k15(theta[:n], sizes, X, y, c)
        _same_bits(g, alone_g[:n], "n = %d" % n)
        _same_bits(cst, alone_c[:n], "costs at n = %d" % n)
    probes = list(PROBES)
    # ld = P: rows alternate alignment where P is odd
    whole_g, whole_c = _k15(theta, sizes, X, y, c)
    _written(whole_g, whole_c, "n = 300")
    _same_bits(whole_g[probes], alone_g, "n = 300, ld = P")
    _same_bits(whole_c[probes], alone_c, "costs at n = 300")
    wide_ld = (P // 64 + 1) * 64
    layouts = [("ld = %d, ld_grad = %d" % (wide_ld, P + 5), dict(ld=wide_ld, ld_grad=P + 5)),
               ("ld = P, ld_grad = %d" % wide_ld, dict(ld_grad=wide_ld)),
               ("rows one element off 16 bytes", dict(shift=1, grad_shift=3)),
               ("ld = %d one element off 16 bytes" % wide_ld, dict(ld=wide_ld, shift=1, ld_grad=P + 1))]
    for what, layout in layouts:
        g, cst = _k15(theta, sizes, X, y, c, **layout)
        _same_bits(g, whole_g, what)
        _same_bits(cst, whole_c, "costs, " + what)
    # the minibatch as a view of a (B, D0 + 4) buffer
    ext = torch.full((B, sizes[0] + 4), 1e30, dtype=TORCH[dt], device=gpu)
    ext[:, :sizes[0]] = X
    view = ext[:, :sizes[0]]
    assert view.stride(0) == sizes[0] + 4 and not view.is_contiguous()
    g, cst = _k15(theta, sizes, view, y, c)
    _same_bits(g, whole_g, "ldx = D0 + 4")
    _same_bits(cst, whole_c, "costs, ldx = D0 + 4")
    # and the raw gradient: the same launch without the prior term
    raw, cst = _k15(theta[probes].contiguous(), sizes, X, y, c, add_prior=False)
    _same_bits(cst, alone_c, "the cost carries its weight prior either way")
    assert not torch.equal(raw, alone_g)


# ---- d. refusals ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes, top, dt", [pytest.param(*c, id=_id(*c)) for c in K.CEILINGS])
def test_one_batch_past_the_ceiling_is_refused_and_the_ceiling_runs(gpu, sizes, top, dt):
    B = top + 1
    assert K.lds_bytes(sizes, B, K.ESIZE[dt]) == 0 and kernels.bnn_particles_lds_bytes(sizes, B, TORCH[dt]) == 0
    theta, X, y = _dev(gpu, *K.make_data(sizes, B, dt, n=2))
    P, c = K.C.n_params(sizes), K.consts(B)
    grad = torch.full((2 * P,), CANARY, dtype=TORCH[dt], device=gpu)
    costs = torch.full((2,), CANARY, dtype=TORCH[dt], device=gpu)
    with pytest.raises(_lib.SgmcmcLibraryError, match=REFUSED):
        kernels.bnn_particles_cost_grad(theta.reshape(-1), 2, P, sizes, X, y, grad, P, costs, c["batch_size"], c["n_examples"],
                                        c["wdecay"], c["prior_mean"], c["prior_var"])
    torch.cuda.synchronize()
    assert bool((grad == CANARY).all()) and bool((costs == CANARY).all())      # nothing was launched
    # the largest accepted batch then runs in the same process
    case = K.case(sizes, top, dt)
    theta, X, y = _dev(gpu, case.theta, case.X, case.y)
    grad, costs = _k15(theta, sizes, X, y, case.consts)
    _written(grad, costs, (sizes, top))
    _check_values(case, grad, costs, "%s after the refusal of B = %d" % (_id(sizes, top, dt), B))


# ---- e. the head's guard ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [pytest.param(K.F32, id="f32"), pytest.param(K.F64, id="f64")])
@pytest.mark.parametrize("log_var", [-50.0, -30.0, 30.0])
def test_the_head_stays_finite_and_accurate_at_extreme_log_var(gpu, dt, log_var):
    sizes, B = [2, 4, 6, 3, 1], 5
    case = K.case(sizes, B, dt, log_var=(log_var,) * K.N_PARTICLES)
    assert np.all(case.theta[:, -1] == dt(log_var)) and np.all(np.isfinite(case.truth_grad.astype(np.float64)))
    if log_var == -50.0:                                  # exp(s) is far below the guard: 1e-16 carries the division
        assert np.exp(log_var) < 1e-5 * 1e-16
    theta, X, y = _dev(gpu, case.theta, case.X, case.y)
    grad, costs = _k15(theta, sizes, X, y, case.consts)
    _written(grad, costs, log_var)
    _check_values(case, grad, costs, "%s log_var %g" % (_id(sizes, B, dt), log_var))


@pytest.mark.parametrize("dt", [pytest.param(K.F32, id="f32"), pytest.param(K.F64, id="f64")])
def test_a_nan_particle_keeps_to_its_own_row(gpu, dt):
    sizes, B = [2, 4, 6, 3, 1], 5
    rows, X, y = K.make_data(sizes, B, dt, n=5, seed=2)
    c = K.consts(B)
    healthy, X, y = _dev(gpu, rows, X, y)
    sick = healthy.clone()
    sick[2, 3] = float("nan")                             # a weight of the first layer
    want_g, want_c = _k15(healthy, sizes, X, y, c)
    _written(want_g, want_c, "healthy")
    n, P = sick.shape
    grad = torch.full((n * P,), CANARY, dtype=TORCH[dt], device=gpu)
    costs = torch.full((n,), CANARY, dtype=TORCH[dt], device=gpu)
    kernels.bnn_particles_cost_grad(sick.reshape(-1), n, P, sizes, X, y, grad, P, costs, c["batch_size"], c["n_examples"],
                                    c["wdecay"], c["prior_mean"], c["prior_var"])
    grad = grad.reshape(n, P)
    assert bool(torch.isnan(grad[2]).all()) and bool(torch.isnan(costs[2]))
    keep = [0, 1, 3, 4]
    _same_bits(grad[keep], want_g[keep], "the neighbours of a NaN particle")
    _same_bits(costs[keep], want_c[keep], "the neighbours' costs")


# ---- f. capture -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes, B, dt", [pytest.param(*c, id=_id(*c)) for c in (K.FULL_LDS[0], K.FULL_LDS[2])])
def test_the_opt_in_at_the_full_lds_replays_the_eager_bits(gpu, sizes, B, dt):
    from pysgmcmc_amd.samplers.base_classes import graph_capture
    assert K.lds_bytes(sizes, B, K.ESIZE[dt]) == K.LDS_MAX and {K.FULL_LDS[0][2], K.FULL_LDS[2][2]} == {K.F32, K.F64}
    case = K.case(sizes, B, dt)
    theta, X, y = _dev(gpu, case.theta, case.X, case.y)
    n, P, c = K.N_PARTICLES, case.P, case.consts
    want_g, want_c = _k15(theta, sizes, X, y, c)
    flat = theta.reshape(-1).contiguous()
    grad = torch.zeros(n * P, dtype=TORCH[dt], device=gpu)
    costs = torch.zeros(n, dtype=TORCH[dt], device=gpu)

    def call():
        kernels.bnn_particles_cost_grad(flat, n, P, sizes, X, y, grad, P, costs, c["batch_size"], c["n_examples"], c["wdecay"],
                                        c["prior_mean"], c["prior_var"])

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, capture_error_mode="thread_local"):         # one stream, no parallel branches
        call()
    torch.cuda.synchronize()
    assert float(grad.abs().sum()) == 0.0                 # captured, not run
    for _ in range(2):
        grad.zero_()
        costs.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same_bits(grad.reshape(n, P), want_g, "the replayed gradient")
        _same_bits(costs, want_c, "the replayed costs")
    _check_values(case, grad.reshape(n, P), costs, "%s replayed" % _id(sizes, B, dt))
