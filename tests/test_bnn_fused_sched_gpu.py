"""The whole-step BNN kernel with a stepsize schedule inside a launch and with the relativistic SGHMC update
(include/sgmcmc_hip_fused.h, csrc/sgmcmc_bnn_fused.hip).

- a table of equal stepsizes == the by-value launch, bit for bit;
- a ramp inside one launch == the by-value kernel stepped one step per launch at each step's stepsize, bit for bit
  (this pins the table's derivation to the by-value one); chunking under the ramp is bit-exact;
- the relativistic update phase is K3: theta', p' == ``kernels.rsghmc_step`` on the gradient row the step left;
- relativistic whole steps track ``next(sampler)`` (GEMM path) and the float64 oracle trajectory;
- many chains per launch, ``FusedBNNChains`` of relativistic samplers, shared ramps, disagreeing schedules, windows
  the chains hold pending;
- ``BayesianNeuralNetwork.train`` under the burn-in ramp takes the fused path;
- the entry points' refusals."""
import ctypes
import re
from itertools import islice

import numpy as np
import pytest
import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd._lib import SgmcmcLibraryError, lib
from pysgmcmc_amd.data_batches import Placeholder, generate_batches
from pysgmcmc_amd.models.bayesian_neural_network import BayesianNeuralNetwork, BNNCost, init_mlp_params
from pysgmcmc_amd.samplers import RelativisticSGHMCSampler, SGHMCSampler, SGLDSampler
from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
from pysgmcmc_amd.stepsize_schedules import BurnInRampStepsizeSchedule, ConstantStepsizeSchedule

pytestmark = pytest.mark.gpu

SIZES, B, N = [1, 50, 50, 50, 1], 20, 100
P = 5252
WDECAY, PRIOR_MEAN, PRIOR_VAR = 1.0, 1e-6, 0.01
ROWS = {"sghmc": ("theta", "V", "grad", "tau", "g", "v_hat", "minv"),
        "sgld": ("theta", "grad", "tau", "g", "v_hat", "minv"),
        "rsghmc": ("theta", "p", "grad")}
# the samplers' other scalars in the order of kernels.step_scalars_table
OTHER = {"sghmc": (100.0, 0.05), "sgld": (1.0, 100.0), "rsghmc": (1.0, 1.0, 1.0, 0.0)}
EPS = {"sghmc": 0.01, "sgld": 1e-3, "rsghmc": 1e-3}
DTS = [torch.float32, torch.float64]
IDS = ["f32", "f64"]


def _sinc():
    rng = np.random.RandomState(1)
    X = rng.rand(N, 1)
    return X, np.sinc(X * 10 - 5).sum(axis=1)


def _n_params(sizes):
    return sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1


# ---- the C entry points through kernels.*, on rows of the test's own ------------------------------------------------

def _fresh(kind, gpu, dt, n_chains=1, stride=P, n_params=P, seed=3):
    g = torch.Generator().manual_seed(seed)
    rows = {k: torch.zeros(n_chains * stride, dtype=dt, device=gpu) for k in ROWS[kind]}
    rows["theta"] = (torch.randn(n_chains * stride, generator=g, dtype=torch.float64) * 0.3).to(dt).to(gpu)
    for k in ("tau", "g", "v_hat", "minv"):
        if k in rows:
            rows[k].fill_(1.0)
    if kind == "rsghmc":
        rows["p"] = (torch.randn(n_chains * stride, generator=g, dtype=torch.float64) * 0.7).to(dt).to(gpu)
    return rows


def _data(gpu, dt):
    X, y = _sinc()
    return torch.tensor(X, dtype=dt, device=gpu).contiguous(), torch.tensor(y, dtype=dt, device=gpu).contiguous()


def _launch(kind, rows, X, y, starts, eps, first_step, n_steps, burn, seed, costs, table=None, xi=None, n_chains=1,
            stride=None, other=None, sizes=SIZES, batch=B):
    o = OTHER[kind] if other is None else other
    net = (sizes, X, y, starts, batch, float(batch), float(X.shape[0]), WDECAY, PRIOR_MEAN, PRIOR_VAR)
    kw = dict(xi=xi, n_chains=n_chains, chain_stride=stride, scalars_steps=table)
    r = [rows[k] for k in ROWS[kind]]
    if kind == "sghmc":
        kernels.bnn_fused_sghmc_steps(*r, *net, eps, o[0], o[1], first_step, n_steps, burn, seed, costs, **kw)
    elif kind == "sgld":
        kernels.bnn_fused_sgld_steps(*r, *net, eps, o[1], o[0], first_step, n_steps, burn, seed, costs, **kw)
    else:
        kernels.bnn_fused_rsghmc_steps(*r, *net, eps, *o, first_step, n_steps, seed, costs, **kw)


def _starts(gpu, n, n_chains=1, seed=0):
    return torch.tensor(np.random.RandomState(seed).randint(0, N - B + 1, size=n_chains * n).astype(np.int32), device=gpu)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("kind", ["sghmc", "sgld", "rsghmc"])
def test_table_rows_equal_the_device_scalars_block(gpu, kind, dt):
    """Row t of the host-built table == the block sgmcmc_*_scalars_* stores on the device for stepsize t (same bits)."""
    ramp = BurnInRampStepsizeSchedule(1e-4, 1e-2, burn_in_steps=9)
    eps = [next(ramp) for _ in range(12)]
    table = kernels.step_scalars_table(kind, eps, *OTHER[kind], dtype=dt, device=gpu)
    block = torch.zeros(8, dtype=dt, device=gpu)
    for t, e in enumerate(eps):
        kernels.step_scalars(kind, block, e, *OTHER[kind])
        assert torch.equal(table[t], block[:5]), (kind, t, table[t], block[:5])


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("kind", ["sghmc", "sgld"])
def test_table_of_equal_stepsizes_is_the_by_value_launch(gpu, kind, dt):
    """14 steps across the burn-in switch (step 6): every state row and every cost, bit for bit."""
    X, y = _data(gpu, dt)
    starts = _starts(gpu, 14)
    a, b = _fresh(kind, gpu, dt), _fresh(kind, gpu, dt)
    ca, cb = torch.empty(14, dtype=dt, device=gpu), torch.empty(14, dtype=dt, device=gpu)
    _launch(kind, a, X, y, starts, EPS[kind], 0, 14, 6, 77, ca)
    table = kernels.step_scalars_table(kind, [EPS[kind]] * 14, *OTHER[kind], dtype=dt, device=gpu)
    _launch(kind, b, X, y, starts, 123.0, 0, 14, 6, 77, cb, table=table)       # (the by-value stepsize is not read)
    for k in ROWS[kind]:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(ca, cb) and torch.isfinite(ca).all()
    assert not torch.equal(a["theta"], _fresh(kind, gpu, dt)["theta"])


# ---- samplers ----------------------------------------------------------------------------------------------------------

def _ramp():
    return BurnInRampStepsizeSchedule(1e-4, 1e-2, burn_in_steps=9)


def _chain(gpu, dt, kind, schedule=None, seed=5, burn=6, init_seed=3, shared=None, **hyper):
    X, y = _sinc()
    xp, yp = Placeholder(dtype=dt, device=gpu), Placeholder(dtype=dt, device=gpu)
    gen = generate_batches(X, y, xp, yp, B, seed=1)
    if shared is not None:                            # one resident dataset for a group; own window stream per chain
        gen = type(shared)(shared.x_dev, shared.y_dev, xp, yp, shared.batch_size, np.random.RandomState(seed))
    params = init_mlp_params(1, hidden=(50, 50, 50), seed=init_seed, dtype=dt, device=gpu)
    common = dict(params=params, cost_fun=BNNCost(xp, yp, batch_size=B, n_examples=N), batch_generator=gen,
                  session=gpu, dtype=dt, seed=seed)
    if kind == "sghmc":
        s = SGHMCSampler(stepsize_schedule=schedule or ConstantStepsizeSchedule(0.01), burn_in_steps=burn, mdecay=0.05,
                         scale_grad=float(N), **common)
    elif kind == "sgld":
        s = SGLDSampler(stepsize_schedule=schedule or ConstantStepsizeSchedule(1e-3), burn_in_steps=burn, A=1.0,
                        scale_grad=float(N), **common)
    else:
        s = RelativisticSGHMCSampler(stepsize_schedule=schedule or ConstantStepsizeSchedule(0.001), **hyper, **common)
    s.sample_format = "view"
    return s


def _one_step_launches(s, kind, eps_list):
    """The EXISTING by-value entry point, one step per launch, each at its own stepsize, on the sampler's own rows."""
    gen, cost = s.batch_generator, s.cost_fun
    n = len(eps_list)
    starts = torch.as_tensor(gen.next_starts(n), dtype=torch.int32).to(s.device)
    costs = torch.empty(n, dtype=s._torch_dtype, device=s.device)
    rows = [s.arena.row(k) for k in ROWS[kind]]
    net = (s._bnn_layer_sizes(), gen.x_dev, gen.y_dev.reshape(-1))
    tail = (gen.batch_size, cost.batch_size, cost.n_examples, cost.wdecay, cost.prior_mean, cost.prior_var)
    for t, e in enumerate(eps_list):
        st, ct = starts[t:t + 1].contiguous(), costs[t:t + 1]
        if kind == "sghmc":
            kernels.bnn_fused_sghmc_steps(*rows, *net, st, *tail, e, s.scale_grad, s.mdecay, t, 1, s.burn_in_steps,
                                          s._philox_seed, ct)
        elif kind == "sgld":
            kernels.bnn_fused_sgld_steps(*rows, *net, st, *tail, e, s.scale_grad, s.A, t, 1, s.burn_in_steps,
                                         s._philox_seed, ct)
        else:
            kernels.bnn_fused_rsghmc_steps(*rows, *net, st, *tail, e, s.mass, s.speed_of_light, s.D, s.Bhat, t, 1,
                                           s._philox_seed, ct)
    return costs


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("kind", ["sghmc", "sgld", "rsghmc"])
def test_ramp_in_one_launch_is_the_by_value_kernel_step_by_step(gpu, kind, dt):
    """Chain A: the ramp inside ONE launch of 12 steps (table). Chain B: twelve one-step launches of the by-value entry
    point at the ramp's stepsizes. The relativistic by-value launches (m = c = 1) multiply by 1 / m^2 c^2 = 1 where the
    table form divides by 1: both exact, so the bits agree there too."""
    a, b = _chain(gpu, dt, kind, _ramp()), _chain(gpu, dt, kind, _ramp())
    ramp = _ramp()
    eps = [next(ramp) for _ in range(12)]
    costs_a = a.fused_bnn_steps(12)
    costs_b = _one_step_launches(b, kind, eps)
    for k in ROWS[kind]:
        assert torch.equal(a.arena.row(k), b.arena.row(k)), k
    assert torch.equal(costs_a, costs_b) and torch.isfinite(costs_a).all()
    assert a.n_iterations == 12 and a.epsilon == eps[-1] == 1e-2
    # a constant schedule gives another chain: the ramp was really applied
    c = _chain(gpu, dt, kind)
    c.fused_bnn_steps(12)
    assert not torch.equal(a.arena.row("theta"), c.arena.row("theta"))


@pytest.mark.parametrize("kind", ["sghmc", "sgld", "rsghmc"])
def test_chunking_under_the_ramp_is_bit_exact(gpu, kind):
    a, b, c = (_chain(gpu, torch.float32, kind, _ramp()) for _ in range(3))
    ca = a.fused_bnn_steps(12)
    cb = torch.cat([b.fused_bnn_steps(5), b.fused_bnn_steps(7)])       # the ramp ends inside the second chunk
    cc = torch.cat([c.fused_bnn_steps(1) for _ in range(12)])          # every chunk at one stepsize: by value
    for other, costs in ((b, cb), (c, cc)):
        for k in ROWS[kind]:
            assert torch.equal(a.arena.row(k), other.arena.row(k)), k
        assert torch.equal(ca, costs)
        assert other.epsilon == a.epsilon == 1e-2


# ---- the relativistic update phase is K3 -------------------------------------------------------------------------------

@pytest.mark.parametrize("inject", [True, False], ids=["injected_xi", "philox"])
@pytest.mark.parametrize("other", [(1.0, 1.0, 1.0, 0.0), (1.5, 0.7, 1.0, 0.0)], ids=["m1_c1_pow2", "m1.5_c0.7"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_relativistic_update_phase_is_k3(gpu, dt, other, inject):
    X, y = _data(gpu, dt)
    rows = _fresh("rsghmc", gpu, dt)
    theta0, p0 = rows["theta"].clone(), rows["p"].clone()
    xi = None
    if inject:
        xi = torch.tensor(np.random.default_rng(8).normal(size=(1, P)), dtype=dt, device=gpu).contiguous()
    cost = torch.empty(1, dtype=dt, device=gpu)
    seed, step = 11, 7
    _launch("rsghmc", rows, X, y, _starts(gpu, 1, seed=4), 2e-3, step, 1, 0, seed, cost, xi=xi, other=other)
    grad_decay = WDECAY / ((P + 3e-16) * N)           # the weight-prior term K8 leaves to the update
    kernels.rsghmc_step(theta0, p0, rows["grad"], 2e-3, *other, xi=None if xi is None else xi[0].contiguous(),
                        seed=seed, step=step, grad_decay=grad_decay)
    assert torch.equal(rows["theta"], theta0) and torch.equal(rows["p"], p0)
    assert torch.isfinite(rows["theta"]).all() and float(rows["grad"].abs().max()) > 0


# ---- relativistic whole steps against next(sampler) and the float64 oracle ----------------------------------------------

@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_relativistic_fused_steps_track_the_gemm_path(gpu, dt):
    a, b = _chain(gpu, dt, "rsghmc"), _chain(gpu, dt, "rsghmc")
    assert b.fused_bnn_available() and torch.equal(a.arena.row("p"), b.arena.row("p"))
    costs_a = torch.stack([c.reshape(()).clone() for _, c in islice(a, 14)])
    costs_b = b.fused_bnn_steps(14)
    tol = 2e-4 if dt == torch.float32 else 1e-9
    for k in ("theta", "p"):
        ra, rb = a.arena.row(k), b.arena.row(k)
        dev = float((ra - rb).abs().max()) / float(ra.abs().max())
        print("relativistic K8 vs next(sampler), %s, %s: %.3g of max |.|" % (dt, k, dev))
        assert dev <= tol, k
    assert torch.allclose(costs_a, costs_b, rtol=1e-4 if dt == torch.float32 else 1e-9)
    assert b.n_iterations == 14
    next(a); next(b)                                          # the chain continues seamlessly on the per-step path
    ta = a.arena.row("theta")
    assert float((ta - b.arena.row("theta")).abs().max()) <= 2 * tol * float(ta.abs().max())


def _split(flat, sizes):
    out, off = [], 0
    for l in range(len(sizes) - 1):
        nin, nout = sizes[l], sizes[l + 1]
        out.append(flat[off:off + nin * nout].reshape(nin, nout))
        off += nin * nout
        out.append(flat[off:off + nout])
        off += nout
    out.append(flat[off:off + 1].reshape(1, 1))
    return out


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_relativistic_fused_steps_track_the_fp64_oracle(gpu, oracle, dt):
    """14 steps with injected noise against the float64 trajectory of ``oracle.bnn_cost_and_grad`` +
    ``opbyop_rsghmc_step`` from the same start, windows and noise. Bar: 2e-4 (f32) / 1e-9 (f64) of max |.|, the bar the
    fused SGHMC kernel and the GEMM path meet against their golden trajectory. The per-step path (``next(sampler)``) is
    run on the same trajectory and both deviations are printed. Measured on an MI355X after 14 steps, K8 and the per-step
    path alike: f32 theta 1.7e-7, p 1.6e-7 of max |.|; f64 theta 4e-18, p 9e-17 (the bar holds with room, so it is not widened)."""
    n = 14
    npdt = np.float32 if dt == torch.float32 else np.float64
    xi_h = np.random.default_rng(21).normal(size=(n, P)).astype(npdt)
    xi = torch.tensor(xi_h, device=gpu)
    a, b = _chain(gpu, dt, "rsghmc"), _chain(gpu, dt, "rsghmc")
    theta0 = b.arena.row("theta").cpu().numpy().astype(np.float64)
    p0 = b.arena.row("p").cpu().numpy().astype(np.float64)
    # K8 on chain b's rows, windows from its generator
    starts_h = b.batch_generator.next_starts(n)
    costs = torch.empty(n, dtype=dt, device=gpu)
    gen = b.batch_generator
    kernels.bnn_fused_rsghmc_steps(b.arena.row("theta"), b.arena.row("p"), b.arena.row("grad"), SIZES, gen.x_dev,
                                   gen.y_dev.reshape(-1), torch.as_tensor(starts_h, dtype=torch.int32).to(gpu), B, B, N,
                                   WDECAY, PRIOR_MEAN, PRIOR_VAR, 0.001, 1.0, 1.0, 1.0, 0.0, 0, n, b._philox_seed, costs,
                                   xi=xi)
    # the per-step path on chain a: same windows (same generator seed), same noise
    a.noise_source = lambda step, n_: xi[step]
    costs_a = torch.stack([c.reshape(()).clone() for _, c in islice(a, n)])
    # float64 oracle
    Xh, yh = gen.x_dev.cpu().numpy().astype(np.float64), gen.y_dev.cpu().numpy().astype(np.float64).reshape(-1, 1)
    st = oracle.OpByOpState(theta0, np.float64)
    st.p = p0.reshape(-1, 1).copy()
    costs_o = []
    for t in range(n):
        w = slice(int(starts_h[t]), int(starts_h[t]) + B)
        c64, g64 = oracle.bnn_cost_and_grad(_split(st.theta.ravel().copy(), SIZES), Xh[w], yh[w], float(B), float(N),
                                            WDECAY, PRIOR_MEAN, PRIOR_VAR)
        costs_o.append(c64)
        oracle.opbyop_rsghmc_step(st, np.concatenate([g.ravel() for g in g64]), 0.001, 1.0, 1.0, 1.0, 0.0,
                                  xi_h[t].astype(np.float64))
    tol = 2e-4 if dt == torch.float32 else 1e-9
    worst = {}
    for name, s in (("K8", b), ("next(sampler)", a)):
        for k, ref in (("theta", st.theta.ravel()), ("p", st.p.ravel())):
            got = s.arena.row(k).cpu().numpy().astype(np.float64)
            worst[name, k] = float(np.abs(got - ref).max() / np.abs(ref).max())
            print("relativistic %s vs the fp64 oracle after %d steps, %s, %s: %.3g of max |.|" % (name, n, dt, k, worst[name, k]))
    for k in ("theta", "p"):
        assert worst["K8", k] <= tol, (k, worst)
    rt = 1e-4 if dt == torch.float32 else 1e-9
    assert np.allclose(costs.cpu().numpy(), np.array(costs_o), rtol=rt)
    assert np.allclose(costs_a.cpu().numpy(), np.array(costs_o), rtol=rt)


# ---- many chains -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_table", [False, True], ids=["by_value", "table"])
def test_five_relativistic_chains_in_one_launch(gpu, with_table):
    """blockIdx = chain: 5 chains in one launch == 5 single-chain launches with seed_base + c (bit-exact)."""
    dt, n_steps = torch.float32, 9
    stride = ((P + 63) // 64) * 64
    X, y = _data(gpu, dt)
    starts = _starts(gpu, n_steps, n_chains=5).view(5, n_steps)
    table = None
    if with_table:
        eps = [1e-3 + 2e-4 * t for t in range(n_steps)]
        table = kernels.step_scalars_table("rsghmc", eps, *OTHER["rsghmc"], dtype=dt, device=gpu)
    multi = _fresh("rsghmc", gpu, dt, n_chains=5, stride=stride)
    init = {k: v.clone() for k, v in multi.items()}
    cm = torch.empty(5 * n_steps, dtype=dt, device=gpu)
    _launch("rsghmc", multi, X, y, starts.reshape(-1).contiguous(), 1e-3, 2, n_steps, 0, 100, cm, table=table, n_chains=5,
            stride=stride)
    for c in range(5):
        one = {k: v[c * stride:(c + 1) * stride].clone() for k, v in init.items()}
        c1 = torch.empty(n_steps, dtype=dt, device=gpu)
        _launch("rsghmc", one, X, y, starts[c].contiguous(), 1e-3, 2, n_steps, 0, 100 + c, c1, table=table, n_chains=1,
                stride=stride)
        for k in ("theta", "p"):
            assert torch.equal(multi[k][c * stride:c * stride + P], one[k][:P]), (c, k)
            assert torch.equal(multi[k][c * stride + P:(c + 1) * stride], init[k][c * stride + P:(c + 1) * stride])
        assert torch.equal(cm[c * n_steps:(c + 1) * n_steps], c1)
    assert not torch.equal(multi["theta"][:P], multi["theta"][stride:stride + P])


def _relativistic_members(gpu, n, schedule, seed0=40):
    first = _chain(gpu, torch.float32, "rsghmc", schedule(), seed=seed0, init_seed=seed0)
    members = [first]
    for c in range(1, n):
        members.append(_chain(gpu, torch.float32, "rsghmc", schedule(), seed=seed0 + c, init_seed=seed0 + c,
                              shared=first.batch_generator))
    return members


@pytest.mark.parametrize("schedule", [lambda: ConstantStepsizeSchedule(0.001), _ramp], ids=["constant", "shared_ramp"])
def test_group_of_relativistic_chains_equals_individual_chains(gpu, schedule):
    group = FusedBNNChains(_relativistic_members(gpu, 6, schedule))
    solo = _relativistic_members(gpu, 6, schedule)
    assert group.n_chains == 6 and group.theta().shape == (6, P)
    costs = torch.cat([group.steps(5), group.steps(9)], dim=1)
    for c, s in enumerate(solo):
        c1 = torch.cat([s.fused_bnn_steps(5), s.fused_bnn_steps(9)])
        for k in ("theta", "p"):
            assert torch.equal(group.samplers[c].arena.row(k), s.arena.row(k)), (c, k)
        assert torch.equal(costs[c], c1)
        assert group.samplers[c].epsilon == s.epsilon
    assert group.n_iterations == 14 and not torch.equal(group.theta()[0], group.theta()[1])
    # a member keeps working as an ordinary sampler on the shared memory
    a, b = group.samplers[2], solo[2]
    next(a); next(b)
    assert torch.allclose(a.arena.row("theta"), b.arena.row("theta"), rtol=1e-5, atol=1e-6)


def test_groups_refuse_mismatched_chains_and_disagreeing_schedules(gpu):
    members = _relativistic_members(gpu, 3, _ramp)
    members[1].stepsize_schedule = BurnInRampStepsizeSchedule(1e-4, 1e-2, burn_in_steps=5)
    group = FusedBNNChains(members)
    before = group.theta().clone()
    with pytest.raises(ValueError, match="one stepsize sequence"):
        group.steps(4)
    torch.cuda.synchronize()
    assert torch.equal(group.theta(), before)
    # hyper-parameters of the relativistic sampler are compared, sampler classes are not mixed
    ok = _relativistic_members(gpu, 2, _ramp, seed0=60)
    heavy = _chain(gpu, torch.float32, "rsghmc", _ramp(), seed=61, init_seed=61, shared=ok[0].batch_generator, mass=2.0)
    with pytest.raises(ValueError, match="differs from chain 0"):
        FusedBNNChains([ok[0], heavy])
    sghmc = _chain(gpu, torch.float32, "sghmc", seed=61, init_seed=61, shared=ok[0].batch_generator)
    with pytest.raises(ValueError, match="does not fit"):
        FusedBNNChains([ok[0], sghmc])


def _sghmc_pair(gpu, dt):
    first = _chain(gpu, dt, "sghmc", seed=5, init_seed=5)
    return [first, _chain(gpu, dt, "sghmc", seed=6, init_seed=6, shared=first.batch_generator)]


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_group_takes_each_chains_pending_window_first(gpu, dt):
    """A chain resumed from a ``state_dict`` with a ``pending_window`` (or stepped with ``next()`` under window prefetch)
    holds a window its generator has already drawn. The group hands it to the kernel as that chain's first start, as
    ``fused_bnn_steps`` does: same rows, same costs, nothing left pending, generators at the same place."""
    grouped, twins = _sghmc_pair(gpu, dt), _sghmc_pair(gpu, dt)
    for pair in (grouped, twins):
        for s, start in zip(pair, (17, 63)):
            s._pending_window = (start, False)
    costs = FusedBNNChains(grouped).steps(5)
    for c, (a, b) in enumerate(zip(grouped, twins)):
        c1 = b.fused_bnn_steps(5)
        for k in a._FUSED_ROWS:
            assert torch.equal(a.arena.row(k), b.arena.row(k)), (c, k)
        assert torch.equal(costs[c], c1) and torch.isfinite(c1).all(), c
        assert a._pending_window is None and b._pending_window is None
        assert int(a.batch_generator.next_starts(1)[0]) == int(b.batch_generator.next_starts(1)[0]), c
        assert a.n_iterations == b.n_iterations == 5


# ---- the user-visible hole ---------------------------------------------------------------------------------------------

def test_bnn_train_under_the_burn_in_ramp_takes_the_fused_path(gpu):
    """``BayesianNeuralNetwork(stepsize_schedule=BurnInRampStepsizeSchedule(...)).train`` used to die in its first
    512-step chunk. Terms of ``test_bnn_train_uses_the_fused_path``; the MSE bar is the reference's for a constant 0.01
    (``test_train_predict.py:48``), the ramp ends there."""
    X, y = _sinc()
    Xt = np.linspace(0, 1, 100)[:, None]
    yt = np.sinc(Xt * 10 - 5).sum(axis=1)
    res = {}
    for fused in (True, False):
        bnn = BayesianNeuralNetwork(session=gpu, dtype=torch.float32, burn_in_steps=1000, n_nets=10, seed=1,
                                    stepsize_schedule=BurnInRampStepsizeSchedule(1e-3, 1e-2, 1000))
        bnn.use_fused_steps = fused
        bnn.train(X, y)
        assert bnn.used_fused_steps is fused and len(bnn.samples) == 10
        assert bnn.sampler.epsilon == 1e-2
        m, v = bnn.predict(Xt)
        res[fused] = (m, bnn.sampler.n_iterations)
        mse = float(np.mean((yt - m) ** 2))
        print("ramp 1e-3 -> 1e-2 over 1000 steps, fused=%s: %d iterations, test MSE %.3g" % (fused, res[fused][1], mse))
        assert mse < 0.1
    assert res[True][1] == res[False][1]
    assert np.abs(res[True][0] - res[False][0]).max() < 0.2
    # four chains through the fused group, every chain with its own copy of the ramp
    four = BayesianNeuralNetwork(session=gpu, dtype=torch.float32, burn_in_steps=1000, sample_steps=100, n_nets=20, seed=1,
                                 n_chains=4, stepsize_schedule=BurnInRampStepsizeSchedule(1e-3, 1e-2, 1000))
    four.train(X, y)
    assert four.used_fused_steps and four.chains.n_chains == 4 and len(four.samples) == 20
    assert four.sampler.n_iterations == 1000 + 5 * 100 + 1 and all(s.epsilon == 1e-2 for s in four.chains.samplers)
    m, v = four.predict(Xt)
    print("4 chains under the ramp: test MSE %.3g" % float(np.mean((yt - m) ** 2)))
    assert np.isfinite(m).all() and np.isfinite(v).all()


# ---- refusals: host checks only, nothing launched, nothing written ------------------------------------------------------

_RS, _RB, _RN = [3, 7, 13, 1], 5, 40            # n_params 147


def _refusal_case(gpu, kind):
    rng = np.random.default_rng(9)
    X = torch.tensor(rng.uniform(-1, 1, size=(_RN, 3)).astype(np.float32), device=gpu)
    y = torch.tensor(rng.normal(size=_RN).astype(np.float32), device=gpu)
    rows = {k: torch.tensor(rng.normal(size=148).astype(np.float32), device=gpu)[:147] for k in ROWS[kind]}
    costs = torch.full((1,), 7.0, device=gpu)
    return rows, X, y, torch.zeros(1, dtype=torch.int32, device=gpu), costs


def _refused(gpu, kind, rows, X, y, starts, costs, msg, **kw):
    watched = list(rows.values()) + [costs]
    before = [t.clone() for t in watched if t is not None]
    with pytest.raises(SgmcmcLibraryError, match=re.escape(msg)):
        _launch(kind, rows, X, y, starts, 1e-3, 0, 1, 0, 0, costs, sizes=_RS, batch=_RB, **kw)
    torch.cuda.synchronize()
    for t, b in zip([t for t in watched if t is not None], before):
        assert torch.equal(t, b)


def test_refusals_of_the_new_entry_points(gpu):
    assert _n_params(_RS) == 147
    # a NULL table to a _sched_ entry (the wrapper never passes one: the C entry directly)
    for kind in ("sghmc", "sgld"):
        rows, X, y, starts, costs = _refusal_case(gpu, kind)
        before = {k: v.clone() for k, v in rows.items()}
        f = getattr(lib(), "sgmcmc_bnn_fused_%s_sched_steps_f32" % kind)
        arr = (ctypes.c_int * len(_RS))(*_RS)
        rc = f(*[rows[k].data_ptr() for k in ROWS[kind]], 147, 148, 1, arr, 3, X.data_ptr(), y.data_ptr(), _RN,
               starts.data_ptr(), _RB, float(_RB), float(_RN), WDECAY, PRIOR_MEAN, PRIOR_VAR, None, float(_RN), 0.05, 0, 1,
               0, 0, None, costs.data_ptr(), torch.cuda.current_stream(gpu).cuda_stream)
        assert rc == -1 and b"scalars_steps is NULL" in lib().sgmcmc_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(rows[k], before[k]) for k in rows) and float(costs[0]) == 7.0
    rows, X, y, starts, costs = _refusal_case(gpu, "rsghmc")
    _refused(gpu, "rsghmc", dict(rows, p=None), X, y, starts, costs, "NULL argument")
    buf = torch.zeros(147 + 4, device=gpu)
    _refused(gpu, "rsghmc", dict(rows, p=buf[1:148]), X, y, starts, costs, "16-B aligned")
    _refused(gpu, "rsghmc", dict(rows, theta=buf[1:148]), X, y, starts, costs, "16-B aligned")
    _refused(gpu, "rsghmc", rows, X, y, starts, costs, "n_params % 4 == 0", xi=torch.zeros(147, device=gpu))
    table = kernels.step_scalars_table("sghmc", [1e-3], *OTHER["sghmc"], dtype=torch.float32, device=gpu)
    rows, X, y, starts, costs = _refusal_case(gpu, "sghmc")
    _refused(gpu, "sghmc", rows, X, y, starts, costs, "n_params % 4 == 0", xi=torch.zeros(147, device=gpu), table=table)
    _refused(gpu, "sghmc", dict(rows, minv=buf[1:148]), X, y, starts, costs, "16-B aligned", table=table)
    # the accepted twin of these launches runs
    rows, X, y, starts, costs = _refusal_case(gpu, "rsghmc")
    _launch("rsghmc", rows, X, y, starts, 1e-3, 0, 1, 0, 0, costs, sizes=_RS, batch=_RB)
    torch.cuda.synchronize()
    assert torch.isfinite(rows["theta"]).all() and float(costs[0]) != 7.0
