"""The whole-step BNN kernel keeping every k-th sample in a device trace inside the launch
(include/sgmcmc_hip_fused_trace.h, csrc/sgmcmc_bnn_fused.hip, the FUSED_TRACE instantiations).

- the kept rows are the chain: bit for bit the ``theta`` of a twin chain advanced by untraced launches that end at the kept
  steps, for each update x f32 / f64 x by value / table, two small nets (P = 147: odd rows, scalar loops, a 3-element tail of
  the update; P = 68: pair paths, no tail), two phases; rows outside the kept ones are not touched;
- tracing leaves the chain alone: every state row and every cost equal the untraced launch's;
- the burn-in switch between two kept steps; several chains per launch, with padding between their slabs;
- chunks through ``fused_bnn_steps(trace=...)`` thin as one run; ``FusedBNNChains.collect`` is one launch and the tensor it
  was; ``DeviceTrace.record(fused=True)`` feeds the per-parameter ESS."""
import ctypes

import numpy as np
import pytest
import torch

from pysgmcmc_amd import _lib, kernels
from pysgmcmc_amd.data_batches import Placeholder, generate_batches
from pysgmcmc_amd.diagnostics.device_trace import DeviceTrace, effective_n_all, effective_sample_sizes_of
from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
from pysgmcmc_amd.samplers import RelativisticSGHMCSampler, SGHMCSampler, SGLDSampler
from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
from pysgmcmc_amd.stepsize_schedules import BurnInRampStepsizeSchedule, ConstantStepsizeSchedule

pytestmark = pytest.mark.gpu

N = 40
NETS = {"p147": ([3, 7, 13, 1], 5), "p68": ([2, 6, 6, 1], 4)}       # layer sizes, batch
WDECAY, PRIOR_MEAN, PRIOR_VAR = 1.0, 1e-6, 0.01
ROWS = {"sghmc": ("theta", "V", "grad", "tau", "g", "v_hat", "minv"),
        "sgld": ("theta", "grad", "tau", "g", "v_hat", "minv"),
        "rsghmc": ("theta", "p", "grad")}
# the samplers' scalars after eps, in the order of kernels.step_scalars / step_scalars_table
OTHER = {"sghmc": (40.0, 0.05), "sgld": (1.0, 40.0), "rsghmc": (1.5, 0.7, 1.0, 0.0)}
EPS = {"sghmc": 0.01, "sgld": 1e-3, "rsghmc": 1e-3}
KINDS = ["sghmc", "sgld", "rsghmc"]
DTS = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
STEPS, EVERY, ROW0, CAP = 13, 4, 2, 7


def _n_params(sizes):
    return sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1


def _stride(sizes):
    return (_n_params(sizes) + 3) // 4 * 4


def _data(gpu, dt, sizes):
    rng = np.random.RandomState(1)
    X = rng.rand(N, sizes[0])
    y = np.sinc(X * 10 - 5).sum(axis=1)
    return torch.tensor(X, dtype=dt, device=gpu).contiguous(), torch.tensor(y, dtype=dt, device=gpu).contiguous()


def _fresh(kind, gpu, dt, sizes, n_chains=1, seed=3):
    n = n_chains * _stride(sizes)
    g = torch.Generator().manual_seed(seed)
    rows = {k: torch.zeros(n, dtype=dt, device=gpu) for k in ROWS[kind]}
    rows["theta"] = (torch.randn(n, generator=g, dtype=torch.float64) * 0.3).to(dt).to(gpu)
    for k in ("tau", "g", "v_hat", "minv"):
        if k in rows:
            rows[k].fill_(1.0)
    if kind == "rsghmc":
        rows["p"] = (torch.randn(n, generator=g, dtype=torch.float64) * 0.7).to(dt).to(gpu)
    return rows


def _clone(rows):
    return {k: v.clone() for k, v in rows.items()}


def _starts(gpu, n, batch, n_chains=1, seed=0):
    return torch.tensor(np.random.RandomState(seed).randint(0, N - batch + 1, size=n_chains * n).astype(np.int32), device=gpu)


def _stepsizes(table):
    if not table:
        return None
    ramp = BurnInRampStepsizeSchedule(1e-4, 1e-2, burn_in_steps=9)
    return [next(ramp) for _ in range(STEPS)]


def _launch(kind, rows, net, X, y, starts, t0, t1, burn, seed, costs, eps_list=None, n_chains=1, **trace):
    """Steps [t0, t1) of the run (first_step = t0) through the one Python caller of every entry point."""
    sizes, batch = net
    table = None
    if eps_list is not None:
        table = kernels.step_scalars_table(kind, eps_list[t0:t1], *OTHER[kind], dtype=costs.dtype, device=costs.device)
    kernels.bnn_fused_steps(kind, [rows[k] for k in ROWS[kind]], sizes, X, y, starts, batch, float(batch), float(N), WDECAY,
                            PRIOR_MEAN, PRIOR_VAR, (EPS[kind],) + OTHER[kind], t0, t1 - t0, burn, seed, costs,
                            n_chains=n_chains, chain_stride=_stride(sizes), scalars_steps=table, **trace)


def _kept_steps(phase, n_steps=STEPS, every=EVERY):
    """1-based counts of steps after which a sample is kept."""
    return [t + 1 for t in range(n_steps) if (phase + t + 1) % every == 0]


def _snapshots(kind, rows, net, X, y, starts, burn, seed, eps_list, kept):
    """theta after each step of ``kept``, from UNTRACED launches that end exactly there (and one more to the run's end)."""
    P, dt, gpu = _n_params(net[0]), rows["theta"].dtype, rows["theta"].device
    out, t0 = [], 0
    for t1 in kept + ([STEPS] if kept[-1] != STEPS else []):
        _launch(kind, rows, net, X, y, starts[t0:t1].contiguous(), t0, t1, burn, seed, torch.empty(t1 - t0, dtype=dt, device=gpu),
                eps_list)
        if t1 in kept:
            out.append(rows["theta"][:P].clone())
        t0 = t1
    return torch.stack(out)


def _nan_trace(gpu, dt, *shape):
    return torch.full(shape, float("nan"), dtype=dt, device=gpu)


def _check_trace(trace, want, row0=ROW0):
    k = want.shape[0]
    assert torch.equal(trace[row0:row0 + k], want)
    assert torch.isnan(trace[:row0]).all() and torch.isnan(trace[row0 + k:]).all()
    assert torch.isfinite(want).all() and not torch.equal(want[0], want[-1])


@pytest.mark.parametrize("phase", [0, 3])
@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("table", [False, True], ids=["by_value", "table"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_rows_are_the_chain_and_tracing_leaves_it_alone(gpu, kind, dt, table, net, phase):
    """13 steps, every 4th kept, into rows 2.. of a NaN-filled trace of 7 rows: phase 0 keeps steps 4, 8, 12, phase 3 keeps
    steps 1, 5, 9, 13 (the launch's first and last). The burn-in of SGHMC / SGLD ends at step 6, inside the launch."""
    sizes, batch = NETS[net]
    P = _n_params(sizes)
    X, y = _data(gpu, dt, sizes)
    starts = _starts(gpu, STEPS, batch)
    eps_list = _stepsizes(table)
    a = _fresh(kind, gpu, dt, sizes)
    b, c = _clone(a), _clone(a)
    ca, cb = torch.empty(STEPS, dtype=dt, device=gpu), torch.empty(STEPS, dtype=dt, device=gpu)
    trace = _nan_trace(gpu, dt, CAP, P)
    _launch(kind, a, NETS[net], X, y, starts, 0, STEPS, 6, 77, ca, eps_list, trace=trace, trace_every=EVERY, trace_row=ROW0,
            trace_phase=phase)
    _launch(kind, b, NETS[net], X, y, starts, 0, STEPS, 6, 77, cb, eps_list)
    kept = _kept_steps(phase)
    assert kept == ([4, 8, 12] if phase == 0 else [1, 5, 9, 13])
    _check_trace(trace, _snapshots(kind, c, NETS[net], X, y, starts, 6, 77, eps_list, kept))
    # the traced chain is the untraced one: every row (the padding of the row included) and every cost
    for k in ROWS[kind]:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    assert torch.equal(ca, cb) and torch.isfinite(ca).all()
    if phase == 3:
        assert torch.equal(trace[ROW0 + 3], a["theta"][:P])        # the last kept row is where the chain stands


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("kind", ["sghmc", "sgld"])
def test_burn_in_switch_between_two_kept_steps(gpu, kind, dt):
    """burn_in_steps = 6 falls between the kept steps 4 and 8. Against a run that stays in burn-in (13): the same row at
    step 4, another at step 8 -- the switch took place inside the traced launch, where the snapshot twin has it."""
    net = NETS["p147"]
    sizes, batch = net
    P = _n_params(sizes)
    X, y = _data(gpu, dt, sizes)
    starts = _starts(gpu, STEPS, batch, seed=4)
    a = _fresh(kind, gpu, dt, sizes)
    c, d = _clone(a), _clone(a)
    costs = torch.empty(STEPS, dtype=dt, device=gpu)
    trace, still = _nan_trace(gpu, dt, CAP, P), _nan_trace(gpu, dt, CAP, P)
    kw = dict(trace_every=EVERY, trace_row=ROW0, trace_phase=0)
    _launch(kind, a, net, X, y, starts, 0, STEPS, 6, 77, costs, trace=trace, **kw)
    _check_trace(trace, _snapshots(kind, c, net, X, y, starts, 6, 77, None, [4, 8, 12]))
    _launch(kind, d, net, X, y, starts, 0, STEPS, STEPS, 77, costs, trace=still, **kw)
    assert torch.equal(trace[ROW0], still[ROW0]) and not torch.equal(trace[ROW0 + 1], still[ROW0 + 1])
    for k in ROWS[kind]:
        assert torch.equal(a[k], c[k]), k


def _raw_traced_launch(kind, rows, net, X, y, starts, n_steps, burn, seed, costs, n_chains, trace, trace_stride, capacity, row,
                       every, phase):
    """The C entry itself: the one way to a chain stride of the trace above capacity * P."""
    sizes, batch = net
    dt = costs.dtype
    real = ctypes.c_float if dt == torch.float32 else ctypes.c_double
    f = getattr(_lib.lib(), "sgmcmc_bnn_fused_trace_steps_" + ("f32" if dt == torch.float32 else "f64"))
    ptrs = [rows[k].data_ptr() for k in ROWS[kind]]
    # the entry's order: SGLD takes eps, scale_grad, A
    o = OTHER[kind]
    scalars = [EPS[kind]] + ([o[1], o[0]] if kind == "sgld" else list(o))
    with torch.cuda.device(costs.device):
        rc = f(KINDS.index(kind), (ctypes.c_void_p * len(ptrs))(*ptrs), len(ptrs), _n_params(sizes), _stride(sizes), n_chains,
               (ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, X.data_ptr(), y.data_ptr(), N, starts.data_ptr(), batch,
               float(batch), float(N), WDECAY, PRIOR_MEAN, PRIOR_VAR, (real * len(scalars))(*scalars), len(scalars), None, 0,
               n_steps, burn, seed, None, costs.data_ptr(), trace.data_ptr(), trace_stride, capacity, row, every, phase,
               torch.cuda.current_stream(costs.device).cuda_stream)
    _lib.check(rc, "sgmcmc_bnn_fused_trace_steps")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_several_chains_fill_their_own_slabs(gpu, kind, dt):
    """Three chains (chain_stride 148 for 147 parameters) in one launch: chain c's slab is the trace of the same chain
    launched alone; with a trace chain stride above capacity * P the padding between the slabs stays as it was."""
    net = NETS["p147"]
    sizes, batch = net
    P, stride, m = _n_params(sizes), _stride(sizes), 3
    assert (P, stride) == (147, 148)
    X, y = _data(gpu, dt, sizes)
    starts = _starts(gpu, STEPS, batch, n_chains=m, seed=2)
    init = _fresh(kind, gpu, dt, sizes, n_chains=m)
    multi, padded = _clone(init), _clone(init)
    cm, cp = torch.empty(m * STEPS, dtype=dt, device=gpu), torch.empty(m * STEPS, dtype=dt, device=gpu)
    trace = _nan_trace(gpu, dt, m, CAP, P)
    _launch(kind, multi, net, X, y, starts, 0, STEPS, 6, 100, cm, n_chains=m, trace=trace, trace_every=EVERY, trace_row=ROW0,
            trace_phase=3)
    pad = 5
    slabs = _nan_trace(gpu, dt, m, CAP * P + pad)
    _raw_traced_launch(kind, padded, net, X, y, starts, STEPS, 6, 100, cp, m, slabs, CAP * P + pad, CAP, ROW0, EVERY, 3)
    for c in range(m):
        one = {k: v[c * stride:(c + 1) * stride].clone() for k, v in init.items()}
        c1 = torch.empty(STEPS, dtype=dt, device=gpu)
        solo = _nan_trace(gpu, dt, CAP, P)
        _launch(kind, one, net, X, y, starts[c * STEPS:(c + 1) * STEPS].contiguous(), 0, STEPS, 6, 100 + c, c1, trace=solo,
                trace_every=EVERY, trace_row=ROW0, trace_phase=3)
        assert torch.equal(trace[c][ROW0:ROW0 + 4], solo[ROW0:ROW0 + 4]) and torch.isfinite(solo[ROW0:ROW0 + 4]).all(), c
        assert torch.isnan(trace[c][:ROW0]).all() and torch.isnan(trace[c][ROW0 + 4:]).all()
        assert torch.equal(slabs[c][:CAP * P].view(CAP, P)[ROW0:ROW0 + 4], solo[ROW0:ROW0 + 4]), c
        assert torch.isnan(slabs[c][:ROW0 * P]).all() and torch.isnan(slabs[c][(ROW0 + 4) * P:]).all(), c
        for k in ROWS[kind]:
            assert torch.equal(multi[k][c * stride:(c + 1) * stride], one[k]), (c, k)
            assert torch.equal(padded[k][c * stride:(c + 1) * stride], one[k]), (c, k)
        assert torch.equal(cm[c * STEPS:(c + 1) * STEPS], c1) and torch.equal(cp[c * STEPS:(c + 1) * STEPS], c1)
    assert not torch.equal(trace[0][ROW0], trace[1][ROW0])


# ---- samplers ----------------------------------------------------------------------------------------------------------

def _chain(gpu, dt, kind, net="p147", schedule=None, seed=5, burn=6):
    sizes, batch = NETS[net]
    rng = np.random.RandomState(1)
    X = rng.rand(N, sizes[0])
    y = np.sinc(X * 10 - 5).sum(axis=1)
    xp, yp = Placeholder(dtype=dt, device=gpu), Placeholder(dtype=dt, device=gpu)
    gen = generate_batches(X, y, xp, yp, batch, seed=1)
    params = init_mlp_params(sizes[0], hidden=tuple(sizes[1:-1]), seed=3, dtype=dt, device=gpu)
    common = dict(params=params, cost_fun=BNNCost(xp, yp, batch_size=batch, n_examples=N), batch_generator=gen,
                  session=gpu, dtype=dt, seed=seed)
    if kind == "sghmc":
        s = SGHMCSampler(stepsize_schedule=schedule or ConstantStepsizeSchedule(0.01), burn_in_steps=burn, mdecay=0.05,
                         scale_grad=float(N), **common)
    elif kind == "sgld":
        s = SGLDSampler(stepsize_schedule=schedule or ConstantStepsizeSchedule(1e-3), burn_in_steps=burn, A=1.0,
                        scale_grad=float(N), **common)
    else:
        s = RelativisticSGHMCSampler(stepsize_schedule=schedule or ConstantStepsizeSchedule(0.001), **common)
    s.sample_format = "view"
    return s


def _ramp():
    return BurnInRampStepsizeSchedule(1e-4, 1e-2, burn_in_steps=9)


@pytest.mark.parametrize("schedule", [None, _ramp], ids=["constant", "ramp"])
@pytest.mark.parametrize("kind", KINDS)
def test_chunks_thin_as_one_run(gpu, kind, schedule):
    """Chunks of 5, 7 and 1 steps with keep_every = 4 keep steps 4 | 8, 12 | none: the trace of one chunk of 13."""
    dt = torch.float32
    mk = (lambda: None) if schedule is None else schedule
    a, b, c = (_chain(gpu, dt, kind, schedule=mk()) for _ in range(3))
    assert a.fused_bnn_available()
    P = a.arena.n
    whole, parts = DeviceTrace(P, 3, gpu, dt), DeviceTrace(P, 3, gpu, dt)
    ca = a.fused_bnn_steps(13, whole, keep_every=4)
    seen, cb = [], []
    for n in (5, 7, 1):
        cb.append(b.fused_bnn_steps(n, parts, keep_every=4))
        seen.append((len(parts), parts.steps_since_kept))
    assert seen == [(1, 1), (3, 0), (3, 1)] and (len(whole), whole.steps_since_kept) == (3, 1)
    assert torch.equal(whole.values(), parts.values()) and torch.isfinite(whole.values()).all()
    assert not torch.equal(whole.values()[0], whole.values()[2])
    cc = c.fused_bnn_steps(13)                                  # the untraced call: same chain, same costs
    for k in ROWS[kind]:
        assert torch.equal(a.arena.row(k), b.arena.row(k)) and torch.equal(a.arena.row(k), c.arena.row(k)), k
    assert torch.equal(ca, cc) and torch.equal(ca, torch.cat(cb))
    assert a.n_iterations == b.n_iterations == 13 and a.epsilon == b.epsilon == c.epsilon
    assert whole.param_shapes == list(a.arena.shapes) and whole.param_offsets == list(a.arena.offsets)
    # a full trace refuses the next kept sample before anything moves
    with pytest.raises(IndexError):
        a.fused_bnn_steps(3, whole, keep_every=4)
    assert a.n_iterations == 13


def _sinc(n=100):
    rng = np.random.RandomState(1)
    X = rng.rand(n, 1)
    return X, np.sinc(X * 10 - 5).sum(axis=1)


@pytest.fixture(scope="module")
def collected(gpu):
    """``collect(4, every=5)`` of three sinc-net chains whose burn-in ends at step 7, the looped twin's tensor, and how
    often the launch was asked for."""
    X, y = _sinc()
    kw = dict(batch_size=20, seed=31, dtype=torch.float32, device=gpu, burn_in_steps=7)
    group, twin = FusedBNNChains.for_dataset(X, y, 3, **kw), FusedBNNChains.for_dataset(X, y, 3, **kw)
    calls, launch = [], kernels.bnn_fused_steps

    def counting(*args, **kwargs):
        calls.append(kwargs.get("trace_every"))
        return launch(*args, **kwargs)

    kernels.bnn_fused_steps = counting
    try:
        out = group.collect(4, every=5)
    finally:
        kernels.bnn_fused_steps = launch
    looped = torch.empty_like(out)
    for k in range(4):
        twin.steps(5)
        looped[:, k].copy_(twin.theta().clone())
    return group, twin, out, looped, calls


def test_collect_is_one_launch_and_the_same_tensor(gpu, collected):
    group, twin, out, looped, calls = collected
    assert calls == [5]                                         # ONE launch, thinning by 5
    assert out.shape == (3, 4, 5252) and out.is_contiguous()
    assert torch.equal(out, looped) and torch.isfinite(out).all()
    assert not torch.equal(out[0, 0], out[0, 3]) and not torch.equal(out[0], out[1])
    for a, b in zip(group.samplers, twin.samplers):
        for k in a._FUSED_ROWS:
            assert torch.equal(a.arena.row(k), b.arena.row(k)), k
        assert a.n_iterations == b.n_iterations == 20
    assert torch.equal(group.theta(), out[:, 3]) and group.n_iterations == twin.n_iterations == 20


def test_traces_feed_the_device_ess(gpu, collected):
    _, _, out, looped, _ = collected
    assert torch.equal(effective_n_all(out), effective_n_all(looped))
    s, twin = _chain(gpu, torch.float32, "sghmc"), _chain(gpu, torch.float32, "sghmc")
    s.param_names = twin.param_names = ["w1", "b1", "w2", "b2", "w3", "b3", "log_var"]
    trace = DeviceTrace.record(s, 12, keep_every=2, fused=True)
    assert len(trace) == 12 and trace.steps_since_kept == 0 and s.n_iterations == 24
    # the same samples as stepping the whole-step kernel two steps per launch
    for i in range(12):
        twin.fused_bnn_steps(2)
        assert torch.equal(trace.values()[i], twin.arena.row("theta")), i
    ess = effective_sample_sizes_of(trace)
    assert list(ess) == s.param_names
    for name, shape in zip(s.param_names, s.arena.shapes):
        assert ess[name].dtype == torch.int64 and tuple(ess[name].shape) == tuple(shape) and ess[name].is_cuda
    flat = torch.cat([ess[n].reshape(-1) for n in s.param_names])
    assert torch.equal(flat, effective_n_all(trace.values())) and int(flat.min()) >= 0 and int(flat.max()) > 0
    # a sampler that does not fit the kernel is refused, not stepped another way
    s.noise_source = object()
    with pytest.raises(ValueError, match="fused=True needs"):
        DeviceTrace.record(s, 2, fused=True)
