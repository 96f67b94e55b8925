"""K10, the effective sample size of every parameter from device traces (csrc/sgmcmc_ess.hip, include/sgmcmc_hip_diag.h),
and its public front end (``diagnostics.DeviceTrace``, ``effective_n_all``, ``effective_sample_sizes_of``).

The yardsticks are ``oracle.sgmcmc_oracle.effective_n`` (the reference's loop, m >= 2; it divides by zero at m = 1) and the
package's scalar ``diagnostics.effective_n`` (m = 1). ``ess`` and ``stop_lag`` must EQUAL them column by column; ``raw`` is
compared with the same formula in numpy float64 at relative 1e-10 (summation orders differ by ~1e-13 at most; on the fixed
inputs below no evaluated rho pair is closer to zero than 3e-6 and no raw closer to an integer than 2.9e-4, so the integers
cannot move). Outputs sit between guard elements that must survive."""
import time

import numpy as np
import pytest
import torch

from pysgmcmc_amd import diagnostics, kernels
from pysgmcmc_amd.diagnostics.sampler_diagnostics import effective_n

pytestmark = pytest.mark.gpu

PAD = 8
SHAPES = [(1, 100, 256, True, 0.0), (2, 100, 256, True, 0.0), (4, 400, 128, False, 0.0), (3, 57, 256, True, 1e3),
          (2, 1000, 64, True, 0.0)]                      # (m, n, P, rounded to f32, offset), in the order they are drawn
_CACHE = {}


def _inputs():
    """The five AR(1) inputs, drawn in order from ONE RandomState(0)."""
    if "x" not in _CACHE:
        rng = np.random.RandomState(0)
        out = []
        for m, n, P, f32, off in SHAPES:
            phi = rng.choice([0.0, 0.5, 0.9, 0.97], size=P)
            x = np.zeros((m, n, P))
            e = rng.randn(m, n, P)
            x[:, 0] = e[:, 0]
            for i in range(1, n):
                x[:, i] = phi * x[:, i - 1] + np.sqrt(1 - phi ** 2) * e[:, i]
            x = x * rng.lognormal(0, 2, size=P) + off
            if f32:
                x = x.astype(np.float32).astype(np.float64)
            out.append(x)
        _CACHE["x"] = out
    return _CACHE["x"]


def _ref_column(x):
    """The oracle's loop on one (m, n) float64 column -> (raw, final t, smallest |rho_{t-1} + rho_t| evaluated); B = 0 at m = 1."""
    m, n = x.shape
    B = n * np.var(x.mean(axis=1), ddof=1) if m > 1 else 0.0
    W = np.mean(np.var(x, axis=1, ddof=1))
    Vhat = W * (n - 1) / n + B / n
    rho = np.ones(n)
    negative, t, margin = False, 1, np.inf
    while not negative and t < n:
        d = x[:, t:] - x[:, :n - t]
        rho[t] = 1.0 - (np.sum(d * d) / (m * (n - t))) / (2.0 * Vhat)
        if not t % 2:
            negative = (rho[t - 1] + rho[t]) < 0
            margin = min(margin, abs(rho[t - 1] + rho[t]))
        t += 1
    return m * n / (1.0 + 2.0 * rho[1:t].sum()), t, margin


def _reference(k, oracle):
    """(ess, raw, stop_lag) of input k from the yardsticks, column by column."""
    key = ("ref", k)
    if key not in _CACHE:
        x = _inputs()[k]
        m, n, P = x.shape
        if m >= 2:
            ess = np.array([oracle.effective_n(x[:, :, j]) for j in range(P)], np.int64)
        else:
            ess = np.array([effective_n(torch.as_tensor(x[:, :, j])) for j in range(P)], np.int64)
        cols = [_ref_column(x[:, :, j]) for j in range(P)]
        _CACHE[key] = (ess, np.array([c[0] for c in cols]), np.array([c[1] for c in cols], np.int32))
    return _CACHE[key]


class _Guarded(object):
    """ess / raw / stop_lag as slices of larger buffers whose other elements must keep their value."""

    def __init__(self, P, dev):
        self.P = P
        self.full = [torch.full((P + 2 * PAD,), -77, dtype=torch.int64, device=dev),
                     torch.full((P + 2 * PAD,), -77.5, dtype=torch.float64, device=dev),
                     torch.full((P + 2 * PAD,), -77, dtype=torch.int32, device=dev)]
        self.ess, self.raw, self.stop = [f[PAD:PAD + P] for f in self.full]

    def numpy(self):
        for f, v in zip(self.full, (-77, -77.5, -77)):
            h = f.cpu().numpy()
            assert (h[:PAD] == v).all() and (h[PAD + self.P:] == v).all(), "a guard element was overwritten"
        return self.ess.cpu().numpy(), self.raw.cpu().numpy(), self.stop.cpu().numpy()


def _run(chains, dev, **kw):
    P = chains[0].shape[-1] if not torch.is_tensor(chains) else chains.shape[-1]
    out = _Guarded(int(P), dev)
    kernels.ess_variogram(chains, out.ess, out.raw, out.stop, **kw)
    return out.numpy()


def _assert_matches(got, ref, what):
    ess, raw, stop = got
    ref_ess, ref_raw, ref_stop = ref
    print("%s: ess %d..%d, stop lag %d..%d, max rel raw diff %.3g" % (
        what, ess.min(), ess.max(), stop.min(), stop.max(), np.max(np.abs(raw - ref_raw) / np.abs(ref_raw))))
    assert np.array_equal(stop, ref_stop), "%s: stop lags differ at %s" % (what, np.flatnonzero(stop != ref_stop)[:8])
    assert np.array_equal(ess, ref_ess), "%s: ess differs at %s" % (what, np.flatnonzero(ess != ref_ess)[:8])
    assert np.all(np.abs(raw - ref_raw) <= 1e-10 * np.abs(ref_raw)), what
    assert np.array_equal(ess, raw.astype(np.int64))


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_equals_the_oracle_on_every_column(gpu, oracle, k):
    m, n, P, f32, off = SHAPES[k]
    x = _inputs()[k]
    ref = _reference(k, oracle)
    got64 = _run(torch.as_tensor(x, device=gpu), gpu)
    _assert_matches(got64, ref, "shape %s as f64" % (SHAPES[k],))
    if f32:
        got32 = _run(torch.as_tensor(x.astype(np.float32), device=gpu), gpu)
        _assert_matches(got32, ref, "shape %s as f32" % (SHAPES[k],))
        assert np.array_equal(got32[1].view(np.uint64), got64[1].view(np.uint64)), "f32 and f64 input give different raw bits"
        assert np.array_equal(got32[0], got64[0]) and np.array_equal(got32[2], got64[2])
    # the public function, on the (m, n, P) tensor and (one chain) on the (n, P) matrix
    xt = torch.as_tensor(x, device=gpu)
    ess, raw, stop = diagnostics.effective_n_all(xt if m > 1 else xt[0], details=True)
    assert ess.dtype == torch.int64 and raw.dtype == torch.float64 and stop.dtype == torch.int32 and ess.shape == (P,)
    assert np.array_equal(ess.cpu().numpy(), ref[0]) and np.array_equal(stop.cpu().numpy(), ref[2])
    assert np.array_equal(raw.cpu().numpy().view(np.uint64), got64[1].view(np.uint64))
    assert torch.equal(diagnostics.effective_n_all(xt), ess)


def test_layouts_paths_and_geometries_give_the_same_bits(gpu, oracle):
    k = 1                                                    # (2, 100, 256), f32
    x = _inputs()[k].astype(np.float32)
    m, n, P = x.shape
    ref = _reference(k, oracle)
    base = _run(torch.as_tensor(x, device=gpu), gpu)
    _assert_matches(base, ref, "stacked")

    def same(got, what):
        assert np.array_equal(got[1].view(np.uint64), base[1].view(np.uint64)), "%s: raw bits differ" % what
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2]), what

    # separate per-chain buffers, row pitch ld > P, NaN between the rows
    ld = P + 7
    bufs = []
    for c in range(m):
        b = torch.full((n, ld), float("nan"), dtype=torch.float32, device=gpu)
        b[:, :P] = torch.as_tensor(x[c], device=gpu)
        bufs.append(b[:, :P])
    assert bufs[0].stride(0) == ld and bufs[0].data_ptr() != bufs[1].data_ptr()
    same(_run(bufs, gpu), "separate buffers, ld > P")
    same(_run(bufs, gpu, ld=ld), "separate buffers, explicit ld")
    # a base pointer 4 bytes past a 256-byte boundary
    flat = torch.full((m * n * P + 256,), float("nan"), dtype=torch.float32, device=gpu)
    lead = ((-flat.data_ptr()) % 256) // 4 + 1
    shifted = flat[lead:lead + m * n * P].view(m, n, P)
    assert shifted.data_ptr() % 256 == 4
    shifted.copy_(torch.as_tensor(x, device=gpu))
    same(_run(shifted, gpu), "base 4 bytes past a 256-byte boundary")
    # both paths, forced and chosen by size; every workgroup size; twice
    same(_run(torch.as_tensor(x, device=gpu), gpu), "second launch")
    xt = torch.as_tensor(x, device=gpu)
    for staging in ("lds", "global"):
        same(_run(xt, gpu, staging=staging), staging)
        same(_run(xt, gpu, staging=staging), staging + ", second launch")
    for bt in (64, 128, 192, 256):                           # 2 x 100 x 256 x 4 B = 200 KiB: auto takes the global path at 256
        same(_run(xt, gpu, launch=kernels.LaunchConfig(block_threads=bt)), "block_threads %d" % bt)
        same(_run(xt, gpu, staging="global", launch=kernels.LaunchConfig(block_threads=bt)), "global, block_threads %d" % bt)
    from pysgmcmc_amd._lib import SgmcmcLibraryError
    with pytest.raises(SgmcmcLibraryError, match="does not fit the LDS"):
        _run(xt, gpu, staging="lds", launch=kernels.LaunchConfig(block_threads=256))
    # f64 elements: LDS and global path
    x64 = torch.as_tensor(_inputs()[k], device=gpu)
    for staging in ("lds", "global"):
        same(_run(x64, gpu, staging=staging), "f64 " + staging)
    # widths around the wave and workgroup edges: columns repeat those of the base input
    for width in (1, 63, 65, 5252, 70001):
        idx = np.arange(width) % P
        wide = torch.as_tensor(x, device=gpu)[:, :, torch.as_tensor(idx, device=gpu)].contiguous()
        for staging in ("lds", "global"):
            got = _run(wide, gpu, staging=staging)
            assert np.array_equal(got[1].view(np.uint64), base[1][idx].view(np.uint64)), (width, staging)
            assert np.array_equal(got[0], ref[0][idx]) and np.array_equal(got[2], ref[2][idx]), (width, staging)


def test_degenerate_columns(gpu, oracle):
    rng = np.random.RandomState(1)
    x = rng.randn(2, 50, 70)
    for j, v in ((0, 0.0), (33, 0.1), (63, -1e6), (64, 3.0), (69, 1e-30)):
        x[:, :, j] = v                                       # constant columns, at wave edges too
    for dt in (np.float32, np.float64):
        xd = x.astype(dt)
        for staging in ("lds", "global"):
            ess, raw, stop = _run(torch.as_tensor(xd, device=gpu), gpu, staging=staging)
            for j in range(70):
                if j in (0, 33, 63, 64, 69):
                    assert ess[j] == 0 and np.isnan(raw[j]) and stop[j] == 1, (j, ess[j], raw[j], stop[j])
                else:
                    r = _ref_column(xd[:, :, j].astype(np.float64))
                    assert ess[j] == oracle.effective_n(xd[:, :, j].astype(np.float64)) and stop[j] == r[1], j
                    assert abs(raw[j] - r[0]) <= 1e-10 * abs(r[0])
    # the shortest traces the estimator is defined for
    for n in (2, 3):
        for m in (2, 5):
            x = np.random.RandomState(10 * n + m).randn(m, n, 96)
            ess, raw, stop = _run(torch.as_tensor(x, device=gpu), gpu)
            assert (stop == n).all()
            for j in range(96):
                assert ess[j] == oracle.effective_n(x[:, :, j]), (n, m, j, raw[j])
                assert abs(raw[j] - _ref_column(x[:, :, j])[0]) <= 1e-10 * abs(raw[j])
    # one chain: the product's scalar function (the oracle's is undefined at m = 1)
    x = np.random.RandomState(7).randn(1, 3, 40)
    ess, raw, stop = _run(torch.as_tensor(x, device=gpu), gpu)
    assert [int(e) for e in ess] == [effective_n(torch.as_tensor(x[:, :, j])) for j in range(40)]
    # P = 0: nothing is launched, nothing is written
    out = kernels.ess_variogram(torch.zeros(2, 5, 0, device=gpu), torch.zeros(0, dtype=torch.int64, device=gpu))
    assert out.numel() == 0


def _sinc_chain(dev, seed, use_hip_graph=False):
    """The 3 x 50 tanh sinc BNN of ``__graft_entry__.smoke`` (5 252 parameters, f32), Philox noise."""
    from pysgmcmc_amd.data_batches import Placeholder, generate_batches
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
    from pysgmcmc_amd.samplers import SGHMCSampler
    from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule
    rng = np.random.RandomState(1)
    X = rng.rand(100, 1)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    xp = Placeholder(dtype=torch.float32, device=dev)
    yp = Placeholder(dtype=torch.float32, device=dev)
    params = init_mlp_params(1, seed=3, dtype=torch.float32, device=dev)
    cost = BNNCost(xp, yp, batch_size=20, n_examples=100)
    s = SGHMCSampler(params=params, cost_fun=cost, batch_generator=generate_batches(X, y, xp, yp, 20, seed=1),
                     stepsize_schedule=ConstantStepsizeSchedule(0.01), burn_in_steps=50, mdecay=0.05,
                     scale_grad=100.0, session=dev, dtype=torch.float32, seed=seed)
    s.use_hip_graph = use_hip_graph
    return s


BURN, KEPT, EVERY = 50, 200, 2


def _recorded(dev, seed, use_hip_graph=False):
    s = _sinc_chain(dev, seed, use_hip_graph)
    s.sample_format = "device"
    for _ in range(BURN):
        next(s)
    trace = diagnostics.DeviceTrace.record(s, KEPT, keep_every=EVERY)
    assert s.sample_format == "device"
    return s, trace


@pytest.fixture(scope="module")
def bnn_traces(gpu):
    """Two recorded chains (seeds 5 and 6), and the parent's only way to the same numbers: the column loop of the scalar
    ``effective_n`` over the same device traces, timed once after a warm-up call."""
    chains = [_recorded(gpu, seed) for seed in (5, 6)]
    traces = [t for _, t in chains]
    both = torch.stack([t.values() for t in traces])          # (2, n, P), on the device
    effective_n(both[:, :, 0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop = np.array([effective_n(both[:, :, j]) for j in range(both.shape[2])], np.int64)
    torch.cuda.synchronize()
    return {"samplers": [s for s, _ in chains], "traces": traces, "loop": loop, "loop_seconds": time.perf_counter() - t0}


@pytest.mark.parametrize("use_hip_graph", [False, True])
def test_record_does_not_change_the_chain(gpu, use_hip_graph):
    _, trace = _recorded(gpu, 5, use_hip_graph)
    assert len(trace) == KEPT and trace.values().shape == (KEPT, 5252) and trace.values().is_cuda
    plain = _sinc_chain(gpu, 5, use_hip_graph)
    plain.sample_format = "view"
    rows = []
    for step in range(BURN + KEPT * EVERY):
        next(plain)
        if step >= BURN and (step - BURN) % EVERY == EVERY - 1:
            rows.append(plain.arena.row("theta").clone())
    want = torch.stack(rows)
    assert torch.equal(trace.values().view(torch.int32), want.view(torch.int32)), "the recorded rows differ from plain next(sampler)"
    assert not torch.equal(want[0], want[-1])


def test_public_api_on_two_bnn_chains(gpu, bnn_traces):
    traces, loop = bnn_traces["traces"], bnn_traces["loop"]
    ess, raw, stop = diagnostics.effective_n_all(traces, details=True)
    assert ess.shape == (5252,) and ess.is_cuda
    got = ess.cpu().numpy()
    bad = np.flatnonzero(got != loop)
    # data-dependent input: a column within 1e-9 of an integer or of a stop boundary may differ, at most 5 of 5 252
    x = torch.stack([t.values() for t in traces]).double().cpu().numpy()
    for j in bad:
        r, _, margin = _ref_column(x[:, :, j])
        near = min(r - np.floor(r), np.ceil(r) - r) < 1e-9 or margin < 1e-9
        assert near, "column %d: kernel %d, effective_n %d, raw %r, stop margin %r" % (j, got[j], loop[j], r, margin)
    print("columns skipped as within 1e-9 of a boundary: %d of %d; ess %d..%d, stop lag %d..%d" % (
        len(bad), got.size, got.min(), got.max(), int(stop.min()), int(stop.max())))
    assert len(bad) <= 5
    assert torch.equal(diagnostics.effective_n_all(torch.stack([t.values() for t in traces])), ess)
    # the reference's per-variable dictionary
    sampler = bnn_traces["samplers"][0]
    per_var = diagnostics.effective_sample_sizes_of(traces)
    assert list(per_var) == list(sampler.param_names) and len(per_var) == len(sampler.arena.shapes)
    for name, shp, off, size in zip(sampler.param_names, sampler.arena.shapes, sampler.arena.offsets, sampler.arena.sizes):
        assert per_var[name].shape == tuple(shp) and per_var[name].dtype == torch.int64
        assert torch.equal(per_var[name].reshape(-1), ess[off:off + size])
    named = diagnostics.effective_sample_sizes_of(torch.stack([t.values() for t in traces]), param_shapes=sampler.arena.shapes,
                                                  names=["p%d" % i for i in range(len(sampler.arena.shapes))])
    assert list(named) == ["p%d" % i for i in range(len(sampler.arena.shapes))]
    assert all(torch.equal(a, b) for a, b in zip(named.values(), per_var.values()))


def _median_ms(fn, reps=11):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def test_one_launch_beats_the_column_loop(gpu, bnn_traces):
    """Records, not gates, except ``kernel < loop``: 2 chains x 200 samples x 5 252 f32 parameters (LDS path: 100 KiB slab)."""
    traces = bnn_traces["traces"]
    mats = [t.values() for t in traces]
    ess = torch.empty(5252, dtype=torch.int64, device=gpu)
    kernel_ms = _median_ms(lambda: kernels.ess_variogram(mats, ess))
    global_ms = _median_ms(lambda: kernels.ess_variogram(mats, ess, staging="global"))
    api_ms = _median_ms(lambda: diagnostics.effective_n_all(traces))
    loop_ms = bnn_traces["loop_seconds"] * 1e3
    print("ESS of 5252 parameters, 2 x 200 samples: kernel %.3f ms (LDS path; global path %.3f ms; effective_n_all %.3f ms), "
          "column loop of effective_n %.1f ms, ratio %.0f" % (kernel_ms, global_ms, api_ms, loop_ms, loop_ms / kernel_ms))
    assert kernel_ms < loop_ms


def test_at_ten_million_parameters(gpu):
    """P = 10 002 434, n = 32, one f32 chain (1.3 GB; LDS path, 8 KiB slab per workgroup): finishes, and 64 columns drawn
    with a fixed seed equal the scalar function."""
    P, n = 10002434, 32
    g = torch.Generator(device=gpu)
    g.manual_seed(11)
    x = torch.randn(n, P, generator=g, device=gpu, dtype=torch.float32)
    x *= torch.exp(2.0 * torch.randn(P, generator=g, device=gpu, dtype=torch.float32))
    out = _Guarded(P, gpu)
    kernels.ess_variogram(x, out.ess, out.raw, out.stop)
    torch.cuda.synchronize()
    ms = _median_ms(lambda: kernels.ess_variogram(x, out.ess, out.raw, out.stop), reps=3)
    nbytes = x.numel() * 4
    print("ESS of %d parameters, 1 x %d samples: %.2f ms, %.2f GB of trace, %.0f GB/s (LDS path)" % (P, n, ms, nbytes / 1e9, nbytes / ms / 1e6))
    cols = np.random.RandomState(3).choice(P, 64, replace=False)
    cols[:2] = (0, P - 1)
    full = [f.clone() for f in out.full]
    ess = out.ess[torch.as_tensor(cols, device=gpu)].cpu().numpy()
    stop = out.stop[torch.as_tensor(cols, device=gpu)].cpu().numpy()
    for f, v in zip(full, (-77, -77.5, -77)):
        assert bool((f[:PAD] == v).all()) and bool((f[PAD + P:] == v).all()), "a guard element was overwritten"
    host = x[:, torch.as_tensor(cols, device=gpu)].double().cpu()
    for i, j in enumerate(cols):
        assert ess[i] == effective_n(host[None, :, i]), (j, ess[i])
        assert stop[i] == _ref_column(host[None, :, i].numpy())[1], j
    assert bool(torch.isfinite(out.raw).all())
