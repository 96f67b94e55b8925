"""K12, R-hat and the effective sample size of every parameter from one strided trace of up to 4096 chains
(csrc/sgmcmc_chain_diag.hip, include/sgmcmc_hip_chains.h), and its public front end (``kernels.chain_diag``,
``diagnostics.chain_diagnostics_all``, ``gelman_rubin_all``, ``FusedBNNChains.diagnose``).

The yardsticks are ``oracle.sgmcmc_oracle.effective_n`` and ``oracle.sgmcmc_oracle.gelman_rubin`` for m >= 2; for m = 1
(where the oracle divides by zero) the package's scalar ``diagnostics.effective_n`` and ``sqrt((n - 1) / n)``. ``ess`` and
``stop_lag`` must EQUAL them column by column; ``raw`` and ``rhat`` are compared with the same formulas in numpy float64 at
relative 1e-10, the bar of test_device_ess_gpu.py. On the nine fixed inputs below no evaluated rho pair is closer to zero
than 1.3e-4, no raw closer to an integer than 3.8e-5 and the stop lags span 2..64 (computed on a CPU with the yardsticks),
while the kernel's summation order (groups of 16 chains) and numpy's differ by at most 7e-15 relative in raw and 6e-15 in
R-hat on the columns ``contract_column`` was run on, so the integers cannot move and 1e-10 is four orders above what the
orders differ by. Outputs sit between guard elements that must survive.

``contract_column`` restates the header's summation order in plain Python; a handful of columns per input must give the
kernel's bits exactly (Python floats are IEEE doubles with one rounding per operation, the kernel is built without
contraction, and f64 division and square root are correctly rounded on both sides)."""
import math

import numpy as np
import pytest
import torch

from pysgmcmc_amd import diagnostics, kernels
from pysgmcmc_amd.diagnostics.sampler_diagnostics import effective_n

pytestmark = pytest.mark.gpu

PAD = 8
# (m, n, P, rounded to f32, offset), in the order they are drawn: one chain; exactly one group; a one-chain second group;
# more than 64 chains; the workload's 256 chains; a ragged last group at an offset of 1e3; long n; n = 3 (the tail loop
# only); n = 2 (a single lag)
SHAPES = [(1, 40, 70, True, 0.0), (16, 30, 130, True, 0.0), (17, 30, 130, True, 0.0), (65, 24, 65, False, 0.0),
          (256, 20, 200, True, 0.0), (300, 12, 70, True, 1e3), (33, 64, 64, True, 0.0), (40, 3, 66, True, 0.0),
          (5, 2, 10, False, 0.0)]
_CACHE = {}


def _inputs():
    """The nine AR(1) inputs, drawn in order from ONE RandomState(0). A third of the columns get a per-chain shift, so the
    chains disagree there and R-hat runs from 0.94 to 14."""
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
            shift = (rng.rand(P) < 0.33) * rng.randn(m, 1, P) * 2.0
            x = (x + shift) * rng.lognormal(0, 2, size=P) + off
            if f32:
                x = x.astype(np.float32).astype(np.float64)
            out.append(x)
        _CACHE["x"] = out
    return _CACHE["x"]


def contract_column(x):
    """The summation order of include/sgmcmc_hip_chains.h on ONE column: x[c][i] as plain Python floats ->
    (raw, ess, stop_lag, rhat). Chains in groups of 16 consecutive chains; group sums added in ascending group order."""
    m, n = len(x), len(x[0])
    groups = [range(g, min(g + 16, m)) for g in range(0, m, 16)]
    x0, dn = x[0][0], float(n)

    def over_groups(chain_term):                      # ascending chains inside a group from 0.0, then ascending groups from 0.0
        total = 0.0
        for grp in groups:
            part = 0.0
            for c in grp:
                part += chain_term(c)
            total += part
        return total

    def shifted_mean(c):
        s = 0.0
        for v in x[c]:
            s += v - x0
        return s / dn

    def variance(c):
        mean, q = shifted_mean(c), 0.0
        for v in x[c]:
            d = (v - x0) - mean
            q += d * d
        return q / (dn - 1.0)

    mean_sum, var_sum, B = over_groups(shifted_mean), over_groups(variance), 0.0
    if m > 1:
        grand = mean_sum / float(m)

        def squared_deviation(c):
            d = shifted_mean(c) - grand
            return d * d

        B = dn * (over_groups(squared_deviation) / float(m - 1))
    W = var_sum / float(m)
    vhat = W * (dn - 1.0) / dn + B / dn
    if vhat == 0.0 or not math.isfinite(vhat):
        return float("nan"), 0, 1, float("nan")
    rhat = math.sqrt(vhat / W) if W != 0.0 else float("inf")
    rho_sum, prev, stop = 0.0, 1.0, n
    for t in range(1, n):
        cnt, s = n - t, 0.0
        for grp in groups:
            a = [0.0, 0.0, 0.0, 0.0]                  # four interleaved partial sums, carried from chain to chain of the group
            for c in grp:
                for i in range(cnt):
                    d = x[c][i + t] - x[c][i]
                    a[i % 4 if i < cnt - cnt % 4 else 0] += d * d
            s += (a[0] + a[1]) + (a[2] + a[3])
        rho = 1.0 - s / ((2.0 * vhat) * (float(m) * float(cnt)))
        rho_sum += rho
        if t % 2 == 0 and prev + rho < 0.0:
            stop = t + 1
            break
        prev = rho
    raw = (float(m) * dn) / (1.0 + 2.0 * rho_sum)
    return raw, int(raw), stop, rhat


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


def _reference_of(x, oracle):
    """(rhat, ess, raw, stop_lag) of an (m, n, P) float64 array from the yardsticks, column by column."""
    m, n, P = x.shape
    if m >= 2:
        ess = np.array([oracle.effective_n(x[:, :, j]) for j in range(P)], np.int64)
        rhat = np.asarray(oracle.gelman_rubin(x), np.float64)
    else:
        ess = np.array([effective_n(torch.as_tensor(x[:, :, j])) for j in range(P)], np.int64)
        rhat = np.full(P, math.sqrt((n - 1.0) / n))
    cols = [_ref_column(x[:, :, j]) for j in range(P)]
    return rhat, ess, np.array([c[0] for c in cols]), np.array([c[1] for c in cols], np.int32)


def _reference(k, oracle):
    key = ("ref", k)
    if key not in _CACHE:
        _CACHE[key] = _reference_of(_inputs()[k], oracle)
    return _CACHE[key]


class _Guarded(object):
    """rhat / ess / raw / stop_lag as slices of larger buffers whose other elements must keep their value."""
    FILL = (-77.25, -77, -77.5, -77)

    def __init__(self, P, dev):
        self.P = P
        self.full = [torch.full((P + 2 * PAD,), v, dtype=dt, device=dev)
                     for v, dt in zip(self.FILL, (torch.float64, torch.int64, torch.float64, torch.int32))]
        self.rhat, self.ess, self.raw, self.stop = [f[PAD:PAD + P] for f in self.full]

    def numpy(self, untouched=()):
        for i, (f, v) in enumerate(zip(self.full, self.FILL)):
            h = f.cpu().numpy()
            assert (h[:PAD] == v).all() and (h[PAD + self.P:] == v).all(), "a guard element was overwritten"
            if i in untouched:
                assert (h == v).all(), "a buffer that was not passed was written"
        return self.rhat.cpu().numpy(), self.ess.cpu().numpy(), self.raw.cpu().numpy(), self.stop.cpu().numpy()


def _run(trace, dev, **kw):
    out = _Guarded(int(trace.shape[-1]), dev)
    kernels.chain_diag(trace, out.rhat, out.ess, out.raw, out.stop, **kw)
    return out.numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(got, base, what):
    assert np.array_equal(_bits(got[0]), _bits(base[0])), "%s: rhat bits differ" % what
    assert np.array_equal(_bits(got[2]), _bits(base[2])), "%s: raw bits differ" % what
    assert np.array_equal(got[1], base[1]) and np.array_equal(got[3], base[3]), what


def _assert_matches(got, ref, what):
    rhat, ess, raw, stop = got
    ref_rhat, ref_ess, ref_raw, ref_stop = ref
    print("%s: rhat %.4g..%.4g, ess %d..%d, stop lag %d..%d, max rel diff raw %.3g rhat %.3g" % (
        what, rhat.min(), rhat.max(), ess.min(), ess.max(), stop.min(), stop.max(),
        np.max(np.abs(raw - ref_raw) / np.abs(ref_raw)), np.max(np.abs(rhat - ref_rhat) / np.abs(ref_rhat))))
    assert np.array_equal(stop, ref_stop), "%s: stop lags differ at %s" % (what, np.flatnonzero(stop != ref_stop)[:8])
    assert np.array_equal(ess, ref_ess), "%s: ess differs at %s" % (what, np.flatnonzero(ess != ref_ess)[:8])
    assert np.all(np.abs(raw - ref_raw) <= 1e-10 * np.abs(ref_raw)), what
    assert np.all(np.abs(rhat - ref_rhat) <= 1e-10 * np.abs(ref_rhat)), what
    assert np.array_equal(ess, raw.astype(np.int64))


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_equals_the_yardsticks_on_every_column(gpu, oracle, k):
    m, n, P, f32, off = SHAPES[k]
    x = _inputs()[k]
    ref = _reference(k, oracle)
    xt = torch.as_tensor(x, device=gpu)
    got64 = _run(xt, gpu)
    _assert_matches(got64, ref, "shape %s as f64" % (SHAPES[k],))
    if f32:
        got32 = _run(torch.as_tensor(x.astype(np.float32), device=gpu), gpu)
        _assert_matches(got32, ref, "shape %s as f32" % (SHAPES[k],))
        _same(got32, got64, "f32 and f64 elements")
    # the header's summation order in plain Python: the kernel's bits on a handful of columns
    for j in list(range(0, P, max(1, P // 6)))[:7]:
        raw, ess, stop, rhat = contract_column([[float(v) for v in row] for row in x[:, :, j]])
        print("  column %d: raw %r (contract %r), rhat %r (contract %r)" % (j, got64[2][j], raw, got64[0][j], rhat))
        assert (ess, stop) == (got64[1][j], got64[3][j]), j
        assert _bits(np.float64(raw)) == _bits(got64[2][j]) and _bits(np.float64(rhat)) == _bits(got64[0][j]), j
    # the public functions, on the (m, n, P) tensor and (one chain) on the (n, P) matrix
    arg = xt if m > 1 else xt[0]
    rhat, ess, raw, stop = diagnostics.chain_diagnostics_all(arg, details=True)
    assert (rhat.dtype, ess.dtype, raw.dtype, stop.dtype) == (torch.float64, torch.int64, torch.float64, torch.int32)
    assert rhat.shape == ess.shape == raw.shape == stop.shape == (P,) and rhat.is_cuda
    _same((rhat.cpu().numpy(), ess.cpu().numpy(), raw.cpu().numpy(), stop.cpu().numpy()), got64, "chain_diagnostics_all")
    pair = diagnostics.chain_diagnostics_all(arg)
    assert len(pair) == 2 and torch.equal(pair[0].view(torch.int64), rhat.view(torch.int64)) and torch.equal(pair[1], ess)
    only = diagnostics.gelman_rubin_all(arg)
    assert only.dtype == torch.float64 and only.shape == (P,)
    assert np.array_equal(_bits(only.cpu().numpy()), _bits(got64[0])), "gelman_rubin_all differs from the full call's rhat"
    # a sequence of matrices in buffers of their own: stacked once, same bits
    if 1 < m <= 17:
        _same([t.cpu().numpy() for t in diagnostics.chain_diagnostics_all([xt[c].clone() for c in range(m)], details=True)],
              got64, "a sequence of matrices")


@pytest.mark.parametrize("k", [0, 1, 8])
def test_up_to_sixteen_chains_give_k10_s_bits(gpu, k):
    x = _inputs()[k]
    P = x.shape[2]
    for dt in ([np.float64, np.float32] if SHAPES[k][3] else [np.float64]):
        xt = torch.as_tensor(x.astype(dt), device=gpu)
        got = _run(xt, gpu)
        ess = torch.empty(P, dtype=torch.int64, device=gpu)
        raw = torch.empty(P, dtype=torch.float64, device=gpu)
        stop = torch.empty(P, dtype=torch.int32, device=gpu)
        kernels.ess_variogram(xt, ess, raw, stop)
        assert np.array_equal(_bits(got[2]), _bits(raw.cpu().numpy())), "raw differs from K10's bits"
        assert np.array_equal(got[1], ess.cpu().numpy()) and np.array_equal(got[3], stop.cpu().numpy())


@pytest.mark.parametrize("k", [2, 4, 5])
def test_geometry_and_layout_give_the_same_bits(gpu, oracle, k):
    m, n, P, f32, off = SHAPES[k]
    x = _inputs()[k].astype(np.float32)
    xt = torch.as_tensor(x, device=gpu)
    base = _run(xt, gpu)
    _assert_matches(base, _reference(k, oracle), "auto waves")
    for waves in (1, 2, 4, 8, 16):                           # 16 waves over 2 groups at m = 17: 14 waves without a group
        _same(_run(xt, gpu, waves=waves), base, "waves = %d" % waves)
    # a base pointer one element past a 256-byte boundary
    flat = torch.full((m * n * P + 256,), float("nan"), dtype=torch.float32, device=gpu)
    lead = ((-flat.data_ptr()) % 256) // 4 + 1
    shifted = flat[lead:lead + m * n * P].view(m, n, P)
    assert shifted.data_ptr() % 256 == 4
    shifted.copy_(xt)
    _same(_run(shifted, gpu), base, "base one element past a 256-byte boundary")
    # rows of a wider buffer, NaN between them
    wide = torch.full((m, n, P + 3), float("nan"), dtype=torch.float32, device=gpu)
    wide[:, :, :P] = xt
    view = wide[:, :, :P]
    assert view.stride(1) == P + 3 and view.data_ptr() == wide.data_ptr()
    _same(_run(view, gpu), base, "ld = P + 3")
    _same(_run(view, gpu, waves=2), base, "ld = P + 3, 2 waves")
    # the first n rows of a trace with capacity n + 5, NaN behind them
    longer = torch.full((m, n + 5, P), float("nan"), dtype=torch.float32, device=gpu)
    longer[:, :n] = xt
    view = longer[:, :n]
    assert view.stride(0) == (n + 5) * P and view.data_ptr() == longer.data_ptr()
    _same(_run(view, gpu), base, "chain_stride > n * ld")
    # column slices at offset 1, around the wave's width: the same columns of the full call
    for width in (1, 63, 65):
        got = _run(xt[:, :, 1:1 + width], gpu)
        _same(got, [b[1:1 + width] for b in base], "columns 1 .. %d" % width)
        got = _run(xt[:, :, 1:1 + width], gpu, waves=4)
        _same(got, [b[1:1 + width] for b in base], "columns 1 .. %d, 4 waves" % width)


# Chain counts at which the host takes another path: 65 groups (two table buffers of 33 280 B each: more than 64 KiB of
# dynamic LDS), 161 groups (two buffers no longer fit 160 KiB: one buffer, two barriers per reduction) and the limit, 4096
# chains (256 groups, one buffer of 128 KiB); the last group of the first two is ragged. (m, n, P)
LARGE = [(1030, 4, 66), (2563, 3, 65), (4096, 5, 70)]


def _large_input(m, n, P):
    """White noise with a per-chain shift in every third column and per-column scales, rounded to f32. On a CPU, with the
    yardsticks: no evaluated rho pair is closer to zero than 1.7e-5 and no raw closer to an integer than 1.7e-3 on the three
    inputs, and the kernel's order and numpy's differ by 5e-16 relative, so ``ess`` and ``stop_lag`` must equal the oracle's."""
    key = ("large", m)
    if key not in _CACHE:
        rng = np.random.RandomState(m)
        x = rng.randn(m, n, P)
        x[:, :, ::3] += rng.randn(m, 1, len(range(0, P, 3)))
        x *= rng.lognormal(0, 2, size=P)
        _CACHE[key] = x.astype(np.float32).astype(np.float64)
    return _CACHE[key]


@pytest.mark.parametrize("m,n,P", LARGE)
def test_chain_counts_that_take_the_other_host_paths(gpu, oracle, m, n, P):
    x = _large_input(m, n, P)
    xt = torch.as_tensor(x.astype(np.float32), device=gpu)
    base = _run(xt, gpu)
    _assert_matches(base, _reference_of(x, oracle), "%d chains" % m)
    for waves in (1, 4, 16):
        _same(_run(xt, gpu, waves=waves), base, "%d chains, waves = %d" % (m, waves))
    _same(_run(xt.double(), gpu), base, "%d chains, f64 elements" % m)
    out = _Guarded(P, gpu)
    kernels.chain_diag(xt, rhat=out.rhat)
    assert np.array_equal(_bits(out.numpy(untouched=(1, 2, 3))[0]), _bits(base[0])), "R-hat only"
    for j in (0, P - 1):
        raw, ess, stop, rhat = contract_column([[float(v) for v in row] for row in x[:, :, j]])
        assert (ess, stop) == (base[1][j], base[3][j]), j
        assert _bits(np.float64(raw)) == _bits(base[2][j]) and _bits(np.float64(rhat)) == _bits(base[0][j]), j


@pytest.mark.parametrize("k", [2, 4])
def test_rhat_only_mode(gpu, k):
    x = _inputs()[k]
    P = x.shape[2]
    for dt in (np.float64, np.float32):
        xt = torch.as_tensor(x.astype(dt), device=gpu)
        full = _run(xt, gpu)
        for waves in (None, 1, 16):
            out = _Guarded(P, gpu)
            got = kernels.chain_diag(xt, rhat=out.rhat, waves=waves)
            assert got[0] is out.rhat and got[1:] == (None, None, None)
            rhat = out.numpy(untouched=(1, 2, 3))[0]
            assert np.array_equal(_bits(rhat), _bits(full[0])), "the moments-only launch gives other rhat bits"
        # and each output alone gives the bits of the full call
        out = _Guarded(P, gpu)
        kernels.chain_diag(xt, stop_lag=out.stop)
        assert np.array_equal(out.numpy(untouched=(0, 1, 2))[3], full[3])
        out = _Guarded(P, gpu)
        kernels.chain_diag(xt, raw=out.raw)
        assert np.array_equal(_bits(out.numpy(untouched=(0, 1, 3))[2]), _bits(full[2]))


def test_degenerate_columns(gpu, oracle):
    m, n, P = 20, 10, 70
    clean = np.random.RandomState(1).randn(m, n, P)
    x = clean.copy()
    for j, v in ((0, 0.1), (63, -1e6), (64, 3.0)):
        x[:, :, j] = v                                       # constant columns, at the wave's edges too
    x[17, 4, 33] = float("nan")                              # one NaN sample, in the second group
    x[:, :, 69] = np.arange(m, dtype=np.float64)[:, None] * 0.5 - 2.0    # chains each constant at a value of its own
    planted = (0, 33, 63, 64, 69)
    for dt in (np.float32, np.float64):
        ref = _run(torch.as_tensor(clean.astype(dt), device=gpu), gpu)
        _assert_matches(ref, _reference_of(clean.astype(dt).astype(np.float64), oracle), "no planted columns, %s" % dt.__name__)
        for waves in (None, 1, 2):
            rhat, ess, raw, stop = got = _run(torch.as_tensor(x.astype(dt), device=gpu), gpu, waves=waves)
            for j in (0, 33, 63, 64):
                assert np.isnan(rhat[j]) and ess[j] == 0 and np.isnan(raw[j]) and stop[j] == 1, (j, rhat[j], ess[j], raw[j], stop[j])
            assert rhat[69] == np.inf and stop[69] == n and ess[69] == int(m * n / (1.0 + 2.0 * (n - 1)))
            assert abs(raw[69] - m * n / (1.0 + 2.0 * (n - 1))) <= 1e-10 * raw[69]
            keep = np.array([j for j in range(P) if j not in planted])
            _same([g[keep] for g in got], [r[keep] for r in ref], "the neighbours of the planted columns")
    # P = 0: nothing is launched, nothing is written
    out = kernels.chain_diag(torch.zeros(20, 5, 0, device=gpu), rhat=torch.zeros(0, dtype=torch.float64, device=gpu))
    assert out[0].numel() == 0


@pytest.mark.parametrize("rhat_only", [False, True])
def test_the_call_is_legal_under_stream_capture(gpu, rhat_only):
    from pysgmcmc_amd.samplers.base_classes import graph_capture
    xt = torch.as_tensor(_inputs()[4].astype(np.float32), device=gpu)
    P = xt.shape[2]
    eager = _run(xt, gpu)
    outs = [torch.zeros(P, dtype=dt, device=gpu) for dt in (torch.float64, torch.int64, torch.float64, torch.int32)]
    args = (outs[0],) if rhat_only else tuple(outs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # the first launch of the kernel outside the capture
        kernels.chain_diag(xt, *args)
    torch.cuda.current_stream().wait_stream(side)
    for t in outs:
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):                                   # a single-kernel graph
        kernels.chain_diag(xt, *args)
    torch.cuda.synchronize()
    assert all(float(t.double().abs().sum()) == 0.0 for t in outs)   # captured, not run
    g.replay()
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in outs]
    assert np.array_equal(_bits(got[0]), _bits(eager[0])), "rhat of the replayed graph"
    if rhat_only:
        assert all(float(t.double().abs().sum()) == 0.0 for t in outs[1:])
    else:
        _same(got, eager, "the replayed graph")


def test_public_path_on_eighty_bnn_chains(gpu, oracle):
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    rng = np.random.RandomState(1)
    X = rng.rand(100, 1)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    chains = FusedBNNChains.for_dataset(X, y, 80, burn_in_steps=20, device=gpu)
    chains.steps(60)
    t = chains.collect(12, every=2)
    assert tuple(t.shape) == (80, 12, 5252) and t.is_cuda
    rhat, ess, raw, stop = chains.diagnose(t, details=True)
    pair = chains.diagnose(t)
    assert len(pair) == 2 and torch.equal(pair[1], ess) and torch.equal(pair[0].view(torch.int64), rhat.view(torch.int64))
    assert torch.equal(diagnostics.gelman_rubin_all(t).view(torch.int64), rhat.view(torch.int64))
    x = t.double().cpu().numpy()
    ref_rhat, ref_ess, ref_raw, ref_stop = _reference_of(x, oracle)
    rhat, ess, raw, stop = rhat.cpu().numpy(), ess.cpu().numpy(), raw.cpu().numpy(), stop.cpu().numpy()
    print("80 chains x 12 samples x 5252 parameters: rhat %.4g..%.4g (max rel diff %.3g), ess %d..%d, stop lag %d..%d" % (
        rhat.min(), rhat.max(), np.max(np.abs(rhat - ref_rhat) / ref_rhat), ess.min(), ess.max(), stop.min(), stop.max()))
    assert np.all(np.abs(rhat - ref_rhat) <= 1e-10 * ref_rhat)
    # data-dependent input: a column within 1e-9 of an integer or of a stop boundary may differ, at most 5 of 5 252
    bad = np.flatnonzero((ess != ref_ess) | (stop != ref_stop))
    for j in bad:
        r, _, margin = _ref_column(x[:, :, j])
        near = min(r - np.floor(r), np.ceil(r) - r) < 1e-9 or margin < 1e-9
        assert near, "column %d: kernel %d / lag %d, oracle %d / lag %d, raw %r, stop margin %r" % (
            j, ess[j], stop[j], ref_ess[j], ref_stop[j], r, margin)
    print("columns excepted as within 1e-9 of a boundary: %d of %d" % (len(bad), ess.size))
    assert len(bad) <= 5
    good = np.setdiff1d(np.arange(ess.size), bad)
    assert np.all(np.abs(raw[good] - ref_raw[good]) <= 1e-10 * np.abs(ref_raw[good]))
    # the trace is still what predict reads
    mean, var = chains.predict(np.linspace(0.0, 1.0, 9).reshape(-1, 1), t)
    assert tuple(mean.shape) == tuple(var.shape) == (9,) and bool(torch.isfinite(mean).all()) and bool((var >= 0).all())


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


def test_timing_record(gpu):
    """A record, not a gate: the full diagnosis and the R-hat-only launch at (256, 20, 5252) f32."""
    g = torch.Generator(device=gpu)
    g.manual_seed(5)
    x = torch.randn(256, 20, 5252, generator=g, device=gpu, dtype=torch.float32)
    outs = [torch.empty(5252, dtype=dt, device=gpu) for dt in (torch.float64, torch.int64, torch.float64, torch.int32)]
    full_ms = _median_ms(lambda: kernels.chain_diag(x, *outs))
    rhat_ms = _median_ms(lambda: kernels.chain_diag(x, outs[0]))
    print("K12 at 256 chains x 20 samples x 5252 parameters (f32): full diagnosis %.3f ms, R-hat only %.3f ms (stop lag %d..%d)"
          % (full_ms, rhat_ms, int(outs[3].min()), int(outs[3].max())))
    assert bool(torch.isfinite(outs[0]).all()) and bool((outs[1] > 0).all())
