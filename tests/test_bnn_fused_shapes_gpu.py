"""The whole-step BNN kernel (csrc/sgmcmc_bnn_fused.hip) at every kind of shape its C entry accepts, step by step
against a high-precision reference assembled from the oracle:

- the gradient row the kernel leaves behind == ``oracle.bnn_cost_and_grad`` in float64 on the kernel's own starting
  theta and window, minus the weight-prior term the kernel folds into the update (per tensor; the biases and the
  log-variance entry element by element);
- the cost == the oracle's float64 cost;
- theta, V, tau, g, v_hat and minv after the step == the C oracle's SGHMC / SGLD update of the starting state with the
  kernel's gradient row and the K5 noise stream of (seed_base + chain, step), bit for bit;
- one launch of n steps == n one-step launches, bit for bit (LDS theta' carry, in-launch window prefetch, burn-in switch
  inside the launch).

The shapes reach the scalar (odd width / odd offset) loops, the in-place window loads (window > 512 lanes), batches
larger than the workgroup, a batch of 1, one and eight weight layers, and LDS use above 64 KiB up to the 160 KiB limit.
The C entry's refusals are checked on the host side (nothing launched)."""
import ctypes
import re
from itertools import islice

import numpy as np
import pytest
import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd._lib import SgmcmcLibraryError, lib

pytestmark = pytest.mark.gpu

WDECAY, PRIOR_MEAN, PRIOR_VAR = 1.0, 1e-6, 0.01
EPS = {"sghmc": 0.01, "sgld": 1e-3}
MDECAY, SGLD_A = 0.05, 1.0
GRAD_TOL = {np.float32: 3e-5, np.float64: 1e-12}
COST_TOL = {np.float32: 2e-6, np.float64: 1e-12}
FLOOR = {np.float32: 1e-9, np.float64: 1e-300}
ROWS = {"sghmc": ("theta", "V", "grad", "tau", "g", "v_hat", "minv"),
        "sgld": ("theta", "grad", "tau", "g", "v_hat", "minv")}
PAD = 4321.0                                   # sentinel in the padding between chains
LDS_LIMIT = 160 * 1024
T0 = 3                                         # first step index of a case: the Philox step is never 0
N_STEPS = 4                                    # steps T0..T0+3, burn-in ends after T0+1: the switch falls inside

# (layer sizes, batch, n_data): what each row reaches is in the id
SHAPES = [
    pytest.param([1, 50, 50, 50, 1], 20, 100, id="default_3x50"),
    pytest.param([3, 7, 13, 1], 5, 40, id="odd_widths_odd_offsets"),
    pytest.param([4, 50, 49, 50, 1], 16, 64, id="paired_and_scalar_mixed"),
    pytest.param([26, 50, 50, 50, 1], 20, 100, id="window_520_in_place"),
    pytest.param([16, 8, 1], 32, 100, id="window_512_prefetch"),
    pytest.param([16, 8, 1], 33, 100, id="window_528_in_place"),
    pytest.param([2, 6, 6, 1], 600, 700, id="batch_600_over_workgroup"),     # f64: 140 KB of LDS
    pytest.param([5, 1], 7, 30, id="single_weight_layer"),
    pytest.param([3, 8, 8, 8, 8, 8, 8, 8, 1], 12, 50, id="eight_weight_layers"),
    pytest.param([6, 10, 1], 1, 20, id="batch_of_1"),
]
# the largest f32 launch the kernel accepts (exactly 160 KiB of LDS) and its twin with one more input (refused)
NEAR_LIMIT, NEAR_LIMIT_B = [78, 106, 138, 1], 31
OVER_LIMIT = [79, 106, 138, 1]


def _n_params(sizes):
    return sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1


def _lds_bytes(sizes, batch, esize):
    """bnn_fused_entry's LDS formula: activations (act_off), deltas (del_off), the target window (lds_y), rounded up to
    4 elements, then the parameter copy, after 160 B of reduction scratch."""
    elems = batch * sum(sizes) + batch * sum(sizes[1:]) + batch
    elems = (elems + 3) & ~3
    return 160 + (elems + _n_params(sizes)) * esize


def _split(flat, sizes):
    """Flat parameter row -> [W1 (in, out), b1, ..., WL, bL, log_var (1, 1)] (the kernel's order and layout)."""
    out, off = [], 0
    for l in range(len(sizes) - 1):
        nin, nout = sizes[l], sizes[l + 1]
        out.append(flat[off:off + nin * nout].reshape(nin, nout))
        off += nin * nout
        out.append(flat[off:off + nout])
        off += nout
    out.append(flat[off:off + 1].reshape(1, 1))
    assert off + 1 == flat.size
    return out


def _abs_scales(params, Xw, yw, batch, n_examples):
    """Per-element magnitudes the f32 rounding is measured against: for the bias of layer l, sum_b |delta_l| with
    |delta| propagated through |W| (no cancellation); for the log-variance entry, the sum of the magnitudes of its
    terms."""
    L = (len(params) - 1) // 2
    hs = [Xw]
    for l in range(L):
        a = hs[-1] @ params[2 * l] + params[2 * l + 1]
        hs.append(np.tanh(a) if l < L - 1 else a)
    s = float(params[-1].ravel()[0])
    es = np.exp(s)
    inv = 1.0 / (es + 1e-16)
    r = yw - hs[-1]
    D = np.abs(r) * (inv / batch)
    bias = [None] * L
    for l in range(L - 1, -1, -1):
        bias[l] = D.sum(axis=0)
        if l:
            D = (D @ np.abs(params[2 * l]).T) * (1.0 - hs[l] * hs[l])
    sse = float((r * r).sum())
    lvp_den = 2.0 * PRIOR_VAR + 3e-16
    lv = (sse * 0.5 * es * inv * inv + 0.5 * batch) / batch + abs(2.0 * (s - np.log(PRIOR_MEAN)) / lvp_den) / n_examples
    return bias, lv


def _assert_same(got, want, what):
    """Bit-equality of two host arrays of the same float dtype (tests/test_hip_parity.py's idiom)."""
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    if not np.array_equal(got.view(u), want.view(u)):
        idx = np.flatnonzero(got.view(u) != want.view(u))
        raise AssertionError("%s: %d/%d elements differ, first idx %d gpu=%r oracle=%r" % (
            what, idx.size, got.size, idx[0], got[idx[0]], want[idx[0]]))


def _launch(kind, rows, sizes, X, y, starts, batch, first_step, n_steps, burn, seed_base, costs, n_chains=1,
            stride=None, xi=None):
    n_data = X.shape[0]
    common = (sizes, X, y, starts, batch, float(batch), float(n_data), WDECAY, PRIOR_MEAN, PRIOR_VAR, EPS[kind],
              float(n_data))
    if kind == "sghmc":
        kernels.bnn_fused_sghmc_steps(rows["theta"], rows["V"], rows["grad"], rows["tau"], rows["g"], rows["v_hat"],
                                      rows["minv"], *common, MDECAY, first_step, n_steps, burn, seed_base, costs,
                                      xi=xi, n_chains=n_chains, chain_stride=stride)
    else:
        kernels.bnn_fused_sgld_steps(rows["theta"], rows["grad"], rows["tau"], rows["g"], rows["v_hat"], rows["minv"],
                                     *common, SGLD_A, first_step, n_steps, burn, seed_base, costs, xi=xi,
                                     n_chains=n_chains, chain_stride=stride)


def _data(sizes, n_data, npdt, rng):
    X = rng.uniform(-1.0, 1.0, size=(n_data, sizes[0])).astype(npdt)
    y = (np.sin(3.0 * X.sum(axis=1)) + 0.3 * rng.normal(size=n_data)).astype(npdt)
    return X, y


def _chain_state(kind, sizes, npdt, rng):
    """A starting state away from the trivial one: non-zero biases, log-variance away from 0, sampler statistics
    that are not all ones; the gradient row is NaN so an element the kernel does not write shows."""
    parts = []
    for l in range(len(sizes) - 1):
        parts.append(rng.normal(size=sizes[l] * sizes[l + 1]) / np.sqrt(sizes[l]))
        parts.append(rng.normal(size=sizes[l + 1]) * 0.3)
    parts.append([-1.5 + 0.2 * rng.normal()])
    theta = np.concatenate(parts)
    P = theta.size
    st = {"theta": theta, "V": rng.normal(size=P) * 1e-3, "grad": np.full(P, np.nan),
          "tau": 1.0 + rng.uniform(size=P), "g": rng.normal(size=P) * 0.5, "v_hat": rng.uniform(0.5, 2.0, size=P),
          "minv": rng.uniform(0.5, 1.5, size=P)}
    return {k: st[k].astype(npdt) for k in ROWS[kind]}


def _check_step(oracle, kind, sizes, Xh, yh, B, before, after, cost, start, step, burn, xi, what, stats):
    """One step of one chain: gradient row and cost against fp64, the update bit-exact against the C oracle."""
    npdt = before["theta"].dtype.type
    P, n_data = before["theta"].size, Xh.shape[0]
    Xw, yw = Xh[start:start + B], yh[start:start + B].reshape(-1, 1)
    params = _split(before["theta"].astype(np.float64), sizes)
    cost64, g64 = oracle.bnn_cost_and_grad(params, Xw, yw, float(B), float(n_data), WDECAY, PRIOR_MEAN, PRIOR_VAR)
    coef = WDECAY / ((P + 3e-16) * n_data)           # the weight-prior gradient the kernel leaves to the update
    gk = _split(after["grad"].astype(np.float64), sizes)
    tol, floor = GRAD_TOL[npdt], FLOOR[npdt]
    for i, (got, g, p) in enumerate(zip(gk, g64, params)):
        ref = g - coef * p
        err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
        assert err <= tol * scale + floor, "%s: gradient tensor %d off by %.3g (max |g64| %.3g)" % (what, i, err, scale)
        stats["grad"] = max(stats["grad"], err / max(scale, floor))
    bias_scale, lv_scale = _abs_scales(params, Xw, yw, B, n_data)
    for l, sc in enumerate(bias_scale):
        ref = g64[2 * l + 1] - coef * params[2 * l + 1]
        err = np.abs(gk[2 * l + 1] - ref)
        bad = np.flatnonzero(err > tol * sc + floor)
        assert bad.size == 0, "%s: bias %d element %d off by %.3g (scale %.3g)" % (what, l, bad[0], err[bad[0]],
                                                                                  sc[bad[0]])
    ref = float(g64[-1].ravel()[0]) - coef * float(params[-1].ravel()[0])
    err = abs(float(gk[-1].ravel()[0]) - ref)
    assert err <= tol * lv_scale + floor, "%s: log-variance gradient off by %.3g (scale %.3g)" % (what, err, lv_scale)
    cerr = abs(float(cost) - float(cost64))
    assert cerr <= COST_TOL[npdt] * abs(float(cost64)), "%s: cost %r vs fp64 %r" % (what, float(cost), float(cost64))
    stats["cost"] = max(stats["cost"], cerr / abs(float(cost64)))
    # the update: the C oracle's operator on the starting state with the kernel's own gradient row and the K5 stream
    st = oracle.CState(before["theta"], npdt)
    for k in ROWS[kind]:
        if k not in ("theta", "grad"):
            getattr(st, k)[:] = before[k]
    adapt = step < burn or burn == 0
    gd = WDECAY / ((P + (2.0 * 1e-16 + 1e-16)) * n_data)
    if kind == "sghmc":
        oracle.c_sghmc_step(st, after["grad"], EPS[kind], float(n_data), MDECAY, adapt, xi=xi, grad_decay=gd)
    else:
        oracle.c_sgld_step(st, after["grad"], EPS[kind], SGLD_A, float(n_data), adapt, xi=xi, grad_decay=gd)
    for k in ROWS[kind]:
        if k != "grad":
            _assert_same(after[k], getattr(st, k), "%s: %s" % (what, k))


def _run_case(gpu, oracle, kind, dt, sizes, batch, n_data, n_chains=1, seed=0):
    """N_STEPS one-step launches checked against the reference from the kernel's own state, then one launch of
    N_STEPS steps from the same start, bit-equal to the series. Returns the largest relative errors seen."""
    npdt = np.float32 if dt == torch.float32 else np.float64
    rng = np.random.default_rng([seed, batch, n_chains] + list(sizes))
    P = _n_params(sizes)
    assert _lds_bytes(sizes, batch, np.dtype(npdt).itemsize) <= LDS_LIMIT
    stride = P if n_chains == 1 else (P + 3) // 4 * 4
    Xh_t, yh_t = _data(sizes, n_data, npdt, rng)
    X, y = torch.tensor(Xh_t, device=gpu), torch.tensor(yh_t, device=gpu)
    Xh, yh = Xh_t.astype(np.float64), yh_t.astype(np.float64)
    starts = rng.integers(0, n_data - batch + 1, size=(n_chains, N_STEPS)).astype(np.int32)
    starts[:, 1] = n_data - batch                   # the last valid window
    starts[-1, 3] = 0
    assert (starts + batch <= n_data).all()
    init = {k: np.full(n_chains * stride, PAD, npdt) for k in ROWS[kind]}
    for c in range(n_chains):
        for k, v in _chain_state(kind, sizes, npdt, rng).items():
            init[k][c * stride:c * stride + P] = v
    rows0 = {k: torch.tensor(v, device=gpu) for k, v in init.items()}
    rows = {k: v.clone() for k, v in rows0.items()}
    burn, seed_base = T0 + 2, 1000 + 17 * seed
    stats = {"grad": 0.0, "cost": 0.0}
    series = []
    host = {k: v.cpu().numpy().copy() for k, v in rows.items()}
    for t in range(N_STEPS):
        step = T0 + t
        cost = torch.full((n_chains,), float("nan"), dtype=dt, device=gpu)
        _launch(kind, rows, sizes, X, y, torch.tensor(starts[:, t].copy(), device=gpu), batch, step, 1, burn,
                seed_base, cost, n_chains, stride)
        new = {k: v.cpu().numpy().copy() for k, v in rows.items()}
        cost_h = cost.cpu().numpy()
        for c in range(n_chains):
            xi = torch.empty(P, dtype=dt, device=gpu)
            kernels.philox_normal(xi, seed_base + c, step)
            sl = slice(c * stride, c * stride + P)
            _check_step(oracle, kind, sizes, Xh, yh, batch, {k: v[sl] for k, v in host.items()},
                        {k: v[sl].copy() for k, v in new.items()}, cost_h[c], int(starts[c, t]), step, burn,
                        xi.cpu().numpy(), "%s %s %s b=%d chain %d step %d" % (kind, npdt.__name__, sizes, batch, c, step),
                        stats)
            if stride > P:                            # the padding between chains is never written
                for k in ROWS[kind]:
                    assert (new[k][c * stride + P:(c + 1) * stride] == PAD).all(), (k, c)
        series.append(cost)
        host = new
    one = {k: v.clone() for k, v in rows0.items()}
    costs = torch.full((n_chains * N_STEPS,), float("nan"), dtype=dt, device=gpu)
    _launch(kind, one, sizes, X, y, torch.tensor(starts.reshape(-1), device=gpu), batch, T0, N_STEPS, burn,
            seed_base, costs, n_chains, stride)
    for k in ROWS[kind]:
        _assert_same(one[k].cpu().numpy(), rows[k].cpu().numpy(), "one launch of %d steps vs the series: %s"
                     % (N_STEPS, k))
    _assert_same(costs.view(n_chains, N_STEPS).cpu().numpy(), torch.stack(series, dim=1).cpu().numpy(),
                 "one launch vs the series: costs")
    print("%s %s %s B=%d chains=%d LDS=%d B: max rel gradient err %.3g, max rel cost err %.3g" % (
        kind, npdt.__name__, sizes, batch, n_chains, _lds_bytes(sizes, batch, np.dtype(npdt).itemsize),
        stats["grad"], stats["cost"]))
    return stats


@pytest.mark.parametrize("kind", ["sghmc", "sgld"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("sizes,batch,n_data", SHAPES)
def test_steps_against_the_fp64_reference(gpu, oracle, sizes, batch, n_data, dt, kind):
    _run_case(gpu, oracle, kind, dt, sizes, batch, n_data)


@pytest.mark.parametrize("kind", ["sghmc", "sgld"])
@pytest.mark.parametrize("dt,sizes", [(torch.float32, [1, 100, 100, 100, 1]), (torch.float64, [1, 70, 70, 70, 1])],
                         ids=["f32_3x100", "f64_3x70"])
def test_large_lds_launches(gpu, oracle, dt, sizes, kind):
    """f32 above 64 KiB of LDS (the hipFuncSetAttribute branch) and both dtypes far above the 91 KB of the f64
    default net."""
    esize = 4 if dt == torch.float32 else 8
    assert _lds_bytes(sizes, 20, esize) > 125 * 1024
    _run_case(gpu, oracle, kind, dt, sizes, 20, 100)


@pytest.mark.parametrize("kind", ["sghmc", "sgld"])
def test_largest_accepted_launch(gpu, oracle, kind):
    """A launch that declares all 160 KiB of LDS runs, and computes what the reference computes."""
    assert _lds_bytes(NEAR_LIMIT, NEAR_LIMIT_B, 4) == LDS_LIMIT
    _run_case(gpu, oracle, kind, torch.float32, NEAR_LIMIT, NEAR_LIMIT_B, 64)


@pytest.mark.parametrize("kind", ["sghmc", "sgld"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_three_chains_with_odd_n_params(gpu, oracle, dt, kind):
    """n_params = 147: chain_stride 148, the update's tail quad belongs to the last lane of each chain; every chain
    is its own reference chain with seed_base + c, and the padding element stays untouched."""
    assert _n_params([3, 7, 13, 1]) % 4 == 3
    _run_case(gpu, oracle, kind, dt, [3, 7, 13, 1], 5, 40, n_chains=3, seed=1)


def _sampler(gpu, dt, X, y, hidden, batch):
    from pysgmcmc_amd.data_batches import Placeholder, generate_batches
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost, init_mlp_params
    from pysgmcmc_amd.samplers import SGHMCSampler
    from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule
    xp, yp = Placeholder(dtype=dt, device=gpu), Placeholder(dtype=dt, device=gpu)
    params = init_mlp_params(X.shape[1], hidden=hidden, seed=3, dtype=dt, device=gpu)
    s = SGHMCSampler(params=params, cost_fun=BNNCost(xp, yp, batch_size=batch, n_examples=X.shape[0]),
                     batch_generator=generate_batches(X, y, xp, yp, batch, seed=1),
                     stepsize_schedule=ConstantStepsizeSchedule(0.01), burn_in_steps=6, mdecay=0.05,
                     scale_grad=float(X.shape[0]), session=gpu, dtype=dt, seed=5)
    s.sample_format = "view"
    return s


def test_lds_limit_host_facts(gpu):
    """The shape one input wider than the largest accepted launch is refused before anything runs; the sampler's own
    (more conservative) LDS estimate never offers the fused path for a shape the kernel refuses."""
    assert _lds_bytes(OVER_LIMIT, NEAR_LIMIT_B, 4) > LDS_LIMIT >= _lds_bytes(NEAR_LIMIT, NEAR_LIMIT_B, 4)
    rng = np.random.default_rng(5)
    accepted = {}
    for sizes in (NEAR_LIMIT, OVER_LIMIT):
        P = _n_params(sizes)
        Xh, yh = _data(sizes, 64, np.float32, rng)
        X, y = torch.tensor(Xh, device=gpu), torch.tensor(yh, device=gpu)
        rows = {k: torch.tensor(v, device=gpu) for k, v in _chain_state("sghmc", sizes, np.float32, rng).items()}
        rows["grad"].zero_()
        before = {k: v.clone() for k, v in rows.items()}
        cost = torch.full((1,), 7.0, device=gpu)
        try:
            _launch("sghmc", rows, sizes, X, y, torch.zeros(1, dtype=torch.int32, device=gpu), NEAR_LIMIT_B, 0, 1, 0,
                    0, cost)
            torch.cuda.synchronize()
            accepted[tuple(sizes)] = True
        except SgmcmcLibraryError as e:
            assert "LDS" in str(e) and "160 KiB" in str(e), str(e)
            torch.cuda.synchronize()
            for k in rows:
                assert torch.equal(rows[k], before[k]), k
            assert float(cost[0]) == 7.0
            accepted[tuple(sizes)] = False
        s = _sampler(gpu, torch.float32, Xh.astype(np.float64), yh.astype(np.float64), tuple(sizes[1:-1]), NEAR_LIMIT_B)
        assert s.arena.n >= P and s._bnn_layer_sizes() == sizes
        assert not s.fused_bnn_available() or accepted[tuple(sizes)], sizes
    assert accepted == {tuple(NEAR_LIMIT): True, tuple(OVER_LIMIT): False}


# ---- refusals of the C entry: host checks only, nothing launched, nothing written

_RS, _RB, _RN = [3, 7, 13, 1], 5, 40            # n_params 147
_RP = _n_params(_RS)


def _refusal_args(gpu, kind):
    rng = np.random.default_rng(9)
    Xh, yh = _data(_RS, _RN, np.float32, rng)
    rows = {k: torch.tensor(rng.normal(size=2 * 148).astype(np.float32), device=gpu) for k in ROWS[kind]}
    kw = dict(rows={k: v[:_RP] for k, v in rows.items()}, sizes=list(_RS), X=torch.tensor(Xh, device=gpu),
              y=torch.tensor(yh, device=gpu), starts=torch.zeros(1, dtype=torch.int32, device=gpu), batch=_RB,
              first_step=0, n_steps=1, burn=0, seed_base=0, costs=torch.full((2,), 7.0, device=gpu))
    return rows, kw


def _misaligned(gpu, kw, name):
    buf = torch.zeros(_RP + 4, device=gpu)
    buf[1:1 + _RP].copy_(kw["rows"][name])
    kw["rows"] = dict(kw["rows"], **{name: buf[1:1 + _RP]})
    return buf


def _two_chains(gpu, kw, rows, stride):
    kw["rows"], kw["n_chains"], kw["stride"] = dict(rows), 2, stride
    kw["starts"] = torch.zeros(2, dtype=torch.int32, device=gpu)


REFUSALS = {
    "zero_layers": ("1..8 layers", lambda gpu, kw, rows: kw.update(sizes=[3])),
    "nine_layers": ("1..8 layers", lambda gpu, kw, rows: kw.update(sizes=[3, 2, 2, 2, 2, 2, 2, 2, 2, 1])),
    "last_layer_wider_than_1": ("one unit", lambda gpu, kw, rows: kw.update(sizes=[3, 7, 2])),
    "layer_size_0": ("bad layer size", lambda gpu, kw, rows: kw.update(sizes=[3, 0, 13, 1])),
    "layer_size_negative": ("bad layer size", lambda gpu, kw, rows: kw.update(sizes=[3, 7, -2, 1])),
    "batch_over_n_data": ("bad batch", lambda gpu, kw, rows: kw.update(batch=_RN + 1)),
    "batch_0": ("bad batch", lambda gpu, kw, rows: kw.update(batch=0)),
    "theta_misaligned": ("16-B aligned", lambda gpu, kw, rows: kw.update(keep=_misaligned(gpu, kw, "theta"))),
    "minv_misaligned": ("16-B aligned", lambda gpu, kw, rows: kw.update(keep=_misaligned(gpu, kw, "minv"))),
    "xi_with_odd_n_params": ("n_params % 4 == 0",
                             lambda gpu, kw, rows: kw.update(xi=torch.zeros(_RP, device=gpu))),
    "chain_stride_not_multiple_of_4": ("chain_stride", lambda gpu, kw, rows: _two_chains(gpu, kw, rows, _RP)),
    "chain_stride_below_n_params": ("chain_stride", lambda gpu, kw, rows: _two_chains(gpu, kw, rows, 144)),
}


@pytest.mark.parametrize("kind", ["sghmc", "sgld"])
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(gpu, kind, case):
    msg, mutate = REFUSALS[case]
    rows, kw = _refusal_args(gpu, kind)
    mutate(gpu, kw, rows)
    kw.pop("keep", None)
    watched = list(rows.values()) + list(kw["rows"].values()) + [kw["costs"]]
    before = [t.clone() for t in watched]
    with pytest.raises(SgmcmcLibraryError, match=re.escape(msg)):
        _launch(kind, **kw)
    torch.cuda.synchronize()
    for t, b in zip(watched, before):
        assert torch.equal(t, b)


@pytest.mark.parametrize("kind", ["sghmc", "sgld"])
@pytest.mark.parametrize("delta", [-1, 1])
def test_refusal_n_params_mismatch(gpu, kind, delta):
    """The wrapper derives n_params from the sizes; the C entry is called directly with one too few / too many."""
    rows, kw = _refusal_args(gpu, kind)
    before = {k: v.clone() for k, v in rows.items()}
    f = getattr(lib(), "sgmcmc_bnn_fused_%s_steps_f32" % kind)
    arr = (ctypes.c_int * len(_RS))(*_RS)
    ptrs = [rows[k].data_ptr() for k in ROWS[kind]]
    tail = (_RP + delta, _RP + delta, 1, arr, len(_RS) - 1, kw["X"].data_ptr(), kw["y"].data_ptr(), _RN,
            kw["starts"].data_ptr(), _RB, float(_RB), float(_RN), WDECAY, PRIOR_MEAN, PRIOR_VAR, EPS[kind], float(_RN),
            MDECAY if kind == "sghmc" else SGLD_A, 0, 1, 0, 0, None, kw["costs"].data_ptr(),
            torch.cuda.current_stream(gpu).cuda_stream)
    rc = f(*ptrs, *tail)
    assert rc != 0 and b"n_params does not match" in lib().sgmcmc_last_error()
    torch.cuda.synchronize()
    for k in rows:
        assert torch.equal(rows[k], before[k]), k
    assert (kw["costs"] == 7.0).all()


# ---- the in-place window branch through the public API: 30 features, the default 3 x 50 net, batch 20

def _thirty_features():
    rng = np.random.RandomState(1)
    X = rng.rand(100, 30)
    y = np.sinc(X[:, :3] * 10 - 5).sum(axis=1)
    return X, y


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_thirty_features_track_the_gemm_path(gpu, dt):
    X, y = _thirty_features()
    assert 20 * 30 > 512                                   # the window is loaded in place, not prefetched
    a, b = _sampler(gpu, dt, X, y, (50, 50, 50), 20), _sampler(gpu, dt, X, y, (50, 50, 50), 20)
    assert b.fused_bnn_available()
    costs_a = torch.stack([c.reshape(()).clone() for _, c in islice(a, 14)])
    costs_b = b.fused_bnn_steps(14)
    tol = 2e-4 if dt == torch.float32 else 1e-9
    ta, tb = a.arena.row("theta"), b.arena.row("theta")
    assert float((ta - tb).abs().max()) <= tol * float(ta.abs().max())
    assert torch.allclose(costs_a, costs_b, rtol=1e-4 if dt == torch.float32 else 1e-9)
    assert float((a.arena.row("minv") - b.arena.row("minv")).abs().max()) <= tol * float(a.arena.row("minv").abs().max())
    assert b.n_iterations == 14 and not b.is_burning_in


def test_bnn_train_at_thirty_features_takes_the_fused_path(gpu):
    from pysgmcmc_amd.models.bayesian_neural_network import BayesianNeuralNetwork
    X, y = _thirty_features()
    bnn = BayesianNeuralNetwork(session=gpu, dtype=torch.float32, burn_in_steps=200, sample_steps=20, n_nets=4, seed=1)
    bnn.train(X, y)
    assert bnn.used_fused_steps and len(bnn.samples) == 4
    m, v = bnn.predict(X[:10])
    assert np.isfinite(m).all() and np.isfinite(v).all()
