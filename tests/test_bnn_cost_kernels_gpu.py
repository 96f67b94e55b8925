"""The BNN cost path's small kernels (csrc/sgmcmc_bnn_cost.hip, and the sum(theta^2) slicing side job of
csrc/sgmcmc_bnn_gemm.hip), each called directly and compared element by element with a float64 numpy reference computed
from the same (already rounded) inputs:

- ``bnn_head`` and the head folded into ``bnn_head_last_layer_backward``: delta, cost, d cost/d log_var, the last-bias
  gradient and mse (computed in double, then rounded to T);
- ``bnn_last_layer_backward``, ``tanh_backward_colsum``, ``tanh_backward`` and the column half of the fused head: the
  elementwise tanh' products and the column sums / weight gradient accumulated in T;
- ``tanh_rowdot`` and ``bias_tanh``: bias + tanh and the output unit's row dot product;
- the sum(theta^2) slices of ``tanh_rowdot`` and ``bnn_dense_tanh``, and the head's own sum over the statistics records.

Every bar is written at its assert (``u`` is the unit roundoff of T). The constants make every prior and beta term at least
1e-2 of the result it enters, and the inputs keep every sum free of cancellation, so a dropped or doubled term, row or
record moves a result by far more than its bar. The statistics records are small integers: every slice and every
sum(theta^2) is exact in any order and must be equal, not close. Every output buffer, one element past its end, the
records past the count, statistics 1..3 of each record and the unused slices hold NaN: nothing outside the contract may be
written, and nothing NaN may be read.

The C entries' refusals are checked on the host with dummy pointers (the calls fail before anything is launched), and
so is the float64 head reference against ``oracle.bnn_cost_and_grad``: those tests need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd._lib import lib

NAN = float("nan")
DTS = [torch.float32, torch.float64]
NPT = {torch.float32: np.float32, torch.float64: np.float64}
UNIT = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
INT = {torch.float32: torch.int32, torch.float64: torch.int64}

# constants under which every prior / beta term matters (batch_size != rows), and the library's own
SMALL = dict(n_examples=2.5, n_params=37.0, wdecay=3.0, prior_mean=0.5, prior_var=2.0)
REALISTIC = dict(n_examples=1000.0, n_params=5252.0, wdecay=1.0, prior_mean=1e-6, prior_var=0.01)
BETA = 0.37

_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Largest error per kernel, dtype and output as a fraction of its bar (shown with ``-s``)."""
    yield
    for key in sorted(_WORST):
        print("bar fraction %-44s %.3g" % ("/".join(key), _WORST[key]))


def _check(key, got, ref, bar, what):
    got = np.asarray(got, np.float64).ravel()
    ref, bar = [np.asarray(x, np.float64) for x in (ref, bar)]
    ref, bar = [x.ravel() if x.size == got.size else np.broadcast_to(x, got.shape) for x in (ref, bar)]
    err = np.abs(got - ref)
    ok = err <= bar                                   # NaN anywhere: not ok
    if got.size:
        frac = float(np.max(np.divide(err, bar, out=np.zeros_like(err), where=bar > 0)))
        _WORST[key] = max(_WORST.get(key, 0.0), frac)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError("%s: %d of %d outside the bar; first at %d: got %r ref %r bar %r"
                             % (what, int((~ok).sum()), got.size, i, got[i], ref[i], bar[i]))


def _ulp_bar(ref, dt, n_ulp=1.0):
    """n ulp of T at float32(ref) in f32; relative 1e-13 in f64 (values computed in double, then rounded to T)."""
    ref = np.asarray(ref, np.float64)
    if dt == torch.float32:
        return n_ulp * np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64)
    return 1e-13 * np.abs(ref)


def _tanh_bar(ref, dt):
    """4 ulp of T at the reference tanh (the device libm's tanhf / tanh, plus the rounding of a + bias in T)."""
    ref = np.abs(np.asarray(ref, np.float64))
    return 4.0 * np.spacing(ref.astype(NPT[dt])).astype(np.float64)


def _nan_buf(n, dt, dev, lead=0):
    """NaN-filled device buffer with ``lead`` elements before and one after a view of n elements."""
    buf = torch.full((lead + n + 1,), NAN, dtype=dt, device=dev)
    return buf, buf[lead:lead + n]


def _put(arr, dt, dev, lead=0):
    a = np.ascontiguousarray(np.asarray(arr, NPT[dt]).ravel())
    buf, view = _nan_buf(a.size, dt, dev, lead)
    view.copy_(torch.from_numpy(a))
    return buf, view


def _rounded(arr, dt):
    return np.asarray(arr, NPT[dt]).astype(np.float64)


def _bits(t):
    return t.view(INT[t.dtype]) if t.dtype in INT else t


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _untouched(buf, lo, hi):
    """buf[lo:hi] still holds the NaN it was filled with."""
    return bool(torch.isnan(buf[lo:hi]).all())


def _workspace(nparts, dev, rng, extra=8):
    """A statistics workspace as a step kernel leaves it (csrc/sgmcmc_stream.hpp): float64, element 0 the record count as
    uint64, statistic s of record i at 4 + 4 i + s. Statistic 0 = small integers; the rest of the header, statistics 1..3
    and ``extra`` records past the count are NaN."""
    recs = rng.randint(1, 6, size=nparts).astype(np.float64)
    ws = np.full(4 + 4 * (nparts + extra), np.nan)
    ws[4:4 + 4 * nparts:4] = recs
    t = torch.from_numpy(ws).to(dev)
    t.view(torch.int64)[0] = nparts
    return t, recs


def _slices(recs, n_slices):
    """Slice s = the records [s len, min((s + 1) len, nparts)), len = ceil(nparts / n_slices)."""
    n = recs.size
    ln = -(-n // n_slices)
    return np.array([recs[s * ln:min((s + 1) * ln, n)].sum() for s in range(n_slices)])


def _consts(rows, base=SMALL):
    k = dict(base)
    k["batch_size"] = float(rows) if base is REALISTIC else 1.3 * rows + 0.7
    return k


def _head_ref(mean, y, s, tsq, k, last_bias, fold, add_bias):
    """Loss head in float64, formula by formula as oracle.sgmcmc_oracle.bnn_cost_and_grad (mean without the last bias
    when add_bias; the prior's gradient omitted when fold)."""
    mean, y = np.asarray(mean, np.float64), np.asarray(y, np.float64)
    B = mean.size
    bs, nex = k["batch_size"], k["n_examples"]
    es = np.exp(s)
    inv = 1.0 / (es + 1e-16)
    dscale = -(inv / bs)
    r = y - (mean + (last_bias if add_bias else 0.0))
    sse, sumr = float(np.sum(r * r)), float(np.sum(r))
    wp_den, lvp_den = k["n_params"] + 3e-16, 2.0 * k["prior_var"] + 3e-16
    d = s - np.log(k["prior_mean"])
    log_like = (-(sse * (0.5 * inv)) - 0.5 * s * B) / bs
    lvp = -(d * d) / lvp_den - 0.5 * np.log(k["prior_var"])
    wp = (-0.5 * k["wdecay"]) * tsq / wp_den
    coef = 0.0 if fold else k["wdecay"] / (wp_den * nex)
    return dict(r=r, delta=r * dscale, dscale=dscale, inv=inv, es=es, bs=bs,
                cost=-(log_like + lvp / nex + wp / nex),
                ds=-((sse * (0.5 * es * inv * inv) - 0.5 * B) / bs + (-2.0 * d / lvp_den) / nex) + coef * s,
                gb=sumr * dscale + coef * last_bias, mse=sse / B)


def _head_inputs(rng, rows, dt, last_bias, add_bias, mean=None):
    """Pre-bias means, and targets below mean + bias by 0.5 .. 1.5: every residual negative, every delta positive."""
    if mean is None:
        mean = _rounded(rng.uniform(-1.0, 1.0, rows), dt)
    y = _rounded(mean + (last_bias if add_bias else 0.0) - rng.uniform(0.5, 1.5, rows), dt)
    return mean, y


def _h(rng, rows, cols):
    """Activations in (0, 1) (no cancellation in sum h * dvec), one in ten saturated (h > 0.999: 1 - h^2 cancels)."""
    h = rng.uniform(0.02, 0.98, (rows, cols))
    sat = rng.rand(rows, cols) < 0.1
    h[sat] = 1.0 - rng.uniform(1e-5, 9e-4, int(sat.sum()))
    return h


def _signed(rng, n):
    return rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)


def _colsum_depth(rows):
    """Longest chain of additions of a column sum: ceil(rows / 64) per row lane, 2 shuffles, 16 waves, the beta term."""
    return -(-rows // 64) + 19


def _scalars(dev, dt):
    """cost, d/d log_var, last-bias gradient, mse at 0, 2, 4, 6 of one NaN buffer: the odd slots must stay NaN."""
    sc = torch.full((8,), NAN, dtype=dt, device=dev)
    return sc, sc[0:1], sc[2:3], sc[4:5], sc[6:7]


def _check_scalars(key, sc, ref, dt, grad_b, prop=None):
    """The head's scalars: 1 ulp of float32(ref) / 1e-13 relative, plus what an inexact mean propagates (``prop``)."""
    prop = prop or {}
    got = sc.cpu().numpy().astype(np.float64)
    assert np.isnan(got[1::2]).all(), "a head output wrote past its element"
    for name, slot in (("cost", 0), ("ds", 2), ("mse", 6)) + ((("gb", 4),) if grad_b else ()):
        _check(key + (name,), got[slot], ref[name], _ulp_bar(ref[name], dt) + prop.get(name, 0.0), "%s %s" % (key, name))
    if not grad_b:
        assert np.isnan(got[4]), "grad_last_bias_out=None wrote its slot"


# ---------------------------------------------------------------------------------------------------------------------
# host: the reference, the refusals
# ---------------------------------------------------------------------------------------------------------------------

def test_head_reference_equals_the_oracle():
    """The float64 head reference == oracle.bnn_cost_and_grad's cost, d cost/d log_var and last-bias gradient on a tiny
    full net (to 1e-13)."""
    from oracle import sgmcmc_oracle
    rng = np.random.RandomState(0)
    sizes = [3, 6, 5, 1]
    params = []
    for a, b in zip(sizes[:-1], sizes[1:]):
        params += [rng.randn(a, b) / np.sqrt(a), rng.randn(b) * 0.3]
    params.append(np.full((1, 1), 0.4))
    X, Y = rng.rand(7, 3), rng.rand(7, 1)
    k = dict(SMALL, batch_size=9.1)
    k["n_params"] = float(sum(p.size for p in params))
    cost, grads = sgmcmc_oracle.bnn_cost_and_grad(params, X, Y, k["batch_size"], k["n_examples"], k["wdecay"],
                                                  k["prior_mean"], k["prior_var"])
    h = X
    for l in range(len(sizes) - 2):
        h = np.tanh(h @ params[2 * l] + params[2 * l + 1])
    mean = (h @ params[-3]).ravel()
    tsq = float(sum((p ** 2).sum() for p in params))
    ref = _head_ref(mean, Y.ravel(), 0.4, tsq, k, float(params[-2][0]), fold=False, add_bias=True)
    for got, want in ((ref["cost"], cost), (ref["ds"], grads[-1][0, 0]), (ref["gb"], grads[-2][0])):
        assert abs(got - want) <= 1e-13 * abs(want), (got, want)
    # the last weight gradient: sum_r h[r] delta[r] + the prior term
    coef = k["wdecay"] / ((k["n_params"] + 3e-16) * k["n_examples"])
    gw = h.T @ ref["delta"] + coef * params[-3].ravel()
    assert np.allclose(gw, grads[-3].ravel(), rtol=1e-13, atol=0)


P = ctypes.c_void_p(4096)          # never dereferenced: every call below fails on the host first
D6 = (10.0, 2.5, 37.0, 3.0, 0.5, 2.0)


def _head_call(sfx, mean=P, y=P, lv=P, tsq=P, ws=None, lb=P, B=8, flags=0, delta=P, cost=P, gs=P, gb=P, mse=P):
    return getattr(lib(), "sgmcmc_bnn_head_" + sfx)(mean, y, lv, tsq, ws, lb, B, *D6, flags, delta, cost, gs, gb, mse, None)


def _fused_call(sfx, parts=1, rows=8, cols=8, mean=P, tsq=P, lb=P, bias=P, beta=0.0, gb=P, w=P, h=P):
    return getattr(lib(), "sgmcmc_bnn_head_last_layer_backward_" + sfx)(
        mean, parts, P, P, tsq, lb, rows, cols, *D6, 2, w, h, bias, beta, P, P, gb, P, P, P, P, None)


REFUSALS = [
    ("bnn_head: grad_last_bias_out without last_bias", lambda s: _head_call(s, lb=None)),
    ("bnn_head: B == 0", lambda s: _head_call(s, B=0)),
    ("bnn_head: neither theta_sumsq nor stats_ws", lambda s: _head_call(s, tsq=None)),
    ("bnn_head: no delta", lambda s: _head_call(s, delta=None)),
    ("fused head: 0 mean parts", lambda s: _fused_call(s, parts=0)),
    ("fused head: 4097 mean parts", lambda s: _fused_call(s, parts=4097)),
    ("fused head: 2 parts at 1025 rows", lambda s: _fused_call(s, parts=2, rows=1025)),
    ("fused head: 4096 parts at 1025 rows", lambda s: _fused_call(s, parts=4096, rows=1025)),
    ("fused head: beta without bias_prev", lambda s: _fused_call(s, bias=None, beta=0.5)),
    ("fused head: grad_last_bias_out without last_bias", lambda s: _fused_call(s, lb=None)),
    ("fused head: no tsq_parts", lambda s: _fused_call(s, tsq=None)),
    ("fused head: no rows", lambda s: _fused_call(s, rows=0)),
    ("fused head: no columns", lambda s: _fused_call(s, cols=0)),
    ("last_layer_backward: beta without bias_prev",
     lambda s: getattr(lib(), "sgmcmc_bnn_last_layer_backward_" + s)(P, P, P, 8, 8, None, 0.5, P, P, P, None)),
    ("last_layer_backward: no h",
     lambda s: getattr(lib(), "sgmcmc_bnn_last_layer_backward_" + s)(P, P, None, 8, 8, P, 0.5, P, P, P, None)),
    ("tanh_backward_colsum: beta without bias",
     lambda s: getattr(lib(), "sgmcmc_tanh_backward_colsum_" + s)(P, P, 8, 8, None, 0.5, P, None)),
    ("tanh_backward_colsum: no colsum",
     lambda s: getattr(lib(), "sgmcmc_tanh_backward_colsum_" + s)(P, P, 8, 8, P, 0.5, None, None)),
    ("tanh_backward: no h", lambda s: getattr(lib(), "sgmcmc_tanh_backward_" + s)(P, None, 8, None)),
    ("tanh_rowdot: stats_ws without tsq_parts",
     lambda s: getattr(lib(), "sgmcmc_bias_tanh_rowdot_" + s)(P, P, P, 8, 8, P, P, None, None)),
    ("tanh_rowdot: tsq_parts without stats_ws",
     lambda s: getattr(lib(), "sgmcmc_bias_tanh_rowdot_" + s)(P, P, P, 8, 8, P, None, P, None)),
    ("tanh_rowdot: no w", lambda s: getattr(lib(), "sgmcmc_bias_tanh_rowdot_" + s)(P, P, None, 8, 8, P, None, None, None)),
    ("tanh_rowdot: 2^31 rows",
     lambda s: getattr(lib(), "sgmcmc_bias_tanh_rowdot_" + s)(P, P, P, 2 ** 31, 8, P, None, None, None)),
    ("bias_tanh: no bias", lambda s: getattr(lib(), "sgmcmc_bias_tanh_" + s)(P, None, 8, 8, None)),
]


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("what,call", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_cost_path_entries_refuse_what_they_cannot_take(sfx, what, call):
    assert call(sfx) == -1, what                                   # SGMCMC_EINVAL, before any launch
    assert lib().sgmcmc_last_error(), what


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("rows,cols", [(1, 2 ** 32 - 2 ** 24 + 1), (2 ** 32 - 2 ** 24 + 1, 1), (2 ** 16, 2 ** 16 - 2 ** 8 + 1),
                                       (2 ** 16, 2 ** 16), (2 ** 40, 2 ** 40)])
def test_bias_tanh_refuses_more_than_its_32_bit_index_can_step(sfx, rows, cols):
    """The scalar path steps a 32-bit index by up to 65536 x 256 = 2^24 lanes: past 2^32 - 2^24 elements it would wrap and
    loop (elements tanh'd twice, lanes that never leave). The host refuses those sizes, products that overflow included."""
    rc = getattr(lib(), "sgmcmc_bias_tanh_" + sfx)(P, P, rows, cols, None)
    assert rc == -1 and b"2^32 - 2^24" in lib().sgmcmc_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the loss head
# ---------------------------------------------------------------------------------------------------------------------

HEAD_B = [1, 63, 64, 65, 1023, 1024, 1025, 5000]
HEAD_NPARTS = [None, 0, 1, 4095, 4096, 4097, 10007]          # None: sum(theta^2) as a float64 scalar


def _run_head(dev, dt, mean, y, s, lb, k, fold, add_bias, grad_b, tsq_scalar=None, ws=None):
    B = mean.size
    mb, mv = _put(mean, dt, dev)
    yb, yv = _put(y, dt, dev)
    _, sv = _put([s], dt, dev)
    _, lbv = _put([lb], dt, dev)
    tq = None if ws is not None else torch.tensor([tsq_scalar], dtype=torch.float64, device=dev)
    db, dv = _nan_buf(B, dt, dev)
    sc, c, gs, gb, mse = _scalars(dev, dt)
    kernels.bnn_head(mv, yv, sv, tq, k["batch_size"], k["n_examples"], k["n_params"], k["wdecay"], k["prior_mean"],
                     k["prior_var"], dv, c, gs, mse, fold_prior_grad=fold, stats_workspace=ws, last_bias=lbv,
                     grad_last_bias_out=gb if grad_b else None, add_last_bias=add_bias)
    assert _untouched(mb, B, B + 1) and _untouched(yb, B, B + 1)
    return db, sc


def _head_case(dev, dt, rng, B, nparts, fold, add_bias, grad_b, s=0.7, base=SMALL):
    k = _consts(B, base)
    lb = float(NPT[dt](-0.3))
    s = float(NPT[dt](s))
    mean, y = _head_inputs(rng, B, dt, lb, add_bias)
    if nparts is None:
        ws, tsq = None, 41.0
    else:
        ws, recs = _workspace(nparts, dev, rng)
        tsq = float(recs.sum())
        ws0 = ws.clone()
    ref = _head_ref(mean, y, s, tsq, k, lb, fold, add_bias)
    db, sc = _run_head(dev, dt, mean, y, s, lb, k, fold, add_bias, grad_b, tsq_scalar=tsq, ws=ws)
    key = ("bnn_head", str(dt)[6:])
    what = (B, nparts, fold, add_bias, grad_b, s)
    assert _untouched(db, B, B + 1), what
    _check(key + ("delta",), db[:B].cpu().numpy(), ref["delta"], _ulp_bar(ref["delta"], dt), "delta %r" % (what,))
    _check_scalars(key, sc, ref, dt, grad_b)
    if ws is not None:
        assert _same_bits(ws, ws0), "the head wrote into the statistics workspace"
    # a second launch: the same bits
    db2, sc2 = _run_head(dev, dt, mean, y, s, lb, k, fold, add_bias, grad_b, tsq_scalar=tsq, ws=ws)
    assert _same_bits(db, db2) and _same_bits(sc, sc2), what


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B", HEAD_B)
def test_head_equals_fp64(gpu, dt, B):
    """bnn_head at batches around the 64-lane waves and the 1024-lane block, sum(theta^2) as a scalar or from 0 .. 10 007
    records (the 4-record loop starts at 4096), every flag on and off."""
    rng = np.random.RandomState(B)
    for nparts in HEAD_NPARTS:
        for flags in range(8):
            _head_case(gpu, dt, rng, B, nparts, bool(flags & 1), bool(flags & 2), bool(flags & 4))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_head_at_the_log_var_extremes_and_the_library_constants(gpu, dt):
    """log_var -40 (the 1e-16 guard dominates exp(s)), +20, and the library's own constants (n_examples 1000, wdecay 1,
    prior_mean 1e-6, prior_var 0.01, batch_size == rows): finite and to the same bars."""
    rng = np.random.RandomState(7)
    for s in (-40.0, 20.0):
        for B in (1, 1025):
            _head_case(gpu, dt, rng, B, 4097, False, True, True, s=s)
            _head_case(gpu, dt, rng, B, None, True, False, True, s=s)
    for B in (20, 256, 5000):
        _head_case(gpu, dt, rng, B, None, False, True, True, s=-6.9, base=REALISTIC)
        _head_case(gpu, dt, rng, B, 10007, False, True, True, s=-2.0, base=REALISTIC)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the column kernels
# ---------------------------------------------------------------------------------------------------------------------

COL_ROWS = [1, 2, 63, 64, 65, 192, 193, 255, 256, 257, 448, 449, 512, 1000, 1024, 1025, 4099]
COL_SHAPES = ([(r, c) for r in COL_ROWS for c in (1, 15, 16, 17, 50, 130)]
              + [(1, 2048), (65, 2049), (257, 2048), (449, 2049), (1025, 2048), (4099, 2049)])


def _elem_bar(dvw, h, u):
    """delta_prev / tanh': 4 u |delta_or_dvec * w| (1 + h^2) -- 1 - h*h cancels near |h| = 1, so no plain ulp bar."""
    return 4.0 * u * np.abs(dvw) * (1.0 + h * h)


def _colsum_parts(dvw, h, u):
    """Reference, elementwise bar and sum of |terms| of delta_prev = dvw * (1 - h^2)."""
    terms = dvw * (1.0 - h * h)
    return terms, _elem_bar(dvw, h, u)


def _col_case_inputs(rng, rows, cols, dt):
    h = _rounded(_h(rng, rows, cols), dt)
    w = _rounded(_signed(rng, cols), dt)
    bias = _rounded(_signed(rng, cols), dt)
    return h, w, bias


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_last_layer_backward_equals_fp64(gpu, dt):
    """delta_prev = dvec w (1 - h^2), colsum = sum_r delta_prev + beta bias_prev, gw = sum_r h dvec + beta w at every row
    branch (4-row trips while r + 192 < rows, the 64-row tail) and column-block edge."""
    u, key = UNIT[dt], ("last_layer_backward", str(dt)[6:])
    rng = np.random.RandomState(11)
    for rows, cols in COL_SHAPES:
        h, w, bias = _col_case_inputs(rng, rows, cols, dt)
        dvec = _rounded(rng.uniform(0.5, 1.5, rows) / rows, dt)
        for beta in (0.0, BETA):
            bt = float(NPT[dt](beta))
            what = (rows, cols, beta)
            hb, hv = _put(h, dt, gpu)
            _, dvv = _put(dvec, dt, gpu)
            _, wv = _put(w, dt, gpu)
            _, bv = _put(bias, dt, gpu)
            runs = []
            for _ in range(2):
                dpb, dpv = _nan_buf(rows * cols, dt, gpu)
                csb, csv = _nan_buf(cols, dt, gpu)
                gwb, gwv = _nan_buf(cols, dt, gpu)
                kernels.bnn_last_layer_backward(dvv, wv, hv.view(rows, cols), dpv.view(rows, cols), csv, gwv,
                                                bias_prev=bv if beta else None, beta=bt)
                runs.append((dpb, csb, gwb))
            assert all(_same_bits(a, b) for a, b in zip(*runs)), what
            dpb, csb, gwb = runs[0]
            assert _untouched(dpb, rows * cols, None) and _untouched(csb, cols, None) and _untouched(gwb, cols, None), what
            assert _untouched(hb, rows * cols, None), what
            H = h.reshape(rows, cols)
            terms, ebar = _colsum_parts(dvec[:, None] * w[None, :], H, u)
            _check(key + ("delta_prev",), dpb[:rows * cols].cpu().numpy(), terms, ebar, "delta_prev %r" % (what,))
            depth = _colsum_depth(rows)
            cs_ref = terms.sum(0) + bt * bias
            cs_bar = (depth + 4) * u * (np.abs(terms).sum(0) + abs(bt) * np.abs(bias)) + ebar.sum(0)
            _check(key + ("colsum",), csb[:cols].cpu().numpy(), cs_ref, cs_bar, "colsum %r" % (what,))
            hd = H * dvec[:, None]
            gw_ref = hd.sum(0) + bt * w
            gw_bar = (depth + 4) * u * (np.abs(hd).sum(0) + abs(bt) * np.abs(w))
            _check(key + ("gw",), gwb[:cols].cpu().numpy(), gw_ref, gw_bar, "gw %r" % (what,))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_tanh_backward_colsum_equals_fp64(gpu, dt):
    """delta *= 1 - h^2 in place and colsum = sum_r delta + beta bias at every row branch and column-block edge."""
    u, key = UNIT[dt], ("tanh_backward_colsum", str(dt)[6:])
    rng = np.random.RandomState(12)
    for rows, cols in COL_SHAPES:
        h, _, bias = _col_case_inputs(rng, rows, cols, dt)
        delta = _rounded(rng.uniform(0.5, 1.5, (rows, cols)) / rows * rng.choice([-1.0, 1.0], cols)[None, :], dt)
        for beta in (0.0, BETA):
            bt = float(NPT[dt](beta))
            what = (rows, cols, beta)
            hb, hv = _put(h, dt, gpu)
            _, bv = _put(bias, dt, gpu)
            runs = []
            for _ in range(2):
                db, dv = _put(delta, dt, gpu)
                csb, csv = _nan_buf(cols, dt, gpu)
                kernels.tanh_backward_colsum(dv.view(rows, cols), hv.view(rows, cols), csv, bias=bv if beta else None, beta=bt)
                runs.append((db, csb))
            assert all(_same_bits(a, b) for a, b in zip(*runs)), what
            db, csb = runs[0]
            assert _untouched(db, rows * cols, None) and _untouched(csb, cols, None), what
            terms, ebar = _colsum_parts(delta.reshape(rows, cols), h.reshape(rows, cols), u)
            _check(key + ("delta",), db[:rows * cols].cpu().numpy(), terms, ebar, "delta %r" % (what,))
            cs_ref = terms.sum(0) + bt * bias
            cs_bar = (_colsum_depth(rows) + 4) * u * (np.abs(terms).sum(0) + abs(bt) * np.abs(bias)) + ebar.sum(0)
            _check(key + ("colsum",), csb[:cols].cpu().numpy(), cs_ref, cs_bar, "colsum %r" % (what,))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_tanh_backward_equals_fp64(gpu, dt):
    u, key = UNIT[dt], ("tanh_backward", str(dt)[6:])
    rng = np.random.RandomState(13)
    for n in (1, 63, 255, 256, 257, 100003):
        h = _rounded(_h(rng, 1, n).ravel() * rng.choice([-1.0, 1.0], n), dt)
        delta = _rounded(_signed(rng, n), dt)
        _, hv = _put(h, dt, gpu)
        db, dv = _put(delta, dt, gpu)
        kernels.tanh_backward(dv, hv)
        db2, dv2 = _put(delta, dt, gpu)
        kernels.tanh_backward(dv2, hv)
        assert _same_bits(db, db2) and _untouched(db, n, None), n
        terms, ebar = _colsum_parts(delta, h, u)
        _check(key + ("delta",), dv.cpu().numpy(), terms, ebar, "tanh_backward %d" % n)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the loss head folded into the last layer's backward
# ---------------------------------------------------------------------------------------------------------------------

def _run_fused(dev, dt, mean_parts, y, s, tsq_slices, lb, k, fold, add_bias, grad_b, h, w, bias, beta):
    """One launch; mean_parts [n_parts, rows]; tsq_parts = the given slices, NaN after them (17 elements)."""
    n_parts, rows = mean_parts.shape
    cols = w.size
    mb, mv = _put(mean_parts, dt, dev)
    yb, yv = _put(y, dt, dev)
    _, sv = _put([s], dt, dev)
    _, lbv = _put([lb], dt, dev)
    tb = torch.full((17,), NAN, dtype=torch.float64, device=dev)
    tb[:len(tsq_slices)] = torch.tensor(np.asarray(tsq_slices, np.float64), device=dev)
    hb, hv = _put(h, dt, dev)
    _, wv = _put(w, dt, dev)
    _, bv = _put(bias, dt, dev)
    sc, c, gs, gb, mse = _scalars(dev, dt)
    dpb, dpv = _nan_buf(rows * cols, dt, dev)
    csb, csv = _nan_buf(cols, dt, dev)
    gwb, gwv = _nan_buf(cols, dt, dev)
    kernels.bnn_head_last_layer_backward(mv.view(n_parts, rows) if n_parts > 1 else mv, yv, sv, tb, lbv, k["batch_size"],
                                         k["n_examples"], k["n_params"], k["wdecay"], k["prior_mean"], k["prior_var"], wv,
                                         hv.view(rows, cols), bv if beta else None, beta, c, gs, gb if grad_b else None, mse,
                                         dpv.view(rows, cols), csv, gwv, fold_prior_grad=fold, add_last_bias=add_bias)
    assert _untouched(dpb, rows * cols, None) and _untouched(csb, cols, None) and _untouched(gwb, cols, None)
    assert _untouched(tb, len(tsq_slices), None) and _untouched(mb, mean_parts.size, None) and _untouched(yb, rows, None)
    return sc, dpb, csb, gwb


def _fused_case(dev, dt, rng, rows, cols, n_parts, beta, fold, add_bias, grad_b, s=0.7, compare_separate=False):
    u, key = UNIT[dt], ("head_last_layer_backward", str(dt)[6:])
    what = (rows, cols, n_parts, beta, fold, add_bias, grad_b, s)
    k = _consts(rows)
    lb, s, bt = float(NPT[dt](-0.3)), float(NPT[dt](s)), float(NPT[dt](beta))
    n_tsq = 16 if (n_parts > 1 or rows >= 16) else rows            # min(16, workgroups of the forward launch)
    slices = rng.randint(1, 40, n_tsq).astype(np.float64)
    if n_parts == 1:
        parts = _rounded(rng.uniform(-1.0, 1.0, (1, rows)), dt)
    else:                                                         # positive parts of a mean in 0.5 .. 1.5
        parts = _rounded(rng.uniform(0.5, 1.5, (n_parts, rows)) / n_parts, dt)
    mean_ref = parts.sum(0)
    per = -(-n_parts // 4)
    mean_bar = (per + 3 + 4) * u * np.abs(parts).sum(0) if n_parts > 1 else np.zeros(rows)
    if n_parts > 1:
        # the per-row mean the launch adds up in T, seen through a probe launch: y = 0, log_var = 0, batch_size = 1
        # (dvec = mean exactly), one column with w = 1, h = 0 (delta_prev = dvec exactly)
        kp = dict(k, batch_size=1.0)
        _, dp, _, _ = _run_fused(dev, dt, parts, np.zeros(rows), 0.0, np.zeros(n_tsq), lb, kp, True, False, False,
                                 np.zeros((rows, 1)), np.ones(1), np.zeros(1), 0.0)
        _check(key + ("mean",), dp[:rows].cpu().numpy(), mean_ref, mean_bar, "summed mean %r" % (what,))
    _, y = _head_inputs(rng, rows, dt, lb, add_bias, mean=mean_ref)
    h, w, bias = _col_case_inputs(rng, rows, cols, dt)
    ref = _head_ref(mean_ref, y, s, float(slices.sum()), k, lb, fold, add_bias)
    out = _run_fused(dev, dt, parts, y, s, slices, lb, k, fold, add_bias, grad_b, h, w, bias, bt)
    out2 = _run_fused(dev, dt, parts, y, s, slices, lb, k, fold, add_bias, grad_b, h, w, bias, bt)
    assert all(_same_bits(a, b) for a, b in zip(out, out2)), what
    sc, dpb, csb, gwb = out
    # what the inexact mean propagates (0 with one part): through the residuals into dvec, sse and sum r
    e_dv = abs(ref["dscale"]) * mean_bar
    dsse = float(np.sum(2.0 * np.abs(ref["r"]) * mean_bar + mean_bar ** 2))
    prop = dict(cost=0.5 * ref["inv"] / ref["bs"] * dsse, ds=0.5 * ref["es"] * ref["inv"] ** 2 / ref["bs"] * dsse,
                mse=dsse / rows, gb=abs(ref["dscale"]) * float(mean_bar.sum()))
    _check_scalars(key, sc, ref, dt, grad_b, prop)
    H = h.reshape(rows, cols)
    dvec = ref["delta"]
    terms, ebar = _colsum_parts(dvec[:, None] * w[None, :], H, u)
    ebar = ebar + np.abs(w)[None, :] * (1.0 + H * H) * e_dv[:, None]
    _check(key + ("delta_prev",), dpb[:rows * cols].cpu().numpy(), terms, ebar, "delta_prev %r" % (what,))
    depth = _colsum_depth(rows)
    cs_ref = terms.sum(0) + bt * bias
    cs_bar = (depth + 4) * u * (np.abs(terms).sum(0) + abs(bt) * np.abs(bias)) + ebar.sum(0)
    _check(key + ("colsum",), csb[:cols].cpu().numpy(), cs_ref, cs_bar, "colsum %r" % (what,))
    hd = H * dvec[:, None]
    gw_ref = hd.sum(0) + bt * w
    gw_bar = (depth + 4) * u * (np.abs(hd).sum(0) + abs(bt) * np.abs(w)) + (np.abs(H) * e_dv[:, None]).sum(0)
    _check(key + ("gw",), gwb[:cols].cpu().numpy(), gw_ref, gw_bar, "gw %r" % (what,))
    if compare_separate:
        # one part: bit-equal to bnn_head (sum(theta^2) as the same integer) + last_layer_backward
        db, sc1 = _run_head(dev, dt, parts[0], y, s, lb, k, fold, add_bias, grad_b, tsq_scalar=float(slices.sum()))
        _, hv = _put(h, dt, dev)
        _, wv = _put(w, dt, dev)
        _, bv = _put(bias, dt, dev)
        dp2, cs2, gw2 = _nan_buf(rows * cols, dt, dev)[0], _nan_buf(cols, dt, dev)[0], _nan_buf(cols, dt, dev)[0]
        kernels.bnn_last_layer_backward(db[:rows], wv, hv.view(rows, cols), dp2[:rows * cols].view(rows, cols), cs2[:cols],
                                        gw2[:cols], bias_prev=bv if beta else None, beta=bt)
        assert _same_bits(dp2, dpb) and _same_bits(cs2, csb) and _same_bits(gw2, gwb), what
        assert _same_bits(sc1, sc), what


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_fused_head_columns_equal_fp64(gpu, dt):
    """One mean part at every row branch and column-block edge of the column workgroups (rows up to 4099: no 1024-row limit
    with one part), beta 0 and 0.37, the flags in turn; sum(theta^2) from min(16, rows) slices; bit-equal to the separate
    head + last-layer backward launches."""
    rng = np.random.RandomState(14)
    for i, (rows, cols) in enumerate(COL_SHAPES):
        for j, beta in enumerate((0.0, BETA)):
            f = 2 * i + j
            _fused_case(gpu, dt, rng, rows, cols, 1, beta, bool(f & 1), bool(f & 2), bool(f & 4), compare_separate=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n_parts", [2, 3, 4, 5, 8, 31, 32, 33, 88, 4096])
def test_fused_head_partial_means_equal_fp64(gpu, dt, n_parts):
    """The mean as n_parts partial dot products per row (prefetched up to 32 parts, the 4-part loop and its remainder past
    that; a second pass over the mean rows past 256 rows). 32 and 88: what bnn_dense_tanh_dot_parts gives at 256 x 2048 and
    256 x 4864 on 256 compute units."""
    rng = np.random.RandomState(n_parts)
    for i, rows in enumerate((1, 16, 255, 256, 257, 1000, 1024)):
        _fused_case(gpu, dt, rng, rows, 17, n_parts, BETA, bool(i & 1), True, True)
    if n_parts == 32:
        _fused_case(gpu, dt, rng, 256, 2048, 32, BETA, True, True, True)          # configs[2]'s shape


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_fused_head_at_the_log_var_extremes(gpu, dt):
    rng = np.random.RandomState(15)
    for s in (-40.0, 20.0):
        _fused_case(gpu, dt, rng, 257, 50, 1, BETA, False, True, True, s=s, compare_separate=True)
        _fused_case(gpu, dt, rng, 1000, 17, 33, BETA, False, True, True, s=s)


ONE_HEAD_SHAPES = [(r, c) for r in (1, 63, 65, 257, 1025) for c in (1, 17)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_the_plain_and_the_fused_head_are_one_head(gpu, dt):
    """bnn_head (sum(theta^2) given directly) and bnn_head_last_layer_backward (one mean part, the same total as small
    integers in tsq_parts) on identical inputs: cost, d cost/d log_var, the last-bias gradient and mse are the same bits,
    and the fused delta_prev[r][c] is (delta[r] * w[c]) * (1 - h[r][c]^2) formed in T from the plain head's delta. Rows: one
    lane, either side of a wave, past one four-row trip, past one 1024-lane block stride; columns: one, one past a block."""
    rng = np.random.RandomState(18)
    one = NPT[dt](1)
    for i, (rows, cols) in enumerate(ONE_HEAD_SHAPES):
        fold, add_bias = bool(i & 1), bool(i & 2)
        k = _consts(rows)
        lb, s, bt = float(NPT[dt](-0.3)), float(NPT[dt](0.7)), float(NPT[dt](BETA))
        mean, y = _head_inputs(rng, rows, dt, lb, add_bias)
        h, w, bias = _col_case_inputs(rng, rows, cols, dt)
        slices = rng.randint(1, 40, min(16, rows)).astype(np.float64)
        db, sc_plain = _run_head(gpu, dt, mean, y, s, lb, k, fold, add_bias, True, tsq_scalar=float(slices.sum()))
        sc_fused, dpb, _, _ = _run_fused(gpu, dt, mean[None, :], y, s, slices, lb, k, fold, add_bias, True, h, w, bias, bt)
        assert _same_bits(sc_plain, sc_fused), (rows, cols, sc_plain.tolist(), sc_fused.tolist())
        delta = db[:rows].cpu().numpy()
        hT, wT = np.asarray(h, NPT[dt]).reshape(rows, cols), np.asarray(w, NPT[dt])
        want = (delta[:, None] * wT[None, :]) * (one - hT * hT)          # one rounding per operation, in T
        got = dpb[:rows * cols].cpu().numpy().reshape(rows, cols)
        assert want.dtype == got.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (rows, cols)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: bias + tanh, the row dot product and the sum(theta^2) slices
# ---------------------------------------------------------------------------------------------------------------------

RD_ROWS = [1, 5, 15, 16, 17, 256]
RD_COLS = [1, 3, 4, 50, 1024, 1028, 2048, 2052, 4100]
SLICE_NPARTS = [0, 1, 15, 16, 17, 10007]


def _rowdot_inputs(rng, rows, cols, dt):
    """a + bias = +-(0.05 .. 4.5) with one sign per row (no cancellation in the row's dot product; tanh saturates up to
    1 - 2.5e-4), w > 0."""
    sign = rng.choice([-1.0, 1.0], rows)[:, None]
    bias = _rounded(rng.uniform(-0.5, 0.5, cols), dt)
    a = _rounded(sign * rng.uniform(0.05, 4.5, (rows, cols)) - bias[None, :], dt)
    w = _rounded(rng.uniform(0.5, 1.5, cols), dt)
    return a, bias, w


def _tanh_ref(a, bias, dt):
    """tanh(a + bias) in extended precision, rounded to float64."""
    z = a.astype(np.longdouble)
    if bias is not None:
        z = z + bias.astype(np.longdouble)[None, :]
    return np.tanh(z).astype(np.float64)


def _rowdot_case(dev, dt, rng, rows, cols, with_bias, lead, nparts):
    u, key = UNIT[dt], ("tanh_rowdot", str(dt)[6:])
    what = (rows, cols, with_bias, lead, nparts)
    a, bias, w = _rowdot_inputs(rng, rows, cols, dt)
    if not with_bias:
        a = _rounded(a + bias[None, :], dt)
    ws, recs = _workspace(nparts, dev, rng) if nparts is not None else (None, None)
    runs = []
    for _ in range(2):
        ab, av = _put(a, dt, dev, lead)
        _, bv = _put(bias, dt, dev, lead)
        _, wv = _put(w, dt, dev, lead)
        ob, ov = _nan_buf(rows, dt, dev)
        tb = torch.full((17,), NAN, dtype=torch.float64, device=dev) if ws is not None else None
        kernels.tanh_rowdot(av.view(rows, cols), wv, ov, stats_workspace=ws, tsq_parts=tb, bias=bv if with_bias else None)
        runs.append((ab, ob) + ((tb,) if tb is not None else ()))
    assert all(_same_bits(x, y) for x, y in zip(*runs)), what
    ab, ob = runs[0][:2]
    assert _untouched(ab, 0, lead) and _untouched(ab, lead + rows * cols, None) and _untouched(ob, rows, None), what
    h_ref = _tanh_ref(a.reshape(rows, cols), bias if with_bias else None, dt)
    hbar = _tanh_bar(h_ref, dt)
    _check(("bias_tanh(rowdot)", str(dt)[6:], "h"), ab[lead:lead + rows * cols].cpu().numpy(), h_ref, hbar, "h %r" % (what,))
    depth = -(-cols // 64) + 9                     # cols / 64 per lane (4 per quad), 6 shuffles, 3 waves
    terms = h_ref * w[None, :]
    _check(key + ("out",), ob[:rows].cpu().numpy(), terms.sum(1),
           (depth + 4) * u * np.abs(terms).sum(1) + (hbar * np.abs(w)[None, :]).sum(1), "out %r" % (what,))
    if ws is not None:
        tb = runs[0][2]
        n_slices = min(16, rows)
        got = tb.cpu().numpy()
        assert np.array_equal(got[:n_slices], _slices(recs, n_slices)), (what, got[:n_slices], _slices(recs, n_slices))
        assert np.isnan(got[n_slices:]).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows", RD_ROWS)
def test_tanh_rowdot_equals_fp64(gpu, dt, rows):
    """Bias on and off; aligned (quad path: one-quad loop up to 1024 columns, two-quad loop past that) and one element off
    (scalar path); the slices of 0 .. 10 007 records in turn."""
    rng = np.random.RandomState(100 + rows)
    i = 0
    for cols in RD_COLS:
        for with_bias in (True, False):
            for lead in (0, 1):
                _rowdot_case(gpu, dt, rng, rows, cols, with_bias, lead, (SLICE_NPARTS + [None])[i % 7])
                i += 1
    for nparts in SLICE_NPARTS:
        _rowdot_case(gpu, dt, rng, rows, 4, True, 0, nparts)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_bias_tanh_equals_fp64(gpu, dt):
    """Quad path (cols % 4 == 0, aligned) and scalar path (odd widths, or one element off), 4 ulp of T."""
    rng = np.random.RandomState(16)
    key = ("bias_tanh", str(dt)[6:], "h")
    for rows in RD_ROWS:
        for cols in RD_COLS:
            for lead in (0, 1):
                what = (rows, cols, lead)
                a, bias, _ = _rowdot_inputs(rng, rows, cols, dt)
                runs = []
                for _ in range(2):
                    ab, av = _put(a, dt, gpu, lead)
                    bb, bv = _put(bias, dt, gpu, lead)
                    kernels.bias_tanh(av.view(rows, cols), bv)
                    runs.append(ab)
                ab = runs[0]
                assert _same_bits(ab, runs[1]), what
                assert _untouched(ab, 0, lead) and _untouched(ab, lead + rows * cols, None), what
                h_ref = _tanh_ref(a.reshape(rows, cols), bias, dt)
                _check(key, ab[lead:lead + rows * cols].cpu().numpy(), h_ref, _tanh_bar(h_ref, dt), "bias_tanh %r" % (what,))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", [(32, 1024), (256, 2048), (256, 4864)])
def test_dense_tanh_slices_equal_the_exact_record_sums(gpu, M, N):
    """bnn_dense_tanh's side job: 16 slices of the records, equal to the exact integer sums of their contiguous ranges.
    32 x 1024 is exactly 16 output tiles; 256 x 4864 runs a second launch of half tiles, which must not slice again."""
    rng = np.random.RandomState(M + N)
    K = 64
    g = torch.Generator(device=gpu).manual_seed(M + N)
    h = torch.rand(M, K, device=gpu, generator=g)
    W = torch.randn(K, N, device=gpu, generator=g) / 8
    b = torch.randn(N, device=gpu, generator=g) * 0.3
    for nparts in SLICE_NPARTS:
        ws, recs = _workspace(nparts, gpu, rng)
        ws0 = ws.clone()
        tb = torch.full((17,), NAN, dtype=torch.float64, device=gpu)
        out = torch.empty(M, N, device=gpu)
        kernels.bnn_dense_tanh(h, W, b, out, stats_workspace=ws, tsq_parts=tb)
        got = tb.cpu().numpy()
        assert np.array_equal(got[:16], _slices(recs, 16)), (M, N, nparts, got[:16], _slices(recs, 16))
        assert np.isnan(got[16]) and _same_bits(ws, ws0) and bool(torch.isfinite(out).all()), (M, N, nparts)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: a real statistics workspace
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_step_kernels_workspace_has_the_layout_the_synthetic_ones_assume(gpu):
    """A theta_sq_only SGHMC step over the benchmark's 10 002 434 parameters (integers -3 .. 3, theta' = theta) leaves a
    record count and records whose statistic 0 adds up to sum(theta^2) exactly; the head, the rowdot slicer and the dense
    slicer read it as that layout."""
    n = 10_002_434
    dt = torch.float32
    rng = np.random.RandomState(17)
    theta_np = rng.randint(-3, 4, n).astype(np.float32)
    exact = float((theta_np.astype(np.int64) ** 2).sum())
    theta = torch.from_numpy(theta_np).to(gpu)
    st = kernels.StepStats(n, gpu)
    zeros = torch.zeros(n, device=gpu)
    kernels.sghmc_step(theta, zeros.clone(), zeros.clone(), None, None, None, torch.ones(n, device=gpu), None, 0.0, 1.0,
                       0.0, False, xi=zeros, stats=st, opts=dict(theta_sq_only=True))
    assert torch.equal(theta.cpu(), torch.from_numpy(theta_np))
    ws = st.workspace.view(torch.float64)
    nrec = int(st.workspace.view(torch.int64)[0])
    assert 16 <= nrec and 32 * (1 + nrec) <= st.workspace.numel()
    rec = ws[4:4 + 4 * nrec].view(nrec, 4).cpu().numpy()
    # (statistics 1..3 are not asserted: the cost path reads statistic 0 only, and the synthetic workspaces hold NaN there)
    assert float(rec[:, 0].sum()) == exact and (rec[:, 0] == np.round(rec[:, 0])).all()
    # the head
    B, k = 300, _consts(300)
    mean, y = _head_inputs(rng, B, dt, -0.3, True)
    ref = _head_ref(mean, y, 0.7, exact, k, float(np.float32(-0.3)), False, True)
    _, sc = _run_head(gpu, dt, mean, y, float(np.float32(0.7)), float(np.float32(-0.3)), k, False, True, True, ws=ws)
    _check_scalars(("bnn_head(step workspace)", "float32"), sc, ref, dt, True)
    # the rowdot slicer and the fused head that adds its slices
    a, bias, w = _rowdot_inputs(rng, 16, 64, dt)
    _, av = _put(a, dt, gpu)
    _, bv = _put(bias, dt, gpu)
    _, wv = _put(w, dt, gpu)
    _, ov = _nan_buf(16, dt, gpu)
    tb = torch.full((17,), NAN, dtype=torch.float64, device=gpu)
    kernels.tanh_rowdot(av.view(16, 64), wv, ov, stats_workspace=ws, tsq_parts=tb, bias=bv)
    slices = tb.cpu().numpy()
    assert np.array_equal(slices[:16], _slices(rec[:, 0], 16)) and np.isnan(slices[16])
    assert slices[:16].sum() == exact
    # the dense slicer
    tb2 = torch.full((17,), NAN, dtype=torch.float64, device=gpu)
    hd = torch.rand(256, 64, device=gpu)
    kernels.bnn_dense_tanh(hd, torch.randn(64, 2048, device=gpu) / 8, torch.zeros(2048, device=gpu),
                           torch.empty(256, 2048, device=gpu), stats_workspace=ws, tsq_parts=tb2)
    assert np.array_equal(tb2.cpu().numpy()[:16], slices[:16])
