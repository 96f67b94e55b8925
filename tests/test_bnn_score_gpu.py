"""K13 on the GPU (``kernels.bnn_score`` / ``models.heldout_score``, include/sgmcmc_hip_score.h): the held-out score of device
traces, layer by layer, in both dtypes. Each numpy reference is computed from the kernel's OWN output of the layer below it,
so every bound is the rounding of one layer; u = 2^-53.

1. means     bit for bit ``kernels.bnn_predict``'s; ``ens_mean`` / ``ens_var`` bit for bit K11's.
2. loglik    against the header's formula in numpy on the kernel's ``means``: 8 u (|a_s| + d^2 b_s) per element (two
             algebraically different numpy forms differ by up to 0.46 of that here; the device exp adds 1-2 ulp of b).
3. rows      ``row_lppd`` against M + log sum exp(l - M) - log S in numpy on the kernel's ``loglik``:
             4 (S + 8) u (1 + |M_r| + |lppd_r|). ``row_pwaic`` against the two-pass variance with ddof = 1:
             4 S u var + delta^2, delta = 4 S u max|l| (a shift delta of the mean moves the variance by delta^2).
             S = 1: ``row_lppd`` is ``loglik[0]`` bit for bit and ``row_pwaic`` exactly 0.
4. sums      ``sample_loglik`` and ``summary`` against numpy sums of the kernel's ``loglik`` and row outputs:
             2 N u sum|terms| (lane-strided partials and a tree against numpy's pairwise order).
5. end to end, f64: ``row_lppd`` against the float64 forward pass of the oracle's statements pushed through
             ``diagnostics.model_diagnostics``. Log-sum-exp is 1-Lipschitz in the sup norm, so the bound per row is
             max_s (2 |d| b_s e + b_s e^2) with e = 1e-12 max(1, |truth|), the project's f64 bar for the forward loops,
             plus check 3's bound. f32 rests on checks 1-4 and K11's parity test.
6. layout    bit for bit: all rows == one row per call; all samples == one sample per call (``loglik``); the pointer table of
             padded buffers == the contiguous tensor, aligned and shifted by one element; a second call.
7. bounds    nothing is written past an output; leaving the optional outputs out changes no bit of the others; NaN padding
             between n_params and ld leaks nowhere.
8. capture   the call inside a captured graph, replayed once, gives the eager call's bits.
9. API       ``FusedBNNChains.collect`` -> ``score``; ``BayesianNeuralNetwork.score(on_device=True)`` against the host path.

y[r] = the float64 truth of sample 0 + 0.05 randn, except y[last] = 20: every sample's log density there is below -800, so
exp(l) underflows to 0 and an unshifted log(mean(exp(l))) would be -inf. Row counts 1, 63, 65, 131, 515 (the edges of a
64-lane row workgroup, and past the 256-lane stride of the sum kernels); sample counts 1, 2, 65 contiguous (65 crosses one
64-sample LDS block) and 66 as a pointer table of 3 x 22 padded buffers.
"""
import numpy as np
import pytest
import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd.diagnostics import model_diagnostics
from pysgmcmc_amd.models import BayesianNeuralNetwork, heldout_score
from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params

pytestmark = pytest.mark.gpu

SHAPES = [pytest.param([1, 50, 50, 50, 1], id="default_3x50"), pytest.param([3, 7, 13, 1], id="odd_widths")]
DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.float64, id="f64")]
NP = {torch.float32: np.float32, torch.float64: np.float64}
M, N_PER = 3, 22                                # the pointer table: 3 chains x 22 samples
S_ALL = M * N_PER
ROWS = (1, 63, 65, 131, 515)
CONTIGUOUS = ((1, 1), (1, 2), (5, 13))          # (m, n): S = 1, 2, 65
U = 2.0 ** -53
LOG_2PI = 1.8378770664093453
F64_TOL = 1e-12
OUTPUTS = ("means", "row_lppd", "row_pwaic", "ens_mean", "ens_var", "loglik", "sample_loglik", "summary")


def _n_params(sizes):
    return sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1


def _forward64(flat, sizes, X):
    """The oracle's forward statements (``oracle.bnn_forward``) layer by layer in float64, for a net of any depth."""
    h, off = X, 0
    for l in range(len(sizes) - 1):
        nin, nout = sizes[l], sizes[l + 1]
        W = flat[off:off + nin * nout].reshape(nin, nout)
        off += nin * nout
        h = h @ W + flat[off:off + nout]
        off += nout
        if l < len(sizes) - 2:
            h = np.tanh(h)
    return h[:, 0]


_CASES = {}


def _case(sizes, dt):
    """Samples, test rows, targets and the float64 truth for one (net, dtype), computed once and shared (never modified)."""
    key = (tuple(sizes), dt)
    if key not in _CASES:
        npdt, P, rows = NP[dt], _n_params(sizes), max(ROWS)
        rng = np.random.RandomState(len(sizes) * 131 + sizes[0])
        base = torch.cat([p.reshape(-1) for p in init_mlp_params(sizes[0], hidden=sizes[1:-1], seed=5)]).numpy()
        theta = base[None, :] + 0.1 * rng.randn(S_ALL, P)
        theta[:, -1] = np.log(1e-3) + 0.07 * np.arange(S_ALL) - 0.011 * rng.rand(S_ALL)
        theta = theta.astype(npdt)
        X = rng.uniform(-1.0, 1.0, size=(rows, sizes[0])).astype(npdt)
        truth = np.stack([_forward64(theta[s].astype(np.float64), sizes, X.astype(np.float64)) for s in range(S_ALL)])
        y = (truth[0] + 0.05 * rng.randn(rows)).astype(npdt)
        _CASES[key] = dict(P=P, theta=theta, X=X, truth=truth, y=y)
    return _CASES[key]


def _targets(case, N):
    y = case["y"][:N].copy()
    y[-1] = 20.0
    return y


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d/%d elements differ, first at %s" % (what, len(bad), g.size, bad[0]))


def _contiguous(gpu, case, m, n):
    return torch.from_numpy(case["theta"][:m * n].reshape(m, n, case["P"]).copy()).to(gpu)


def _pointer_table(gpu, case, dt, shift=0):
    """M separate buffers, each with two NaN rows in front of and behind its slab and rows of ld = P + 3 whose padding is
    NaN; ``shift`` moves every slab by that many elements."""
    P, ld = case["P"], case["P"] + 3
    views = []
    for c in range(M):
        buf = torch.full(((N_PER + 4) * ld + 8,), float("nan"), dtype=dt, device=gpu)
        v = torch.as_strided(buf, (N_PER, P), (ld, 1), 2 * ld + shift)
        v.copy_(torch.from_numpy(case["theta"][c * N_PER:(c + 1) * N_PER]))
        views.append(v)
    return views


def _empty(S, N, dt, dev, optional=True):
    f64 = torch.float64
    out = dict(means=torch.empty(S, N, dtype=dt, device=dev), loglik=None, sample_loglik=None, summary=None)
    for name in ("row_lppd", "row_pwaic", "ens_mean", "ens_var"):
        out[name] = torch.empty(N, dtype=f64, device=dev)
    if optional:
        out.update(loglik=torch.empty(S, N, dtype=f64, device=dev), sample_loglik=torch.empty(S, dtype=f64, device=dev),
                   summary=torch.empty(3, dtype=f64, device=dev))
    return out


def _score(chains, sizes, X, y, S, optional=True, out=None):
    out = _empty(S, X.shape[0], X.dtype, X.device, optional) if out is None else out
    kernels.bnn_score(chains, sizes, X, y, out["means"], out["row_lppd"], out["row_pwaic"], out["ens_mean"], out["ens_var"],
                      loglik=out["loglik"], sample_loglik=out["sample_loglik"], summary=out["summary"])
    return out


def _loglik(means, log_var, y):
    """The header's statements in numpy float64."""
    lv = log_var.astype(np.float64)[:, None]
    a = -0.5 * (LOG_2PI + lv)
    b = 0.5 / (np.exp(lv) + 1e-16)
    d = y.astype(np.float64)[None, :] - means.astype(np.float64)
    return a - (d * d) * b, a, b, d


def _row_bounds(ll):
    """(want_lppd, bound_lppd, want_pwaic, bound_pwaic) of check 3 from an (S, N) float64 ``loglik``."""
    S = ll.shape[0]
    top = ll.max(axis=0)
    lppd = top + np.log(np.exp(ll - top).sum(axis=0)) - np.log(float(S))
    b_lppd = 4.0 * (S + 8) * U * (1.0 + np.abs(top) + np.abs(lppd))
    if S > 1:
        var = ((ll - ll.mean(axis=0)) ** 2).sum(axis=0) / (S - 1)
    else:
        var = np.zeros(ll.shape[1])
    delta = 4.0 * S * U * np.abs(ll).max(axis=0)
    return lppd, b_lppd, var, 4.0 * S * U * var + delta * delta


def _check_numbers(case, sizes, dt, chains, got, S, N, X, y):
    """Checks 1-5 and the finiteness half of 7 on one call's outputs."""
    tag = (sizes, NP[dt].__name__, S, N)
    g = {k: (v.cpu().numpy() if v is not None else None) for k, v in got.items()}
    for name in OUTPUTS:
        assert np.all(np.isfinite(g[name])), (name, tag)
    # 1. K11's bits
    k11 = torch.empty(S, N, dtype=dt, device=X.device)
    em = torch.empty(N, dtype=torch.float64, device=X.device)
    ev = torch.empty(N, dtype=torch.float64, device=X.device)
    kernels.bnn_predict(chains, sizes, X, k11, ens_mean=em, ens_var=ev)
    _same_bits(got["means"], k11, "means %s" % (tag,))
    _same_bits(got["ens_mean"], em, "ens_mean %s" % (tag,))
    _same_bits(got["ens_var"], ev, "ens_var %s" % (tag,))
    # 2. loglik from the kernel's means
    yh = y.cpu().numpy()
    want, a, b, d = _loglik(g["means"], case["theta"][:S, -1], yh)
    bound = 8.0 * U * (np.abs(a) + d * d * b)
    err = np.abs(g["loglik"] - want)
    assert np.all(err <= bound), ("loglik", tag, float((err / bound).max()))
    # the hopeless row: every density underflows, and the lppd is finite all the same
    assert np.all(want[:, -1] < -800.0) and np.all(np.exp(want[:, -1]) == 0.0), tag
    assert np.isfinite(g["row_lppd"][-1]) and g["row_lppd"][-1] < -800.0, tag
    # 3. the rows from the kernel's loglik
    ll = g["loglik"]
    lppd, b_lppd, var, b_var = _row_bounds(ll)
    err = np.abs(g["row_lppd"] - lppd)
    assert np.all(err <= b_lppd), ("row_lppd", tag, float((err / b_lppd).max()))
    if S == 1:
        _same_bits(got["row_lppd"], ll[0], "row_lppd of one sample")
        assert np.all(g["row_pwaic"] == 0.0) and not np.any(np.signbit(g["row_pwaic"]))
    else:
        err = np.abs(g["row_pwaic"] - var)
        assert np.all(err <= b_var), ("row_pwaic", tag, float((err / b_var).max()))
        assert np.all(g["row_pwaic"] > 0.0)
    # 4. the sums from the kernel's loglik and row outputs
    err = np.abs(g["sample_loglik"] - ll.sum(axis=1))
    assert np.all(err <= 2.0 * N * U * np.abs(ll).sum(axis=1)), ("sample_loglik", tag, float(err.max()))
    sq = (g["ens_mean"] - yh.astype(np.float64)) ** 2
    for k, terms in enumerate((g["row_lppd"], g["row_pwaic"], sq)):
        err = abs(g["summary"][k] - terms.sum())
        assert err <= 2.0 * N * U * np.abs(terms).sum(), ("summary[%d]" % k, tag, err)
    # 5. end to end against the float64 truth (f64 only)
    if dt == torch.float64:
        truth = case["truth"][:S, :N]
        ref = model_diagnostics.log_pointwise_predictive_density(
            model_diagnostics.pointwise_log_likelihood(truth, case["theta"][:S, -1], yh))
        e = F64_TOL * np.maximum(1.0, np.abs(truth))
        dd = np.abs(yh[None, :] - truth)
        lipschitz = (2.0 * dd * b * e + b * e * e).max(axis=0)
        err = np.abs(g["row_lppd"] - ref)
        assert np.all(err <= lipschitz + b_lppd), ("end to end", tag, float((err / (lipschitz + b_lppd)).max()))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sizes", SHAPES)
def test_every_layer_against_numpy_on_the_layer_below(gpu, sizes, dt):
    case = _case(sizes, dt)
    Xall = torch.from_numpy(case["X"]).to(gpu)
    table = _pointer_table(gpu, case, dt)
    for N in ROWS:
        X = Xall[:N].contiguous()
        y = torch.from_numpy(_targets(case, N)).to(gpu)
        for (m, n) in CONTIGUOUS:
            chains = _contiguous(gpu, case, m, n)
            _check_numbers(case, sizes, dt, chains, _score(chains, sizes, X, y, m * n), m * n, N, X, y)
        _check_numbers(case, sizes, dt, table, _score(table, sizes, X, y, S_ALL), S_ALL, N, X, y)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sizes", SHAPES)
def test_layouts_give_the_same_bits(gpu, sizes, dt):
    case = _case(sizes, dt)
    N = 131
    X = torch.from_numpy(case["X"][:N].copy()).to(gpu)
    y = torch.from_numpy(_targets(case, N)).to(gpu)
    whole = _contiguous(gpu, case, M, N_PER)
    got = _score(whole, sizes, X, y, S_ALL)
    # all rows in one call == one row per call
    by_row = [_score(whole, sizes, X[r:r + 1].contiguous(), y[r:r + 1].contiguous(), S_ALL) for r in range(N)]
    _same_bits(torch.cat([o["loglik"] for o in by_row], dim=1), got["loglik"], "loglik, one row per call")
    for name in ("row_lppd", "row_pwaic", "ens_mean", "ens_var"):
        _same_bits(torch.cat([o[name] for o in by_row]), got[name], name + ", one row per call")
    # all samples in one call == one sample per call
    flat = whole.view(S_ALL, case["P"])
    by_sample = torch.cat([_score(flat[s:s + 1], sizes, X, y, 1)["loglik"] for s in range(S_ALL)], dim=0)
    _same_bits(by_sample, got["loglik"], "loglik, one sample per call")
    # the pointer table of padded buffers == the contiguous tensor, aligned or shifted by one element; a second call
    others = [("pointer table, shift %d" % shift, _score(_pointer_table(gpu, case, dt, shift), sizes, X, y, S_ALL))
              for shift in (0, 1)]
    others.append(("a second call", _score(whole, sizes, X, y, S_ALL)))
    for what, other in others:
        for name in OUTPUTS:
            _same_bits(other[name], got[name], "%s of %s" % (name, what))
            assert torch.isfinite(other[name]).all(), (name, what)     # the NaN padding leaks nowhere


@pytest.mark.parametrize("dt", DTYPES)
def test_nothing_is_written_past_the_outputs(gpu, dt):
    sizes = [3, 7, 13, 1]
    case = _case(sizes, dt)
    N, S, sentinel = 65, 65, -4321.0
    X = torch.from_numpy(case["X"][:N].copy()).to(gpu)
    y = torch.from_numpy(_targets(case, N)).to(gpu)
    chains = _contiguous(gpu, case, 5, 13)
    shapes = dict(means=(S, N), row_lppd=(N,), row_pwaic=(N,), ens_mean=(N,), ens_var=(N,), loglik=(S, N),
                  sample_loglik=(S,), summary=(3,))
    big, out = {}, {}
    for name in OUTPUTS:
        numel = int(np.prod(shapes[name]))
        big[name] = torch.full((numel + 64,), sentinel, dtype=dt if name == "means" else torch.float64, device=gpu)
        out[name] = big[name][:numel].view(shapes[name])
    _score(chains, sizes, X, y, S, out=out)
    for name in OUTPUTS:
        numel = int(np.prod(shapes[name]))
        assert bool((big[name][numel:] == sentinel).all()), name
        assert bool((big[name][:numel] != sentinel).all()) and bool(torch.isfinite(big[name][:numel]).all()), name
    # the optional outputs left out: the others keep their bits, each optional output alone as well
    alone = _score(chains, sizes, X, y, S, optional=False)
    for name in ("means", "row_lppd", "row_pwaic", "ens_mean", "ens_var"):
        _same_bits(alone[name], out[name], name + " without the optional outputs")
    for name in ("loglik", "sample_loglik", "summary"):
        one = _empty(S, N, dt, gpu, optional=False)
        one[name] = torch.empty(shapes[name], dtype=torch.float64, device=gpu)
        _score(chains, sizes, X, y, S, out=one)
        for other in ("row_lppd", "row_pwaic", name):
            _same_bits(one[other], out[other], "%s with %s alone" % (other, name))


@pytest.mark.parametrize("dt", DTYPES)
def test_the_call_is_legal_under_stream_capture(gpu, dt):
    from pysgmcmc_amd.samplers.base_classes import graph_capture
    sizes = [1, 50, 50, 50, 1]
    case = _case(sizes, dt)
    N = 131
    X = torch.from_numpy(case["X"][:N].copy()).to(gpu)
    y = torch.from_numpy(_targets(case, N)).to(gpu)
    chains = _contiguous(gpu, case, 5, 13)
    eager = _score(chains, sizes, X, y, 65)
    outs = {k: torch.zeros_like(v) for k, v in eager.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # the first launch of each kernel outside the capture
        _score(chains, sizes, X, y, 65, out=outs)
    torch.cuda.current_stream().wait_stream(side)
    for t in outs.values():
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        _score(chains, sizes, X, y, 65, out=outs)
    torch.cuda.synchronize()
    assert float(outs["means"].abs().sum()) == 0.0 and float(outs["row_lppd"].abs().sum()) == 0.0     # captured, not run
    g.replay()
    torch.cuda.synchronize()
    for name in OUTPUTS:
        _same_bits(outs[name], eager[name], name + " of the replayed graph")


def test_chain_group_collects_and_scores(gpu):
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    rng = np.random.RandomState(3)
    X = rng.uniform(-3.0, 3.0, size=(60, 1))
    y = np.sinc(X[:, 0]) + 0.05 * rng.randn(60)
    chains = FusedBNNChains.for_dataset(X, y, 4, seed=2, device=gpu, burn_in_steps=4)
    trace = chains.collect(6, every=2)
    Xt = np.linspace(-3.0, 3.0, 37).reshape(-1, 1)
    yt = np.sinc(Xt[:, 0]) + 0.05 * rng.randn(37)
    got = chains.score(Xt, yt, trace, pointwise=True, per_sample=True)
    Xd = torch.as_tensor(Xt, dtype=torch.float32, device=gpu)
    yd = torch.as_tensor(yt, dtype=torch.float32, device=gpu)
    want = heldout_score(trace, Xd, yd, [1, 50, 50, 50, 1], pointwise=True, per_sample=True)
    for name, a, b in zip(got._fields, got, want):
        assert a.device == trace.device and a.dtype == torch.float64, name
        _same_bits(a, b, name)
    for name in ("lppd", "p_waic", "elpd_waic", "rmse"):
        assert getattr(got, name).dim() == 0 and bool(torch.isfinite(getattr(got, name))), name
    assert tuple(got.loglik.shape) == (24, 37) and tuple(got.sample_loglik.shape) == (24,)
    for name in ("row_lppd", "row_pwaic", "ens_mean", "ens_var"):
        assert tuple(getattr(got, name).shape) == (37,), name
    plain = chains.score(Xd, yd, trace)
    assert plain.loglik is None and plain.sample_loglik is None
    _same_bits(plain.row_lppd, got.row_lppd, "row_lppd without the optional outputs")
    # the scalars are the summary's: elpd_waic == sum(row_lppd) - p_waic, with K13's sums within check 4's bound of numpy's
    rows, pw = got.row_lppd.cpu().numpy(), got.row_pwaic.cpu().numpy()
    lppd_sum = float(got.lppd) * 37
    assert abs(lppd_sum - rows.sum()) <= 2.0 * 37 * U * np.abs(rows).sum() + 4.0 * U * abs(rows.sum())
    assert abs(float(got.p_waic) - pw.sum()) <= 2.0 * 37 * U * pw.sum()
    assert abs(float(got.elpd_waic) - (rows.sum() - pw.sum())) <= 2.0 * 37 * U * (np.abs(rows).sum() + pw.sum()) + 4.0 * U * abs(
        rows.sum())
    sq = (got.ens_mean.cpu().numpy() - yd.cpu().numpy().astype(np.float64)) ** 2
    want_rmse = np.sqrt(sq.sum() / 37)
    assert abs(float(got.rmse) - want_rmse) <= (37 + 4) * U * want_rmse
    # and the ensemble moments are predict's
    mean, var = chains.predict(Xd, trace)
    _same_bits(got.ens_mean, mean, "ens_mean")
    _same_bits(got.ens_var, var, "ens_var")


@pytest.mark.parametrize("dt", DTYPES)
def test_bnn_score_on_device_matches_the_host_path(gpu, dt):
    rng = np.random.RandomState(4)
    X = rng.uniform(-3.0, 3.0, size=(50, 1))
    y = np.sinc(X[:, 0]) + 0.05 * rng.randn(50)
    bnn = BayesianNeuralNetwork(session=gpu, dtype=dt, n_nets=4, n_iters=60, burn_in_steps=10, sample_steps=2, seed=1)
    bnn.train(X, y)
    assert len(bnn.samples) == 4
    Xt = np.linspace(-3.0, 3.0, 41).reshape(-1, 1)
    yt = np.sinc(Xt[:, 0]) + 0.05 * rng.randn(41)
    host, dev = bnn.score(Xt, yt), bnn.score(Xt, yt, on_device=True)
    assert sorted(host) == sorted(dev) == ["elpd_waic", "lppd", "p_waic", "rmse", "row_lppd", "row_pwaic"]
    # the two paths' own networks' outputs, back in the normalised units, and the targets as both paths round them
    scale = float(bnn.y_std)
    host_f, noise = bnn.predict(Xt, return_individual_predictions=True)
    dev_f, _ = bnn.predict(Xt, return_individual_predictions=True, on_device=True)
    norm = lambda f: (f.astype(np.float64) - bnn.y_mean) / scale
    yn = ((yt - bnn.y_mean) / scale).astype(NP[dt]).astype(np.float64)
    log_var = np.array([float(net[-1].reshape(-1)[0]) for net in bnn.samples])
    ll_host = model_diagnostics.pointwise_log_likelihood(norm(host_f), log_var, yn)
    ll_dev = model_diagnostics.pointwise_log_likelihood(norm(dev_f), log_var, yn)
    d_ll = np.abs(ll_dev - ll_host).max(axis=0)
    # log-sum-exp is 1-Lipschitz in the sup norm: the rows move by no more than the log densities do
    for got in (host, dev):
        assert got["row_lppd"].shape == got["row_pwaic"].shape == (41,)
        assert np.all(np.isfinite(got["row_lppd"])) and np.all(got["row_pwaic"] >= 0.0)
    err = np.abs(dev["row_lppd"] - host["row_lppd"])
    print("\nbnn.score(on_device=True) %s: max |row_lppd difference| %.3e, max |l difference| %.3e" % (
        NP[dt].__name__, err.max(), d_ll.max()))
    assert np.all(err <= d_ll + 1e-9 * (1.0 + np.abs(host["row_lppd"])))
    assert abs(dev["lppd"] - host["lppd"]) <= d_ll.max() + 1e-9 * (1.0 + abs(host["lppd"]))
    # rmse: the ensemble mean moves by at most the outputs' largest move, and so does the root mean square of the errors
    d_f = float(np.abs(dev_f.astype(np.float64) - host_f.astype(np.float64)).max())
    assert abs(dev["rmse"] - host["rmse"]) <= d_f + 1e-9 * (1.0 + host["rmse"])
    # the statement itself, in the caller's units
    want = model_diagnostics.log_pointwise_predictive_density(ll_host) - np.log(scale)
    assert np.all(np.abs(host["row_lppd"] - want) <= 1e-9 * (1.0 + np.abs(want)))
    for got in (host, dev):
        assert np.isclose(got["elpd_waic"], got["row_lppd"].sum() - got["p_waic"], rtol=1e-12, atol=1e-12)
        assert np.isclose(got["lppd"], got["row_lppd"].mean(), rtol=1e-12, atol=1e-12)
