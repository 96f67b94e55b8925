"""K11 on the GPU (``kernels.bnn_predict`` / ``models.posterior_predictive``, include/sgmcmc_hip_predict.h): the posterior
predictive of device traces at every shape class the forward loops branch on, in both dtypes.

1. parity   ``means`` against the float64 forward pass of the oracle on the float64-widened samples
            (``oracle.bnn_forward``; for nets that are not four weight layers deep the same numpy statements layer by layer,
            pinned to ``bnn_forward`` bit for bit where both apply). f64: 1e-12 * max(1, |truth|), the project's bar for these
            loops (GRAD_TOL / COST_TOL of tests/test_bnn_fused_shapes_gpu.py). f32: the kernel's maximum error against 4 x the
            maximum error of ``mlp_forward`` in float32 on the CPU over the same samples and rows + 4 * 2^-23 * max|truth| (a
            different tanhf and a different summation order per layer; an indexing mistake is orders of magnitude larger).
2. layout   bit for bit: all rows in one call == one row per call; all samples == one sample per call; the pointer table
            of padded buffers == the contiguous tensor; aligned rows == the same data shifted by one element.
3. ensemble ``ens_mean`` / ``ens_var`` against numpy float64 on the kernel's own ``means``: sequential against pairwise
            summation of S terms, so 4 * S * 2^-53 * max|means| for the mean, and for the variance that relative bound plus
            the mean's absolute term squared (a shift d of the mean moves the variance by d^2). Equal bits over two calls;
            S = 1 gives a variance of exactly 0.
4. noise    ``noise_var`` within 4 ulp of ``np.exp`` in the element type.
5. bounds   nothing is written past (S, n_rows); NaN padding between n_params and ld and between the chains' slabs never leaks.
6. capture  the call inside a captured graph, replayed once, gives the eager call's bits.
7. API      ``FusedBNNChains.collect`` -> ``predict``; ``BayesianNeuralNetwork.predict(on_device=True)`` against ``predict()``.

Row counts 1, tile - 1, tile + 1 and 2 * tile + 3 for the tile the host picks (``kernels.bnn_predict_row_tile``); sample
counts 1, 2 and 65; m = 3 separate buffers with ld = n_params + 3 and one contiguous (m, n, P) tensor.
"""
import numpy as np
import pytest
import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd.models import BayesianNeuralNetwork, posterior_predictive
from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params, mlp_forward

pytestmark = pytest.mark.gpu

SHAPES = [
    pytest.param([1, 50, 50, 50, 1], id="default_3x50"),                   # 16-byte rows, pair loops
    pytest.param([3, 7, 13, 1], id="odd_widths_odd_offsets"),              # scalar loops; 147 parameters: element alignment
    pytest.param([4, 50, 49, 50, 1], id="paired_and_scalar_mixed"),
    pytest.param([5, 1], id="single_weight_layer"),
    pytest.param([3, 8, 8, 8, 8, 8, 8, 8, 1], id="eight_weight_layers"),
]
DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.float64, id="f64")]
NP = {torch.float32: np.float32, torch.float64: np.float64}
M, N_PER = 3, 22                                # the pointer table: 3 chains x 22 samples; the first 65 are "S = 65"
S_ALL = M * N_PER
F64_TOL = 1e-12


def _n_params(sizes):
    return sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1


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


def _forward64(oracle, params, X):
    """The oracle's forward pass in float64; its statements layer by layer for a net of another depth."""
    L = (len(params) - 1) // 2
    h = X
    for l in range(L - 1):
        h = np.tanh(h @ params[2 * l] + params[2 * l + 1])
    mean = (h @ params[2 * L - 2] + params[2 * L - 1])[:, 0]
    if L == 4:
        want = oracle.bnn_forward(params, X)
        assert np.array_equal(mean, want[:, 0]) and np.array_equal(want[:, 1], np.full(len(X), params[-1][0, 0]))
    return mean


_CASES = {}


def _case(oracle, sizes, dt):
    """Samples, test rows and their references for one (net, dtype), computed once and shared (never modified):
    sample s = init_mlp_params flattened + 0.1 * randn, a distinct log_var each; X uniform in [-1, 1]."""
    key = (tuple(sizes), dt)
    if key not in _CASES:
        npdt, P = NP[dt], _n_params(sizes)
        tile = kernels.bnn_predict_row_tile(sizes, dt)
        rows = 2 * tile + 3
        rng = np.random.RandomState(len(sizes) * 131 + sizes[0])
        base = torch.cat([p.reshape(-1) for p in init_mlp_params(sizes[0], hidden=sizes[1:-1], seed=5)]).numpy()
        theta = base[None, :] + 0.1 * rng.randn(S_ALL, P)
        theta[:, -1] = np.log(1e-3) + 0.07 * np.arange(S_ALL) - 0.011 * rng.rand(S_ALL)
        theta = theta.astype(npdt)
        X = rng.uniform(-1.0, 1.0, size=(rows, sizes[0])).astype(npdt)
        X64 = X.astype(np.float64)
        truth = np.stack([_forward64(oracle, _split(theta[s].astype(np.float64), sizes), X64) for s in range(S_ALL)])
        cpu = None
        if dt == torch.float32:
            with torch.no_grad():
                cpu = np.stack([mlp_forward([torch.from_numpy(p.copy()) for p in _split(theta[s], sizes)],
                                            torch.from_numpy(X))[:, 0].numpy() for s in range(S_ALL)])
        _CASES[key] = dict(P=P, tile=tile, rows=rows, theta=theta, X=X, truth=truth, cpu=cpu)
    return _CASES[key]


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
    """The first m * n samples as one contiguous (m, n, P) device tensor."""
    return torch.from_numpy(case["theta"][:m * n].reshape(m, n, case["P"]).copy()).to(gpu)


def _pointer_table(gpu, case, dt, shift=0):
    """M separate buffers, each with two NaN rows in front of and behind its slab and rows of ld = P + 3 whose padding
    is NaN; ``shift`` moves every slab by that many elements (the alignment of its rows with it)."""
    P, ld = case["P"], case["P"] + 3
    views = []
    for c in range(M):
        buf = torch.full(((N_PER + 4) * ld + 8,), float("nan"), dtype=dt, device=gpu)
        v = torch.as_strided(buf, (N_PER, P), (ld, 1), 2 * ld + shift)
        v.copy_(torch.from_numpy(case["theta"][c * N_PER:(c + 1) * N_PER]))
        views.append(v)
    return views


def _run(chains, sizes, X, S, ens=False, noise=False):
    N, dt, dev = X.shape[0], X.dtype, X.device
    means = torch.empty(S, N, dtype=dt, device=dev)
    nv = torch.empty(S, dtype=dt, device=dev) if noise else None
    em = torch.empty(N, dtype=torch.float64, device=dev) if ens else None
    ev = torch.empty(N, dtype=torch.float64, device=dev) if ens else None
    kernels.bnn_predict(chains, sizes, X, means, noise_var=nv, ens_mean=em, ens_var=ev)
    return means, nv, em, ev


def _parity_bound(case, dt, truth, rows=None):
    """(bound array or scalar, reference error): the f64 bar, or the f32 bound of the module docstring."""
    if dt == torch.float64:
        return F64_TOL * np.maximum(1.0, np.abs(truth)), 0.0
    cpu = case["cpu"][:truth.shape[0], :truth.shape[1]]
    ref_err = float(np.abs(cpu.astype(np.float64) - truth).max())
    return 4.0 * ref_err + 4.0 * 2.0 ** -23 * float(np.abs(truth).max()), ref_err


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sizes", SHAPES)
def test_means_against_the_fp64_forward_pass(gpu, oracle, sizes, dt):
    case = _case(oracle, sizes, dt)
    X = torch.from_numpy(case["X"]).to(gpu)
    tile = case["tile"]
    for (m, n) in ((1, 1), (2, 1), (5, 13)):
        for rows in (1, tile - 1, tile + 1, 2 * tile + 3):
            S = m * n
            means = _run(_contiguous(gpu, case, m, n), sizes, X[:rows].contiguous(), S)[0]
            got = means.cpu().numpy().astype(np.float64)
            truth = case["truth"][:S, :rows]
            bound, ref_err = _parity_bound(case, dt, truth)
            err = np.abs(got - truth)
            if S == 65 and rows == 2 * tile + 3:
                print("\nbnn_predict parity %s %s tile %d: kernel max error %.3e, float32 mlp_forward on the CPU %.3e, "
                      "max|truth| %.3e" % (sizes, NP[dt].__name__, tile, err.max(), ref_err, np.abs(truth).max()))
            assert np.all(np.isfinite(got)), (m, n, rows)
            assert np.all(err <= bound), (m, n, rows, float(err.max()), float(np.max(bound)))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sizes", SHAPES)
def test_layouts_give_the_same_bits(gpu, oracle, sizes, dt):
    case = _case(oracle, sizes, dt)
    X = torch.from_numpy(case["X"]).to(gpu)
    rows = case["rows"]
    whole = _contiguous(gpu, case, M, N_PER)
    means, nv, _, _ = _run(whole, sizes, X, S_ALL, noise=True)
    # all rows in one call == one row per call (and every row count in between, tile edges included)
    by_row = torch.cat([_run(whole, sizes, X[r:r + 1].contiguous(), S_ALL)[0] for r in range(rows)], dim=1)
    _same_bits(by_row, means, "one row per call")
    for k in (case["tile"] - 1, case["tile"] + 1):
        _same_bits(_run(whole, sizes, X[:k].contiguous(), S_ALL)[0], means[:, :k], "%d rows" % k)
    # all samples in one call == one sample per call
    flat = whole.view(S_ALL, case["P"])
    by_sample = torch.cat([_run(flat[s:s + 1], sizes, X, 1)[0] for s in range(S_ALL)], dim=0)
    _same_bits(by_sample, means, "one sample per call")
    # the pointer table of padded buffers == the contiguous tensor, aligned or shifted by one element; the NaN padding
    # behind n_params and around the slabs leaks nowhere
    for shift in (0, 1):
        tm, tnv, _, _ = _run(_pointer_table(gpu, case, dt, shift), sizes, X, S_ALL, noise=True)
        _same_bits(tm, means, "pointer table, shift %d" % shift)
        _same_bits(tnv, nv, "noise_var of the pointer table, shift %d" % shift)
    # a contiguous tensor shifted by one element, and the views a 3-D tensor is cut into
    shifted = torch.empty(S_ALL * case["P"] + 1, dtype=dt, device=gpu)[1:].view(M, N_PER, case["P"])
    shifted.copy_(whole)
    assert shifted.data_ptr() % 16 != 0 and whole.data_ptr() % 16 == 0
    _same_bits(_run(shifted, sizes, X, S_ALL)[0], means, "contiguous tensor shifted by one element")
    _same_bits(_run(list(whole.unbind(0)), sizes, X, S_ALL)[0], means, "the chains of the tensor as a table")
    assert torch.isfinite(means).all() and torch.isfinite(nv).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sizes", SHAPES)
def test_ensemble_moments_and_noise_variance(gpu, oracle, sizes, dt):
    case = _case(oracle, sizes, dt)
    X = torch.from_numpy(case["X"]).to(gpu)
    u = 2.0 ** -53
    for (m, n) in ((1, 1), (1, 2), (5, 13)):
        S = m * n
        chains = _contiguous(gpu, case, m, n)
        means, nv, em, ev = _run(chains, sizes, X, S, ens=True, noise=True)
        x = means.cpu().numpy().astype(np.float64)
        want_mean = x.mean(axis=0)
        want_var = ((x - want_mean) ** 2).mean(axis=0)
        d = 4.0 * S * u * np.abs(x).max()
        assert np.all(np.abs(em.cpu().numpy() - want_mean) <= d), S
        assert np.all(np.abs(ev.cpu().numpy() - want_var) <= 4.0 * S * u * want_var + d * d), S
        if S == 1:
            assert np.all(ev.cpu().numpy() == 0.0)
            _same_bits(em, x[0], "the mean of one sample")
        # equal inputs, equal bits
        means2, nv2, em2, ev2 = _run(chains, sizes, X, S, ens=True, noise=True)
        for a, b, what in ((means2, means, "means"), (nv2, nv, "noise_var"), (em2, em, "ens_mean"), (ev2, ev, "ens_var")):
            _same_bits(a, b, what + " of a second call")
        # exp(log_var) within 4 ulp of numpy's in the element type
        log_var = case["theta"][:S, -1]
        want_nv = np.exp(log_var)
        assert want_nv.dtype == NP[dt]
        assert np.all(np.abs(nv.cpu().numpy().astype(np.float64) - want_nv.astype(np.float64)) <= 4.0 * np.spacing(want_nv)), S


@pytest.mark.parametrize("dt", DTYPES)
def test_nothing_is_written_past_the_outputs(gpu, oracle, dt):
    sizes = [3, 7, 13, 1]
    case = _case(oracle, sizes, dt)
    rows, S, sentinel = case["tile"] + 1, 65, -4321.0
    X = torch.from_numpy(case["X"][:rows].copy()).to(gpu)
    big = {name: torch.full((numel + 64,), sentinel, dtype=d, device=gpu)
           for name, numel, d in (("means", S * rows, dt), ("noise_var", S, dt), ("ens_mean", rows, torch.float64),
                                  ("ens_var", rows, torch.float64))}
    kernels.bnn_predict(_contiguous(gpu, case, 5, 13), sizes, X, big["means"][:S * rows].view(S, rows),
                        noise_var=big["noise_var"][:S], ens_mean=big["ens_mean"][:rows], ens_var=big["ens_var"][:rows])
    for name, numel in (("means", S * rows), ("noise_var", S), ("ens_mean", rows), ("ens_var", rows)):
        assert bool((big[name][numel:] == sentinel).all()), name
        assert bool((big[name][:numel] != sentinel).all()) and bool(torch.isfinite(big[name][:numel]).all()), name
    # optional outputs left out are not touched either: the means alone are the same bits
    alone = _run(_contiguous(gpu, case, 5, 13), sizes, X, S)[0]
    _same_bits(alone, big["means"][:S * rows].view(S, rows), "means without the optional outputs")


@pytest.mark.parametrize("dt", DTYPES)
def test_the_call_is_legal_under_stream_capture(gpu, oracle, dt):
    from pysgmcmc_amd.samplers.base_classes import graph_capture
    sizes = [1, 50, 50, 50, 1]
    case = _case(oracle, sizes, dt)
    X = torch.from_numpy(case["X"]).to(gpu)
    chains = _contiguous(gpu, case, 5, 13)
    eager = _run(chains, sizes, X, 65, ens=True, noise=True)
    outs = [torch.zeros_like(t) for t in eager]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # the first launch of each kernel outside the capture
        kernels.bnn_predict(chains, sizes, X, outs[0], noise_var=outs[1], ens_mean=outs[2], ens_var=outs[3])
    torch.cuda.current_stream().wait_stream(side)
    for t in outs:
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        kernels.bnn_predict(chains, sizes, X, outs[0], noise_var=outs[1], ens_mean=outs[2], ens_var=outs[3])
    torch.cuda.synchronize()
    assert float(outs[0].abs().sum()) == 0.0              # captured, not run
    g.replay()
    torch.cuda.synchronize()
    for got, want, what in zip(outs, eager, ("means", "noise_var", "ens_mean", "ens_var")):
        _same_bits(got, want, what + " of the replayed graph")


def test_chain_group_collects_and_predicts(gpu):
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    rng = np.random.RandomState(3)
    X = rng.uniform(-3.0, 3.0, size=(60, 1))
    y = np.sinc(X[:, 0]) + 0.05 * rng.randn(60)
    chains = FusedBNNChains.for_dataset(X, y, 4, seed=2, device=gpu, burn_in_steps=4)
    trace = chains.collect(6, every=2)
    assert tuple(trace.shape) == (4, 6, 5252)
    Xt = np.linspace(-3.0, 3.0, 37).reshape(-1, 1)
    mean, var = chains.predict(Xt, trace)
    assert mean.dtype == var.dtype == torch.float64 and tuple(mean.shape) == tuple(var.shape) == (37,)
    assert mean.device == trace.device and torch.isfinite(mean).all() and torch.isfinite(var).all() and bool((var >= 0).all())
    Xd = torch.as_tensor(Xt, dtype=torch.float32, device=gpu)
    mean2, var2 = posterior_predictive(trace, Xd, [1, 50, 50, 50, 1])
    _same_bits(mean, mean2, "ens_mean")
    _same_bits(var, var2, "ens_var")
    f, noise = chains.predict(Xd, trace, return_individual_predictions=True)
    assert tuple(f.shape) == (24, 37) and tuple(noise.shape) == (24,) and f.dtype == noise.dtype == torch.float32
    f2, noise2 = posterior_predictive(list(trace.unbind(0)), Xd, [1, 50, 50, 50, 1], return_individual_predictions=True)
    _same_bits(f, f2, "means")
    _same_bits(noise, noise2, "noise_var")
    want_noise = np.exp(trace[:, :, -1].reshape(-1).cpu().numpy().astype(np.float64))
    assert np.all(np.abs(noise.cpu().numpy().astype(np.float64) - want_noise) <= np.spacing(want_noise.astype(np.float32)))
    x = f.double().cpu().numpy()
    assert np.allclose(mean.cpu().numpy(), x.mean(0), rtol=0, atol=1e-13 * np.abs(x).max())


@pytest.mark.parametrize("dt", DTYPES)
def test_bnn_predict_on_device_matches_the_host_path(gpu, oracle, dt):
    rng = np.random.RandomState(4)
    X = rng.uniform(-3.0, 3.0, size=(50, 1))
    y = np.sinc(X[:, 0]) + 0.05 * rng.randn(50)
    bnn = BayesianNeuralNetwork(session=gpu, dtype=dt, n_nets=4, n_iters=60, burn_in_steps=10, sample_steps=2, seed=1)
    bnn.train(X, y)
    assert len(bnn.samples) == 4
    Xt = np.linspace(-3.0, 3.0, 41).reshape(-1, 1)
    host_f, host_noise = bnn.predict(Xt, return_individual_predictions=True)
    dev_f, dev_noise = bnn.predict(Xt, return_individual_predictions=True, on_device=True)
    assert isinstance(dev_f, np.ndarray) and dev_f.shape == host_f.shape == (4, 41) and dev_noise.shape == host_noise.shape
    assert dev_f.dtype == host_f.dtype and dev_noise.dtype == host_noise.dtype
    # the truth, in the normalised units the networks work in: float64 forward passes of the kept (widened) networks
    xn = ((Xt - bnn.x_mean) / bnn.x_std).astype(NP[dt]).astype(np.float64)
    truth = np.stack([_forward64(oracle, [p.detach().cpu().numpy().astype(np.float64) for p in net], xn)
                      for net in bnn.samples])
    scale = float(bnn.y_std)
    norm = lambda f: (f.astype(np.float64) - bnn.y_mean) / scale
    host_err = float(np.abs(norm(host_f) - truth).max())
    dev_err = float(np.abs(norm(dev_f) - truth).max())
    # check 1's bound, the host path standing in for the float32 reference; the un-normalisation on the host rounds both
    # paths once more in the element type
    eps = float(np.finfo(NP[dt]).eps)
    unnorm = 2.0 * eps * float(np.abs(host_f).max()) / scale
    if dt == torch.float64:
        bound = F64_TOL * max(1.0, float(np.abs(truth).max())) + unnorm
    else:
        bound = 4.0 * host_err + 4.0 * 2.0 ** -23 * float(np.abs(truth).max()) + unnorm
    print("\nbnn.predict(on_device=True) %s: device max error %.3e, host path %.3e (normalised units)" % (
        NP[dt].__name__, dev_err, host_err))
    assert dev_err <= bound, (dev_err, bound)
    assert np.all(np.abs(dev_f.astype(np.float64) - host_f.astype(np.float64)) <= scale * (bound + host_err))
    # exp(log_var) * y_std^2: both paths exponentiate the same stored log-variances
    assert np.allclose(dev_noise, host_noise, rtol=8.0 * eps, atol=0.0)
    # the ensemble: a mean of 4 outputs moves by at most the outputs' bound; a variance mean((f - mu)^2) by at most
    # 4 * spread * d + 4 * d^2 when every f moves by d (both f and mu move)
    host_m, host_v = bnn.predict(Xt)
    dev_m, dev_v = bnn.predict(Xt, on_device=True)
    assert dev_m.shape == host_m.shape == (41,) and dev_v.shape == host_v.shape == (41,)
    d = scale * (bound + host_err)
    spread = float(np.abs(host_f.astype(np.float64) - host_f.astype(np.float64).mean(0)).max())
    assert np.all(np.abs(dev_m - host_m) <= d + 4.0 * eps * float(np.abs(host_m).max()))
    assert np.all(np.abs(dev_v - host_v) <= 4.0 * spread * d + 4.0 * d * d + 8.0 * eps * float(np.abs(host_v).max()))
    # the flattened networks are kept until train() runs again
    kept = bnn._kept_matrix[0]
    bnn.predict(Xt, on_device=True)
    assert bnn._kept_matrix[0] is kept and kept.is_cuda and tuple(kept.shape) == (4, 5252)
