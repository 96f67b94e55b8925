"""The small-net core (csrc/sgmcmc_bnn_small_net.hpp) on the GPU where ``predict_grad_cases.NETS`` never takes it: K11
(``kernels.bnn_predict``), K13 (``kernels.bnn_score``) and K14 (``kernels.bnn_predict_grad``) at every row tile 1 .. 32, at LDS
footprints up to the full 160 KiB, at layers wider than the workgroup, and at every grid: one tile per workgroup, several
(K11's own walk loop), and grid.y == 1 (S >= 4096). The nets, the restated plans and the references are tests/small_net_cases.py;
that the nets reach all of this is asserted without a GPU in tests/test_bnn_small_net_cases.py.

a. parity    ``means`` (K11) against the float64 forward statements, ``grads`` (K14) against the float64 backward sweep, K14's
             ``means`` K11's bits. f64: 1e-12 * max(1, |truth|), the project's bar. f32: 4 x the maximum error of the kernel's own
             statements in the kernel's order (``small_net_cases.kernel_order``: k-ordered fma chains, float32 emulated through
             float64) over the same samples and rows + 4 * 2^-23 * max|truth|; the factor 4 is the project's allowance for a
             different tanhf. torch's float32 error on the CPU is printed beside it and bounds nothing: its blocked sums are
             more accurate than ANY sequential chain at a wide layer. Outputs start as NaN and end finite.
b. bits      all rows in one call == one row per call; row r of sample s has the same bits from K11, K13 and K14, which pick
             different tiles for one net; the pointer table of NaN-padded buffers (ld = P + 3, both alignments of a row) ==
             the contiguous tensor at the nets that need all 160 KiB.
c. bounds    nothing is written past an output at the largest footprints.
d. walk      K11 and K13 at S = 65: grid.y = 64, 2 * 64 * tile + tile + 3 rows; and K11, K14 at tile 1.
e. one group grid.y == 1 at S = 4100: one workgroup walks every tile; S = 4095 (grid.y = 2) gives the same bits.
f. blocks    K13's 64-sample LDS blocks and 16-deep load groups at S = 23, 128 and 4100.
g. capture   the opt-in to more than 64 KiB of dynamic LDS inside a captured graph, at 148 KB and at the full 160 KiB.

Rows are 1, tile - 1, tile + 1 and 2 * tile + 3 for the tile the host picks; S = 5 samples as (1, 1) and (5, 1) unless stated.

What no test of the VALUES can see, here or elsewhere (tried by hand, profiles/bnn_small_net_tiles.txt): a region or a pair access
that is merely misaligned (the LDS replays it: cycles, not bits), a tile walk that visits tiles more than once (equal bits
written again), and a missing LDS opt-in where the runtime launches without it. Those are for the measuring tools.
"""
import numpy as np
import pytest
import torch

import predict_grad_cases as C
import small_net_cases as N
from pysgmcmc_amd import _lib, kernels

pytestmark = pytest.mark.gpu

SHAPES = [pytest.param(sizes, id=name) for sizes, name in zip(N.NETS, N.NET_IDS)]
DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.float64, id="f64")]
NP = {torch.float32: np.float32, torch.float64: np.float64}
ESIZE = {torch.float32: 4, torch.float64: 8}
F64_TOL = 1e-12
U = 2.0 ** -53
LOG_2PI = 1.8378770664093453
S5 = 5
M, N_PER = 3, 2                                   # the pointer table: 3 chains x 2 samples, samples 0 .. 5 of a case
S_CASE = M * N_PER
LAYOUTS = ((1, 1), (5, 1))
WALK_NET = [3, 7, 13, 1]
NAN = float("nan")


# ---- cases: samples, rows and references, computed once and shared (never modified) ----------------------------------------

_CASES = {}


def _tiles(sizes, dt):
    """(K11's tile, K14's tile) by the restated plans, pinned to the library's; None where the plan refuses."""
    tiles = []
    for kernel, binding in ((N.K11, kernels.bnn_predict_row_tile), (N.K14, kernels.bnn_predict_grad_row_tile)):
        plan = N.plan(sizes, kernel, ESIZE[dt])
        if plan is None:
            with pytest.raises(_lib.SgmcmcLibraryError, match="160 KiB"):
                binding(sizes, dt)
            tiles.append(None)
        else:
            assert binding(sizes, dt) == plan["tile"], (sizes, kernel, dt)
            tiles.append(plan["tile"])
    return tiles


def _case(sizes, dt, rows=None, S=S_CASE, key=None, references=None):
    """``references``: the samples that get a truth (and, in f32, the kernel-order and torch references); all by default."""
    key = (tuple(sizes), dt, key)
    if key not in _CASES:
        t11, t14 = _tiles(sizes, dt)
        if rows is None:
            rows = 2 * max(t11 or 1, t14 or 1) + 3
        theta, X = N.make_data(sizes, NP[dt], rows, S)
        ref = np.arange(S) if references is None else np.asarray(references)
        case = dict(P=C.n_params(sizes), t11=t11, t14=t14, rows=rows, theta=theta, X=X, ref=ref, ko=None, cpu=None)
        if t11 is not None:
            case["truth"] = N.truth64(theta[ref], X, sizes)
            if dt == torch.float32:
                case["ko"] = N.kernel_order_all(theta[ref], X, sizes)
                case["cpu"] = N.torch_cpu(theta[ref], X, sizes)
        _CASES[key] = case
    return _CASES[key]


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d/%d elements differ, first at %s" % (what, len(bad), g.size, bad[0]))


def _contiguous(gpu, case, m, n):
    """The first m * n samples as one contiguous (m, n, P) device tensor."""
    return torch.from_numpy(case["theta"][:m * n].reshape(m, n, case["P"]).copy()).to(gpu)


def _pointer_table(gpu, case, dt, shift):
    """M separate buffers, each with two NaN rows in front of and behind its slab and rows of ld = P + 3 whose padding is
    NaN; ``shift`` moves every slab by that many elements (the alignment of its rows with it)."""
    P, ld = case["P"], case["P"] + 3
    views = []
    for c in range(M):
        buf = torch.full(((N_PER + 4) * ld + 8,), NAN, dtype=dt, device=gpu)
        v = torch.as_strided(buf, (N_PER, P), (ld, 1), 2 * ld + shift)
        v.copy_(torch.from_numpy(case["theta"][c * N_PER:(c + 1) * N_PER]))
        views.append(v)
    return views


def _k11(chains, sizes, X, S, ens=False):
    """(means, ens_mean, ens_var); every output starts as NaN, so an element that is not written shows."""
    rows, dt, dev = X.shape[0], X.dtype, X.device
    means = torch.full((S, rows), NAN, dtype=dt, device=dev)
    em, ev = ((torch.full((rows,), NAN, dtype=torch.float64, device=dev) for _ in range(2)) if ens else (None, None))
    kernels.bnn_predict(chains, sizes, X, means, ens_mean=em, ens_var=ev)
    return means, em, ev


def _k14(chains, sizes, X, S, ens=False):
    """(means, grads, ens_mean, ens_var, dmean, dvar), NaN before the call."""
    rows, dt, dev, D0 = X.shape[0], X.dtype, X.device, sizes[0]
    means = torch.full((S, rows), NAN, dtype=dt, device=dev)
    grads = torch.full((S, rows, D0), NAN, dtype=dt, device=dev)
    ens4 = [None] * 4
    if ens:
        ens4 = [torch.full(shape, NAN, dtype=torch.float64, device=dev) for shape in ((rows,), (rows,), (rows, D0), (rows, D0))]
    kernels.bnn_predict_grad(chains, sizes, X, means, grads, *ens4)
    return (means, grads) + tuple(ens4)


K13_OUTPUTS = ("means", "row_lppd", "row_pwaic", "ens_mean", "ens_var", "loglik", "sample_loglik", "summary")


def _k13(chains, sizes, X, y, S):
    rows, dt, dev, f64 = X.shape[0], X.dtype, X.device, torch.float64
    out = dict(means=torch.full((S, rows), NAN, dtype=dt, device=dev), loglik=torch.full((S, rows), NAN, dtype=f64, device=dev),
               sample_loglik=torch.full((S,), NAN, dtype=f64, device=dev), summary=torch.full((3,), NAN, dtype=f64, device=dev))
    for name in ("row_lppd", "row_pwaic", "ens_mean", "ens_var"):
        out[name] = torch.full((rows,), NAN, dtype=f64, device=dev)
    kernels.bnn_score(chains, sizes, X, y, out["means"], out["row_lppd"], out["row_pwaic"], out["ens_mean"], out["ens_var"],
                      loglik=out["loglik"], sample_loglik=out["sample_loglik"], summary=out["summary"])
    return out


def _targets(case, rows, gpu):
    """y[r] = the float64 truth of the first referenced sample + 0.05 randn, in the case's dtype."""
    rng = np.random.RandomState(7)
    y = (case["truth"][0][0][:rows] + 0.05 * rng.randn(rows)).astype(case["X"].dtype)
    return torch.from_numpy(y).to(gpu)


def _parity(dt, got, truth, ko):
    """(error, bound, the restatement's maximum error): the f64 bar, or the f32 bound of the module docstring over the very
    samples and rows of ``truth``."""
    err = np.abs(got.astype(np.float64) - truth)
    if dt == torch.float64:
        return err, F64_TOL * np.maximum(1.0, np.abs(truth)), 0.0
    ref_err = float(np.abs(ko.astype(np.float64) - truth).max())
    return err, 4.0 * ref_err + 4.0 * 2.0 ** -23 * float(np.abs(truth).max()), ref_err


def _check(case, dt, which, got, samples, rows, what):
    """Finite, and within the bound of the truth of ``samples`` (indices into the case's referenced samples) and ``rows``."""
    k = {"means": 0, "grads": 1}[which]
    got = got.detach().cpu().numpy()
    assert np.all(np.isfinite(got)), (which, what)
    truth = case["truth"][k][samples][:, :rows]
    ko = None if case["ko"] is None else case["ko"][k][samples][:, :rows]
    assert got.shape == truth.shape, (which, what, got.shape, truth.shape)
    err, bound, ref_err = _parity(dt, got, truth, ko)
    assert np.all(err <= bound), (which, what, float(err.max()), float(np.max(bound)))
    cpu_err = 0.0 if case["cpu"] is None else float(np.abs(case["cpu"][k][samples][:, :rows].astype(np.float64) - truth).max())
    return float(err.max()), ref_err, cpu_err, float(np.abs(truth).max())


def _refused(gpu, sizes, dt):
    """The plan refuses: the binding says so, nothing is launched, no output is touched."""
    theta, X = N.make_data(sizes, NP[dt], 2, 1)
    chains, x = torch.from_numpy(theta).to(gpu), torch.from_numpy(X).to(gpu)
    y = torch.zeros(2, dtype=dt, device=gpu)
    for call in (lambda: _k11(chains, sizes, x, 1), lambda: _k14(chains, sizes, x, 1), lambda: _k13(chains, sizes, x, y, 1)):
        with pytest.raises(_lib.SgmcmcLibraryError, match="160 KiB"):
            call()
    means = torch.full((1, 2), NAN, dtype=dt, device=gpu)
    grads = torch.full((1, 2, sizes[0]), NAN, dtype=dt, device=gpu)
    with pytest.raises(_lib.SgmcmcLibraryError, match="bnn_predict: .*160 KiB"):
        kernels.bnn_predict(chains, sizes, x, means)
    with pytest.raises(_lib.SgmcmcLibraryError, match="bnn_predict_grad: .*160 KiB"):
        kernels.bnn_predict_grad(chains, sizes, x, means, grads)
    torch.cuda.synchronize()
    assert bool(torch.isnan(means).all()) and bool(torch.isnan(grads).all())


# ---- a. parity at every net of the table ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sizes", SHAPES)
def test_parity_at_every_tile_and_footprint(gpu, sizes, dt):
    case = _case(sizes, dt)
    if case["t11"] is None or case["t14"] is None:
        assert case["t11"] is None and case["t14"] is None and N.table_cell(sizes, N.K11, ESIZE[dt]) is None
        return _refused(gpu, sizes, dt)
    X = torch.from_numpy(case["X"]).to(gpu)
    for (m, n) in LAYOUTS:
        S = m * n
        chains = _contiguous(gpu, case, m, n)
        samples = np.arange(S)
        for kernel, tile in ((N.K11, case["t11"]), (N.K14, case["t14"])):
            for rows in sorted({1, tile - 1, tile + 1, 2 * tile + 3} - {0}):
                x = X[:rows].contiguous()
                what = (kernel, m, n, rows)
                k11 = _k11(chains, sizes, x, S)[0]
                stats = [_check(case, dt, "means", k11, samples, rows, what)]
                if kernel == N.K14:
                    means, grads = _k14(chains, sizes, x, S)[:2]
                    _same_bits(means, k11, "K14's means against K11's %s" % (what,))
                    stats.append(_check(case, dt, "grads", grads, samples, rows, what))
                    if len(sizes) == 2:
                        _same_bits(grads, np.repeat(case["theta"][:S, None, :sizes[0]], rows, axis=1), "a copy of W_1")
                if S == S5 and rows == 2 * tile + 3:
                    cell = N.table_cell(sizes, kernel, ESIZE[dt])
                    assert cell[0] == tile
                    for which, (err, ref_err, cpu_err, top) in zip(("means", "grads"), stats):
                        if (kernel == N.K11) == (which == "means"):
                            print("\nsmall-net parity %s %s %s %s tile %d lds %d B: kernel max error %.3e, kernel-order restatement "
                                  "%.3e, torch on the CPU %.3e, max|truth| %.3e" % (
                                      kernel, which, sizes, NP[dt].__name__, tile, cell[1], err, ref_err, cpu_err, top))


# ---- b. equal bits across tiles ------------------------------------------------------------------------------------------------

# the (net, dtype) pairs the plans accept; the refusals are the parity test's
ACCEPTED = [pytest.param(sizes, dt, id="%s-f%d" % (name, 8 * ESIZE[dt]))
            for sizes, name in zip(N.NETS, N.NET_IDS) for dt in (torch.float32, torch.float64)
            if N.k11_plan(sizes, ESIZE[dt]) is not None and N.k14_plan(sizes, ESIZE[dt]) is not None]
assert len(ACCEPTED) == 2 * len(N.NETS) - 4


@pytest.mark.parametrize("sizes, dt", ACCEPTED)
def test_the_three_entries_give_one_row_the_same_bits_whatever_their_tiles(gpu, sizes, dt):
    case = _case(sizes, dt)
    X = torch.from_numpy(case["X"]).to(gpu)
    chains = _contiguous(gpu, case, S5, 1)
    rows = case["rows"]                                   # 2 * tile + 3 of the larger of the two tiles
    k11 = _k11(chains, sizes, X, S5)[0]
    k14_means, k14_grads = _k14(chains, sizes, X, S5)[:2]
    k13 = _k13(chains, sizes, X, _targets(case, rows, gpu), S5)
    assert bool(torch.isfinite(k11).all()) and bool(torch.isfinite(k14_grads).all())
    _same_bits(k14_means, k11, "K14's means against K11's (tiles %d and %d)" % (case["t14"], case["t11"]))
    _same_bits(k13["means"], k11, "K13's means against K11's")
    for name in K13_OUTPUTS:
        assert bool(torch.isfinite(k13[name]).all()), name
    # all rows in one call == one row per call: every row as row 0 of a tile of its own
    by_row = [_k11(chains, sizes, X[r:r + 1].contiguous(), S5)[0] for r in range(rows)]
    _same_bits(torch.cat(by_row, dim=1), k11, "K11, one row per call")
    by_row = [_k14(chains, sizes, X[r:r + 1].contiguous(), S5)[:2] for r in range(rows)]
    _same_bits(torch.cat([g[0] for g in by_row], dim=1), k11, "K14's means, one row per call")
    _same_bits(torch.cat([g[1] for g in by_row], dim=1), k14_grads, "K14's grads, one row per call")
    # each kernel's own 2 * tile + 3 rows, where that is fewer
    for tile, run in ((case["t11"], lambda x: _k11(chains, sizes, x, S5)[0]), (case["t14"], lambda x: _k14(chains, sizes, x, S5)[0])):
        k = 2 * tile + 3
        _same_bits(run(X[:k].contiguous()), k11[:, :k], "%d rows" % k)


TABLE_NETS = [pytest.param(sizes, id="x".join(map(str, sizes))) for sizes in list(N.FULL_LDS_NETS) + [[2, 1279, 1]]]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sizes", TABLE_NETS)
def test_the_pointer_table_of_padded_rows_at_the_largest_parameter_copies(gpu, sizes, dt):
    case = _case(sizes, dt)
    X = torch.from_numpy(case["X"]).to(gpu)
    whole = _contiguous(gpu, case, 1, S_CASE)
    k11 = _k11(whole, sizes, X, S_CASE)[0]
    k14 = _k14(whole, sizes, X, S_CASE)[:2]
    y = _targets(case, case["rows"], gpu)
    k13 = _k13(whole, sizes, X, y, S_CASE)
    assert bool(torch.isfinite(k11).all())
    # a one-element shift, none, and the shift that puts the first row of every slab on 16 bytes (ld = P + 3 leaves at most
    # one row of a slab there): both branches of the row copy, with and without a tail of n_params % (16 / esize) elements
    PER = 16 // ESIZE[dt]
    aligned = set()
    for shift in sorted({0, 1, -2 * (case["P"] + 3) % PER}):
        table = _pointer_table(gpu, case, dt, shift)
        for v in table:
            aligned |= {(v.data_ptr() + i * v.stride(0) * ESIZE[dt]) % 16 == 0 for i in range(N_PER)}
        _same_bits(_k11(table, sizes, X, S_CASE)[0], k11, "K11, pointer table, shift %d" % shift)
        got = _k14(table, sizes, X, S_CASE)[:2]
        _same_bits(got[0], k11, "K14's means, pointer table, shift %d" % shift)
        _same_bits(got[1], k14[1], "K14's grads, pointer table, shift %d" % shift)
        assert bool(torch.isfinite(got[1]).all())         # the NaN padding leaks nowhere
        got = _k13(table, sizes, X, y, S_CASE)
        for name in K13_OUTPUTS:
            _same_bits(got[name], k13[name], "K13's %s, pointer table, shift %d" % (name, shift))
    assert aligned == {True, False}                       # both branches of the row copy ran
    print("\nsmall-net pointer table %s %s: parameter copy %d B, n_params %% %d = %d" % (
        sizes, NP[dt].__name__, case["P"] * ESIZE[dt], PER, case["P"] % PER))


# ---- c. nothing is written past the outputs ------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes, dt", [pytest.param([100, 194, 1], torch.float64, id="100x194x1-f64"),
                                       pytest.param([100, 389, 1], torch.float32, id="100x389x1-f32")])
def test_nothing_is_written_past_the_outputs_at_the_largest_footprints(gpu, sizes, dt):
    case = _case(sizes, dt)
    sentinel, S, D0 = -4321.0, S5, sizes[0]
    chains = _contiguous(gpu, case, S5, 1)
    for tile, kernel in ((case["t11"], N.K11), (case["t14"], N.K14)):
        rows = tile + 1
        X = torch.from_numpy(case["X"][:rows].copy()).to(gpu)
        numels = dict(means=S * rows, ens_mean=rows, ens_var=rows)
        if kernel == N.K14:
            numels.update(grads=S * rows * D0, dmean=rows * D0, dvar=rows * D0)
        big = {name: torch.full((64 + numel + 64,), sentinel, dtype=dt if name in ("means", "grads") else torch.float64, device=gpu)
               for name, numel in numels.items()}
        inner = {name: big[name][64:64 + numel] for name, numel in numels.items()}
        if kernel == N.K11:
            kernels.bnn_predict(chains, sizes, X, inner["means"].view(S, rows), ens_mean=inner["ens_mean"], ens_var=inner["ens_var"])
            exact = dict(zip(("means", "ens_mean", "ens_var"), _k11(chains, sizes, X, S, ens=True)))
        else:
            kernels.bnn_predict_grad(chains, sizes, X, inner["means"].view(S, rows), inner["grads"].view(S, rows, D0),
                                     inner["ens_mean"], inner["ens_var"], inner["dmean"].view(rows, D0), inner["dvar"].view(rows, D0))
            exact = dict(zip(("means", "grads", "ens_mean", "ens_var", "dmean", "dvar"), _k14(chains, sizes, X, S, ens=True)))
        for name, numel in numels.items():
            assert bool((big[name][:64] == sentinel).all()) and bool((big[name][64 + numel:] == sentinel).all()), (kernel, name)
            assert bool(torch.isfinite(inner[name]).all()), (kernel, name)
            _same_bits(exact[name].reshape(-1), inner[name], "%s %s into exact-size outputs" % (kernel, name))
        assert bool((inner["means"] != sentinel).all())
        _check(case, dt, "means", inner["means"].view(S, rows), np.arange(S), rows, kernel)
        if kernel == N.K14:
            _check(case, dt, "grads", inner["grads"].view(S, rows, D0), np.arange(S), rows, kernel)


# ---- d. K11 and K13 walk tiles -------------------------------------------------------------------------------------------------

def _loglik(means, log_var, y):
    """The score header's statements in numpy float64."""
    lv = log_var.astype(np.float64)[:, None]
    a = -0.5 * (LOG_2PI + lv)
    b = 0.5 / (np.exp(lv) + 1e-16)
    d = y.astype(np.float64)[None, :] - means.astype(np.float64)
    return a - (d * d) * b, a, b, d


def _row_bounds(ll):
    """(want_lppd, bound_lppd, want_pwaic, bound_pwaic) from an (S, N) float64 ``loglik``: check 3 of tests/test_bnn_score_gpu.py."""
    S = ll.shape[0]
    top = ll.max(axis=0)
    lppd = top + np.log(np.exp(ll - top).sum(axis=0)) - np.log(float(S))
    b_lppd = 4.0 * (S + 8) * U * (1.0 + np.abs(top) + np.abs(lppd))
    var = ((ll - ll.mean(axis=0)) ** 2).sum(axis=0) / (S - 1) if S > 1 else np.zeros(ll.shape[1])
    delta = 4.0 * S * U * np.abs(ll).max(axis=0)
    return lppd, b_lppd, var, 4.0 * S * U * var + delta * delta


def _check_score(case, got, S, y, what):
    """Checks 2 to 4 of tests/test_bnn_score_gpu.py, each layer against numpy on the kernel's own layer below."""
    g = {k: v.cpu().numpy() for k, v in got.items()}
    rows = g["means"].shape[1]
    for name in K13_OUTPUTS:
        assert np.all(np.isfinite(g[name])), (name, what)
    yh = y.cpu().numpy()
    want, a, b, d = _loglik(g["means"], case["theta"][:S, -1], yh)
    bound = 8.0 * U * (np.abs(a) + d * d * b)
    err = np.abs(g["loglik"] - want)
    assert np.all(err <= bound), ("loglik", what, float((err / bound).max()))
    ll = g["loglik"]
    lppd, b_lppd, var, b_var = _row_bounds(ll)
    err = np.abs(g["row_lppd"] - lppd)
    assert np.all(err <= b_lppd), ("row_lppd", what, float((err / b_lppd).max()))
    err = np.abs(g["row_pwaic"] - var)
    assert np.all(err <= b_var), ("row_pwaic", what, float((err / b_var).max()))
    err = np.abs(g["sample_loglik"] - ll.sum(axis=1))
    assert np.all(err <= 2.0 * rows * U * np.abs(ll).sum(axis=1)), ("sample_loglik", what, float(err.max()))
    sq = (g["ens_mean"] - yh.astype(np.float64)) ** 2
    for k, terms in enumerate((g["row_lppd"], g["row_pwaic"], sq)):
        err = abs(g["summary"][k] - terms.sum())
        assert err <= 2.0 * rows * U * np.abs(terms).sum(), ("summary[%d]" % k, what, err)


def _check_moments(means, em, ev, what):
    """``ens_mean`` / ``ens_var`` against numpy float64 on the kernel's own ``means``: check 3 of tests/test_bnn_predict_gpu.py."""
    x = means.cpu().numpy().astype(np.float64)
    S = x.shape[0]
    want_mean = x.mean(axis=0)
    want_var = ((x - want_mean) ** 2).mean(axis=0)
    d = 4.0 * S * U * np.abs(x).max()
    assert np.all(np.abs(em.cpu().numpy() - want_mean) <= d), what
    assert np.all(np.abs(ev.cpu().numpy() - want_var) <= 4.0 * S * U * want_var + d * d), what


@pytest.mark.parametrize("dt", DTYPES)
def test_k11_and_k13_walk_several_tiles(gpu, dt):
    sizes, S = WALK_NET, 65
    tile = kernels.bnn_predict_row_tile(sizes, dt)
    gy = N.grid_y(S, 10 ** 6)
    assert gy == 64
    rows = 2 * gy * tile + tile + 3                       # two full rounds of every workgroup and a ragged third
    assert N.grid_y(S, -(-rows // tile)) == gy and -(-rows // tile) == 2 * gy + 2
    case = _case(sizes, dt, rows=rows, S=S, key="walk")
    X = torch.from_numpy(case["X"]).to(gpu)
    chains = _contiguous(gpu, case, 5, 13)
    means, em, ev = _k11(chains, sizes, X, S, ens=True)
    err, ref_err, cpu_err, top = _check(case, dt, "means", means, np.arange(S), rows, "walk")
    print("\nsmall-net K11 tile walk %s %s tile %d, %d rows: kernel max error %.3e, kernel-order restatement %.3e, torch on the "
          "CPU %.3e, max|truth| %.3e" % (sizes, NP[dt].__name__, tile, rows, err, ref_err, cpu_err, top))
    # the same rows in calls of at most grid.y * tile rows: no workgroup walks a second tile there
    step = gy * tile
    parts = [_k11(chains, sizes, X[lo:lo + step].contiguous(), S)[0] for lo in range(0, rows, step)]
    assert len(parts) == 3
    _same_bits(torch.cat(parts, dim=1), means, "K11's means in calls of one tile per workgroup")
    # K13 inherits the loop
    y = _targets(case, rows, gpu)
    k13 = _k13(chains, sizes, X, y, S)
    _same_bits(k13["means"], means, "K13's means against K11's")
    _same_bits(k13["ens_mean"], em, "K13's ens_mean against K11's")
    _same_bits(k13["ens_var"], ev, "K13's ens_var against K11's")
    _check_score(case, k13, S, y, "walk")


@pytest.mark.parametrize("dt", DTYPES)
def test_k11_and_k14_walk_tiles_of_one_row(gpu, dt):
    sizes, S = [2, 1279, 1], 65
    assert kernels.bnn_predict_row_tile(sizes, dt) == kernels.bnn_predict_grad_row_tile(sizes, dt) == 1
    gy = N.grid_y(S, 10 ** 6)
    rows = 2 * gy + 1 + 3
    assert rows == 132 and N.grid_y(S, rows) == gy == 64
    case = _case(sizes, dt, rows=rows, S=S, key="walk")
    X = torch.from_numpy(case["X"]).to(gpu)
    chains = _contiguous(gpu, case, 5, 13)
    k11 = _k11(chains, sizes, X, S)[0]
    means, grads = _k14(chains, sizes, X, S)[:2]
    stats = _check(case, dt, "means", k11, np.arange(S), rows, "walk"), _check(case, dt, "grads", grads, np.arange(S), rows, "walk")
    for which, (err, ref_err, cpu_err, top) in zip(("means", "grads"), stats):
        print("\nsmall-net tile walk %s %s %s tile 1, %d rows: kernel max error %.3e, kernel-order restatement %.3e, torch on the "
              "CPU %.3e, max|truth| %.3e" % (which, sizes, NP[dt].__name__, rows, err, ref_err, cpu_err, top))
    _same_bits(means, k11, "K14's means against K11's")
    parts11 = [_k11(chains, sizes, X[lo:lo + gy].contiguous(), S)[0] for lo in range(0, rows, gy)]
    parts14 = [_k14(chains, sizes, X[lo:lo + gy].contiguous(), S)[:2] for lo in range(0, rows, gy)]
    assert len(parts11) == 3
    _same_bits(torch.cat(parts11, dim=1), k11, "K11's means in calls of one tile per workgroup")
    _same_bits(torch.cat([p[0] for p in parts14], dim=1), k11, "K14's means in calls of one tile per workgroup")
    _same_bits(torch.cat([p[1] for p in parts14], dim=1), grads, "K14's grads in calls of one tile per workgroup")


# ---- e. grid.y == 1 and f. K13's sample blocks ----------------------------------------------------------------------------------

S_BIG = 4100
PROBES = (0, 1, 2047, 4095, 4096, 4099)


def _big_case(dt, rows):
    return _case(WALK_NET, dt, rows=rows, S=S_BIG, key=("big", rows), references=PROBES)


@pytest.mark.parametrize("dt", DTYPES)
def test_one_workgroup_walks_every_tile_at_4100_samples(gpu, dt):
    sizes = WALK_NET
    t11, t14 = kernels.bnn_predict_row_tile(sizes, dt), kernels.bnn_predict_grad_row_tile(sizes, dt)
    rows = 2 * max(t11, t14) + 3
    for tile in (t11, t14):
        assert N.grid_y(S_BIG, -(-rows // tile)) == 1 and -(-rows // tile) >= 3
        assert N.grid_y(S_BIG - 5, -(-rows // tile)) == 2
    case = _big_case(dt, rows)
    X = torch.from_numpy(case["X"]).to(gpu)
    chains = torch.from_numpy(case["theta"].reshape(4, 1025, case["P"])).to(gpu)
    assert chains.is_contiguous()
    y = _targets(case, rows, gpu)
    k11, em, ev = _k11(chains, sizes, X, S_BIG, ens=True)
    k14 = _k14(chains, sizes, X, S_BIG, ens=True)
    k13 = _k13(chains, sizes, X, y, S_BIG)
    # parity on the probes, and every entry K11's bits
    probes = list(PROBES)
    _check(case, dt, "means", k11[probes], np.arange(len(probes)), rows, "S = 4100")
    _check(case, dt, "grads", k14[1][probes], np.arange(len(probes)), rows, "S = 4100")
    assert bool(torch.isfinite(k11).all()) and bool(torch.isfinite(k14[1]).all())
    _same_bits(k14[0], k11, "K14's means against K11's")
    _same_bits(k13["means"], k11, "K13's means against K11's")
    # a sample's bits are those of a call with that sample alone
    flat = chains.view(S_BIG, case["P"])
    for s in probes:
        _same_bits(_k11(flat[s:s + 1], sizes, X, 1)[0], k11[s:s + 1], "K11, sample %d alone" % s)
        alone = _k14(flat[s:s + 1], sizes, X, 1)
        _same_bits(alone[0], k11[s:s + 1], "K14's means, sample %d alone" % s)
        _same_bits(alone[1], k14[1][s:s + 1], "K14's grads, sample %d alone" % s)
    # the ensemble
    _check_moments(k11, em, ev, "K11 at S = 4100")
    for got, name in ((k14[2], "ens_mean"), (k13["ens_mean"], "ens_mean")):
        _same_bits(got, em, name)
    for got, name in ((k14[3], "ens_var"), (k13["ens_var"], "ens_var")):
        _same_bits(got, ev, name)
    want_dmean, want_dvar = C.ensemble_statement(k11.cpu().numpy(), k14[1].cpu().numpy(), em.cpu().numpy())
    assert bool(torch.isfinite(k14[4]).all() and torch.isfinite(k14[5]).all())
    _same_bits(k14[4], want_dmean, "dmean of 4100 samples")
    _same_bits(k14[5], want_dvar, "dvar of 4100 samples")
    _check_score(case, k13, S_BIG, y, "S = 4100")
    # S = 4095: grid.y = 2, two workgroups share the tiles; the same bits
    fewer = flat[:S_BIG - 5]
    _same_bits(_k11(fewer, sizes, X, S_BIG - 5)[0], k11[:S_BIG - 5], "K11 at S = 4095")
    got = _k14(fewer, sizes, X, S_BIG - 5)
    _same_bits(got[0], k11[:S_BIG - 5], "K14's means at S = 4095")
    _same_bits(got[1], k14[1][:S_BIG - 5], "K14's grads at S = 4095")
    got = _k13(fewer, sizes, X, y, S_BIG - 5)
    _same_bits(got["means"], k11[:S_BIG - 5], "K13's means at S = 4095")
    _same_bits(got["loglik"], k13["loglik"][:S_BIG - 5], "K13's loglik at S = 4095")


@pytest.mark.parametrize("S", [23, 128, S_BIG])
@pytest.mark.parametrize("dt", DTYPES)
def test_k13_s_sample_blocks(gpu, dt, S):
    """S = 23 ends a block in the middle of a 16-deep load group, S = 128 is two exact blocks of 64, S = 4100 is 64 blocks and a
    group of 4."""
    sizes, rows = WALK_NET, 65
    case = _big_case(dt, rows)
    X = torch.from_numpy(case["X"]).to(gpu)
    chains = torch.from_numpy(case["theta"][:S].copy()).to(gpu)
    y = _targets(case, rows, gpu)
    got = _k13(chains, sizes, X, y, S)
    k11, em, ev = _k11(chains, sizes, X, S, ens=True)
    _same_bits(got["means"], k11, "means")
    _same_bits(got["ens_mean"], em, "ens_mean")
    _same_bits(got["ens_var"], ev, "ens_var")
    _check_score(case, got, S, y, "S = %d" % S)


# ---- g. capture -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel, sizes", [pytest.param(N.K11, [10, 123, 121, 1], id="K11-148KB"),
                                           pytest.param(N.K14, [100, 194, 1], id="K14-160KiB")])
def test_the_lds_opt_in_is_legal_under_stream_capture(gpu, kernel, sizes):
    from pysgmcmc_amd.samplers.base_classes import graph_capture
    dt = torch.float64
    assert N.table_cell(sizes, kernel, 8)[1] == {N.K11: 148224, N.K14: 163840}[kernel]
    case = _case(sizes, dt)
    X = torch.from_numpy(case["X"]).to(gpu)
    chains = _contiguous(gpu, case, S5, 1)
    run = _k11 if kernel == N.K11 else _k14
    eager = run(chains, sizes, X, S5, ens=True)
    outs = [torch.zeros_like(t) for t in eager]

    def call():
        if kernel == N.K11:
            kernels.bnn_predict(chains, sizes, X, outs[0], ens_mean=outs[1], ens_var=outs[2])
        else:
            kernels.bnn_predict_grad(chains, sizes, X, *outs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # the first launch of each kernel outside the capture
        call()
    torch.cuda.current_stream().wait_stream(side)
    for t in outs:
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        call()
    torch.cuda.synchronize()
    assert float(outs[0].abs().sum()) == 0.0              # captured, not run
    g.replay()
    torch.cuda.synchronize()
    for k, (got, want) in enumerate(zip(outs, eager)):
        _same_bits(got, want, "%s output %d of the replayed graph" % (kernel, k))
    _check(case, dt, "means", outs[0], np.arange(S5), case["rows"], "replayed")
