"""The kernel Stein discrepancy kernel K16 (include/sgmcmc_hip_ksd.h, csrc/sgmcmc_ksd.hip) on the GPU: every case of
``ksd_cases.py`` against the fp64 host statement, the f64 sums against the stated order bit for bit, one set of bits across
pitches, alignments, requested outputs and runs with canaries intact, a captured call, duplicated samples;
``models.bnn_posterior_scores`` against K15 and fp64 autograd; ``FusedBNNChains.stein_discrepancy``.

Bar. Entrywise ``|k_p - ref_ij| <= C u_T M_ij`` with ``ref`` the host statement in fp64 on the same inputs, ``M_ij`` the
first-order magnitude of ``ksd_cases.magnitude`` and ``C`` = 8 x the host statement's own worst figure over the table with
its sums in the case's precision (``ksd_cases.C``: 8 x 1.866 in f32, 8 x 5.536 in f64). V, U and the row sums: the same bar
summed over their entries."""
import numpy as np
import pytest
import torch

from pysgmcmc_amd import diagnostics, kernels, models
from pysgmcmc_amd.data_batches import Placeholder
from pysgmcmc_amd.diagnostics import stein
from pysgmcmc_amd.samplers.base_classes import graph_capture

import ksd_cases as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = M.F32, M.F64
CANARY, TAIL = 7.0, 256
KIND_ARGS = {k: dict(kind=v["kernel"], c=v.get("c", 1.0), beta=v.get("beta", -0.5), h2=v.get("bandwidth"))
             for k, v in M.KERNELS.items()}


def _params():
    out = []
    for dt in (F32, F64):
        cases = [(n, d, k) for n, d in M.TABLE for k in M.KERNELS]
        cases += [(n, d, k) for n, d in M.walk_cases(dt) for k in M.KERNELS]
        cases += [(n, d, "imq") for n, d in M.phase_cases(dt)]
        cases += [(n, d, "imq") for n, d in M.CLAMP_CASES]
        out += [pytest.param(n, d, dt, k, id="%dx%d-%s-%s" % (n, d, np.dtype(dt).name, k)) for n, d, k in cases]
    return out


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                     # a copy: the shared references are read-only


def _run(x, s, kern, matrix=True, rows=True, ws=None):
    n = x.shape[0]
    if ws is None:
        ws = kernels.ksd_workspace(n, x)
        ws.fill_(float("nan"))                                        # a partial that is read but never written shows
    K = torch.full((n, n), float("nan"), dtype=x.dtype, device=x.device) if matrix is True else matrix
    r = torch.full((n,), float("nan"), dtype=torch.float64, device=x.device) if rows is True else rows
    stats = kernels.ksd(x, s, ws, matrix=K, row_sums=r, **KIND_ARGS[kern])
    return K, r, stats


def _check(what, ref, dtype, K, rows, stats):
    n = ref.K.shape[0]
    c = M.C[dtype]
    K64 = K.astype(np.float64)
    un = M.units(K64, ref, dtype)
    bar_rows, bar_v, bar_u = M.sum_bars(ref, dtype)
    ur = float(np.max(np.abs(rows - ref.rows) / bar_rows))
    uv, uu = abs(stats[0] - ref.v) / bar_v, abs(stats[1] - ref.u) / bar_u
    print("%s: matrix %.3f, row sums %.3f, V %.3f, U %.3f units of the bar at C = 1; C = %g" % (what, un, ur, uv, uu, c))
    assert np.all(np.isfinite(K64)) and np.array_equal(K64, K64.T), what          # exactly symmetric
    assert un <= c, "%s: an entry is %.2f units off, C = %g" % (what, un, c)
    assert ur <= c and uv <= c and uu <= c, what
    assert stats[0] == stats[2] / (float(n) * n) and stats[1] == (stats[2] - stats[3]) / (float(n) * (n - 1)), what


@pytest.mark.parametrize("n,d,dtype,kern", _params())
def test_every_case_matches_the_host_statement(n, d, dtype, kern):
    ref = M.reference(n, d, dtype, kern)
    x, s = _dev(ref.X), _dev(ref.S)
    K, rows, stats = _run(x, s, kern)
    torch.cuda.synchronize()
    assert torch.equal(x, _dev(ref.X)) and torch.equal(s, _dev(ref.S))
    K, rows, stats = K.cpu().numpy(), rows.cpu().numpy(), stats.cpu().numpy()
    _check("ksd %d x %d %s %s" % (n, d, np.dtype(dtype).name, kern), ref, dtype, K, rows, stats)
    if dtype == F64:
        # the sums of the kernel's own matrix in the stated order, bit for bit (matrix_out is the double itself in f64)
        want_rows, want_total, want_trace = stein.stein_sums(K)
        assert np.array_equal(rows, want_rows) and stats[2] == want_total and stats[3] == want_trace


# ---- one set of bits ------------------------------------------------------------------------------------------------------

def _pitched(a, ld, offset):
    n, d = a.shape
    t = _dev(a)
    buf = torch.full((offset + n * ld + TAIL,), CANARY, dtype=t.dtype, device=DEV)
    view = buf[offset:offset + n * ld].view(n, ld)[:, :d]
    view.copy_(t)
    return buf, view


def _canary_intact(buf, n, d, ld, offset):
    host = buf.cpu().numpy()
    keep = np.ones(host.shape[0], bool)
    for i in range(n):
        keep[offset + i * ld:offset + i * ld + d] = False
    return bool(np.all(host[keep] == CANARY))


def _bits_cases():
    out = []
    for dt in (F32, F64):
        for n, d in [(65, 67), (129, 41)] + M.walk_cases(dt)[1:]:
            out.append(pytest.param(n, d, dt, id="%dx%d-%s" % (n, d, np.dtype(dt).name)))
    return out


@pytest.mark.parametrize("kern", ["imq", "rbf"])
@pytest.mark.parametrize("n,d,dtype", _bits_cases())
def test_bits_do_not_depend_on_pitch_alignment_outputs_or_the_run(n, d, dtype, kern):
    """Dense, 16-byte-aligned pitched and element-shifted odd-pitched layouts of the samples, the scores and the matrix, each
    twice, and calls that ask for fewer outputs: one set of bits, every canary intact."""
    assert d % 2 == 1
    X, S = M.inputs(n, d, dtype)
    x, s = _dev(X), _dev(S)
    K0, r0, st0 = _run(x, s, kern)
    # (ld_x, offset of X, ld_s, offset of S, ld_m, offset of the matrix)
    layouts = [((d // 4 + 1) * 4, 0, (d // 4 + 2) * 4, 0, (n // 4 + 1) * 4, 0), (d, 1, d + 2, 3, n + 1, 1)]
    for ld_x, ox, ld_s, os_, ld_m, om in layouts + layouts:
        bx, vx = _pitched(X, ld_x, ox)
        bs, vs = _pitched(S, ld_s, os_)
        bm = torch.full((om + n * ld_m + TAIL,), CANARY, dtype=x.dtype, device=DEV)
        vm = bm[om:om + n * ld_m].view(n, ld_m)[:, :n]
        rows = torch.full((n + TAIL,), CANARY, dtype=torch.float64, device=DEV)
        _, _, st = _run(vx, vs, kern, matrix=vm, rows=rows[:n])
        assert torch.equal(vm, K0) and torch.equal(rows[:n], r0) and torch.equal(st, st0), (ld_x, ld_s, ld_m)
        assert _canary_intact(bx, n, d, ld_x, ox) and _canary_intact(bs, n, d, ld_s, os_)   # the inputs are only read
        assert _canary_intact(bm, n, n, ld_m, om) and bool(torch.all(rows[n:] == CANARY))
        assert torch.equal(vx, x) and torch.equal(vs, s)
    for matrix, rows in ((None, True), (True, None), (None, None)):
        K, r, st = _run(x, s, kern, matrix=matrix, rows=rows)
        assert torch.equal(st, st0) and (K is None or torch.equal(K, K0)) and (r is None or torch.equal(r, r0))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_a_captured_call_replays_the_eager_bits(dtype):
    n, d = 129, 40
    X, S = M.inputs(n, d, dtype)
    x, s = _dev(X), _dev(S)
    K0, r0, st0 = _run(x, s, "imq")
    ws = kernels.ksd_workspace(n, x)
    K = torch.zeros_like(K0)
    rows, stats = torch.zeros_like(r0), torch.zeros(4, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, capture_error_mode="thread_local"):            # one stream, no parallel branches
        kernels.ksd(x, s, ws, matrix=K, row_sums=rows, stats=stats)
    for _ in range(2):
        K.zero_(), rows.zero_(), stats.zero_()
        graph.replay()
        assert torch.equal(K, K0) and torch.equal(rows, r0) and torch.equal(stats, st0)
    x.copy_(_dev(X) + 0.25 * _dev(S))                                        # a replay reads what the buffers hold then
    graph.replay()
    K1, r1, st1 = _run(x, s, "imq")
    assert torch.equal(K, K1) and torch.equal(stats, st1) and not torch.equal(st1, st0)


@pytest.mark.parametrize("kern", list(M.KERNELS))
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_duplicated_samples_stay_finite_and_symmetric(dtype, kern):
    n, d = 130, 7
    X, S = M.inputs(n, d, dtype)
    X, S = X.copy(), S.copy()
    X[1::2], S[1::2] = X[0::2], S[0::2]                                      # every sample twice: r2 = 0 off the diagonal
    K, rows, stats = _run(_dev(X), _dev(S), kern)
    K, rows, stats = K.cpu().numpy().astype(np.float64), rows.cpu().numpy(), stats.cpu().numpy()
    assert np.all(np.isfinite(K)) and np.all(np.isfinite(rows)) and np.all(np.isfinite(stats))
    assert np.array_equal(K, K.T)
    ref = stein.stein_kernel_matrix(X, S, **M.KERNELS[kern])
    scale = np.abs(ref).max()
    assert np.max(np.abs(K - ref)) <= (1e-4 if dtype == F32 else 1e-12) * scale


def test_device_tensors_go_to_the_kernel_and_stay_on_the_device():
    n, d = 65, 67
    ref = M.reference(n, d, F32, "imq")
    x, s = _dev(ref.X), _dev(ref.S)
    K0, r0, st0 = _run(x, s, "imq")
    r = diagnostics.kernel_stein_discrepancy(x, s, return_matrix=True)
    for f in (r.ksd, r.v_statistic, r.u_statistic, r.row_sums):
        assert f.is_cuda and f.dtype == torch.float64
    assert torch.equal(r.matrix, K0) and torch.equal(r.row_sums, r0)
    assert torch.equal(r.v_statistic, st0[0]) and torch.equal(r.u_statistic, st0[1])
    assert torch.equal(r.ksd, torch.sqrt(torch.clamp(st0[0], min=0.0))) and r.thinning == 1
    chains = diagnostics.kernel_stein_discrepancy(x[:60].reshape(3, 20, d), s[:60].reshape(3, 20, d), kernel="rbf", bandwidth=1.0)
    flat = diagnostics.kernel_stein_discrepancy(x[:60], s[:60], kernel="rbf", bandwidth=1.0, workspace=kernels.ksd_workspace(60, x))
    assert torch.equal(chains.v_statistic, flat.v_statistic) and chains.matrix is None
    trace = diagnostics.DeviceTrace(d, n + 3, DEV)
    for row in x:
        trace.append(row)
    assert torch.equal(diagnostics.kernel_stein_discrepancy(trace, s).v_statistic, st0[0])
    with pytest.raises(ValueError, match="4096.*thin"):
        diagnostics.kernel_stein_discrepancy(torch.zeros(4097, 2, device=DEV), torch.zeros(4097, 2, device=DEV))


# ---- bnn_posterior_scores -------------------------------------------------------------------------------------------------

DEFAULT = [1, 50, 50, 50, 1]
N_ROWS = 40


def _bnn_problem(dt, n=5):
    rng = np.random.RandomState(5)
    X = rng.uniform(-1.0, 1.0, size=(N_ROWS, 1))
    y = np.sinc(X[:, 0] * 2.0) + 0.05 * rng.randn(N_ROWS)
    rows = torch.stack(models.bnn_particles(n, 1, hidden=DEFAULT[1:-1], seed=3, dtype=torch.float64)).numpy()
    rows = rows + 0.1 * rng.randn(*rows.shape)
    rows[:, -1] = -1.0 + 0.3 * rng.randn(n)                                  # log_var
    return (torch.tensor(rows, dtype=dt, device=DEV), torch.tensor(X, dtype=dt, device=DEV), torch.tensor(y, dtype=dt, device=DEV))


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_posterior_scores_are_k15_s_gradient_and_fp64_autograd_s(dt):
    theta, X, y = _bnn_problem(dt)
    n, P = theta.shape
    N = N_ROWS
    assert kernels.bnn_particles_lds_bytes(DEFAULT, N, dt) > 0               # one chunk in both dtypes
    one = models.bnn_posterior_scores(theta, DEFAULT, X, y)
    grad = torch.empty(n * P, dtype=dt, device=DEV)
    costs = torch.empty(n, dtype=dt, device=DEV)
    kernels.bnn_particles_cost_grad(theta.reshape(-1), n, P, DEFAULT, X, y, grad, P, costs, N, N, 1.0, 1e-6, 0.01)
    assert torch.equal(one, grad.view(n, P) * (-float(N)))                   # one chunk: -N x K15's gradient, bit for bit
    # a pitched (chains, n, P) matrix and `out`
    wide = torch.full((n, P + 5), float("nan"), dtype=dt, device=DEV)
    wide[:, :P] = theta
    out = torch.empty(n, P, dtype=dt, device=DEV)
    assert models.bnn_posterior_scores(wide[:, :P], DEFAULT, X, y, out=out) is out and torch.equal(out, one)
    assert torch.equal(models.bnn_posterior_scores(theta[:4].reshape(2, 2, P), DEFAULT, X, y), one[:4])
    three = models.bnn_posterior_scores(theta, DEFAULT, X, y, max_rows=16)   # chunks of 16, 16 and 8 rows
    # fp64 autograd of the full-data cost times -N
    cost = models.BNNParticleCost(DEFAULT, Placeholder().feed(X.double().cpu()), Placeholder().feed(y.double().cpu()), N, N)
    want = models.bnn_posterior_scores(theta.double().cpu(), DEFAULT, X.double().cpu(), y.double().cpu())
    row = theta[0].double().cpu().requires_grad_(True)
    assert torch.equal(want[0], torch.autograd.grad(cost(row), row)[0] * (-float(N)))
    tol = 2e-4 if dt == torch.float32 else 1e-9                              # the bar test_bnn_particles_gpu.py holds K15 to
    for name, got in (("one chunk", one), ("three chunks", three)):
        for p in range(n):
            dev = float((got[p].double().cpu() - want[p]).abs().max() / want[p].abs().max())
            print("%s %s row %d: max|s - s64| / max|s64| = %.3e" % (name, dt, p, dev))
            assert dev <= tol, (name, p, dev)


# ---- FusedBNNChains.stein_discrepancy ---------------------------------------------------------------------------------------

def test_the_chain_group_scores_its_own_trace():
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    rng = np.random.RandomState(3)
    X = rng.uniform(-3.0, 3.0, size=(60, 1))
    y = np.sinc(X[:, 0]) + 0.05 * rng.randn(60)
    for stepsize in (1e-3, 1e-2):
        chains = FusedBNNChains.for_dataset(X, y, 4, seed=2, device=DEV, burn_in_steps=40, stepsize=stepsize)
        trace = chains.collect(32, every=5)                                  # 4 chains x 32 kept samples, 160 steps
        got = chains.stein_discrepancy(trace, return_matrix=True)
        gen = chains.samplers[0].batch_generator
        scores = models.bnn_posterior_scores(trace, DEFAULT, gen.x_dev, gen.y_dev)
        assert scores.shape == (128, trace.shape[2]) and torch.equal(scores, chains.posterior_scores(trace))
        want = diagnostics.kernel_stein_discrepancy(trace, scores, return_matrix=True)
        for a, b in zip(got[:5], want[:5]):
            assert torch.equal(a, b)
        assert got.thinning == 1 and got.matrix.shape == (128, 128)
        ksd, v, u = float(got.ksd), float(got.v_statistic), float(got.u_statistic)
        print("stepsize %g: ksd %.6g, V %.6g, U %.6g" % (stepsize, ksd, v, u))
        assert np.isfinite([ksd, v, u]).all() and ksd > 0 and v > 0
    # a trace of more than 4096 rows in all is thinned evenly
    long = trace[:, :3].repeat(1, 400, 1)                                    # 4 x 1200 rows
    thin = chains.stein_discrepancy(long)
    assert thin.thinning == 2 and thin.row_sums.shape == (2400,)
    x = long[:, ::2].reshape(-1, long.shape[2])
    assert torch.equal(thin.v_statistic, diagnostics.kernel_stein_discrepancy(x, chains.posterior_scores(x)).v_statistic)
