"""The Stein thinning kernel K17 (include/sgmcmc_hip_thin.h, csrc/sgmcmc_stein_thin.hip) on the GPU: bit for bit against the
host statement ``diagnostics.stein.stein_thinning_indices`` at every launch form with canaries and a NaN-filled pitch gap,
ties across the kernel's seams, a batch of diagonal blocks, reproducibility and capture, non-finite input, the refusals,
``diagnostics.stein_thinning`` on device inputs and ``FusedBNNChains.thin`` end to end. Nothing here needs a tolerance: the
contract fixes every rounding."""
import numpy as np
import pytest
import torch

from pysgmcmc_amd import _lib, diagnostics, kernels
from pysgmcmc_amd.diagnostics import stein
from pysgmcmc_amd.samplers.base_classes import graph_capture

import stein_thin_cases as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = M.F32, M.F64
TORCH = {F32: torch.float32, F64: torch.float64}
TAIL = 64
I_CANARY, P_CANARY = -7, -7.0


def _outputs(count):
    return (torch.full((count + TAIL,), I_CANARY, dtype=torch.int32, device=DEV),
            torch.full((count + TAIL,), P_CANARY, dtype=torch.float64, device=DEV))


def _pitched(K, gap=3):
    """K on the device in rows of n + gap elements, the gap filled with NaN."""
    n = K.shape[0]
    buf = torch.full((n, n + gap), float("nan"), dtype=TORCH[K.dtype.type], device=DEV)
    buf[:, :n] = torch.from_numpy(np.array(K)).to(DEV)
    return buf[:, :n]


def _thin(Kd, m, distinct=False, **kw):
    """One call with canary tails behind both outputs: (indices, path) on the host, the tails checked."""
    count = m * kw.get("batch", 1)
    ibuf, pbuf = _outputs(count)
    idx, path = kernels.stein_thin(Kd, m, indices=ibuf[:count], path=pbuf[:count], distinct=distinct, **kw)
    assert idx.data_ptr() == ibuf.data_ptr() and path.data_ptr() == pbuf.data_ptr()
    ih, ph = ibuf.cpu().numpy(), pbuf.cpu().numpy()
    assert np.all(ih[count:] == I_CANARY) and np.all(ph[count:] == P_CANARY)
    return ih[:count], ph[:count]


def _check(K, m, distinct=False):
    want_i, want_p = stein.stein_thinning_indices(K, m, distinct)
    for Kd in (torch.from_numpy(np.array(K)).to(DEV), _pitched(K)):          # dense, and ld_m = n + 3 with NaN in the gap
        got_i, got_p = _thin(Kd, m, distinct)
        assert np.array_equal(got_i, want_i), (K.shape[0], m, distinct, int(Kd.stride(0)))
        assert np.array_equal(got_p, want_p), (K.shape[0], m, distinct, int(Kd.stride(0)))
    return want_i


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", M.SIZES)
def test_picks_and_path_equal_the_host_statement(n, dtype):
    K = M.matrix(n, dtype)
    idx = _check(K, min(n, M.M_SHORT))
    assert idx.min() >= 0 and idx.max() < n
    if n in M.REPEAT_N:
        idx = _check(K, 3 * n)                                               # more picks than rows: rows repeat
        assert idx.min() >= 0 and idx.max() < n


@pytest.mark.parametrize("n", M.DISTINCT_N)
def test_distinct_with_m_equal_n_is_the_host_statement_s_permutation(n):
    idx = _check(M.matrix(n, F32), n, distinct=True)
    assert sorted(idx.tolist()) == list(range(n))


@pytest.mark.parametrize("cols", M.TIES, ids=["-".join(map(str, c)) for c in M.TIES])
def test_ties_across_the_seams_go_to_the_smallest_index(cols):
    dtype = F64 if len(cols) == 4 else F32
    K = M.tie_matrix(cols, dtype)
    Kd = torch.from_numpy(K).to(DEV)
    m = 6
    idx, path = _thin(Kd, m)
    assert idx.tolist() == [cols[0]] * m                                     # the tied columns tie at every step
    want = stein.stein_thinning_indices(K, m)
    assert np.array_equal(idx, want[0]) and np.array_equal(path, want[1])
    m = len(cols) + 2
    idx, path = _thin(Kd, m, distinct=True)
    assert idx.tolist()[:len(cols)] == list(cols)                            # ascending, one after the other
    want = stein.stein_thinning_indices(K, m, distinct=True)
    assert np.array_equal(idx, want[0]) and np.array_equal(path, want[1])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [96, 65])
def test_a_batch_walks_the_diagonal_blocks(n, dtype):
    """Four diagonal blocks of one (4 n + 5)-wide matrix, NaN everywhere else; at n = 65 the blocks start at odd elements."""
    width, m = 4 * n + 5, 20
    big = np.full((width, width), np.nan, dtype=dtype)
    blocks = [M.matrix(n, dtype), M.matrix(n + 1, dtype)[1:, 1:], M.matrix(n + 2, dtype)[2:, 2:], M.matrix(n + 3, dtype)[:n, :n]]
    for p, B in enumerate(blocks):
        big[p * n:(p + 1) * n, p * n:(p + 1) * n] = B
    bd = torch.from_numpy(big).to(DEV)
    for distinct in (False, True):
        idx, path = _thin(bd, m, distinct, n=n, batch=4, batch_stride=n * width + n)
        for p, B in enumerate(blocks):
            one_i, one_p = _thin(torch.from_numpy(np.array(B)).to(DEV), m, distinct)
            assert np.array_equal(idx[p * m:(p + 1) * m], one_i) and np.array_equal(path[p * m:(p + 1) * m], one_p), p
            want = stein.stein_thinning_indices(B, m, distinct)
            assert np.array_equal(one_i, want[0]) and np.array_equal(one_p, want[1])
    # allocated outputs of a batch are (batch, m); path may be left out in the C call only
    i2, p2 = kernels.stein_thin(bd, m, n=n, batch=4, batch_stride=n * width + n)
    assert i2.shape == p2.shape == (4, m) and i2.dtype == torch.int32 and p2.dtype == torch.float64
    ibuf, _ = _outputs(4 * m)
    rc = getattr(_lib.lib(), "sgmcmc_stein_thin_" + ("f32" if dtype == F32 else "f64"))(
        bd.data_ptr(), width, n, m, 4, n * width + n, 0, ibuf.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(ibuf[:4 * m], i2.reshape(-1)) and bool(torch.all(ibuf[4 * m:] == I_CANARY))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_two_runs_and_a_captured_call_give_the_same_bits(dtype):
    n, m = 1025, 40
    Kd = torch.from_numpy(np.array(M.matrix(n, dtype))).to(DEV)
    i0, p0 = kernels.stein_thin(Kd, m)
    i1, p1 = kernels.stein_thin(Kd, m)
    assert torch.equal(i0, i1) and torch.equal(p0, p1)
    idx = torch.zeros(m, dtype=torch.int32, device=DEV)
    path = torch.zeros(m, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, capture_error_mode="thread_local"):            # one stream, no parallel branches
        kernels.stein_thin(Kd, m, indices=idx, path=path)
    for _ in range(2):
        idx.zero_(), path.zero_()
        graph.replay()
        assert torch.equal(idx, i0) and torch.equal(path, p0)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_a_nan_row_leaves_every_index_in_range(dtype):
    for n in (65, 1025):
        K = np.array(M.matrix(n, dtype))
        K[7, :] = np.nan
        K[:, 7] = np.nan
        K[n - 1, 3] = np.inf
        for distinct, m in ((False, 3 * n), (True, n)):
            idx, _ = _thin(torch.from_numpy(K).to(DEV), m, distinct)         # returns: the copy above waited for the launch
            assert idx.min() >= 0 and idx.max() < n
            assert not distinct or sorted(idx.tolist()) == list(range(n))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_refusals_launch_nothing(dtype):
    lib = _lib.lib()
    f = getattr(lib, "sgmcmc_stein_thin_" + ("f32" if dtype == torch.float32 else "f64"))
    Kd = torch.ones(16, 8, dtype=dtype, device=DEV)                          # two blocks of 8 x 8, batch_stride 64
    base = dict(matrix=Kd.data_ptr(), ld_m=8, n=8, m=4, batch=2, batch_stride=64, flags=0)
    ibuf, pbuf = _outputs(18)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**over):
        a = dict(base, indices=ibuf.data_ptr(), path=pbuf.data_ptr(), **over)
        return f(a["matrix"], a["ld_m"], a["n"], a["m"], a["batch"], a["batch_stride"], a["flags"], a["indices"], a["path"], stream)

    for i, (wrong, text) in enumerate(M.REFUSALS):
        assert call(**wrong) == -1 and lib.sgmcmc_last_error() == text       # SGMCMC_EINVAL and its text
        for later, _ in M.REFUSALS[i + 1:]:
            assert call(**dict(later, **wrong)) == -1 and lib.sgmcmc_last_error() == text, (wrong, later)
    torch.cuda.synchronize()
    assert bool(torch.all(ibuf == I_CANARY)) and bool(torch.all(pbuf == P_CANARY))
    assert call() == 0                                                       # and the same arguments, unspoilt, run
    torch.cuda.synchronize()
    assert ibuf[:8].tolist() == [0] * 8 and bool(torch.all(ibuf[8:] == I_CANARY))
    with pytest.raises(_lib.SgmcmcLibraryError, match="stein_thin: DISTINCT needs m <= n"):
        kernels.stein_thin(Kd[:8], 9, distinct=True)


# ---- diagnostics.stein_thinning on device inputs ------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_stein_thinning_of_device_inputs(dt):
    n, d, m = M.GAUSS[0]
    X, S = M.gauss(n, d)
    x, s = torch.tensor(X, dtype=dt, device=DEV), torch.tensor(S, dtype=dt, device=DEV)
    got = diagnostics.stein_thinning(x, s, m)
    assert isinstance(got, diagnostics.SteinThinning)
    for f in (got.indices, got.ksd_path, got.v_path):
        assert f.is_cuda and f.shape == (m,)
    assert got.indices.dtype == torch.int32 and got.v_path.dtype == got.ksd_path.dtype == torch.float64
    want = diagnostics.kernel_stein_discrepancy(x, s, return_matrix=True)
    for a, b in zip(got.discrepancy[:5], want[:5]):
        assert torch.equal(a, b)                                             # the whole set's discrepancy, bit for bit
    assert got.discrepancy.thinning == 1
    idx, path = stein.stein_thinning_indices(got.discrepancy.matrix.cpu().numpy(), m)
    assert np.array_equal(got.indices.cpu().numpy(), idx) and np.array_equal(got.v_path.cpu().numpy(), path)
    assert torch.equal(got.ksd_path, torch.sqrt(torch.clamp(got.v_path, min=0.0)))
    if dt == torch.float64:                                                  # the picks of the host route: gaps of 2.6e-4
        assert np.array_equal(idx, diagnostics.stein_thinning(X, S, m).indices)
    # per chain: each chain on its own diagonal block of the one pooled matrix
    xc, sc = x.view(4, 75, d), s.view(4, 75, d)
    for distinct in (False, True):
        chains = diagnostics.stein_thinning(xc, sc, m, per_chain=True, distinct=distinct)
        assert chains.indices.shape == chains.v_path.shape == chains.ksd_path.shape == (4, m)
        assert torch.equal(chains.discrepancy.matrix, want.matrix)
        for p in range(4):
            blk = want.matrix[75 * p:75 * p + 75, 75 * p:75 * p + 75].contiguous()
            i, v = kernels.stein_thin(blk, m, distinct=distinct)
            assert torch.equal(chains.indices[p], i) and torch.equal(chains.v_path[p], v)
            hi, hv = stein.stein_thinning_indices(blk.cpu().numpy(), m, distinct)
            assert np.array_equal(i.cpu().numpy(), hi) and np.array_equal(v.cpu().numpy(), hv)
    rbf = diagnostics.stein_thinning(x, s, m, kernel="rbf", bandwidth=2.0, workspace=kernels.ksd_workspace(n, x))
    assert not torch.equal(rbf.discrepancy.matrix, want.matrix) and int(rbf.indices.max()) < n
    with pytest.raises(ValueError, match="4096.*thin"):
        diagnostics.stein_thinning(torch.zeros(4097, 2, device=DEV), torch.zeros(4097, 2, device=DEV), 3)


# ---- FusedBNNChains.thin ------------------------------------------------------------------------------------------------------

def test_the_chain_group_thins_its_own_trace():
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    rng = np.random.RandomState(1)
    X = rng.rand(100, 1)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    chains = FusedBNNChains.for_dataset(X, y, 4, seed=2, device=DEV, burn_in_steps=40)
    trace = chains.collect(32, every=10)                                     # 4 chains x 32 kept samples
    P = trace.shape[2]
    flat = trace.reshape(-1, P)
    ensemble, result = chains.thin(trace, 16)
    assert ensemble.shape == (16, P) and result.indices.shape == (16,) and result.indices.dtype == torch.int32
    assert torch.equal(ensemble, flat[result.indices.long()])
    assert result.discrepancy.thinning == 1
    want = diagnostics.stein_thinning(trace, chains.posterior_scores(trace), 16)
    assert torch.equal(result.indices, want.indices) and torch.equal(result.v_path, want.v_path)
    assert torch.equal(result.discrepancy.v_statistic, chains.stein_discrepancy(trace).v_statistic)
    Xd = torch.as_tensor(X, dtype=trace.dtype, device=DEV)
    mean, var = chains.predict(Xd, ensemble)
    assert mean.shape[0] == 100 and var.shape == mean.shape
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all())
    print("KSD of the 128 rows %.6g, of the 16 thinned %.6g, of every 8th %.6g" % (
        float(result.discrepancy.ksd), float(result.ksd_path[-1]),
        float(chains.stein_discrepancy(flat[::8]).ksd)))
    # per chain: 5 rows of every chain, picked on that chain alone, distinct
    ens4, res4 = chains.thin(trace, 5, per_chain=True, distinct=True)
    assert ens4.shape == (20, P) and res4.indices.shape == res4.v_path.shape == (4, 5)
    for c in range(4):
        assert torch.equal(ens4[5 * c:5 * c + 5], trace[c][res4.indices[c].long()])
        assert len(set(res4.indices[c].tolist())) == 5
    # a trace of more than 4096 rows in all is strided first; the indices address the ORIGINAL rows
    long = trace[:2, :3].repeat(1, 700, 1)                                   # (2, 2100, P): stride 2
    ens, res = chains.thin(long, 6)
    assert res.discrepancy.thinning == 2 and res.discrepancy.row_sums.shape == (2100,)
    idx = res.indices.long()
    assert bool(torch.all((idx % 2100) % 2 == 0)) and int(idx.min()) >= 0 and int(idx.max()) < 4200
    assert torch.equal(ens, long.reshape(-1, P)[idx])
    ens, res = chains.thin(long, 6, per_chain=True)
    assert res.indices.shape == (2, 6) and bool(torch.all(res.indices % 2 == 0)) and int(res.indices.max()) < 2100
    for c in range(2):
        assert torch.equal(ens[6 * c:6 * c + 6], long[c][res.indices[c].long()])
