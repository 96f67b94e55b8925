"""K18, the rank normalisation of a strided device trace (csrc/sgmcmc_rank.hip, include/sgmcmc_hip_rank.h), and its public
front end (``kernels.rank_normalize``, ``diagnostics.rank_diagnostics_all``, ``FusedBNNChains.diagnose(rank_normalized=True)``)
against the host statement ``diagnostics.rank``.

What is exact: the tail indicators; the ranks, pinned through z (equal host rank2 <=> identical bits, strictly increasing,
antisymmetric bit for bit); z and z_folded themselves wherever the argument lies on the central branch of AS241
(|p - 0.5| <= 0.425: multiply, add and one divide in a fixed order). On the two tail branches the device's log differs
from the host's in the last place, so the bound there is measured: the largest ulp distance between the device's z and
the host table over ALL 2 N - 1 possible arguments, at N = 8192 and at N = 64, was

    TAIL_ULP_MEASURED = 2 ulp  (N = 8192: 2 ulp, N = 64: 0 ulp, in f32 and f64 alike; on an MI355X)

and the limit is that plus 2, one for each of the two library calls on the path (log, sqrt). The same goes for the R-hat and
raw ESS of ``rank_diagnostics_all`` against the host statement ``rank.rank_diagnostics``: the largest relative difference at
the largest case (N = 8192 as 64 chains of 128, 20 columns) was REL_MEASURED = 4.05e-15 (the raw ESS of tail_hi; the
R-hats differ by 2e-16), the limit is 4 times that because the tail ulps enter through sums of N terms; the smaller cases
came to 6e-15 and 9.6e-15. Both figures are in profiles/rank_diag.txt. Where every z lies on the central branch the agreement is K12's own 1e-10
(tests/test_chain_diag_gpu.py)."""
import numpy as np
import pytest
import torch

from pysgmcmc_amd import diagnostics, kernels
from pysgmcmc_amd.diagnostics import rank

import rank_cases as C

pytestmark = pytest.mark.gpu

TAIL_ULP_MEASURED = 2
TAIL_ULP_LIMIT = TAIL_ULP_MEASURED + 2
REL_MEASURED = 4.05e-15
REL_LIMIT = 4 * REL_MEASURED
DTYPES = [torch.float32, torch.float64]
CANARY = -77.25
NAMES = ("z", "z_folded", "tail_lo", "tail_hi")


def _guarded_outputs(m, n, P, dev, pad=3, which=(0, 1, 2, 3)):
    """Four (2 m, half, P) views with ld_out = P + pad and a longer chain stride inside canary-filled buffers."""
    half = n // 2
    full = [torch.full((2 * m + 1, half + 1, P + pad), CANARY, dtype=torch.float64, device=dev) for _ in range(4)]
    views = [f[:2 * m, :half, :P] if k in which else None for k, f in enumerate(full)]
    return full, views


def _check_canaries(full, views, m, n, P):
    half = n // 2
    for f, v in zip(full, views):
        h = f.cpu().numpy()
        if v is None:
            assert (h == CANARY).all(), "an output that was not passed was written"
        else:
            assert (h[2 * m:] == CANARY).all() and (h[:, half:] == CANARY).all() and (h[:, :, P:] == CANARY).all(), \
                "a canary between or behind the rows was overwritten"


def _run(x, dtype, dev, **kw):
    m, n, P = x.shape
    full, views = _guarded_outputs(m, n, P, dev, **kw)
    kernels.rank_normalize(torch.as_tensor(x, device=dev).to(dtype), *views)
    _check_canaries(full, views, m, n, P)
    return [None if v is None else v.cpu().numpy() for v in views]


def _assert_equals_host(got, x, what):
    """Every assertion of the module docstring on the four outputs of one call. Returns the largest tail ulp distance."""
    m, n, P = x.shape
    half, N = n // 2, 2 * m * (n // 2)
    ref = C.host_statement(x)
    table = rank.z_of_rank2(N)
    r2 = C.pooled_rank2(x)
    worst = 0
    for k in (2, 3):
        if got[k] is not None:
            assert C.same_bits(got[k], ref[k]), "%s: %s differs from the host statement" % (what, NAMES[k])
    for k in (0, 1):
        if got[k] is None:
            continue
        for p in range(P):
            g, w, r = got[k][:, :, p].ravel(), ref[k][:, :, p].ravel(), r2[k][:, :, p].ravel()
            if np.isnan(w).all():
                assert np.isnan(g).all(), "%s: column %d of %s is not all NaN" % (what, p, NAMES[k])
                continue
            assert np.isfinite(g).all(), "%s: column %d of %s" % (what, p, NAMES[k])
            # the ranks: one value of z per rank2, strictly increasing in rank2, antisymmetric bit for bit
            order = np.argsort(r, kind="stable")
            rs, gs = r[order], g[order]
            new = np.diff(rs) > 0
            assert np.array_equal(C.bits(gs[1:])[~new], C.bits(gs[:-1])[~new]), "%s: equal ranks, different z" % what
            assert np.all(np.diff(gs)[new] > 0), "%s: z is not strictly increasing in rank2" % what
            first = np.concatenate([[True], new])
            ur, uz = rs[first], gs[first]                    # one entry per rank2 that occurs, ascending
            at = np.searchsorted(ur, 2 * N + 2 - ur)
            both = (at < ur.size) & (ur != N + 1)
            both[both] = ur[at[both]] == (2 * N + 2 - ur)[both]
            assert np.array_equal(C.bits(uz[both]), C.bits(-uz[at[both]])), "%s: z(rank2) != -z(2 N + 2 - rank2)" % what
            assert (uz[ur == N + 1] == 0.0).all()
            # the values: the host table bit for bit on the central branch, within the measured ulps on the tails
            mid = C.central(r, N)
            assert np.array_equal(C.bits(g[mid]), C.bits(table[r][mid])), "%s: column %d of %s, central branch" % (what, p, NAMES[k])
            if (~mid).any():
                d = int(C.ulp_distance(g[~mid], table[r][~mid]).max())
                worst = max(worst, d)
                assert d <= TAIL_ULP_LIMIT, "%s: column %d of %s is %d ulp from the host table" % (what, p, NAMES[k], d)
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("m,n", C.SHAPES)
def test_every_pattern_at_every_pooled_count(gpu, m, n, dtype):
    P = C.N_PATTERNS if 2 * m * (n // 2) > 2100 else 2 * C.N_PATTERNS + 1
    x = C.pattern_trace(m, n, P)
    got = _run(x, dtype, gpu)
    worst = _assert_equals_host(got, x, "(%d, %d, %d) %s" % (m, n, P, dtype))
    print("(%d, %d, %d) %s: largest tail distance %d ulp" % (m, n, P, dtype, worst))
    # the constant column: z = 0 and both indicators 1 everywhere
    j = C.PATTERNS.index(C._constant)
    assert (got[0][:, :, j] == 0.0).all() and (got[2][:, :, j] == 1.0).all() and (got[3][:, :, j] == 1.0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("m,n", [(2, 4096), (1, 64)])
def test_tail_branch_distance_over_every_possible_argument(gpu, m, n, dtype):
    """The measurement behind TAIL_ULP_LIMIT: three columns that between them hold every rank2 in 2 .. 2 N."""
    x = C.all_rank2_trace(m, n)
    N = m * n
    got = _run(x, dtype, gpu, which=(0,))[0]
    r2 = C.pooled_rank2(x)[0]
    seen = np.unique(r2)
    assert np.array_equal(seen, np.arange(2, 2 * N + 1)), "the three columns do not reach every rank2"
    table = rank.z_of_rank2(N)
    dist = C.ulp_distance(got.ravel(), table[r2.ravel()])
    mid = C.central(r2.ravel(), N)
    print("N = %d %s: largest ulp distance over all %d arguments: %d (central branch: %d)" % (
        N, dtype, seen.size, int(dist.max()), int(dist[mid].max())))
    assert int(dist[mid].max()) == 0
    assert int(dist.max()) <= TAIL_ULP_LIMIT


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_layouts_and_column_counts(gpu, P, dtype):
    """ld > P and chain_stride > n * ld with NaN in the gaps, a base pointer one element past a 256-byte boundary, and a
    trace of one chain passed as (n, P): the bits of the dense call."""
    m, n = 3, 43                                             # odd n, N = 126
    x = C.pattern_trace(m, n, P, seed=1)
    base = _run(x, dtype, gpu)
    _assert_equals_host(base, x, "P = %d" % P)
    xt = torch.as_tensor(x, device=gpu).to(dtype)
    size = xt.element_size()
    flat = torch.full((m * (n + 2) * (P + 5) + 256,), float("nan"), dtype=dtype, device=gpu)
    lead = ((-flat.data_ptr()) % 256) // size + 1
    view = flat[lead:lead + m * (n + 2) * (P + 5)].view(m, n + 2, P + 5)[:, :n, :P]
    assert view.data_ptr() % 256 == size and view.stride(1) == P + 5 and view.stride(0) == (n + 2) * (P + 5)
    view.copy_(xt)
    full, outs = _guarded_outputs(m, n, P, gpu, pad=1)
    kernels.rank_normalize(view, *outs)
    _check_canaries(full, outs, m, n, P)
    for k in range(4):
        assert C.same_bits(outs[k].cpu().numpy(), base[k]), "strided, misaligned input: %s" % NAMES[k]
    # four column blocks of ONE buffer, the layout rank_diagnostics_all uses, at a misaligned base as well
    half = n // 2
    flat = torch.full((2 * m * half * 4 * P + 33,), CANARY, dtype=torch.float64, device=gpu)
    buf = flat[1:1 + 2 * m * half * 4 * P].view(2 * m, half, 4 * P)
    kernels.rank_normalize(xt, *[buf[:, :, k * P:(k + 1) * P] for k in range(4)])
    for k in range(4):
        assert C.same_bits(buf[:, :, k * P:(k + 1) * P].cpu().numpy(), base[k]), "column blocks: %s" % NAMES[k]
    assert float(flat[0]) == CANARY and bool((flat[1 + 2 * m * half * 4 * P:] == CANARY).all())
    # one chain as an (n, P) matrix
    one = _run(x[:1], dtype, gpu)
    z = torch.empty(2, half, P, dtype=torch.float64, device=gpu)
    kernels.rank_normalize(xt[0], z=z)
    assert C.same_bits(z.cpu().numpy(), one[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_each_subset_of_the_outputs(gpu, dtype):
    m, n, P = 5, 206, 11                                     # N = 1030
    x = C.pattern_trace(m, n, P)
    base = _run(x, dtype, gpu)
    for mask in range(1, 16):
        which = tuple(k for k in range(4) if mask >> k & 1)
        got = _run(x, dtype, gpu, which=which)               # the canary check covers the outputs that were not passed
        for k in range(4):
            assert (got[k] is None) == (k not in which)
            if got[k] is not None:
                assert C.same_bits(got[k], base[k]), "outputs %s: %s" % (which, NAMES[k])
    # P = 0: nothing is launched
    out = kernels.rank_normalize(torch.zeros(2, 8, 0, dtype=dtype, device=gpu),
                                 z=torch.zeros(4, 4, 0, dtype=torch.float64, device=gpu))
    assert out[0].numel() == 0


def test_f32_and_f64_elements_give_the_same_bits(gpu):
    x = C.pattern_trace(64, 128, C.N_PATTERNS)               # exactly representable as float32
    a, b = _run(x, torch.float32, gpu), _run(x, torch.float64, gpu)
    for k in range(4):
        assert C.same_bits(a[k], b[k]), NAMES[k]
    # float64 values a float32 cannot hold: denormal doubles and differences below float32's resolution
    rng = np.random.RandomState(4)
    y = np.stack([rng.randint(-9, 9, size=(2, 64)) * 5e-324, 1.0 + rng.randint(0, 50, size=(2, 64)) * 2.0 ** -50], axis=2)
    got = _run(y, torch.float64, gpu)
    ref = rank.rank_normalized_chains(y)
    assert C.same_bits(got[2], ref[2]) and C.same_bits(got[3], ref[3])
    mid = [C.central(r, 128) for r in C.pooled_rank2(y)]
    for k in (0, 1):
        assert np.array_equal(C.bits(got[k][mid[k]]), C.bits(ref[k][mid[k]]))
        assert int(C.ulp_distance(got[k], ref[k]).max()) <= TAIL_ULP_LIMIT


# ---- rank_diagnostics_all -----------------------------------------------------------------------------------------------------

def _tuple_bits_equal(a, b, what):
    assert len(a) == len(b)
    for s, t, name in zip(a, b, rank.RankDiagnostics._fields):
        assert s.dtype == t.dtype and s.shape == t.shape
        if s.dtype == torch.float64:
            assert C.same_bits(s.cpu().numpy(), t.cpu().numpy()), "%s: %s" % (what, name)
        else:
            assert torch.equal(s, t), "%s: %s" % (what, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("m,n,P", [(1, 40, 7), (4, 51, 66), (64, 128, 20)])
def test_rank_diagnostics_all(gpu, m, n, P, dtype):
    x = C.ar_chains(m, n, P, seed=m)
    xt = torch.as_tensor(x, device=gpu).to(dtype)
    arg = xt if m > 1 else xt[0]
    d = diagnostics.rank_diagnostics_all(arg, details=True)
    assert isinstance(d, rank.RankDiagnostics)
    assert [t.dtype for t in d[:3]] == [torch.float64, torch.int64, torch.int64]
    assert all(t.shape == (P,) and t.is_cuda for t in d)
    three = diagnostics.rank_diagnostics_all(arg)
    assert len(three) == 3
    _tuple_bits_equal(three, d[:3], "details=False")
    # K12 applied to K18's own outputs, one array at a time: the same bits, maximum and minimum taken on the device
    half = n // 2
    outs = [torch.empty(2 * m, half, P, dtype=torch.float64, device=gpu) for _ in range(4)]
    kernels.rank_normalize(xt, *outs)
    z, zf, lo, hi = outs
    rz, ez, rawz, _ = diagnostics.chain_diagnostics_all(z, details=True)
    _, elo, rawlo, _ = diagnostics.chain_diagnostics_all(lo, details=True)
    _, ehi, rawhi, _ = diagnostics.chain_diagnostics_all(hi, details=True)
    rf = diagnostics.gelman_rubin_all(zf)
    assert C.same_bits(diagnostics.gelman_rubin_all(z).cpu().numpy(), rz.cpu().numpy())
    want = rank.RankDiagnostics(torch.maximum(rz, rf), ez, torch.minimum(elo, ehi), rz, rf, elo, ehi, rawz, rawlo, rawhi)
    _tuple_bits_equal(d, want, "K12 on K18's outputs")
    # the host statement
    h = rank.rank_diagnostics(x)
    g = [t.cpu().numpy() for t in d]
    rel = 0.0
    for name in ("rhat_rank", "rhat_bulk", "rhat_folded", "raw_bulk", "raw_tail_lo", "raw_tail_hi"):
        a, b = g[rank.RankDiagnostics._fields.index(name)], getattr(h, name)
        assert np.isfinite(b).all() and np.isfinite(a).all(), name
        rel = max(rel, float(np.max(np.abs(a - b) / np.abs(b))))
    print("(%d, %d, %d) %s: largest relative difference to the host statement %.3g; rank R-hat %.4f..%.4f, bulk ESS %d..%d, "
          "tail ESS %d..%d" % (m, n, P, dtype, rel, g[0].min(), g[0].max(), g[1].min(), g[1].max(), g[2].min(), g[2].max()))
    assert rel <= REL_LIMIT
    for name in ("ess_bulk", "ess_tail", "ess_tail_lo", "ess_tail_hi"):
        a, b = g[rank.RankDiagnostics._fields.index(name)], getattr(h, name)
        assert np.all(np.abs(a - b) <= 1), name              # a truncation may fall on either side of an integer
    if m > 1:
        assert (g[0][0::3] > 1.01).all(), "chains of unequal scale pass the rank R-hat"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_central_branch_only_agrees_as_k12_does(gpu, dtype):
    """Columns of four values in near-equal numbers: every normal score lies on the central branch, so K18's outputs equal the
    host's bit for bit and what is left is K12 against numpy: 1e-10 relative and equal integers."""
    m, n, P = 6, 100, 12
    rng = np.random.RandomState(8)
    x = np.stack([(rng.permutation(m * n) % 4).reshape(m, n) * 0.5 - 0.25 for _ in range(P)], axis=2)
    N = 2 * m * (n // 2)
    assert all(C.central(r, N).all() for r in C.pooled_rank2(x))
    got = _run(x, dtype, gpu)
    for k, r in enumerate(rank.rank_normalized_chains(x)):
        assert C.same_bits(got[k], r), NAMES[k]
    d = [t.cpu().numpy() for t in diagnostics.rank_diagnostics_all(torch.as_tensor(x, device=gpu).to(dtype), details=True)]
    h = rank.rank_diagnostics(x)
    for a, b, name in zip(d, h, rank.RankDiagnostics._fields):
        if a.dtype == np.int64:
            assert np.array_equal(a, b), name
        else:
            assert np.all(np.abs(a - b) <= 1e-10 * np.abs(b)), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_degenerate_columns_do_not_touch_their_neighbours(gpu, dtype):
    m, n, P = 4, 30, C.N_PATTERNS
    x = C.pattern_trace(m, n, P)
    d = [t.cpu().numpy() for t in diagnostics.rank_diagnostics_all(torch.as_tensor(x, device=gpu).to(dtype), details=True)]
    bad = [j for j in range(P) if C.pattern_of(j) in C.DEGENERATE or C.pattern_of(j) is C._constant]
    good = [j for j in range(P) if j not in bad]
    for j in bad:
        assert np.isnan(d[0][j]) and d[1][j] == 0 and d[2][j] == 0, j
    assert np.isfinite(d[0][good]).all() and (d[1][good] > 0).all()
    clean = np.ascontiguousarray(x[:, :, good])
    e = [t.cpu().numpy() for t in diagnostics.rank_diagnostics_all(torch.as_tensor(clean, device=gpu).to(dtype), details=True)]
    for a, b, name in zip(d, e, rank.RankDiagnostics._fields):
        assert C.same_bits(a[good].astype(np.float64), b.astype(np.float64)), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_same_bits_under_capture_on_a_second_stream_and_twice_in_a_row(gpu, dtype):
    from pysgmcmc_amd.samplers.base_classes import graph_capture
    m, n, P = 8, 256, 33                                     # N = 2048
    xt = torch.as_tensor(C.ar_chains(m, n, P, seed=3), device=gpu).to(dtype)
    half = n // 2
    eager = [torch.empty(2 * m, half, P, dtype=torch.float64, device=gpu) for _ in range(4)]
    kernels.rank_normalize(xt, *eager)
    again = [torch.full_like(t, CANARY) for t in eager]
    kernels.rank_normalize(xt, *again)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = [torch.full_like(t, CANARY) for t in eager]
    with torch.cuda.stream(side):
        kernels.rank_normalize(xt, *on_side)
    torch.cuda.current_stream().wait_stream(side)
    captured = [torch.zeros_like(t) for t in eager]
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        kernels.rank_normalize(xt, *captured)
    torch.cuda.synchronize()
    assert all(float(t.abs().sum()) == 0.0 for t in captured)            # captured, not run
    g.replay()
    torch.cuda.synchronize()
    for k in range(4):
        want = eager[k].cpu().numpy()
        for other, what in ((again, "second launch"), (on_side, "second stream"), (captured, "graph replay")):
            assert C.same_bits(other[k].cpu().numpy(), want), "%s: %s" % (what, NAMES[k])
    first = diagnostics.rank_diagnostics_all(xt, details=True)
    _tuple_bits_equal(diagnostics.rank_diagnostics_all(xt, details=True), first, "two calls in a row")


def test_fused_chains_diagnose_keeps_its_results_and_takes_the_keyword(gpu):
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    rng = np.random.RandomState(1)
    X = rng.rand(100, 1)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    chains = FusedBNNChains.for_dataset(X, y, 4, burn_in_steps=20, device=gpu)
    chains.steps(40)
    t = chains.collect(12, every=2)
    assert tuple(t.shape)[:2] == (4, 12)
    P = int(t.shape[2])
    # the keyword absent: what chain_diagnostics_all gives, bit for bit
    rhat, ess = chains.diagnose(t)
    ref_rhat, ref_ess = diagnostics.chain_diagnostics_all(t)
    assert C.same_bits(rhat.cpu().numpy(), ref_rhat.cpu().numpy()) and torch.equal(ess, ref_ess)
    four = chains.diagnose(t, details=True)
    assert len(four) == 4 and C.same_bits(four[0].cpu().numpy(), ref_rhat.cpu().numpy()) and torch.equal(four[1], ref_ess)
    # the keyword: three tensors, finite where the parameter is not degenerate
    got = chains.diagnose(t, rank_normalized=True)
    assert len(got) == 3 and [g.dtype for g in got] == [torch.float64, torch.int64, torch.int64]
    assert all(g.shape == (P,) and g.is_cuda for g in got)
    _tuple_bits_equal(got, diagnostics.rank_diagnostics_all(t), "diagnose(rank_normalized=True)")
    detailed = chains.diagnose(t, details=True, rank_normalized=True)
    assert isinstance(detailed, rank.RankDiagnostics)
    alive = torch.isfinite(ref_rhat)
    assert int(alive.sum()) > P // 2
    assert bool(torch.isfinite(got[0][alive]).all()) and bool((got[1][alive] > 0).all()) and bool((got[2][alive] > 0).all())
    print("4 chains x 12 samples x %d parameters: rank R-hat %.3f..%.3f, bulk ESS %d..%d, tail ESS %d..%d" % (
        P, float(got[0][alive].min()), float(got[0][alive].max()), int(got[1][alive].min()), int(got[1][alive].max()),
        int(got[2][alive].min()), int(got[2][alive].max())))
