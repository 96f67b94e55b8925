"""The chain diagnostics kernels (csrc/sgmcmc_kernels.hip, which holds the ``[boundary]`` group of include/sgmcmc_hip.h apart
from the sampler steps; K4's operator is ``MomentsOp`` in csrc/sgmcmc_device.hpp), each called
directly through ``pysgmcmc_amd.kernels`` in f32 and f64 and compared with a float64 reference:

- K4 ``moments_update``: bit-equal to the C oracle's Welford at every size, alignment and launch geometry, and within a
  first-order bound of a two-pass fp64 mean and variance on samples whose |mean| reaches 1e3 sd;
- K6 ``summary``: sum and sum of squares against ``math.fsum``, min and max bit-equal to numpy's (NaN included), at the
  sizes where the block count, the 1024-block cap and the last wave change;
- K7 ``step_stats_finish``: exact sums of hand-written dyadic records at every loop split, up to the workspace's capacity;
- ``rhat_pack`` / ``rhat_finish``: layout, padding, refusals, pitch, shards and the K6 summary, bit-equal to the oracle;
- the R-hat the library hands out (``RhatExchange`` on local chains: the pack, sum and finish of ``cross_chain_rhat``)
  against the fp64 formula on the kernel's own moments and against ``oracle.gelman_rubin`` of the samples, at
  |mean| / sd in {0, 1e2, 1e3, 1e4}, where a sum-form B in f32 cancels.

Every bar is written at its assert in the unit roundoff ``u`` of the dtype it is computed in. Output buffers sit between NaN
(or sentinel) guards that must survive; inputs sit between NaN guards, so a read past the end shows as NaN."""
import math

import numpy as np
import pytest
import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd._lib import SgmcmcLibraryError, lib

pytestmark = pytest.mark.gpu

NAN = float("nan")
DTS = [torch.float32, torch.float64]
NPT = {torch.float32: np.float32, torch.float64: np.float64}
UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}
UNIT = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
U64 = 2.0 ** -53
PAD = 16                                   # guard elements either side (64 / 128 bytes: the view stays 16-byte aligned)

_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Largest error per kernel, dtype and output as a fraction of its bar (shown with ``-s``)."""
    yield
    for key in sorted(_WORST):
        print("bar fraction %-40s %.3g" % ("/".join(key), _WORST[key]))


def _check(key, got, ref, bar, what):
    got, ref, bar = [np.broadcast_to(np.asarray(a, np.float64), np.shape(got)).ravel() for a in (got, ref, bar)]
    err = np.abs(got - ref)
    ok = err <= bar                                   # NaN anywhere: not ok
    if got.size:
        frac = float(np.max(np.divide(err, bar, out=np.zeros_like(err), where=bar > 0)))
        _WORST[key] = max(_WORST.get(key, 0.0), frac)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError("%s: %d of %d outside the bar; first at %d: got %r ref %r bar %r"
                             % (what, int((~ok).sum()), got.size, i, got[i], ref[i], bar[i]))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype])


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, "%s: %d elements differ, first at %d: %r vs %r" % (what, bad.size, bad[0], got.flat[bad[0]],
                                                                           want.flat[bad[0]])


def _guarded(values, dt, gpu, offset=0, fill=NAN):
    """``values`` on the device between ``PAD + offset`` and ``PAD`` guard elements of ``fill``: (buffer, view)."""
    values = np.asarray(values, NPT[dt])
    n = values.size
    buf = torch.full((n + 2 * PAD + offset,), fill, dtype=dt, device=gpu)
    view = buf[PAD + offset:PAD + offset + n]
    if n:
        view.copy_(torch.from_numpy(np.ascontiguousarray(values)))
    return buf, view


def _guards_hold(buf, n, what, offset=0, fill=NAN):
    h = buf.cpu().numpy()
    guards = np.concatenate([h[:PAD + offset], h[PAD + offset + n:]])
    _same_bits(guards, np.full(guards.size, fill, h.dtype), what + " guards")


def _raises_einval(call, match):
    with pytest.raises(SgmcmcLibraryError, match=match):
        call()


# ------------------------------------------------------------------------------------------------------------------
# K4 moments_update
# ------------------------------------------------------------------------------------------------------------------

GEOMETRIES = [None, dict(quads_per_thread=1), dict(quads_per_thread=2), dict(quads_per_thread=4), dict(max_blocks=3),
              dict(block_threads=64, quads_per_thread=2, max_blocks=2), dict(quads_per_thread=4, nontemporal=1)]
K4_SIZES = [1, 2, 3, 4, 5, 1023, 1024, 1025, 70001, 4 * 1024 * 1024 + 3]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", K4_SIZES)
@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
def test_moments_update_is_the_oracle_welford_at_every_geometry(gpu, oracle, dt, n, offset):
    """Five updates (counts 1..5: the count-1 and count-2 edges included) from a non-zero state, at every launch geometry;
    ``offset1`` views fail ``aligned16`` and take the scalar path. Every geometry gives the oracle's bits."""
    npt = NPT[dt]
    rng = np.random.default_rng(n + 7 * offset)
    mean0 = rng.normal(size=n).astype(npt)
    m20 = np.abs(rng.normal(size=n)).astype(npt)
    xs = (rng.normal(size=(5, n)) * 2.0 + 0.5).astype(npt)
    want_mean, want_m2 = mean0.copy(), m20.copy()
    for c in range(1, 6):
        oracle.c_moments_update(xs[c - 1], want_mean, want_m2, c)
    thetas = [_guarded(x, dt, gpu, offset) for x in xs]
    for geo in GEOMETRIES:
        launch = None if geo is None else kernels.LaunchConfig(**geo)
        mbuf, mean = _guarded(mean0, dt, gpu, offset)
        m2buf, m2 = _guarded(m20, dt, gpu, offset)
        for c in range(1, 6):
            kernels.moments_update(thetas[c - 1][1], mean, m2, c, launch=launch)
        what = "K4 n=%d %s %s" % (n, "offset" if offset else "aligned", geo)
        _same_bits(mean.cpu().numpy(), want_mean, what + " mean")
        _same_bits(m2.cpu().numpy(), want_m2, what + " m2")
        _guards_hold(mbuf, n, what + " mean", offset)
        _guards_hold(m2buf, n, what + " m2", offset)
    for buf, _ in thetas:
        _guards_hold(buf, n, "K4 theta (read only)", offset)


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
def test_moments_update_against_two_pass_fp64(gpu, dt):
    """C = 64 samples per parameter, |mean| / sd in {0, 1, 1e2, 1e3} and sd from 1e-3 to 1e3. First-order bounds of
    Welford in T, with X = max |x| and D = max |x - mean| per parameter: mean within C u X, m2 / (C - 1) within
    C u D (X + D) of the two-pass fp64 mean and unbiased variance of the same (T-rounded) samples."""
    npt, u = NPT[dt], UNIT[dt]
    n, C = 4099, 64
    rng = np.random.default_rng(3)
    r = np.array([0.0, 1.0, 1e2, 1e3])[np.arange(n) % 4] * np.sign(rng.normal(size=n))
    sd = 10.0 ** ((np.arange(n) // 4) % 7 - 3)
    x = (r * sd + sd * rng.normal(size=(C, n))).astype(npt)
    xd = torch.from_numpy(x).to(gpu)
    mean = torch.zeros(n, dtype=dt, device=gpu)
    m2 = torch.zeros(n, dtype=dt, device=gpu)
    for t in range(C):
        kernels.moments_update(xd[t], mean, m2, t + 1)
    x64 = x.astype(np.float64)
    mu = x64.mean(axis=0)
    var = ((x64 - mu) ** 2).sum(axis=0) / (C - 1)
    X, D = np.abs(x64).max(axis=0), np.abs(x64 - mu).max(axis=0)
    key = "f32" if dt == torch.float32 else "f64"
    _check(("K4", key, "mean"), mean.cpu().numpy(), mu, C * u * X, "K4 mean vs two-pass fp64")
    _check(("K4", key, "var"), m2.cpu().numpy().astype(np.float64) / (C - 1), var, C * u * D * (X + D),
           "K4 variance vs two-pass fp64")


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
def test_moments_update_count_edges(gpu, oracle, dt):
    """A count T cannot hold: the step is 1 / (T)count, rounded twice (pinned: it is what the oracle does, and it is not
    the correctly rounded 1 / count). count 0 is refused and writes nothing; n = 0 is a no-op."""
    npt = NPT[dt]
    count = 2 ** 24 + 3 if dt == torch.float32 else 2 ** 53 + 3
    step = npt(1) / npt(count)                          # (T)count = count + 1: a tie rounded to even
    assert step != npt(1.0 / count) or dt == torch.float64
    n = 37
    mbuf, mean = _guarded(np.zeros(n), dt, gpu)
    m2buf, m2 = _guarded(np.zeros(n), dt, gpu)
    theta = _guarded(np.ones(n), dt, gpu)[1]
    kernels.moments_update(theta, mean, m2, count)
    got = mean.cpu().numpy()
    _same_bits(got, np.full(n, step, npt), "K4 mean at count %d" % count)
    want_mean, want_m2 = np.zeros(n, npt), np.zeros(n, npt)
    oracle.c_moments_update(np.ones(n, npt), want_mean, want_m2, count)
    _same_bits(got, want_mean, "K4 mean vs oracle at count %d" % count)
    _same_bits(m2.cpu().numpy(), want_m2, "K4 m2 vs oracle at count %d" % count)
    # count 0: refused before any launch, nothing written
    before = (mbuf.cpu().numpy(), m2buf.cpu().numpy())
    _raises_einval(lambda: kernels.moments_update(theta, mean, m2, 0), "count == 0")
    _same_bits(mbuf.cpu().numpy(), before[0], "K4 mean after a refused call")
    _same_bits(m2buf.cpu().numpy(), before[1], "K4 m2 after a refused call")
    # n = 0: zero-length views of guarded buffers are left alone
    e_theta = _guarded(np.zeros(0), dt, gpu)[1]
    ebuf_m, e_mean = _guarded(np.zeros(0), dt, gpu)
    ebuf_v, e_m2 = _guarded(np.zeros(0), dt, gpu)
    kernels.moments_update(e_theta, e_mean, e_m2, 1)
    torch.cuda.synchronize()
    _guards_hold(ebuf_m, 0, "K4 n=0 mean")
    _guards_hold(ebuf_v, 0, "K4 n=0 m2")


# ------------------------------------------------------------------------------------------------------------------
# K6 summary
# ------------------------------------------------------------------------------------------------------------------

K6_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1, 3 * 1024 * 1024 + 7]
K6_KINDS = ["normal", "negative", "positive", "inf", "nan_first", "nan_mid", "nan_last"]


def _k6_data(kind, n, npt, rng):
    z = rng.normal(size=n)
    if kind == "negative":
        return (-(np.abs(z) + 0.5)).astype(npt)       # max < 0: the -inf identity must lose to every element
    if kind == "positive":
        return (np.abs(z) + 0.5).astype(npt)          # min > 0: the +inf identity must lose to every element
    x = z.astype(npt)
    if kind == "inf" and n >= 2:
        x[n // 3], x[n - 1 - n // 3] = np.inf, -np.inf
    elif kind.startswith("nan") and n:
        x[{"nan_first": 0, "nan_mid": n // 2, "nan_last": n - 1}[kind]] = np.nan
    return x


def _summary(x_dev, gpu):
    obuf = torch.full((4 + 2 * PAD,), NAN, dtype=torch.float64, device=gpu)
    out4 = obuf[PAD:PAD + 4]
    wsz = lib().sgmcmc_summary_workspace_bytes()
    wbuf = torch.full((wsz + 256,), 0xA5, dtype=torch.uint8, device=gpu)
    kernels.summary(x_dev, out4, wbuf[:wsz])
    _guards_hold(obuf, 4, "K6 out4")
    tail = wbuf[wsz:].cpu().numpy()
    assert (tail == 0xA5).all(), "K6 wrote past its workspace"
    return out4.cpu().numpy()


@pytest.mark.parametrize("kind", K6_KINDS)
@pytest.mark.parametrize("n", K6_SIZES)
@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
def test_summary_against_fsum_and_numpy(gpu, dt, n, kind):
    """Sum and sum of squares within n u64 sum|x| (resp. sum x^2) of math.fsum; min and max bit-equal to numpy's, NaN
    exactly when an element is NaN (at the first, a middle or the last index); two calls give the same bits. n = 0
    gives the identities {0, 0, +inf, -inf}, from an empty tensor too (whose pointer may be NULL). The input sits between
    NaN guards: a read past either end shows."""
    npt = NPT[dt]
    x = _k6_data(kind, n, npt, np.random.default_rng(n))
    _, xd = _guarded(x, dt, gpu)
    s = _summary(xd, gpu)
    _same_bits(_summary(xd, gpu), s, "K6 repeat")
    key = "f32" if dt == torch.float32 else "f64"
    if n == 0:
        _same_bits(s, np.array([0.0, 0.0, np.inf, -np.inf]), "K6 n=0")
        _same_bits(_summary(torch.empty(0, dtype=dt, device=gpu), gpu), s, "K6 of an empty tensor")
        return
    if kind.startswith("nan"):
        assert np.isnan(s).all(), s                   # every output, min and max included
        return
    x64 = x.astype(np.float64)
    _same_bits(s[2:], np.array([x64.min(), x64.max()]), "K6 min / max (%s, n=%d)" % (kind, n))
    if kind == "inf":
        if n >= 2:
            assert np.isnan(s[0]) and s[1] == np.inf, s
            return
    a = np.abs(x64)
    _check(("K6", key, "sum"), s[0], math.fsum(x64.tolist()), n * U64 * a.sum(), "K6 sum n=%d %s" % (n, kind))
    _check(("K6", key, "sumsq"), s[1], math.fsum((x64 * x64).tolist()), n * U64 * (a * a).sum(),
           "K6 sum of squares n=%d %s" % (n, kind))


# ------------------------------------------------------------------------------------------------------------------
# K7 step_stats_finish
# ------------------------------------------------------------------------------------------------------------------

K7_COUNTS = [1, 255, 256, 257, 2047, 2048, 2049, 2048 * 37 + 1000, 1 << 20]


def _k7(gpu, stats, nrec, rng):
    """Write ``nrec`` records of small dyadic values (sixteenths in [-64, 64]: every sum is exact in any order) into the
    workspace, NaN in the header's spare words and in every record past the count; returns the exact sums."""
    ws = stats.workspace.view(torch.float64)
    cap = ws.numel() // 4 - 1
    assert nrec <= cap
    recs = rng.integers(-1024, 1025, size=(nrec, 4))
    host = np.full(ws.numel(), np.nan)
    host[4:4 + 4 * nrec] = recs.ravel() / 16.0
    ws.copy_(torch.from_numpy(host))
    stats.workspace[:8].view(torch.int64).fill_(nrec)
    return recs.sum(axis=0) / 16.0


@pytest.mark.parametrize("nrec", K7_COUNTS)
def test_step_stats_finish_is_the_exact_sum_of_the_records(gpu, nrec):
    """Record counts at each split of the 8-way unrolled loop (2048 records per trip) and its 256-stride remainder, up
    to the 2^20 records the largest workspace holds. The result must equal the exact sum, bit for bit."""
    stats = kernels.StepStats(256 << 20, gpu)            # a 2^28-parameter launch: the workspace holds 2^20 records
    assert stats.workspace.numel() == ((1 << 20) + 1) * 32
    want = _k7(gpu, stats, nrec, np.random.default_rng(nrec))
    obuf = torch.full((4 + 2 * PAD,), NAN, dtype=torch.float64, device=gpu)
    stats.out = obuf[PAD:PAD + 4]
    kernels.step_stats_finish(stats)
    _same_bits(stats.out.cpu().numpy(), want, "K7 %d records" % nrec)
    _guards_hold(obuf, 4, "K7 out")


@pytest.mark.parametrize("n", [1, 5252, 1 << 20, 10_002_434])
def test_step_stats_finish_at_the_capacity_of_a_chains_workspace(gpu, n):
    """A chain's own StepStats(n) filled to the last record its workspace holds."""
    stats = kernels.StepStats(n, gpu)
    cap = stats.workspace.numel() // 32 - 1
    assert cap >= kernels.step_stats_records(n, kernels.LaunchConfig(block_threads=64))
    want = _k7(gpu, stats, cap, np.random.default_rng(n))
    kernels.step_stats_finish(stats)
    _same_bits(stats.out.cpu().numpy(), want, "K7 n=%d, %d records" % (n, cap))


# ------------------------------------------------------------------------------------------------------------------
# rhat_pack
# ------------------------------------------------------------------------------------------------------------------

def _shard_lens(n, s):
    """Shard lengths for n parameters in s shards: the tight ceil(n / s), RhatExchange's rounding to 4, and (one shard)
    a padded pitch."""
    L = (n + s - 1) // s
    L4 = (L + 3) // 4 * 4
    out = {L}
    if (s - 1) * L4 < n:
        out.add(L4)
    if s == 1:
        out.add(n + 5)
    return sorted(out)


def _pack_ref(mean, m2, count, s, L):
    """[mu | mu*mu | m2 * (1/(count-1))] in T, chunk-major, zero beyond n."""
    npt = mean.dtype.type
    n = mean.size
    inv = npt(1) / npt(count - 1)
    out = np.zeros((s, 3, L), npt)
    mu = np.zeros(s * L, npt)
    var = np.zeros(s * L, npt)
    mu[:n] = mean
    var[:n] = m2 * inv
    out[:, 0, :] = mu.reshape(s, L)
    out[:, 1, :] = (mu * mu).reshape(s, L)
    out[:, 2, :] = var.reshape(s, L)
    return out.ravel()


@pytest.mark.parametrize("n_shards", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [4096, 4099, 70001])
@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
def test_rhat_pack_layout(gpu, oracle, dt, n, n_shards):
    """Bit-equal to the layout computed in T with numpy, and to the oracle; padding reads +0.0 exactly."""
    npt = NPT[dt]
    rng = np.random.default_rng(n * n_shards)
    mean = (rng.normal(size=n) * 3.0).astype(npt)
    m2 = np.abs(rng.normal(size=n) * 50.0).astype(npt)
    md, vd = _guarded(mean, dt, gpu)[1], _guarded(m2, dt, gpu)[1]
    for count in (2, 3, 1000):
        for L in _shard_lens(n, n_shards):
            obuf, out3 = _guarded(np.zeros(3 * n_shards * L), dt, gpu)
            obuf.fill_(NAN)
            kernels.rhat_pack(md, vd, count, out3, n_shards, L)
            got = out3.cpu().numpy()
            what = "rhat_pack n=%d shards=%d L=%d count=%d" % (n, n_shards, L, count)
            _same_bits(got, _pack_ref(mean, m2, count, n_shards, L), what)
            _same_bits(got, oracle.c_rhat_pack(mean, m2, count, n_shards, L), what + " vs oracle")
            _guards_hold(obuf, 3 * n_shards * L, what)


@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
def test_rhat_pack_refusals(gpu, dt):
    """An empty last shard, shards that do not cover n, count < 2: refused, nothing written. count = 2 is accepted."""
    n = 10
    mean, m2 = _guarded(np.arange(n), dt, gpu)[1], _guarded(np.ones(n), dt, gpu)[1]
    cases = [(3, 5, 7, "no empty shard"),             # (3 - 1) * 5 >= 10: shard 2 would be empty
             (3, 3, 7, "no empty shard"),             # 3 * 3 < 10
             (1, n, 1, "count < 2"), (1, n, 0, "count < 2"), (2, 5, 1, "count < 2")]
    for s, L, count, match in cases:
        obuf, out3 = _guarded(np.zeros(3 * s * L), dt, gpu)
        obuf.fill_(NAN)
        _raises_einval(lambda: kernels.rhat_pack(mean, m2, count, out3, s, L), match)
        _guards_hold(obuf, 0, "refused rhat_pack s=%d L=%d count=%d" % (s, L, count), fill=NAN)
    obuf, out3 = _guarded(np.zeros(3 * n), dt, gpu)
    kernels.rhat_pack(mean, m2, 2, out3)
    assert torch.equal(out3[2 * n:], m2)                # m2 * (1 / 1)


# ------------------------------------------------------------------------------------------------------------------
# rhat_finish
# ------------------------------------------------------------------------------------------------------------------

def _chain_sums(m, cnt, n, npt, s=1, L=None, rng=None):
    """Synthetic per-chain moments of m chains, packed (oracle) and summed in T: the input of a finish."""
    L = n if L is None else L
    tot = np.zeros(3 * s * L, npt)
    for c in range(m):
        mean = (rng.normal(size=n) * 0.2).astype(npt)
        m2 = ((cnt - 1) * (0.5 + rng.random(n))).astype(npt)
        tot = tot + _pack_ref(mean, m2, cnt, s, L)
    return tot


def _rhat_formula(sum3, n, ld, m, cnt):
    """fp64 R-hat of the first n columns of [S_mean | S_sq | S_var] (pitch ld)."""
    S = np.asarray(sum3, np.float64)
    s_mean, s_sq, s_var = S[:n], S[ld:ld + n], S[2 * ld:2 * ld + n]
    W = s_var / m
    B = cnt * (s_sq - s_mean * s_mean / m) / (m - 1)
    return np.sqrt((W * (cnt - 1) / cnt + B / cnt) / W)


@pytest.mark.parametrize("cnt", [2, 3, 1000])
@pytest.mark.parametrize("m", [2, 3, 4, 8])
@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
def test_rhat_finish_pitch_summary_and_shards(gpu, oracle, dt, m, cnt):
    """ld > n with NaN in the gap, with and without the K6 summary (same R-hat bits), bit-equal to the oracle, within
    4 u of the fp64 formula on the same sums (centred chains: no cancellation); the summary equals the fp64 sum and max
    of that R-hat; a W = 0 parameter gives NaN and the summary's min and max say so. Finishing the shards of a sharded pack
    one by one gives the full finish's bits."""
    npt, u = NPT[dt], UNIT[dt]
    n, ld = 4099, 4099 + 13
    rng = np.random.default_rng(m * 1000 + cnt)
    tot = _chain_sums(m, cnt, n, npt, rng=rng)
    pitched = np.full(3 * ld, np.nan, npt)
    for r in range(3):
        pitched[r * ld:r * ld + n] = tot[r * n:(r + 1) * n]
    _, sd = _guarded(pitched, dt, gpu)
    rbuf, rhat = _guarded(np.zeros(n), dt, gpu)
    rbuf.fill_(NAN)
    kernels.rhat_finish(sd, n, m, cnt, rhat, ld=ld)
    plain = rhat.cpu().numpy()
    _guards_hold(rbuf, n, "rhat_finish")
    rbuf2, rhat2 = _guarded(np.zeros(n), dt, gpu)
    obuf = torch.full((4 + 2 * PAD,), NAN, dtype=torch.float64, device=gpu)
    kernels.rhat_finish(sd, n, m, cnt, rhat2, obuf[PAD:PAD + 4], kernels.summary_workspace(gpu), ld=ld)
    _guards_hold(rbuf2, n, "rhat_finish + summary")
    _guards_hold(obuf, 4, "rhat_finish summary")
    _same_bits(rhat2.cpu().numpy(), plain, "R-hat with and without the summary")
    _same_bits(plain, oracle.c_rhat_finish(pitched, m, cnt, n=n, ld=ld), "R-hat vs oracle")
    key = "f32" if dt == torch.float32 else "f64"
    want = _rhat_formula(pitched, n, ld, m, cnt)
    _check(("rhat_finish", key, "rhat"), plain, want, 4 * u * want, "R-hat vs fp64 formula")
    s4 = obuf[PAD:PAD + 4].cpu().numpy()
    r64 = plain.astype(np.float64)
    _check(("rhat_finish", key, "summary sum"), s4[0], math.fsum(r64.tolist()), n * U64 * r64.sum(), "summary sum")
    _check(("rhat_finish", key, "summary sumsq"), s4[1], math.fsum((r64 * r64).tolist()), n * U64 * (r64 * r64).sum(),
           "summary sum of squares")
    _same_bits(s4[2:], np.array([r64.min(), r64.max()]), "summary min / max")
    # W = 0 at one parameter (a chain that never moved): R-hat 0/0 = NaN, and the summary's min and max are NaN
    flat = pitched.copy()
    j = n // 2
    flat[j], flat[ld + j], flat[2 * ld + j] = npt(m), npt(m), npt(0)
    _, fd = _guarded(flat, dt, gpu)
    out4 = torch.empty(4, dtype=torch.float64, device=gpu)
    kernels.rhat_finish(fd, n, m, cnt, rhat2, out4, kernels.summary_workspace(gpu), ld=ld)
    assert np.isnan(rhat2[j].item()) and np.isnan(out4.cpu().numpy()).all()
    # shards: the full finish of a plain pack == the finishes of the shards of the sharded pack, concatenated
    for s in (2, 3, 8):
        for L in _shard_lens(n, s):
            rng = np.random.default_rng(m * 1000 + cnt)
            tot_s = _chain_sums(m, cnt, n, npt, s, L, rng)
            parts = []
            for k in range(s):
                nv = min(L, n - k * L)
                shard = torch.from_numpy(tot_s[k * 3 * L:(k + 1) * 3 * L]).to(gpu)
                out = torch.empty(L, dtype=dt, device=gpu)
                kernels.rhat_finish(shard, nv, m, cnt, out, ld=L)
                parts.append(out[:nv].cpu().numpy())
            _same_bits(np.concatenate(parts), plain, "sharded finish s=%d L=%d" % (s, L))


# ------------------------------------------------------------------------------------------------------------------
# The library's R-hat: K4 moments -> pack -> sum over chains -> finish, on chains whose |mean| is far from 0
# ------------------------------------------------------------------------------------------------------------------

RATIOS = [0.0, 1e2, 1e3, 1e4]
M_CHAINS, N_SAMPLES, N_PARAMS = 4, 1000, 2000


def _chains(ratio, npt):
    """4 chains x 1000 samples x 2000 parameters: within-chain sd 1, chain means ratio + 0.1 N(0, 1)."""
    rng = np.random.default_rng(int(ratio) + 11)
    off = rng.normal(size=(M_CHAINS, 1, N_PARAMS)) * 0.1
    return (ratio + off + rng.normal(size=(M_CHAINS, N_SAMPLES, N_PARAMS))).astype(npt)


def _library_rhat(gpu, dt, chains):
    from pysgmcmc_amd.diagnostics.sampler_diagnostics import ChainMoments, RhatExchange
    xd = torch.from_numpy(chains).to(gpu)
    moms = [ChainMoments(N_PARAMS, gpu, dtype=dt) for _ in range(M_CHAINS)]
    for c, mom in enumerate(moms):
        for t in range(N_SAMPLES):
            mom.update(xd[c, t])
    ex = RhatExchange(N_PARAMS, gpu, dtype=dt, mode="allreduce")      # local chains, no process group
    ex.start(moms)
    rhat, summ = ex.finish(with_summary=True)
    assert rhat.dtype == dt and rhat.numel() == N_PARAMS
    return rhat.cpu().numpy(), summ, moms


def _finish_bar(ratio):
    """The exchange is f64: B = cnt (S_sq - S_mean^2 / m) / (m - 1) loses ~u64 (|mean| / sd)^2 of W to cancellation."""
    return 8 * U64 * (1 + ratio * ratio)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
def test_library_rhat_finish_only(gpu, dt, ratio):
    """R-hat from the kernel's own moments against the fp64 formula evaluated on those same moments. f32: within 1 ulp
    (the f64 exchange of f32 moments is exact to far below half an ulp, then one rounding); f64: within 8 u64 (1 + r^2)
    for r = |mean| / sd. A sum-form B in f32 is off by ~0.2 at r = 1e3."""
    npt = NPT[dt]
    got, summ, moms = _library_rhat(gpu, dt, _chains(ratio, npt))
    M = np.stack([mom.mean.cpu().numpy().astype(np.float64) for mom in moms])
    V = np.stack([mom.m2.cpu().numpy().astype(np.float64) for mom in moms]) / (N_SAMPLES - 1)
    B = N_SAMPLES * M.var(axis=0, ddof=1)
    W = V.mean(axis=0)
    want = np.sqrt((W * (N_SAMPLES - 1) / N_SAMPLES + B / N_SAMPLES) / W)
    if dt == torch.float32:
        bar = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    else:
        bar = np.full(want.shape, _finish_bar(ratio))
    key = "f32" if dt == torch.float32 else "f64"
    _check(("rhat finish-only", key, "r=%g" % ratio), got, want, bar, "R-hat (finish only) at |mean|/sd = %g" % ratio)
    assert np.isfinite(summ["max"]) and abs(summ["max"] - want.max()) <= bar.max()


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("dt", DTS, ids=["f32", "f64"])
def test_library_rhat_end_to_end(gpu, oracle, dt, ratio):
    """R-hat against oracle.gelman_rubin of the samples: within 3 u_T (1 + r) (Welford in T: the chain means drift by
    ~u_T |mean| per update) + 8 u64 (1 + r^2) (the f64 finish). With the C oracle, which the kernels equal bit for bit, on these
    samples: f32 1.5e-3 at r = 1e4 (bar 1.8e-3), f64 3.3e-8 (bar 8.9e-8). At r = 1e3 in f32 it must also match
    gelman_rubin_from_chains, the library's own formula on explicit chains."""
    from pysgmcmc_amd.diagnostics.sampler_diagnostics import gelman_rubin_from_chains
    npt, u = NPT[dt], UNIT[dt]
    chains = _chains(ratio, npt)
    got, summ, _ = _library_rhat(gpu, dt, chains)
    want = oracle.gelman_rubin(chains)
    bar = 3 * u * (1 + ratio) + _finish_bar(ratio)
    key = "f32" if dt == torch.float32 else "f64"
    _check(("rhat end-to-end", key, "r=%g" % ratio), got, want, np.full(want.shape, bar),
           "R-hat (end to end) at |mean|/sd = %g" % ratio)
    assert abs(summ["max"] - want.max()) <= bar and abs(summ["mean"] - want.mean()) <= bar
    if dt == torch.float32 and ratio == 1e3:
        ref = gelman_rubin_from_chains(torch.from_numpy(chains).to(gpu)).cpu().numpy()
        _check(("rhat end-to-end", key, "vs gelman_rubin_from_chains"), got, ref, np.full(ref.shape, bar),
               "R-hat vs gelman_rubin_from_chains")


def test_reduce_scatter_exchange_needs_a_process_group(gpu):
    """The sharded exchange has no local form: without a process group it is refused when built."""
    from pysgmcmc_amd.diagnostics.sampler_diagnostics import RhatExchange
    for dt in DTS:
        with pytest.raises(RuntimeError, match="process group"):
            RhatExchange(N_PARAMS, gpu, dtype=dt, mode="reduce_scatter")
