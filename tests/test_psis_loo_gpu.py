"""K19, PSIS-LOO of a device matrix of pointwise log densities (csrc/sgmcmc_psis.hip, include/sgmcmc_hip_psis.h), and its
public front ends (``kernels.psis_loo``, ``diagnostics.psis_loo``, ``models.loo_score``, ``FusedBNNChains.loo``) against the
host statement ``diagnostics.psis.psis_loo_host`` on a copy of the same ``loglik``.

Exact: ``n_tail`` everywhere, ``khat = +inf`` where the host says so, the placement of NaN, ``row_lppd`` against K13's bits,
repeated runs, a column alone against the column in a batch, pitches, canaries, optional outputs, graph replay, and
``summary`` as the stated tree of the device's own rows. Within a measured bound (psis_cases.py, profiles/psis_loo.txt):
``khat``, ``elpd_loo`` and ``log_weights`` against the host, which differ through the vendor's exp / log / log1p / expm1
against numpy's; the tests allow 4 times the largest difference measured over all the cases here."""
import numpy as np
import pytest
import torch

from pysgmcmc_amd import diagnostics, kernels, models
from pysgmcmc_amd.diagnostics import psis

import psis_cases as C

pytestmark = pytest.mark.gpu

F64 = torch.float64
CANARY = -77.25
EPS = np.finfo(np.float64).eps


class Outputs(object):
    """Every output of one call inside a canary-filled buffer of its own; loglik inside a wider NaN-filled one."""

    def __init__(self, ll, dev, pad=3, row_lppd=True, weights=True, summary=True):
        S, n = ll.shape
        self.S, self.n = S, n
        self.buf = torch.full((S + 1, n + pad), float("nan"), dtype=F64, device=dev)
        self.buf[:S, :n] = torch.as_tensor(ll, dtype=F64, device=dev)
        self.loglik = self.buf[:S, :n]
        vec = lambda dt, fill: torch.full((n + 2,), fill, dtype=dt, device=dev)
        self.full = dict(elpd_loo=vec(F64, CANARY), khat=vec(F64, CANARY), n_tail=vec(torch.int32, -77),
                         row_lppd=vec(F64, CANARY), log_weights=torch.full((S + 1, n + pad), CANARY, dtype=F64, device=dev),
                         summary=torch.full((6,), CANARY, dtype=F64, device=dev))
        self.on = dict(elpd_loo=True, khat=True, n_tail=True, row_lppd=row_lppd, log_weights=weights, summary=summary)

    def view(self, name):
        if not self.on[name]:
            return None
        f = self.full[name]
        if name == "log_weights":
            return f[:self.S, :self.n]
        return f[1:5] if name == "summary" else f[1:self.n + 1]

    def run(self, r_eff=1.0):
        kernels.psis_loo(self.loglik, r_eff, **{name: self.view(name) for name in self.full})
        return self

    def result(self):
        """The outputs as numpy arrays (None where off), after the canaries are checked."""
        out = {}
        for name, f in self.full.items():
            h = f.cpu().numpy()
            fill = -77 if name == "n_tail" else CANARY
            if not self.on[name]:
                assert (h == fill).all(), "%s was not passed and was written" % name
                out[name] = None
            elif name == "log_weights":
                assert (h[self.S:] == fill).all() and (h[:, self.n:] == fill).all(), "a canary around log_weights was overwritten"
                out[name] = h[:self.S, :self.n].copy()
            elif name == "summary":
                assert h[0] == fill and h[5] == fill, "a canary around summary was overwritten"
                out[name] = h[1:5].copy()
            else:
                assert h[0] == fill and h[self.n + 1] == fill, "a canary around %s was overwritten" % name
                out[name] = h[1:self.n + 1].copy()
        assert torch.isnan(self.buf[self.S:]).all() and torch.isnan(self.buf[:, self.n:]).all(), "loglik's pitch gap was written"
        return out


def _device(ll, dev, r_eff=1.0, **kw):
    return Outputs(ll, dev, **kw).run(r_eff).result()


def _assert_same_bits(a, b, what):
    for name in a:
        if a[name] is None or b[name] is None:
            continue
        if name == "n_tail":
            assert np.array_equal(a[name], b[name]), "%s: n_tail" % what
        else:
            assert C.same_bits(a[name], b[name]), "%s: %s differs in its bits" % (what, name)


def _assert_against_host(got, ll, r_eff, what):
    """Exact where the statement is exact, within 4 times the measured bound elsewhere. Returns the measured differences."""
    ref = C.host(ll, r_eff)
    d_khat, d_elpd, d_logw = C.compare(got, ref)
    S = ll.shape[0]
    d_lppd = C.rel_or_abs(got["row_lppd"], ref["row_lppd"]) if got["row_lppd"] is not None else 0.0
    print("%s r_eff %.1f: |d khat| %.3e  d elpd_loo %.3e  d log_weights %.3e  d row_lppd %.3e" % (
        what, r_eff, d_khat, d_elpd, d_logw, d_lppd))
    assert max(d_khat, d_elpd, d_logw) <= C.SAME_STATEMENT_LIMIT, "%s: the two sides do not execute the same statement" % what
    assert d_khat <= C.MARGIN * C.KHAT_ABS_MEASURED, "%s: khat is %.3e from the host" % (what, d_khat)
    assert d_elpd <= C.MARGIN * C.ELPD_REL_MEASURED, "%s: elpd_loo is %.3e from the host" % (what, d_elpd)
    assert d_logw <= C.MARGIN * C.LOGW_REL_MEASURED, "%s: log_weights are %.3e from the host" % (what, d_logw)
    # row_lppd: S terms of one ulp each and S roundings of the running sum that may fall differently, then two logs
    assert d_lppd <= (S + 8) * EPS, "%s: row_lppd is %.3e from the host" % (what, d_lppd)
    if got["row_lppd"] is not None:
        assert np.array_equal(np.isnan(got["row_lppd"]), ref["n_tail"] < 0)
    return d_khat, d_elpd, d_logw


@pytest.mark.parametrize("S", C.DRAWS)
def test_every_pattern_at_every_shape(gpu, S):
    for n_rows in C.rows_for(S):
        ll = C.matrix(S, n_rows, seed=S % 7, first=n_rows)
        out = Outputs(ll, gpu)
        for r_eff in C.R_EFFS:
            got = out.run(r_eff).result()
            _assert_against_host(got, ll, r_eff, "S = %d, n_rows = %d" % (S, n_rows))


def test_n_tail_driven_to_four_by_ties_alone(gpu):
    S = 100
    rng = np.random.RandomState(21)
    ll = np.stack([C.ties_at_cut(S, rng, above) for above in (4, 5, 3, 19, 12)], axis=1)
    got = _device(ll, gpu)
    assert list(got["n_tail"]) == [4, 5, 3, 19, 12]
    assert list(np.isposinf(got["khat"])) == [True, False, True, False, False]
    _assert_against_host(got, ll, 1.0, "ties at the cut")


def test_underflow_and_constant_columns(gpu):
    S = 1000
    rng = np.random.RandomState(22)
    ll = np.stack([C.underflow(S, rng), C.constant(S, rng), C.underflow(S, rng), C.gaussian(S, rng)], axis=1)
    got = _device(ll, gpu)
    assert got["n_tail"][0] == got["n_tail"][2] == C.few_above(S) and got["n_tail"][1] == 0
    assert np.isposinf(got["khat"][1]) and np.isfinite(got["khat"][[0, 2, 3]]).all()
    assert np.abs(got["log_weights"][:, 1] + np.log(S)).max() <= 4 * EPS * np.log(S)
    _assert_against_host(got, ll, 1.0, "underflow and constant")


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_nonfinite_column_between_healthy_ones(gpu, poison):
    ll = C.matrix(257, 7, seed=3)
    clean = _device(ll, gpu)
    bad = ll.copy()
    bad[200, 3] = poison
    got = _device(bad, gpu)
    keep = [0, 1, 2, 4, 5, 6]
    assert got["n_tail"][3] == -1 and np.isnan(got["log_weights"][:, 3]).all()
    for name in ("elpd_loo", "khat", "row_lppd"):
        assert np.isnan(got[name][3]), name
        assert C.same_bits(got[name][keep], clean[name][keep]), name
    assert np.array_equal(got["n_tail"][keep], clean["n_tail"][keep])
    assert C.same_bits(got["log_weights"][:, keep], clean["log_weights"][:, keep])
    assert np.isnan(got["summary"][0]) and np.isnan(got["summary"][1]) and got["summary"][3] == 1.0
    assert got["summary"][2] == float((got["khat"] > 0.7).sum())
    _assert_against_host(got, bad, 1.0, "a %s column" % poison)


@pytest.mark.parametrize("S", [25, 257, 4096])
def test_bits_do_not_depend_on_the_call(gpu, S):
    """A second run, a column alone against the batch, dense against padded pitches, optional outputs on or off."""
    n_rows = 67 if S < 4096 else 5
    ll = C.matrix(S, n_rows, seed=5)
    first = Outputs(ll, gpu)
    a = first.run(0.3).result()
    b = first.run(0.3).result()
    _assert_same_bits(a, b, "a second run")
    for r in (0, n_rows // 2, n_rows - 1):
        one = _device(ll[:, r:r + 1], gpu, 0.3, pad=0)
        for name in ("elpd_loo", "khat", "n_tail", "row_lppd"):
            assert C.same_bits(one[name].astype(np.float64), a[name][r:r + 1].astype(np.float64)), "column %d alone: %s" % (r, name)
        assert C.same_bits(one["log_weights"][:, 0], a["log_weights"][:, r]), "column %d alone: log_weights" % r
    _assert_same_bits(_device(ll, gpu, 0.3, pad=0), a, "dense pitches")
    _assert_same_bits(_device(ll, gpu, 0.3, pad=61), a, "wide pitches")
    for row_lppd, weights, summary in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        got = _device(ll, gpu, 0.3, row_lppd=row_lppd, weights=weights, summary=summary)
        _assert_same_bits(got, a, "optional outputs %s" % ((row_lppd, weights, summary),))
        if summary:                                       # the row_lppd sum is formed from the column
            assert C.same_bits(got["summary"], a["summary"])


def test_allocated_outputs_and_no_rows(gpu):
    ll = C.matrix(100, 9, seed=8)
    want = _device(ll, gpu)
    elpd, khat, n_tail = kernels.psis_loo(torch.as_tensor(ll, device=gpu))
    assert elpd.dtype == F64 and khat.dtype == F64 and n_tail.dtype == torch.int32 and tuple(n_tail.shape) == (9,)
    assert C.same_bits(elpd.cpu().numpy(), want["elpd_loo"]) and C.same_bits(khat.cpu().numpy(), want["khat"])
    assert np.array_equal(n_tail.cpu().numpy(), want["n_tail"])
    elpd, khat, n_tail = kernels.psis_loo(torch.empty(100, 0, dtype=F64, device=gpu))
    assert elpd.numel() == khat.numel() == n_tail.numel() == 0
    from pysgmcmc_amd._lib import SgmcmcLibraryError
    with pytest.raises(SgmcmcLibraryError, match=r"psis_loo: elpd_loo is NULL"):       # the library's own check, by name
        rc = kernels.lib().sgmcmc_psis_loo(torch.as_tensor(ll, device=gpu).data_ptr(), 9, 100, 9, 1.0, None, None, None, None,
                                           None, 0, None, None)
        kernels.check(rc, "sgmcmc_psis_loo")


def test_summary_is_the_tree_of_the_devices_rows(gpu):
    ll = C.matrix(64, 700, seed=9)
    ll[5, 123] = np.nan
    got = _device(ll, gpu)
    assert np.isnan(got["summary"][0]) and np.isnan(got["summary"][1])
    assert got["summary"][2] == float((got["khat"] > 0.7).sum()) and got["summary"][3] == 1.0
    ll[5, 123] = 0.0
    got = _device(ll, gpu)
    assert C.same_bits(got["summary"][0], psis.fixed_sum(got["elpd_loo"]))
    assert C.same_bits(got["summary"][1], psis.fixed_sum(got["row_lppd"]))
    assert got["summary"][2] == float((got["khat"] > 0.7).sum()) and got["summary"][3] == 0.0


def test_graph_capture_and_replay(gpu):
    ll = C.matrix(257, 13, seed=10)
    eager = _device(ll, gpu, 2.5)
    out = Outputs(ll, gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        out.run(2.5)                                      # warm-up on the side stream, as capture wants
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    for name, f in out.full.items():
        f.fill_(-77 if name == "n_tail" else CANARY)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out.run(2.5)
    torch.cuda.synchronize()
    assert float((out.full["elpd_loo"] != CANARY).sum()) == 0.0   # captured, not run
    g.replay()
    torch.cuda.synchronize()
    _assert_same_bits(out.result(), eager, "the replayed graph")


def _small_net_case(dev, dtype=torch.float32):
    sizes = [2, 5, 1]
    P = kernels._bnn_n_params(sizes)
    g = torch.Generator().manual_seed(7)
    trace = (0.7 * torch.randn(4, 25, P, generator=g)).to(dtype).to(dev)
    X = torch.randn(23, 2, generator=g).to(dtype).to(dev)
    y = torch.randn(23, generator=g).to(dtype).to(dev)
    return sizes, trace, X, y


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_row_lppd_has_the_bits_of_the_score_kernel(gpu, dtype):
    sizes, trace, X, y = _small_net_case(gpu, dtype)
    score = models.heldout_score(trace, X, y, sizes, pointwise=True)
    assert tuple(score.loglik.shape) == (100, 23)
    row_lppd = torch.empty(23, dtype=F64, device=gpu)
    kernels.psis_loo(score.loglik, row_lppd=row_lppd)
    assert C.same_bits(row_lppd.cpu().numpy(), score.row_lppd.cpu().numpy())


def _assert_loo_result(got, loglik, r_eff, weights, what):
    ll = loglik.cpu().numpy()
    n_rows = ll.shape[1]
    rows = dict(elpd_loo=got.row_elpd.cpu().numpy(), khat=got.khat.cpu().numpy(), n_tail=got.n_tail.cpu().numpy(),
                row_lppd=got.row_lppd.cpu().numpy(), log_weights=got.log_weights.cpu().numpy() if weights else None)
    _assert_against_host(rows, ll, r_eff, what)
    assert (got.log_weights is not None) == weights
    for name in ("elpd_loo", "p_loo", "se", "lppd", "n_bad"):
        v = getattr(got, name)
        assert v.dim() == 0 and v.dtype == F64 and v.device == loglik.device, name
    assert C.same_bits(float(got.elpd_loo), psis.fixed_sum(rows["elpd_loo"]))
    assert C.same_bits(float(got.lppd), psis.fixed_sum(rows["row_lppd"]))
    assert float(got.p_loo) == float(got.lppd) - float(got.elpd_loo)
    want_se = np.sqrt(n_rows * np.var(rows["elpd_loo"]))
    assert abs(float(got.se) - want_se) <= (n_rows + 8) * EPS * want_se + 1e-300
    assert float(got.n_bad) == float((rows["khat"] > 0.7).sum())


def test_loo_score_end_to_end(gpu):
    sizes, trace, X, y = _small_net_case(gpu)
    loglik = models.heldout_score(trace, X, y, sizes, pointwise=True).loglik
    for r_eff, weights in ((1.0, False), (0.3, True)):
        got = models.loo_score(trace, X, y, sizes, r_eff=r_eff, weights=weights)
        assert isinstance(got, diagnostics.PsisLoo) and got.thinning == 1
        _assert_loo_result(got, loglik, r_eff, weights, "loo_score")
        direct = diagnostics.psis_loo(loglik, r_eff, weights)
        assert C.same_bits(direct.row_elpd.cpu().numpy(), got.row_elpd.cpu().numpy())
    # a particle matrix, and a list of chains
    flat = models.loo_score(trace.reshape(100, -1), X, y, sizes)
    listed = models.loo_score([c for c in trace], X, y, sizes)
    one = models.loo_score(trace, X, y, sizes)
    assert C.same_bits(flat.row_elpd.cpu().numpy(), one.row_elpd.cpu().numpy())
    assert C.same_bits(listed.row_elpd.cpu().numpy(), one.row_elpd.cpu().numpy())


def test_loo_score_strides_a_long_trace(gpu):
    sizes = [2, 5, 1]
    P = kernels._bnn_n_params(sizes)
    g = torch.Generator().manual_seed(8)
    trace = (0.5 * torch.randn(3, 4100, P, generator=g)).to(gpu)
    X, y = torch.randn(4, 2, generator=g).to(gpu), torch.randn(4, generator=g).to(gpu)
    got = models.loo_score(trace, X, y, sizes)
    assert got.thinning == 2                              # 3 * 4100 > 8192 >= 3 * 2050
    want = models.loo_score(trace[:, ::2].contiguous(), X, y, sizes)
    assert want.thinning == 1
    assert C.same_bits(got.row_elpd.cpu().numpy(), want.row_elpd.cpu().numpy())
    assert C.same_bits(got.khat.cpu().numpy(), want.khat.cpu().numpy())


def test_chain_group_loo(gpu):
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    rng = np.random.RandomState(3)
    X = rng.uniform(-3.0, 3.0, size=(60, 1))
    y = np.sinc(X[:, 0]) + 0.05 * rng.randn(60)
    chains = FusedBNNChains.for_dataset(X, y, 4, seed=2, device=gpu, burn_in_steps=4)
    trace = chains.collect(8, every=2)
    got = chains.loo(X, y, trace, weights=True)
    Xd = torch.as_tensor(X, dtype=torch.float32, device=gpu)
    yd = torch.as_tensor(y, dtype=torch.float32, device=gpu)
    loglik = chains.score(Xd, yd, trace, pointwise=True).loglik
    assert tuple(loglik.shape) == (32, 60) and tuple(got.log_weights.shape) == (32, 60)
    _assert_loo_result(got, loglik, 1.0, True, "FusedBNNChains.loo")


def test_bnn_loo_defaults_to_the_training_set(gpu):
    from pysgmcmc_amd.models import BayesianNeuralNetwork
    rng = np.random.RandomState(4)
    X = rng.uniform(-3.0, 3.0, size=(50, 1))
    y = np.sinc(X[:, 0]) + 0.05 * rng.randn(50)
    bnn = BayesianNeuralNetwork(session=gpu, dtype=torch.float32, n_nets=6, n_iters=80, burn_in_steps=10, sample_steps=2, seed=1)
    with pytest.raises(ValueError, match="untrained"):
        bnn.loo()
    bnn.train(X, y)
    got = bnn.loo()
    assert sorted(got) == ["elpd_loo", "khat", "lppd", "n_bad", "n_tail", "p_loo", "row_elpd", "row_lppd", "se", "thinning"]
    assert got["row_elpd"].shape == got["khat"].shape == got["n_tail"].shape == (50,) and got["thinning"] == 1
    # 6 draws: M = 2, so nothing is smoothed and every khat is +inf
    assert (got["n_tail"] <= 2).all() and np.isposinf(got["khat"]).all() and got["n_bad"] == 50
    # the same kept networks and the same normalised data as score(on_device=True) hands K13: its row_lppd, shifted alike
    score = bnn.score(X, y, on_device=True)
    assert C.same_bits(got["row_lppd"], score["row_lppd"])
    explicit = bnn.loo(X, y)
    assert C.same_bits(explicit["row_elpd"], got["row_elpd"]) and explicit["elpd_loo"] == got["elpd_loo"]
    assert abs(got["p_loo"] - (got["lppd"] - got["elpd_loo"])) <= 8 * EPS * (abs(got["lppd"]) + abs(got["elpd_loo"]))
    assert (got["row_elpd"] <= got["row_lppd"] + 1e-12).all()            # a harmonic mean lies below the arithmetic one
    with pytest.raises(ValueError, match="go together"):
        bnn.loo(X)
