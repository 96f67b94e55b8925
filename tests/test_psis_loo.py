"""The host statement of PSIS-LOO (``diagnostics.psis``): the generalised Pareto fit against draws of known shape, the whole
estimate against the exact leave-one-out densities of a conjugate model, the structure of the statement at its edges, and
the refusals of ``kernels.psis_loo`` that need no device. The device kernel is pinned to this statement in
tests/test_psis_loo_gpu.py."""
import math

import numpy as np
import pytest
import torch
from scipy.stats import genpareto

from pysgmcmc_amd import diagnostics, kernels
from pysgmcmc_amd.diagnostics import psis

import psis_cases as C


# ---- the generalised Pareto fit

@pytest.mark.parametrize("seed", [100, 101, 102])
def test_gpd_fit_recovers_the_shape(seed):
    rng = np.random.RandomState(seed)
    for k in (-0.2, 0.1, 0.5, 0.9):
        x = np.sort(genpareto.rvs(k, scale=2.0, size=2000, random_state=rng))
        khat, sigma = psis.gpd_fit(x)
        print("seed %d k = %.1f: khat = %.4f sigma = %.4f" % (seed, k, khat, sigma))
        assert abs(khat - k) <= 0.15
        assert sigma > 0.0


def test_gpd_fit_refuses_what_it_cannot_fit():
    with pytest.raises(ValueError, match="at least 5"):
        psis.gpd_fit(np.arange(1.0, 5.0))
    with pytest.raises(ValueError, match="ascending"):
        psis.gpd_fit(np.array([1.0, 3.0, 2.0, 4.0, 5.0]))


# ---- the whole estimate against a model whose leave-one-out densities are known

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_conjugate_normal_loo(seed):
    rng = np.random.RandomState(seed)
    n, S = 40, 4000
    y = rng.randn(n) + 0.7
    y[0] = 4.0
    mean, var = y.sum() / (n + 1.0), 1.0 / (n + 1.0)                    # prior N(0, 1), likelihood N(mu, 1)
    mu = mean + math.sqrt(var) * rng.randn(S)
    ll = -0.5 * math.log(2.0 * math.pi) - 0.5 * (y[None, :] - mu[:, None]) ** 2
    got = psis.psis_loo_host(ll)
    mean_i, var_i = (y.sum() - y) / n, 1.0 / n                          # the posterior without y_i
    exact = -0.5 * np.log(2.0 * math.pi * (1.0 + var_i)) - 0.5 * (y - mean_i) ** 2 / (1.0 + var_i)
    worst = np.abs(got["elpd_loo"] - exact).max()
    print("seed %d: max |elpd_i - exact_i| = %.4f, sums %.4f against %.4f, lppd %.4f, max khat %.3f" % (
        seed, worst, got["elpd_loo"].sum(), exact.sum(), got["row_lppd"].sum(), got["khat"].max()))
    assert worst <= 0.05
    assert abs(got["elpd_loo"].sum() - exact.sum()) <= 0.1
    assert got["row_lppd"].sum() - got["elpd_loo"].sum() >= 1.0
    assert got["khat"].max() < 0.5
    # row_lppd is log mean exp
    m = ll.max(axis=0)
    assert np.allclose(got["row_lppd"], m + np.log(np.exp(ll - m).mean(axis=0)), rtol=0, atol=1e-12)


# ---- structure

def test_constants():
    assert psis.LOG_DBL_MIN == math.log(np.finfo(np.float64).tiny)
    assert psis.MAX_DRAWS == 8192


def test_fixed_sum_is_the_stated_order():
    rng = np.random.RandomState(3)
    for n in (0, 1, 5, 255, 256, 257, 1000):
        v = rng.randn(n) * 10.0 ** rng.randint(-8, 8, size=n)
        part = [0.0] * 256
        for j in range(256):
            for i in range(j, n, 256):
                part[j] = part[j] + v[i]
        h = 128
        while h >= 1:
            for t in range(h):
                part[t] = part[t] + part[t + h]
            h //= 2
        assert C.same_bits(psis.fixed_sum(v), np.float64(part[0]))
    a = rng.randn(7, 300)
    assert C.same_bits(psis.fixed_sum(a, axis=1), np.array([psis.fixed_sum(row) for row in a]))


@pytest.mark.parametrize("S", [2, 16, 25, 100, 257, 1000])
def test_weights_are_normalised_and_nonpositive(S):
    ll = C.matrix(S, len(C.PATTERNS), seed=1)
    for r_eff in C.R_EFFS:
        got = psis.psis_loo_host(ll, r_eff)
        lwn = got["log_weights"]
        assert (lwn <= 0.0).all()
        for r in range(ll.shape[1]):
            assert abs(psis.fixed_sum(np.exp(lwn[:, r])) - 1.0) <= 1e-14
        assert (got["n_tail"] >= 0).all() and (got["n_tail"] <= got["M"]).all()


def _unsmoothed(l):
    lr = -l
    lw = lr - lr.max()
    return lw - (lw.max() + np.log(psis.fixed_sum(np.exp(lw - lw.max()))))


def test_sixteen_draws_are_not_smoothed():
    rng = np.random.RandomState(5)
    ll = C.gaussian(16, rng)[:, None]
    got = psis.psis_loo_host(ll)
    assert got["M"] == 4 and got["n_tail"][0] == 4 and np.isposinf(got["khat"][0])
    assert C.same_bits(got["log_weights"][:, 0], _unsmoothed(ll[:, 0]))


def test_twentyfive_draws_are_smoothed():
    rng = np.random.RandomState(5)
    ll = C.gaussian(25, rng)[:, None]
    got = psis.psis_loo_host(ll)
    assert got["M"] == 5 and got["n_tail"][0] == 5 and np.isfinite(got["khat"][0])
    assert not C.same_bits(got["log_weights"][:, 0], _unsmoothed(ll[:, 0]))


def test_constant_column():
    for S in (2, 64, 1000):
        got = psis.psis_loo_host(np.full((S, 1), -1.25))
        assert got["n_tail"][0] == 0 and np.isposinf(got["khat"][0])
        assert np.allclose(got["log_weights"][:, 0], -math.log(S), rtol=0, atol=1e-15)
        assert abs(got["elpd_loo"][0] + 1.25) <= 1e-14 and abs(got["row_lppd"][0] + 1.25) <= 1e-14


def test_tie_seam():
    """Equal values at the cut stay out of the tail, whatever their draw index; the draws above it are all in."""
    S = 100
    rng = np.random.RandomState(11)
    for above in (4, 5, 12, 19):
        l = C.ties_at_cut(S, rng, above)
        got = psis.psis_loo_host(l[:, None])
        assert got["M"] == 20 and got["n_tail"][0] == above
        assert np.isposinf(got["khat"][0]) == (above <= 4)
    # every value twice: the pair that straddles position S - M - 1 is left out as a whole
    l = -np.repeat(np.arange(50.0), 2)[rng.permutation(S)]
    for r_eff, M in ((1.0, 20), (40.0, 5)):
        got = psis.psis_loo_host(l[:, None], r_eff)
        assert got["M"] == M and got["n_tail"][0] == M - (M % 2 == 1)
    # a permutation of the draws changes which of two equal tail draws gets the larger quantile (the one with the larger
    # index), and nothing else: the same khat and the same multiset of weights
    l = C.every_value_twice(S, rng)
    perm = rng.permutation(S)
    a, b = psis.psis_loo_host(l[:, None]), psis.psis_loo_host(l[perm][:, None])
    assert a["n_tail"][0] == b["n_tail"][0] and C.same_bits(a["khat"], b["khat"])
    assert np.allclose(np.sort(a["log_weights"][:, 0]), np.sort(b["log_weights"][:, 0]), rtol=0, atol=1e-13)
    tail = np.argsort(-l, kind="stable")[S - a["n_tail"][0]:]           # the tail in the order (value, draw index)
    assert (np.diff(a["log_weights"][tail, 0]) >= 0.0).all()


def test_underflow_takes_the_log_dbl_min_cut():
    S = 1000
    rng = np.random.RandomState(13)
    l = C.underflow(S, rng)
    lw = -l - (-l).max()
    got = psis.psis_loo_host(l[:, None])
    assert np.sort(lw)[S - got["M"] - 1] < psis.LOG_DBL_MIN
    assert got["n_tail"][0] == int((lw > psis.LOG_DBL_MIN).sum()) == C.few_above(S)
    assert np.isfinite(got["khat"][0]) and np.isfinite(got["elpd_loo"][0])
    assert abs(psis.fixed_sum(np.exp(got["log_weights"][:, 0])) - 1.0) <= 1e-14


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_nonfinite_column_is_nan_and_alone(poison):
    ll = C.matrix(100, 5, seed=2)
    clean = psis.psis_loo_host(ll)
    ll2 = ll.copy()
    ll2[37, 2] = poison
    got = psis.psis_loo_host(ll2)
    assert got["n_tail"][2] == -1
    for name in ("elpd_loo", "khat", "row_lppd"):
        assert np.isnan(got[name][2])
        keep = [0, 1, 3, 4]
        assert C.same_bits(got[name][keep], clean[name][keep])
    assert np.isnan(got["log_weights"][:, 2]).all()
    assert C.same_bits(got["log_weights"][:, [0, 1, 3, 4]], clean["log_weights"][:, [0, 1, 3, 4]])
    assert np.isnan(got["summary"][0]) and np.isnan(got["summary"][1]) and got["summary"][3] == 1.0


def test_tail_length_and_its_clamp():
    assert psis.tail_length(2) == 1 and psis.tail_length(3) == 1 and psis.tail_length(5) == 1
    assert psis.tail_length(6) == 2 and psis.tail_length(16) == 4 and psis.tail_length(25) == 5
    assert psis.tail_length(224) == 45 and psis.tail_length(225) == 45 and psis.tail_length(226) == 46
    assert psis.tail_length(1000) == 95 and psis.tail_length(8192) == 272
    assert psis.tail_length(8192, 0.3) == 496 and psis.tail_length(8192, 1e-300) == 1639
    assert psis.tail_length(100, 1e6) == 1 and psis.tail_length(2, 1e-300) == 1
    assert psis.tail_length(1000, 2.5) == 60


def test_columns_do_not_see_each_other():
    ll = C.matrix(257, 13, seed=4)
    whole = psis.psis_loo_host(ll, 0.3)
    for r in (0, 5, 12):
        one = psis.psis_loo_host(ll[:, r:r + 1], 0.3)
        for name in ("elpd_loo", "khat", "row_lppd"):
            assert C.same_bits(one[name], whole[name][r:r + 1])
        assert one["n_tail"][0] == whole["n_tail"][r]
        assert C.same_bits(one["log_weights"][:, 0], whole["log_weights"][:, r])


def test_summary_is_the_tree_of_the_rows():
    ll = C.matrix(100, 300, seed=6)
    got = psis.psis_loo_host(ll)
    assert C.same_bits(got["summary"][0], psis.fixed_sum(got["elpd_loo"]))
    assert C.same_bits(got["summary"][1], psis.fixed_sum(got["row_lppd"]))
    assert got["summary"][2] == float((got["khat"] > 0.7).sum()) and got["summary"][3] == 0.0


def test_exports():
    assert diagnostics.psis_loo_host is psis.psis_loo_host and diagnostics.gpd_fit is psis.gpd_fit
    assert diagnostics.psis_loo is psis.psis_loo
    assert diagnostics.PsisLoo._fields[:10] == ("elpd_loo", "p_loo", "se", "lppd", "row_elpd", "row_lppd", "khat", "n_tail",
                                                "n_bad", "log_weights")
    assert kernels.psis_max_draws() == 8192
    from pysgmcmc_amd import models
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    assert callable(models.loo_score) and callable(FusedBNNChains.loo) and callable(models.BayesianNeuralNetwork.loo)


# ---- the refusals of kernels.psis_loo that need no device, and their order

def _ll(S=10, n_rows=3, dtype=torch.float64):
    return torch.zeros(S, n_rows, dtype=dtype)


def test_refusals_and_their_order():
    f64 = torch.float64
    with pytest.raises(TypeError, match=r"^psis_loo: loglik"):
        kernels.psis_loo(np.zeros((10, 3)))
    with pytest.raises(ValueError, match=r"^psis_loo: loglik must be \(S, n_rows\), got \(10,\)"):
        kernels.psis_loo(torch.zeros(10, dtype=f64))
    for S in (0, 1, 8193):
        with pytest.raises(ValueError, match=r"^psis_loo: S = %d draws, must be 2 \.\. 8192" % S):
            kernels.psis_loo(_ll(S), r_eff=-1.0)                       # S wins over r_eff
    for r_eff, text in ((0.0, "0"), (-2.5, "-2.5"), (float("inf"), "inf"), (float("nan"), "nan")):
        with pytest.raises(ValueError, match=r"^psis_loo: r_eff = %s, must be a positive finite number" % text):
            kernels.psis_loo(_ll(dtype=torch.float32), r_eff=r_eff)    # r_eff wins over the dtype
    with pytest.raises(TypeError, match=r"^psis_loo: loglik must be a float64 tensor, got torch.float32"):
        kernels.psis_loo(_ll(dtype=torch.float32))
    with pytest.raises(ValueError, match=r"^psis_loo: the rows of loglik must be dense"):
        kernels.psis_loo(torch.zeros(3, 10, dtype=f64).t())
    with pytest.raises(ValueError, match=r"^psis_loo: ld = 0 is smaller than n_rows = 3"):
        kernels.psis_loo(torch.zeros(1, 3, dtype=f64).expand(10, 3), khat=torch.zeros(2, dtype=f64))   # ld wins over an output
    with pytest.raises(TypeError, match=r"^psis_loo: khat must be a torch.float64 tensor"):
        kernels.psis_loo(_ll(), khat=torch.zeros(3))
    with pytest.raises(TypeError, match=r"^psis_loo: n_tail must be a torch.int32 tensor"):
        kernels.psis_loo(_ll(), n_tail=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"^psis_loo: elpd_loo must be a contiguous \(n_rows,\) = \(3,\) tensor"):
        kernels.psis_loo(_ll(), elpd_loo=torch.zeros(4, dtype=f64), log_weights=torch.zeros(1, dtype=f64))
    with pytest.raises(ValueError, match=r"^psis_loo: row_lppd must be a contiguous"):
        kernels.psis_loo(_ll(), row_lppd=torch.zeros(6, dtype=f64)[::2])
    with pytest.raises(ValueError, match=r"^psis_loo: log_weights must be of shape \(S, n_rows\) = \(10, 3\)"):
        kernels.psis_loo(_ll(), log_weights=torch.zeros(3, 10, dtype=f64))
    with pytest.raises(ValueError, match=r"^psis_loo: ld_w = 0 is smaller than n_rows = 3"):
        kernels.psis_loo(_ll(), log_weights=torch.zeros(1, 3, dtype=f64).expand(10, 3), summary=torch.zeros(3, dtype=f64))
    with pytest.raises(ValueError, match=r"^psis_loo: summary must hold 4"):
        kernels.psis_loo(_ll(), summary=torch.zeros(3, dtype=f64))
    # a well-formed call on the host: there is no CPU route
    from pysgmcmc_amd._lib import SgmcmcLibraryError
    with pytest.raises(SgmcmcLibraryError, match="no CPU"):
        kernels.psis_loo(_ll())
    with pytest.raises(ValueError, match=r"^psis_loo: S = 1 draws"):
        psis.psis_loo_host(np.zeros((1, 3)))
    with pytest.raises(ValueError, match=r"^psis_loo: r_eff = 0, must be a positive finite number"):
        psis.psis_loo_host(np.zeros((4, 3)), 0.0)
