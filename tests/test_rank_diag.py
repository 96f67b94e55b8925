"""Rank-normalised diagnostics without a GPU: the host statement ``diagnostics.rank`` of K18's arithmetic
(include/sgmcmc_hip_rank.h) against a brute-force definition that uses no sort, its tail indicators against numpy's
interpolated quantiles, what the statistics are for (scale differences, heavy tails, i.i.d. draws), and the refusals of
``kernels.rank_normalize`` and of the C entry points, all of which come before a device is needed."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from pysgmcmc_amd import _lib, diagnostics, kernels
from pysgmcmc_amd.diagnostics import rank
from pysgmcmc_amd.diagnostics.sampler_diagnostics import effective_n, gelman_rubin_from_chains

import rank_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_names_are_exported():
    for name in ("rank_normalize", "rank_max_pooled"):
        assert name in kernels.__all__ and callable(getattr(kernels, name))
    for name in ("rank_diagnostics_all", "rank_diagnostics", "rank_normalized_chains", "RankDiagnostics", "rank"):
        assert name in diagnostics.__all__ and hasattr(diagnostics, name)
    assert diagnostics.RankDiagnostics._fields[:3] == ("rhat_rank", "ess_bulk", "ess_tail")
    lib = _lib.lib()
    assert lib.sgmcmc_rank_abi_version() == _lib.RANK_ABI_VERSION == 1
    assert lib.sgmcmc_rank_max_pooled() == _lib.RANK_MAX_POOLED == kernels.rank_max_pooled() >= 8192
    text = open(os.path.join(ROOT, "include", "sgmcmc_hip_rank.h")).read()
    assert "#define SGMCMC_RANK_ABI_VERSION 1" in text and "#define SGMCMC_RANK_MAX_POOLED %d" % _lib.RANK_MAX_POOLED in text
    assert "sgmcmc_rank" not in open(os.path.join(ROOT, "include", "sgmcmc_hip.h")).read()
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    assert inspect.signature(FusedBNNChains.diagnose).parameters["rank_normalized"].default is False


def test_both_new_files_are_build_dependencies():
    deps = [os.path.basename(p) for p in _lib.build_dependencies()]
    assert "sgmcmc_rank.hip" in deps and "sgmcmc_hip_rank.h" in deps
    make = open(os.path.join(ROOT, "pysgmcmc_amd", "csrc", "Makefile")).read()
    assert "sgmcmc_rank.hip" in make and "sgmcmc_hip_rank.h" in make


# ---- the host statement against the definition -------------------------------------------------------------------------------

def _tie_cases():
    rng = np.random.RandomState(3)
    yield "N = 4, distinct", np.array([[0.3, -1.0, 2.0, 0.5]])[:, :, None]
    yield "N = 4, all tied", np.zeros((1, 4, 1))
    yield "N = 4, +-0.0", np.array([[0.0, -0.0, -0.0, 0.0]])[:, :, None]
    yield "m = 1, odd n", rng.randint(0, 5, size=(1, 9, 3)).astype(np.float64)
    yield "odd n, the middle draw is an outlier", np.concatenate(
        [rng.randn(3, 3, 2), np.full((3, 1, 2), 1e9), rng.randn(3, 3, 2)], axis=1)
    yield "ties and signed zeros", rng.choice(np.array([-1.5, -0.0, 0.0, 0.0, 2.0, 7.0]), size=(4, 10, 4))
    yield "the pattern columns", C.pattern_trace(3, 11, C.N_PATTERNS)
    yield "float32 input", rng.randn(2, 8, 2).astype(np.float32)
    yield "every rank2 at N = 24", C.all_rank2_trace(2, 12)


@pytest.mark.parametrize("name,x", list(_tie_cases()), ids=[n for n, _ in _tie_cases()])
def test_host_statement_equals_the_brute_force_definition(name, x):
    got, want = rank.rank_normalized_chains(x), C.brute_normalized(x)
    m, n, P = x.shape
    for g, w, what in zip(got, want, ("z", "z_folded", "tail_lo", "tail_hi")):
        assert g.shape == (2 * m, n // 2, P) and g.dtype == np.float64
        assert C.same_bits(g, w), "%s: %s differs" % (name, what)
    # rank2 by sorting equals rank2 by counting, column by column; twice the average rank of scipy's definition
    s = rank.split_chains(x)
    for p in range(P):
        v = s[:, :, p].ravel()
        if np.all(np.isfinite(v)):
            assert np.array_equal(rank.rank2_of(v), C.brute_rank2(v))


def test_split_drops_the_middle_draw_of_an_odd_chain():
    x = np.arange(2 * 7 * 1, dtype=np.float64).reshape(2, 7, 1)
    s = rank.split_chains(x)
    assert s.shape == (4, 3, 1)
    assert s[:, :, 0].tolist() == [[0, 1, 2], [4, 5, 6], [7, 8, 9], [11, 12, 13]]
    with pytest.raises(ValueError):
        rank.split_chains(np.zeros((2, 3, 1)))


def test_the_table_is_antisymmetric_increasing_and_as241():
    import statistics
    inv = statistics.NormalDist().inv_cdf
    for N in (4, 18, 1000, 8192):
        t = rank.z_of_rank2(N)
        assert t.shape == (2 * N + 1,) and np.isnan(t[:2]).all()
        body = t[2:]
        assert np.all(np.diff(body) > 0), "not strictly increasing"
        assert C.same_bits(body[:N - 1], -body[::-1][:N - 1]) and t[N + 1] == 0.0
        for r in (2, 3, N // 2, N, N + 1):
            assert t[r] == inv((r - 0.75) / (2.0 * N + 0.5))
        # against the quantile function evaluated in the upper half as well: there p is rounded to a multiple of 2^-53 (an
        # error of at most 2^-54, against 2^-55 and less for the mirror image below 0.5), the slope of the quantile function
        # is 1 / pdf(z), and AS241 itself is good to about 1e-16 relative: a few ulp on top
        upper = np.array([inv((r - 0.75) / (2.0 * N + 0.5)) for r in range(N + 2, 2 * N + 1)])
        pdf = np.exp(-0.5 * upper ** 2) / np.sqrt(2.0 * np.pi)
        assert np.all(np.abs(upper - t[N + 2:]) <= 2.0 ** -53 / pdf + 4.0 * np.spacing(upper))


@pytest.mark.parametrize("N", [4, 20, 21, 24, 41, 100, 101, 1000, 1030, 8192])
def test_order_statistic_tails_equal_numpys_interpolated_quantiles(N):
    """0.05 (N - 1) is an integer at N = 21, 41, 101 (the quantile IS an order statistic) and falls strictly between two order
    statistics elsewhere; with distinct values and with ties across the cut."""
    rng = np.random.RandomState(N)
    k_lo, k_hi = rank.tail_order_statistics(N)
    assert k_lo == int(np.floor(0.05 * (N - 1) + 1e-9)) and k_hi == int(np.ceil(0.95 * (N - 1) - 1e-9))
    for v in (rng.randn(N), rng.permutation(N).astype(np.float64), rng.randint(0, 7, size=N).astype(np.float64),
              np.round(rng.randn(N), 1)):
        s = np.sort(v)
        assert np.array_equal(v <= s[k_lo], v <= np.quantile(v, 0.05))
        assert np.array_equal(v >= s[k_hi], v >= np.quantile(v, 0.95))
    # through the public function: N = 2 m (n // 2) pooled draws of one column
    if N % 4 == 0:
        x = rng.randn(2, N // 2, 1) if N >= 8 else rng.randn(1, N, 1)
        _, _, lo, hi = rank.rank_normalized_chains(x)
        pooled = x.ravel()
        assert np.array_equal(lo.ravel() == 1.0, pooled <= np.quantile(pooled, 0.05))
        assert np.array_equal(hi.ravel() == 1.0, pooled >= np.quantile(pooled, 0.95))
        assert set(np.unique(lo)) <= {0.0, 1.0} and set(np.unique(hi)) <= {0.0, 1.0}


def test_degenerate_columns_of_the_host_statement():
    x = C.pattern_trace(2, 10, C.N_PATTERNS)
    outs = rank.rank_normalized_chains(x)
    d = rank.rank_diagnostics(x)
    for j in range(C.N_PATTERNS):
        if C.pattern_of(j) in C.DEGENERATE:
            assert all(np.isnan(o[:, :, j]).all() for o in outs)
            assert np.isnan(d.rhat_rank[j]) and d.ess_bulk[j] == 0 and d.ess_tail[j] == 0
        else:
            assert all(np.isfinite(o[:, :, j]).all() for o in outs)
    j = C.PATTERNS.index(C._constant)
    assert (outs[0][:, :, j] == 0.0).all() and (outs[2][:, :, j] == 1.0).all() and (outs[3][:, :, j] == 1.0).all()
    assert np.isnan(d.rhat_rank[j]) and d.ess_bulk[j] == 0 and np.isnan(d.raw_bulk[j])


# ---- what the statistics are for ---------------------------------------------------------------------------------------------

def test_scale_difference_passes_the_classic_rhat_and_fails_the_rank_rhat():
    rng = np.random.RandomState(11)
    x = rng.randn(8, 400, 1)
    x[4:] *= 3.0                                             # equal means, scales 1 and 3
    classic = float(gelman_rubin_from_chains(torch.as_tensor(x))[0])
    d = rank.rank_diagnostics(x)
    print("classic R-hat %.4f, rank R-hat %.4f (bulk %.4f, folded %.4f)" % (classic, d.rhat_rank[0], d.rhat_bulk[0],
                                                                             d.rhat_folded[0]))
    assert classic < 1.01 < d.rhat_rank[0]
    assert d.rhat_folded[0] > d.rhat_bulk[0]                 # it is the folded draws that see the scale
    same = rank.rank_diagnostics(rng.randn(8, 400, 1))
    assert same.rhat_rank[0] < 1.01


def test_cauchy_chains_give_a_finite_stable_rank_rhat():
    values = []
    for seed in range(6):
        x = np.random.RandomState(seed).standard_cauchy(size=(4, 500, 1))
        d = rank.rank_diagnostics(x)
        values.append(d.rhat_rank[0])
        assert d.ess_bulk[0] > 0 and d.ess_tail[0] > 0
    print("rank R-hat of Cauchy chains over six seeds: %s" % np.round(values, 4))
    assert np.all(np.isfinite(values)) and max(values) < 1.01 and max(values) - min(values) < 0.01


def test_bulk_ess_of_iid_normal_chains_lies_within_effective_n_s_own_spread():
    """For i.i.d. draws the rank transform is monotone and the scores are again (nearly) i.i.d. normal, so ess_bulk is an
    estimate of N with the estimator's own noise. That noise is measured here: ``effective_n`` of the raw split chains over
    24 seeds gives a mean and a standard deviation, and ess_bulk of a 25th seed must lie within 4 standard deviations of
    that mean (and the mean within 10 % of N)."""
    m, n = 4, 250
    N = 2 * m * (n // 2)
    raws = [effective_n(torch.as_tensor(rank.split_chains(np.random.RandomState(100 + s).randn(m, n, 1))[:, :, 0]))
            for s in range(24)]
    mean, sd = float(np.mean(raws)), float(np.std(raws, ddof=1))
    d = rank.rank_diagnostics(np.random.RandomState(99).randn(m, n, 1))
    print("effective_n of raw i.i.d. draws: mean %.1f, sd %.1f of N = %d; ess_bulk %d, ess_tail %d" % (
        mean, sd, N, d.ess_bulk[0], d.ess_tail[0]))
    assert abs(mean - N) < 0.1 * N
    assert abs(d.ess_bulk[0] - mean) <= 4.0 * sd
    assert d.ess_tail[0] > 0


def test_host_rhat_and_ess_are_the_projects_own_formulas():
    x = np.random.RandomState(5).randn(6, 40, 2).cumsum(axis=1) * 0.3 + np.random.RandomState(6).randn(6, 40, 2)
    for p in range(2):
        col = x[:, :, p]
        assert abs(rank.rhat_of(col) - float(gelman_rubin_from_chains(torch.as_tensor(col[:, :, None]))[0])) < 1e-12
        raw = rank.effective_n_raw(col)
        assert abs(raw - effective_n(torch.as_tensor(col))) < 1.0 + 1e-9 * raw        # the FFT path truncates the same value


# ---- refusals: before any device is needed -----------------------------------------------------------------------------------

def _outs(m, n, P, dtype=torch.float64):
    return torch.zeros(2 * m, n // 2, P, dtype=dtype)


def test_wrapper_refusals_come_before_the_device():
    cap = kernels.rank_max_pooled()
    with pytest.raises(ValueError, match="at least 4 samples"):
        kernels.rank_normalize(torch.zeros(2, 3, 5), z=torch.zeros(4, 1, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="pooled draws"):
        kernels.rank_normalize(torch.zeros(2, cap // 2 + 2, 1), z=_outs(2, cap // 2 + 2, 1))
    with pytest.raises(ValueError, match="m = 2049 chains"):
        kernels.rank_normalize(torch.zeros(2049, 4, 1), z=_outs(2049, 4, 1))
    with pytest.raises(TypeError, match="z_folded must be a float64 tensor"):
        kernels.rank_normalize(torch.zeros(2, 8, 5), z_folded=_outs(2, 8, 5, torch.float32))
    with pytest.raises(ValueError, match="tail_lo must be of shape"):
        kernels.rank_normalize(torch.zeros(2, 8, 5), tail_lo=torch.zeros(2, 8, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="tail_hi must be of shape"):
        kernels.rank_normalize(torch.zeros(2, 9, 5), tail_hi=torch.zeros(4, 5, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="at least one of"):
        kernels.rank_normalize(torch.zeros(2, 8, 5))
    with pytest.raises(ValueError, match="share their strides"):
        kernels.rank_normalize(torch.zeros(2, 8, 5), z=_outs(2, 8, 5), z_folded=_outs(2, 8, 10)[:, :, :5])
    with pytest.raises(ValueError, match="dense"):
        kernels.rank_normalize(torch.zeros(2, 8, 10)[:, :, ::2], z=_outs(2, 8, 5))
    with pytest.raises(TypeError):
        kernels.rank_normalize(torch.zeros(2, 8, 5, dtype=torch.int32), z=_outs(2, 8, 5))
    # with every argument in order the only thing missing is the device
    with pytest.raises(_lib.SgmcmcLibraryError, match="no CPU fallback"):
        kernels.rank_normalize(torch.zeros(2, 8, 5), z=_outs(2, 8, 5))
    with pytest.raises(ValueError, match="at least 4 samples"):
        diagnostics.rank_diagnostics_all(torch.zeros(2, 3, 5))
    with pytest.raises(ValueError, match="at most 2048 chains"):
        diagnostics.rank_diagnostics_all(torch.zeros(2049, 4, 1))


def test_c_entry_refusals_name_the_offending_value():
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cap = _lib.RANK_MAX_POOLED

    def call(sfx="f64", trace=p, m=2, n=8, P=2, ld=2, cs=16, outs=(p, None, None, None), ld_out=2, cs_out=8):
        return getattr(lib, "sgmcmc_rank_normalize_" + sfx)(trace, m, n, P, ld, cs, *outs, ld_out, cs_out, None)

    for kw, text in ((dict(m=0), "m = 0 chains"), (dict(m=2049, n=4), "m = 2049 chains"), (dict(n=3), "n = 3 samples"),
                     (dict(n=cap // 2 + 2, cs=10 ** 6), "n = %d exceeds %d pooled draws" % (cap // 2 + 2, cap)),
                     (dict(trace=None), "trace must be non-NULL"), (dict(outs=(None,) * 4), "at least one of z, z_folded"),
                     (dict(ld=1), "ld = 1 is smaller than P = 2"), (dict(cs=15), "chain_stride = 15 is smaller than"),
                     (dict(ld_out=1), "ld_out = 1 is smaller than P = 2"),
                     (dict(cs_out=7), "chain_stride_out = 7 is smaller than (half - 1) * ld_out + P = 8"),
                     (dict(n=2 ** 63 + 5), "exceeds"), (dict(ld=2 ** 62, cs=2 ** 63), "overflows")):
        for sfx in ("f32", "f64"):
            assert call(sfx, **kw) == -1, kw                 # SGMCMC_EINVAL
            message = lib.sgmcmc_last_error().decode()
            assert message.startswith("rank_normalize: ") and text in message, (kw, message)
    # P = 0 is a successful no-op, before the pointers are looked at
    assert call(P=0, ld=0, cs=0, ld_out=0, cs_out=0, trace=None, outs=(None,) * 4) == 0
