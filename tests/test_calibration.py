"""The host statement of the calibration add-on (``diagnostics.calibration``): the CRPS of a mixture of Gaussians against an
independent dense statement, the one-Gaussian closed form and a numerical integral; PIT against scipy; what PIT, coverage and
histogram say about a well-specified and an overconfident ensemble; the edges of the histogram; the units of
``BayesianNeuralNetwork.calibration``; the header's symbols and every refusal that needs no device. The device kernel is
pinned to this statement in tests/test_calibration_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy.stats import kstest, norm

from pysgmcmc_amd import _lib, diagnostics, kernels
from pysgmcmc_amd.diagnostics.calibration import (Calibration, calibration_of_summary, mixture_calibration_host, summary_of)

import calibration_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_calib.h")
EINVAL = -1


# ---- the statement against independent ones

@pytest.mark.parametrize("S", [1, 2, 5, 65, 300])
def test_crps_against_the_dense_statement(S):
    means, var, y = C.ensemble(S, 6, seed=1)
    got = mixture_calibration_host(means, var, y)
    want, first = C.dense_crps(means, var, y)
    worst = np.abs(got["crps"] - want) / np.maximum(1.0, first)
    print("S = %d: max |d| / max(1, T / S) = %.3e" % (S, worst.max()))
    assert (worst <= 16 * C.EPS).all()


def test_one_gaussian_has_the_closed_form():
    rng = np.random.RandomState(3)
    mu, var, y = rng.randn(1, 40), np.array([0.37]), 2.0 * rng.randn(40)
    got = mixture_calibration_host(mu, var, y)
    want = C.gaussian_crps(mu[0], np.sqrt(var[0]), y)
    print("max |d| = %.3e" % np.abs(got["crps"] - want).max())
    assert np.abs(got["crps"] - want).max() <= 16 * C.EPS * max(1.0, np.abs(want).max())
    assert np.abs(got["pit"] - norm.cdf((y - mu[0]) / np.sqrt(var[0]))).max() <= 4 * C.EPS


def test_crps_is_the_integral_of_the_squared_cdf_difference():
    means, var, y = C.ensemble(7, 3, seed=2)
    got = mixture_calibration_host(means, var, y)
    sd = np.sqrt(var)
    for r in range(3):
        lo = min(means[:, r].min(), y[r]) - 12.0 * sd.max()
        hi = max(means[:, r].max(), y[r]) + 12.0 * sd.max()
        x = np.arange(lo, hi, 3e-5)
        F = norm.cdf((x[None, :] - means[:, r, None]) / sd[:, None]).mean(axis=0)
        f = (F - (x >= y[r])) ** 2
        integral = float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(x)))
        print("row %d: closed form %.9f, trapezoid %.9f" % (r, got["crps"][r], integral))
        assert abs(got["crps"][r] - integral) <= 1e-4


def test_pit_is_the_mean_of_the_draws_cdfs():
    means, var, y = C.ensemble(65, 67, seed=4)
    got = mixture_calibration_host(means, var, y)
    want = norm.cdf((y[None, :] - means) / np.sqrt(var)[:, None]).mean(axis=0)
    assert np.abs(got["pit"] - want).max() <= 16 * C.EPS
    assert got["pit"].min() < 0.01 and got["pit"].max() > 0.99      # the cases reach both ends


def test_crps_is_nonnegative_and_grows_with_the_distance():
    means, var, _ = C.ensemble(64, 5, seed=5)
    centre = means.mean(axis=0)
    last = None
    for shift in (0.0, 1.0, 2.0, 5.0, 20.0):
        crps = mixture_calibration_host(means, var, centre + shift)["crps"]
        assert (crps >= 0.0).all()
        if last is not None:
            assert (crps > last).all()
        last = crps
    # far outside the ensemble the score is the distance, less half the ensemble's expected pair distance
    assert np.abs(last - 20.0).max() < 1.0


# ---- what the figures say about an ensemble

def _synthetic(seed=0, S=64, N=400):
    """A mixture per row and targets drawn from that mixture. The noise (sd 0.5) dominates the spread of the draws (0.3), as
    in a BNN that has seen enough data, so shrinking the noise variance makes the predictive markedly too narrow."""
    rng = np.random.RandomState(seed)
    trend = np.sin(np.linspace(0.0, 6.0, N))
    means = trend[None, :] + 0.3 * rng.randn(S, N)
    var = 0.25 * np.exp(0.3 * rng.randn(S))
    pick = rng.randint(0, S, size=N)
    y = means[pick, np.arange(N)] + np.sqrt(var[pick]) * rng.randn(N)
    return means, var, y


def test_a_well_specified_ensemble_is_calibrated():
    means, var, y = _synthetic()
    host = mixture_calibration_host(means, var, y, C.LEVELS, C.N_BINS)
    got = calibration_of_summary(host["pit"], host["crps"], host["summary"], C.LEVELS)
    p = kstest(got.pit, "uniform").pvalue
    print("KS p-value %.3g, coverage %s, calibration error %.4f, histogram %s" % (
        p, got.coverage, got.calibration_error, got.pit_hist))
    assert p > 0.01
    assert (np.abs(got.coverage - np.array(C.LEVELS)) <= 0.05).all()
    assert got.calibration_error == np.abs(got.coverage - np.array(C.LEVELS)).mean()
    assert got.pit_hist.sum() == 400.0 and got.n_bad == 0.0 and got.thinning == 1
    assert got.mean_crps == host["summary"][0] / 400.0


def test_an_overconfident_ensemble_is_found_out():
    means, var, y = _synthetic()
    host = mixture_calibration_host(means, var / 16.0, y, C.LEVELS, C.N_BINS)
    got = calibration_of_summary(host["pit"], host["crps"], host["summary"], C.LEVELS)
    p = kstest(got.pit, "uniform").pvalue
    print("KS p-value %.3g, coverage %s, histogram %s" % (p, got.coverage, got.pit_hist))
    assert p < 1e-3
    assert got.coverage[2] < 0.8                          # the 90 % interval
    assert got.pit_hist[0] + got.pit_hist[-1] > 2 * 40    # the outer bins hold more than their share: a U shape


# ---- summary at its edges

def test_histogram_edges_and_nan_rows():
    pit = np.array([0.0, 0.125, 0.25, 0.5, 0.75, 0.94, 1.0, np.nan, 0.5, 0.875])
    crps = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, np.nan, 9.0])
    s = summary_of(pit, crps, (0.5, 0.75, 0.9), 10)
    assert s.shape == (2 + 3 + 10,)
    assert np.isnan(s[0]) and s[1] == 2.0                 # both NaN rows are counted once, in n_bad alone
    assert list(s[2:5]) == [3.0, 5.0, 6.0]                # closed intervals: 0.25, 0.75, 0.125 and 0.875 are inside theirs
    assert list(s[5:]) == [1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 2.0]     # pit = 1.0 in the last bin
    assert s[5:].sum() == 8.0
    got = calibration_of_summary(pit, crps, s, (0.5, 0.75, 0.9))
    assert isinstance(got, Calibration) and got.n_bad == 2.0
    assert np.array_equal(got.coverage, np.array([3.0, 5.0, 6.0]) / 8.0)
    # nothing asked for: the two leading entries alone
    s = summary_of(pit[:7], crps[:7])
    assert s.shape == (2,) and s[0] == 28.0 and s[1] == 0.0
    # a NaN input poisons its own row only
    means, var, y = C.ensemble(5, 4, seed=6)
    clean = mixture_calibration_host(means, var, y, (0.9,), 4)
    y = y.copy()
    y[2] = np.nan
    bad = mixture_calibration_host(means, var, y, (0.9,), 4)
    keep = [0, 1, 3]
    assert np.isnan(bad["pit"][2]) and np.isnan(bad["crps"][2]) and bad["summary"][1] == 1.0
    assert C.same_bits(bad["pit"][keep], clean["pit"][keep]) and C.same_bits(bad["crps"][keep], clean["crps"][keep])
    assert bad["summary"][3:].sum() == 3.0


# ---- BayesianNeuralNetwork.calibration on the host route

def _tiny_ensemble(normalize):
    from pysgmcmc_amd.models import BayesianNeuralNetwork
    from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params
    bnn = BayesianNeuralNetwork(session="cpu", dtype=torch.float64, n_nets=5, normalize_input=normalize,
                                normalize_output=normalize)
    bnn.is_trained = True
    for k in range(5):
        net = init_mlp_params(3, hidden=(8, 5), seed=k, dtype=torch.float64)
        net[1].normal_(generator=torch.Generator().manual_seed(k))
        net[-1].fill_(-2.0 - 0.1 * k)
        bnn.samples.append(net)
    if normalize:
        bnn.x_mean, bnn.x_std = np.array([0.1, -0.2, 0.3]), np.array([1.5, 0.5, 2.0])
        bnn.y_mean, bnn.y_std = 0.7, 1.9
    return bnn


@pytest.mark.parametrize("normalize", [False, True])
def test_bnn_calibration_on_the_host_is_in_the_caller_s_units(normalize):
    bnn = _tiny_ensemble(normalize)
    rng = np.random.RandomState(0)
    X, y = rng.randn(11, 3), rng.randn(11)
    got = bnn.calibration(X, y, levels=(0.5, 0.9), n_bins=5)
    assert sorted(got) == ["calibration_error", "coverage", "crps", "levels", "mean_crps", "n_bad", "pit", "pit_hist", "thinning"]
    # the statement in the CALLER's units, from predict()'s own outputs
    f, noise = bnn.predict(X, return_individual_predictions=True)           # (5, 11), un-normalised
    want = mixture_calibration_host(f, noise[:, 0], y, (0.5, 0.9), 5)
    assert np.abs(got["pit"] - want["pit"]).max() <= 1e-12
    assert np.abs(got["crps"] - want["crps"]).max() <= 1e-12 * max(1.0, np.abs(want["crps"]).max())
    assert np.isclose(got["mean_crps"], want["crps"].mean(), rtol=1e-12)
    assert np.array_equal(got["pit_hist"], want["summary"][4:]) and got["pit_hist"].sum() == 11.0
    assert np.array_equal(got["coverage"], want["summary"][2:4] / 11.0)
    assert isinstance(got["mean_crps"], float) and isinstance(got["calibration_error"], float)
    assert got["n_bad"] == 0 and got["thinning"] == 1 and list(got["levels"]) == [0.5, 0.9]
    if normalize:
        # the same networks in their own units: crps scales with y_std, everything else stays
        plain = _tiny_ensemble(False)
        raw = plain.calibration((X - bnn.x_mean) / bnn.x_std, (y - bnn.y_mean) / bnn.y_std, levels=(0.5, 0.9), n_bins=5)
        assert C.same_bits(got["pit"], raw["pit"]) and np.array_equal(got["pit_hist"], raw["pit_hist"])
        assert C.same_bits(got["crps"], raw["crps"] * 1.9) and got["mean_crps"] == raw["mean_crps"] * 1.9
        assert np.array_equal(got["coverage"], raw["coverage"])
    assert bnn._kept_matrix is None                     # nothing was flattened for the device


def test_bnn_calibration_refuses_what_it_cannot_score():
    bnn = _tiny_ensemble(False)
    with pytest.raises(TypeError, match="live on cpu"):                     # no host fallback behind on_device=True
        bnn.calibration(np.zeros((4, 3)), np.zeros(4), on_device=True)
    with pytest.raises(ValueError, match="4 rows, y_test 5"):
        bnn.calibration(np.zeros((4, 3)), np.zeros(5))
    bnn.is_trained = False
    with pytest.raises(ValueError, match="untrained"):
        bnn.calibration(np.zeros((4, 3)), np.zeros(4))


# ---- the header, the declarations and the refusals that need no device

def test_the_header_declares_four_exported_symbols_and_version_1():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", text)))
    assert syms == ["sgmcmc_calib_abi_version", "sgmcmc_calib_max_draws", "sgmcmc_mixture_calibration_f32",
                    "sgmcmc_mixture_calibration_f64"], syms
    handle = ctypes.CDLL(_lib.build())
    for name in syms:
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    assert re.search(r"#define\s+SGMCMC_CALIB_ABI_VERSION\s+1\s", open(HEADER).read())
    assert _lib.lib().sgmcmc_calib_abi_version() == _lib.CALIB_ABI_VERSION == 1
    assert _lib.lib().sgmcmc_calib_max_draws() == kernels.calib_max_draws() == 4096
    assert "calib" not in open(os.path.join(ROOT, "include", "sgmcmc_hip.h")).read()      # the boundary is what it was
    deps = [os.path.basename(p) for p in _lib.build_dependencies()]
    assert "sgmcmc_calib.hip" in deps and "sgmcmc_hip_calib.h" in deps
    assert diagnostics.calibration.__module__ == "pysgmcmc_amd.diagnostics.calibration"
    assert diagnostics.mixture_calibration_host is mixture_calibration_host and diagnostics.Calibration is Calibration


REQUIRED = ("means", "var", "y", "pit", "crps")


def _call(sfx, ld=5, S=10, n_rows=5, levels=(0.5, 0.9), n_levels=None, n_bins=10, summary=None, **ptrs):
    """The C entry with dummy DEVICE pointers (never read: every refusal comes before a launch); levels is a HOST array."""
    lib = _lib.lib()
    p = dict({name: 4096 for name in REQUIRED})
    p.update(ptrs)
    arr = None if levels is None else (ctypes.c_double * max(1, len(levels)))(*levels)
    n_levels = (0 if levels is None else len(levels)) if n_levels is None else n_levels
    rc = getattr(lib, "sgmcmc_mixture_calibration_" + sfx)(p["means"], ld, S, n_rows, p["var"], p["y"], arr, n_levels, n_bins,
                                                            p["pit"], p["crps"], summary, None)
    return rc, lib.sgmcmc_last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_entry_refuses_bad_arguments_before_any_launch(sfx):
    def refused(text, **kw):
        rc, msg = _call(sfx, **kw)
        assert rc == EINVAL and msg.startswith(b"mixture_calibration: ") and text in msg, (kw, rc, msg)

    for S in (0, 4097, 2 ** 63):
        refused(b"draws, must be 1 .. 4096", S=S)
    refused(b"n_levels = 17, must be 0 .. 16", levels=(0.5,) * 17)
    refused(b"n_levels = -1, must be 0 .. 16", n_levels=-1)
    refused(b"n_bins = 65, must be 0 .. 64", n_bins=65)
    refused(b"n_bins = -1, must be 0 .. 64", n_bins=-1)
    for bad, text in ((0.0, b"0"), (1.0, b"1"), (-0.5, b"-0.5"), (float("nan"), b"nan")):
        refused(b"levels[1] = " + text + b", must lie in (0, 1)", levels=(0.5, bad))
    assert _call(sfx, n_rows=0, means=None)[0] == 0                        # nothing to do wins over the NULLs
    for name in REQUIRED:
        refused(name.encode() + b" is NULL", **{name: None})
    refused(b"levels is NULL with n_levels = 2", levels=None, n_levels=2)
    refused(b"ld = 4 is smaller than n_rows = 5", ld=4)
    refused(b"extent overflows", ld=2 ** 62)
    refused(b"n_rows = 2147483648 is too large for one launch", n_rows=2 ** 31, ld=2 ** 31)
    # an earlier check wins over a later one
    refused(b"draws, must be", S=0, n_bins=65)
    refused(b"n_levels = 17", levels=(2.0,) * 17)
    refused(b"n_bins = 65", n_bins=65, levels=(0.5, 2.0))
    refused(b"levels[0] = 2", levels=(2.0,), means=None)
    refused(b"means is NULL", means=None, var=None)
    refused(b"crps is NULL", crps=None, levels=None, n_levels=1)
    refused(b"levels is NULL", levels=None, n_levels=1, ld=4)
    refused(b"ld = 4 is smaller", ld=4, n_rows=2 ** 31)
    refused(b"extent overflows", ld=2 ** 62, n_rows=2 ** 31)


def _args(S=10, n_rows=3, dtype=torch.float64):
    return torch.zeros(S, n_rows, dtype=dtype), torch.ones(S, dtype=torch.float64), torch.zeros(n_rows, dtype=dtype)


def test_the_binding_refuses_before_a_device_is_touched():
    f64 = torch.float64
    means, var, y = _args()
    call = kernels.mixture_calibration
    with pytest.raises(TypeError, match=r"^mixture_calibration: means must be an \(S, n_rows\)"):
        call(np.zeros((10, 3)), var, y)
    with pytest.raises(ValueError, match=r"^mixture_calibration: means must be \(S, n_rows\), got \(10,\)"):
        call(torch.zeros(10, dtype=f64), var, y)
    for S in (0, 4097):
        with pytest.raises(ValueError, match=r"^mixture_calibration: S = %d draws, must be 1 \.\. 4096" % S):
            call(torch.zeros(S, 3, dtype=f64), var, y, n_bins=65)           # S wins over n_bins
    with pytest.raises(ValueError, match=r"^mixture_calibration: n_levels = 17, must be 0 \.\. 16"):
        call(means, var, y, levels=(2.0,) * 17)                             # the count wins over the values
    for n_bins in (-1, 65):
        with pytest.raises(ValueError, match=r"^mixture_calibration: n_bins = %d, must be 0 \.\. 64" % n_bins):
            call(means, var, y, levels=(0.5, 1.5), n_bins=n_bins)
    for bad, text in ((0.0, "0"), (1.0, "1"), (-0.5, "-0.5"), (float("nan"), "nan")):
        with pytest.raises(ValueError, match=r"^mixture_calibration: levels\[1\] = %s, must lie in \(0, 1\)" % text):
            call(means.to(torch.float16), var, y, levels=(0.5, bad))        # a level wins over the dtype
    with pytest.raises(TypeError, match=r"^mixture_calibration: means must be a float32 or float64 tensor, got torch.float16"):
        call(means.to(torch.float16), var, y)
    with pytest.raises(TypeError, match=r"^mixture_calibration: var must be a torch.float64 tensor"):
        call(means, var.float(), y)
    with pytest.raises(ValueError, match=r"^mixture_calibration: var must be a contiguous \(S,\) = \(10,\) tensor"):
        call(means, torch.ones(9, dtype=f64), y)
    with pytest.raises(TypeError, match=r"^mixture_calibration: y must be a torch.float64 tensor, like means"):
        call(means, var, y.float())
    with pytest.raises(ValueError, match=r"^mixture_calibration: y must be a contiguous \(n_rows,\) = \(3,\) tensor"):
        call(means, var, torch.zeros(4, dtype=f64))
    with pytest.raises(TypeError, match=r"^mixture_calibration: pit must be a torch.float64 tensor"):
        call(means, var, y, pit=torch.zeros(3))
    with pytest.raises(ValueError, match=r"^mixture_calibration: crps must be a contiguous \(n_rows,\) = \(3,\) tensor"):
        call(means, var, y, crps=torch.zeros(6, dtype=f64)[::2])
    with pytest.raises(TypeError, match=r"^mixture_calibration: summary must be a torch.float64 tensor"):
        call(means, var, y, summary=torch.zeros(2))
    with pytest.raises(ValueError, match=r"^mixture_calibration: summary must hold 2 \+ n_levels \+ n_bins = 14"):
        call(means, var, y, levels=(0.5, 0.9), n_bins=10, summary=torch.zeros(13, dtype=f64))
    with pytest.raises(ValueError, match=r"^mixture_calibration: the rows of means must be dense"):
        call(torch.zeros(3, 10, dtype=f64).t(), var, y)
    with pytest.raises(ValueError, match=r"^mixture_calibration: ld = 0 is smaller than n_rows = 3"):
        call(torch.zeros(1, 3, dtype=f64).expand(10, 3), var, y)
    from pysgmcmc_amd._lib import SgmcmcLibraryError
    with pytest.raises(SgmcmcLibraryError, match=r"no CPU fallback; diagnostics.mixture_calibration_host"):
        call(means, var, y)
    with pytest.raises(SgmcmcLibraryError, match="no CPU"):
        diagnostics.calibration(*_args(dtype=torch.float32))
    with pytest.raises(ValueError, match=r"^mixture_calibration: S = 4097 draws"):
        mixture_calibration_host(np.zeros((4097, 1)), np.ones(4097), np.zeros(1))
    with pytest.raises(ValueError, match=r"^mixture_calibration: levels\[0\] = 1, must lie"):
        mixture_calibration_host(np.zeros((4, 1)), np.ones(4), np.zeros(1), (1.0,), 0)
