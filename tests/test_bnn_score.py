"""The held-out-score add-on (include/sgmcmc_hip_score.h) without a GPU: the header's symbols and its version, the ctypes
declarations, every refusal of the entry before any launch, the Python-side refusals of ``models.heldout_score`` before the
library is reached, ``diagnostics.model_diagnostics`` against independent statements (scipy's logsumexp, numpy's variance),
and the host path of ``BayesianNeuralNetwork.score``. What the kernels compute is checked on the GPU
(tests/test_bnn_score_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pysgmcmc_amd import _lib, kernels
from pysgmcmc_amd.diagnostics import model_diagnostics
from pysgmcmc_amd.diagnostics.device_trace import DeviceTrace
from pysgmcmc_amd.models import BayesianNeuralNetwork, HeldOutScore, heldout_score
from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_score.h")
EINVAL = -1


def _declared_symbols(path=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", text)))


def test_the_header_declares_three_exported_symbols_and_version_1():
    handle = ctypes.CDLL(_lib.build())
    syms = _declared_symbols()
    assert syms == ["sgmcmc_bnn_score_f32", "sgmcmc_bnn_score_f64", "sgmcmc_score_abi_version"], syms
    for name in syms:
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    assert re.search(r"#define\s+SGMCMC_SCORE_ABI_VERSION\s+1\s", open(HEADER).read())
    assert _lib.lib().sgmcmc_score_abi_version() == _lib.SCORE_ABI_VERSION == 1
    # the boundary header and the posterior-predictive add-on are what they were
    assert "score" not in open(os.path.join(ROOT, "include", "sgmcmc_hip.h")).read()
    predict = os.path.join(ROOT, "include", "sgmcmc_hip_predict.h")
    assert _declared_symbols(predict) == ["sgmcmc_bnn_predict_f32", "sgmcmc_bnn_predict_f64", "sgmcmc_bnn_predict_row_tile",
                                          "sgmcmc_predict_abi_version"]
    assert "score" not in open(predict).read() and _lib.lib().sgmcmc_predict_abi_version() == 1
    # the header says that non-finite inputs are not checked
    assert "NOT checked" in open(HEADER).read()
    deps = [os.path.basename(p) for p in _lib.build_dependencies()]
    assert "sgmcmc_bnn_score.hip" in deps and "sgmcmc_hip_score.h" in deps


def test_the_entries_are_declared_with_the_header_s_argument_types():
    lib = _lib.lib()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    # the header's prototypes, argument by argument: pointers -> void *, except the two HOST arrays the entry reads
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for sfx in ("f32", "f64"):
        proto = re.search(r"int\s+sgmcmc_bnn_score_%s\s*\((.*?)\)\s*;" % sfx, text, flags=re.S).group(1)
        want = []
        for arg in (a.strip() for a in proto.split(",")):
            if arg.endswith("*chains"):
                want.append(ctypes.POINTER(vp))
            elif arg == "const int *layer_sizes":
                want.append(ctypes.POINTER(ci))
            elif "*" in arg or arg.startswith("sgmcmc_stream_t"):
                want.append(vp)
            elif arg.startswith("size_t"):
                want.append(sz)
            else:
                assert arg.startswith("int "), arg
                want.append(ci)
        f = getattr(lib, "sgmcmc_bnn_score_" + sfx)
        assert len(want) == 18 and list(f.argtypes) == want, (sfx, proto)
        assert f.restype is ci
    assert lib.sgmcmc_score_abi_version.restype is ci


# ---- the C entry's refusals: host checks first, the dummy device pointers are never dereferenced --------------------------

SIZES = (3, 7, 13, 1)                                   # 147 parameters
REQUIRED = ("X", "y", "means", "row_lppd", "row_pwaic", "ens_mean", "ens_var")


def _call(sfx, m=1, n=7, ld=147, sizes=SIZES, n_layers=None, chains="dummy", n_rows=5, **ptrs):
    lib = _lib.lib()
    arr = None if sizes is None else (ctypes.c_int * len(sizes))(*sizes)
    if chains == "dummy":                               # a real HOST array (it is read) of dummy DEVICE pointers (never read)
        chains = (ctypes.c_void_p * 64)(*[4096 * (c + 1) for c in range(64)])
    p = dict({name: 4096 for name in REQUIRED}, loglik=None, sample_loglik=None, summary=None)
    p.update(ptrs)
    f = getattr(lib, "sgmcmc_bnn_score_" + sfx)
    rc = f(chains, m, n, ld, arr, (len(sizes) - 1) if n_layers is None else n_layers, p["X"], p["y"], n_rows, p["means"],
           p["row_lppd"], p["row_pwaic"], p["ens_mean"], p["ens_var"], p["loglik"], p["sample_loglik"], p["summary"], None)
    return rc, lib.sgmcmc_last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_entry_refuses_bad_arguments_before_any_launch(sfx):
    def refused(text, head=b"bnn_score: ", **kw):
        rc, msg = _call(sfx, **kw)
        assert rc == EINVAL and msg.startswith(head) and text in msg, (kw, rc, msg)

    for m in (0, -1, 65):
        refused(b"chains, must be 1 .. 64", m=m)
    refused(b"chains is NULL", chains=None)
    refused(b"layer_sizes is NULL", sizes=None, n_layers=3)
    for name in REQUIRED:
        refused(name.encode() + b" is NULL", **{name: None})
    holes = (ctypes.c_void_p * 64)(4096, None, 8192)
    refused(b"chains[1] is NULL", chains=holes, m=3)
    refused(b"ld = 146 is smaller than n_params = 147", ld=146)
    refused(b"ld = 0 is smaller", ld=0)
    refused(b"must be < 2^31", m=64, n=2 ** 31 // 64)
    refused(b"must be < 2^31", m=2, n=2 ** 63)                             # no wrap-around
    refused(b"is too large for one launch", n_rows=64 * (2 ** 31 - 1) + 1)
    refused(b"is too large for one launch", n_rows=2 ** 64 - 1)            # no wrap-around
    # the optional outputs change nothing about the refusals
    refused(b"ld = 146 is smaller", ld=146, loglik=4096, sample_loglik=4096, summary=4096)
    # a net K11's plan refuses is refused with K11's text
    for text, sizes in ((b"1..8 layers", (3,) + (4,) * 8 + (1,)), (b"bad layer size", (3, 0, 1)),
                        (b"the last layer must have one unit", (3, 7, 2))):
        refused(text, head=b"bnn_predict: ", sizes=sizes)
    esize = 4 if sfx == "f32" else 8
    refused(b"the parameters alone need more than 160 KiB of LDS", head=b"bnn_predict: ", sizes=(200, 840 // esize, 1),
            ld=10 ** 6)
    refused(b"ONE test row need", head=b"bnn_predict: ", sizes=(100, 1600 // esize, 1), ld=10 ** 6)
    # an earlier check wins over a later one: m, the NULLs in the header's order, chains[c], ld, m * n, n_rows
    refused(b"chains, must be", m=0, X=None)
    refused(b"chains is NULL", chains=None, X=None)
    refused(b"X is NULL", X=None, y=None)
    refused(b"y is NULL", y=None, ens_var=None)
    refused(b"means is NULL", means=None, ld=0)
    refused(b"ens_var is NULL", ens_var=None, chains=holes, m=3)
    refused(b"chains[1] is NULL", chains=holes, m=3, ld=0)
    refused(b"ld = 0 is smaller", ld=0, m=64, n=2 ** 31 // 64)
    refused(b"must be < 2^31", m=64, n=2 ** 31 // 64, n_rows=2 ** 63)
    # nothing to do is a successful no-op, whatever else is passed
    assert _call(sfx, n_rows=0, m=0, X=None)[0] == 0
    assert _call(sfx, n=0, means=None, y=None, sizes=(3, 7, 2))[0] == 0


# ---- Python: refusals that must not reach the library -------------------------------------------------------------------

def _no_library():
    raise AssertionError("the library was asked for")


def test_heldout_score_refuses_before_touching_the_library(monkeypatch):
    monkeypatch.setattr(kernels, "lib", _no_library)
    X, y = torch.zeros(5, 3), torch.zeros(5)
    with pytest.raises(ValueError, match="different widths"):
        heldout_score([torch.zeros(4, 147), torch.zeros(4, 148)], X, y, SIZES)
    with pytest.raises(ValueError, match="heldout_score: the traces are 146 wide, layer sizes .* need 147"):
        heldout_score(torch.zeros(4, 146), X, y, SIZES)
    with pytest.raises(ValueError, match="146 wide"):
        heldout_score(torch.zeros(2, 4, 146), X, y, SIZES)
    with pytest.raises(ValueError, match=r"X must be an \(N, 3\) tensor"):
        heldout_score(torch.zeros(4, 147), torch.zeros(5, 4), y, SIZES)
    with pytest.raises(ValueError, match=r"X must be an \(N, 3\) tensor"):
        heldout_score(torch.zeros(4, 147), np.zeros((5, 3)), y, SIZES)
    with pytest.raises(ValueError, match="layer_sizes"):
        heldout_score(torch.zeros(4, 147), X, y, [3])
    with pytest.raises(ValueError, match="at most 64 separate chains"):
        heldout_score([torch.zeros(4, 147)] * 65, X, y, SIZES)
    # y: (N,) of the traces' dtype and device
    for bad in (torch.zeros(4), torch.zeros(5, 1), torch.zeros(()), np.zeros(5), None):
        with pytest.raises(ValueError, match=r"y must be an \(N,\) = \(5,\) tensor"):
            heldout_score(torch.zeros(4, 147), X, bad, SIZES)
    with pytest.raises(TypeError, match="y must be a torch.float32 tensor on cpu, got torch.float64"):
        heldout_score(torch.zeros(4, 147), X, y.double(), SIZES)
    with pytest.raises(TypeError, match="y must be a torch.float32 tensor on cpu, got torch.float32 on meta"):
        heldout_score(torch.zeros(4, 147), X, torch.zeros(5, device="meta"), SIZES)
    # a CPU tensor: no host path exists, and none is substituted
    for traces in (torch.zeros(4, 147), torch.zeros(2, 4, 147), [torch.zeros(4, 147)] * 3, torch.zeros(4, 150)):
        with pytest.raises(TypeError, match="heldout_score: the traces live on cpu"):
            heldout_score(traces, X, y, SIZES, pointwise=True, per_sample=True)
    full = DeviceTrace(147, 4, "cpu")
    full.advance(4, 1)
    with pytest.raises(TypeError, match="live on cpu"):
        heldout_score(full, X, y, SIZES)
    assert HeldOutScore._fields == ("lppd", "p_waic", "elpd_waic", "rmse", "row_lppd", "row_pwaic", "ens_mean", "ens_var",
                                    "sample_loglik", "loglik")


def test_the_thin_binding_refuses_host_tensors_loudly():
    out = [torch.zeros(5, dtype=torch.float64) for _ in range(4)]
    with pytest.raises(_lib.SgmcmcLibraryError, match="no CPU fallback"):
        kernels.bnn_score(torch.zeros(4, 147), SIZES, torch.zeros(5, 3), torch.zeros(5), torch.zeros(4, 5), *out)
    assert "bnn_score" in kernels.__all__


# ---- diagnostics.model_diagnostics against independent statements -------------------------------------------------------------

def _random_case(seed, S=37, N=23):
    rng = np.random.RandomState(seed)
    means = rng.randn(S, N)
    log_var = np.log(1e-2) + rng.randn(S)
    y = means[0] + 0.3 * rng.randn(N)
    return means, log_var, y


def test_pointwise_log_likelihood_is_the_gaussian_log_density():
    means, log_var, y = _random_case(0)
    got = model_diagnostics.pointwise_log_likelihood(means, log_var, y)
    var = np.exp(log_var)[:, None] + 1e-16
    want = -0.5 * np.log(2.0 * np.pi) - 0.5 * log_var[:, None] - 0.5 * (y[None, :] - means) ** 2 / var
    assert got.shape == (37, 23) and got.dtype == np.float64
    assert np.allclose(got, want, rtol=1e-13, atol=0.0)
    assert model_diagnostics.LOG_2PI == np.log(2.0 * np.pi)
    # float32 inputs are widened, not computed in float32
    got32 = model_diagnostics.pointwise_log_likelihood(means.astype(np.float32), log_var.astype(np.float32),
                                                       y.astype(np.float32))
    again = model_diagnostics.pointwise_log_likelihood(means.astype(np.float32).astype(np.float64),
                                                       log_var.astype(np.float32).astype(np.float64),
                                                       y.astype(np.float32).astype(np.float64))
    assert got32.dtype == np.float64 and np.array_equal(got32, again)
    with pytest.raises(ValueError, match="do not fit"):
        model_diagnostics.pointwise_log_likelihood(means, log_var[:-1], y)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_lppd_against_scipy_logsumexp_and_waic_against_numpy_var(seed):
    from scipy.special import logsumexp
    means, log_var, y = _random_case(seed)
    ll = model_diagnostics.pointwise_log_likelihood(means, log_var, y)
    S, N = ll.shape
    want_rows = logsumexp(ll, axis=0) - np.log(S)
    got_rows = model_diagnostics.log_pointwise_predictive_density(ll)
    assert np.allclose(got_rows, want_rows, rtol=0.0, atol=1e-13 * (1.0 + np.abs(want_rows).max()))
    lppd, p_waic, elpd, row_lppd, row_pwaic = model_diagnostics.waic(ll)
    assert np.array_equal(row_lppd, got_rows)
    want_var = np.var(ll, axis=0, ddof=1)
    assert np.allclose(row_pwaic, want_var, rtol=1e-12, atol=0.0)
    assert np.isclose(lppd, want_rows.mean(), rtol=1e-13) and np.isclose(p_waic, want_var.sum(), rtol=1e-12)
    assert elpd == row_lppd.sum() - p_waic
    want_rmse = np.sqrt(np.mean((means.mean(axis=0) - y) ** 2))
    assert np.isclose(model_diagnostics.ensemble_rmse(means, y), want_rmse, rtol=1e-14)


def test_one_sample_has_no_penalty_and_a_hopeless_row_stays_finite():
    means, log_var, y = _random_case(4, S=1)
    ll = model_diagnostics.pointwise_log_likelihood(means, log_var, y)
    lppd, p_waic, elpd, row_lppd, row_pwaic = model_diagnostics.waic(ll)
    assert p_waic == 0.0 and np.all(row_pwaic == 0.0) and np.array_equal(row_lppd, ll[0]) and elpd == row_lppd.sum()
    # every density of the last row underflows: exp(l) is 0 for all samples, log(mean(exp(l))) would be -inf
    means, log_var, y = _random_case(5)
    y[-1] = 200.0
    ll = model_diagnostics.pointwise_log_likelihood(means, log_var, y)
    assert np.all(ll[:, -1] < -800.0) and np.all(np.exp(ll[:, -1]) == 0.0)
    rows = model_diagnostics.log_pointwise_predictive_density(ll)
    assert np.all(np.isfinite(rows)) and ll[:, -1].max() - np.log(37) <= rows[-1] <= ll[:, -1].max()
    assert np.all(np.isfinite(model_diagnostics.waic(ll)[4]))


# ---- BayesianNeuralNetwork.score: the host path ------------------------------------------------------------------------------

def _tiny_ensemble(normalize):
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
def test_score_on_the_host_is_model_diagnostics_in_the_caller_s_units(monkeypatch, normalize):
    from pysgmcmc_amd.models import scoring
    monkeypatch.setattr(scoring, "heldout_score", lambda *a, **k: _no_library())
    bnn = _tiny_ensemble(normalize)
    rng = np.random.RandomState(0)
    X, y = rng.randn(11, 3), rng.randn(11)
    got = bnn.score(X, y)
    assert sorted(got) == ["elpd_waic", "lppd", "p_waic", "rmse", "row_lppd", "row_pwaic"]
    # the statement, written out: the density of y under network s in the CALLER's units, from predict()'s own outputs
    f, noise = bnn.predict(X, return_individual_predictions=True)           # (5, 11), un-normalised
    ll = -0.5 * np.log(2.0 * np.pi * noise) - 0.5 * (y[None, :] - f) ** 2 / noise
    from scipy.special import logsumexp
    want_rows = logsumexp(ll, axis=0) - np.log(5.0)
    assert got["row_lppd"].shape == got["row_pwaic"].shape == (11,)
    assert np.allclose(got["row_lppd"], want_rows, rtol=0.0, atol=1e-11 * (1.0 + np.abs(want_rows).max()))
    assert np.allclose(got["row_pwaic"], np.var(ll, axis=0, ddof=1), rtol=1e-9, atol=0.0)
    assert np.isclose(got["lppd"], want_rows.mean(), rtol=1e-11)
    assert np.isclose(got["p_waic"], np.var(ll, axis=0, ddof=1).sum(), rtol=1e-9)
    assert np.isclose(got["elpd_waic"], want_rows.sum() - got["p_waic"], rtol=1e-11)
    assert np.isclose(got["rmse"], np.sqrt(np.mean((bnn.predict(X)[0] - y) ** 2)), rtol=1e-12)
    for key in ("lppd", "p_waic", "elpd_waic", "rmse"):
        assert isinstance(got[key], float), key
    if normalize:
        # the same networks scored in their own units: row_lppd shifts by -log(y_std), rmse scales, p_waic stays
        plain = _tiny_ensemble(False)
        xn, yn = (X - bnn.x_mean) / bnn.x_std, (y - bnn.y_mean) / bnn.y_std
        raw = plain.score(xn, yn)
        assert np.allclose(got["row_lppd"], raw["row_lppd"] - np.log(1.9), rtol=0.0, atol=1e-13 * (1 + np.abs(want_rows).max()))
        assert np.array_equal(got["row_pwaic"], raw["row_pwaic"]) and got["p_waic"] == raw["p_waic"]
        assert np.isclose(got["rmse"], raw["rmse"] * 1.9, rtol=1e-15)
        assert np.isclose(got["lppd"], raw["lppd"] - np.log(1.9), rtol=1e-13)
    assert bnn._kept_matrix is None                     # nothing was flattened for the device


def test_score_refuses_what_it_cannot_score():
    bnn = _tiny_ensemble(False)
    with pytest.raises(TypeError, match="live on cpu"):                     # no host fallback behind on_device=True
        bnn.score(np.zeros((4, 3)), np.zeros(4), on_device=True)
    with pytest.raises(ValueError, match="4 rows, y_test 5"):
        bnn.score(np.zeros((4, 3)), np.zeros(5))
    bnn.is_trained = False
    with pytest.raises(ValueError, match="untrained"):
        bnn.score(np.zeros((4, 3)), np.zeros(4))
