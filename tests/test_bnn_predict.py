"""The posterior-predictive add-on (include/sgmcmc_hip_predict.h) without a GPU: the header's symbols and its version, the
ctypes declarations, every refusal of the entry before any launch, the host's pick of the row tile, the Python-side
refusals of ``models.posterior_predictive`` before the library is reached, and ``BayesianNeuralNetwork.predict`` with its
default ``on_device=False`` being the path it was. What the kernels compute is checked on the GPU
(tests/test_bnn_predict_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pysgmcmc_amd import _lib, kernels
from pysgmcmc_amd.diagnostics.device_trace import DeviceTrace
from pysgmcmc_amd.models import BayesianNeuralNetwork, posterior_predictive
from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params, mlp_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_predict.h")
EINVAL = -1


def _declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", text)))


def test_the_header_declares_four_exported_symbols_and_version_1():
    handle = ctypes.CDLL(_lib.build())
    syms = _declared_symbols()
    assert syms == ["sgmcmc_bnn_predict_f32", "sgmcmc_bnn_predict_f64", "sgmcmc_bnn_predict_row_tile",
                    "sgmcmc_predict_abi_version"], syms
    for name in syms:
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    assert re.search(r"#define\s+SGMCMC_PREDICT_ABI_VERSION\s+1\s", open(HEADER).read())
    assert _lib.lib().sgmcmc_predict_abi_version() == _lib.PREDICT_ABI_VERSION == 1
    # no experiment knobs, no process-wide setters (tests/test_boundary.py's rules); the boundary header is not touched
    assert not [n for n in syms if "set_" in n or "get_" in n or "probe" in n]
    assert "predict" not in open(os.path.join(ROOT, "include", "sgmcmc_hip.h")).read()


def test_the_entries_are_declared_with_the_header_s_argument_types():
    lib = _lib.lib()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_bnn_predict_" + sfx)
        assert list(f.argtypes) == [ctypes.POINTER(vp), ci, sz, sz, ctypes.POINTER(ci), ci, vp, sz, vp, vp, vp, vp, vp], sfx
        assert f.restype is ci
    f = lib.sgmcmc_bnn_predict_row_tile
    assert list(f.argtypes) == [ctypes.POINTER(ci), ci, sz] and f.restype is ci
    assert lib.sgmcmc_predict_abi_version.restype is ci


# ---- the C entry's refusals: host checks first, the dummy device pointers are never dereferenced --------------------------

SIZES = (3, 7, 13, 1)                                   # 147 parameters


def _call(sfx, m=1, n=7, ld=147, sizes=SIZES, n_layers=None, chains="dummy", X=4096, n_rows=5, means=4096, noise_var=None,
          ens_mean=None, ens_var=None):
    lib = _lib.lib()
    arr = None if sizes is None else (ctypes.c_int * len(sizes))(*sizes)
    if chains == "dummy":                               # a real HOST array (it is read) of dummy DEVICE pointers (never read)
        chains = (ctypes.c_void_p * 64)(*[4096 * (c + 1) for c in range(64)])
    f = getattr(lib, "sgmcmc_bnn_predict_" + sfx)
    rc = f(chains, m, n, ld, arr, (len(sizes) - 1) if n_layers is None else n_layers, X, n_rows, means, noise_var,
           ens_mean, ens_var, None)
    return rc, lib.sgmcmc_last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_entry_refuses_bad_arguments_before_any_launch(sfx):
    head = b"bnn_predict: "

    def refused(text, **kw):
        rc, msg = _call(sfx, **kw)
        assert rc == EINVAL and msg.startswith(head) and text in msg, (kw, rc, msg)

    for m in (0, -1, 65):
        refused(b"chains, must be 1 .. 64", m=m)
    refused(b"NULL argument", chains=None)
    refused(b"NULL argument", sizes=None, n_layers=3)
    refused(b"NULL argument", X=None)
    refused(b"NULL argument", means=None)
    holes = (ctypes.c_void_p * 64)(4096, None, 8192)
    refused(b"chains[1] is NULL", chains=holes, m=3)
    refused(b"ens_mean and ens_var go together", ens_mean=4096)
    refused(b"ens_mean and ens_var go together", ens_var=4096)
    refused(b"1..8 layers", sizes=(3, 1), n_layers=0)
    refused(b"1..8 layers", sizes=(3,) + (4,) * 8 + (1,))                  # nine weight layers
    refused(b"bad layer size", sizes=(3, 0, 1))
    refused(b"bad layer size", sizes=(0, 7, 1))
    refused(b"bad layer size", sizes=(3, -2, 1))
    refused(b"the last layer must have one unit", sizes=(3, 7, 2))
    refused(b"ld = 146 is smaller than n_params = 147", ld=146)
    refused(b"ld = 0 is smaller", ld=0)
    refused(b"must be < 2^31", m=64, n=2 ** 31 // 64)
    refused(b"must be < 2^31", m=2, n=2 ** 63)                             # no wrap-around
    # the LDS: parameters that do not fit on their own; parameters that fit but leave no room for ONE test row
    esize = 4 if sfx == "f32" else 8
    refused(b"the parameters alone need more than 160 KiB of LDS", sizes=(200, 840 // esize, 1), ld=10 ** 6)
    refused(b"the parameters alone need more than 160 KiB of LDS", sizes=(2 ** 31 - 1, 2 ** 31 - 1, 1), ld=2 ** 63)
    refused(b"ONE test row need", sizes=(100, 1600 // esize, 1), ld=10 ** 6)
    # an earlier check wins over a later one
    refused(b"chains, must be", m=0, X=None)
    refused(b"NULL argument", X=None, ens_mean=4096)
    refused(b"go together", ens_mean=4096, sizes=(3, 7, 2))
    refused(b"the last layer", sizes=(3, 7, 2), ld=0)
    # nothing to do is a successful no-op, whatever else is passed
    assert _call(sfx, n_rows=0, m=0, X=None)[0] == 0
    assert _call(sfx, n=0, means=None, sizes=(3, 7, 2))[0] == 0


def _tile(sizes, esize):
    """The header's rule: the largest power of two <= 32 whose LDS (parameters + X tile + two activation buffers, each
    rounded up to 4 elements) stays within max(40 KiB, twice the parameter copy), at most 160 KiB; else 1."""
    r4 = lambda v: (v + 3) & ~3
    w = r4(kernels._bnn_n_params(list(sizes)))
    widest = max(list(sizes[1:-1]) + [0])
    need = lambda t: (w + r4(t * sizes[0]) + 2 * r4(t * widest)) * esize
    budget = min(max(40 * 1024, 2 * w * esize), 160 * 1024)
    t = 32
    while t > 1 and need(t) > budget:
        t //= 2
    return t if need(t) <= 160 * 1024 else None


@pytest.mark.parametrize("sizes", [(1, 50, 50, 50, 1), (3, 7, 13, 1), (4, 50, 49, 50, 1), (5, 1), (3, 8, 8, 8, 8, 8, 8, 8, 1),
                                   (10, 190, 190, 1), (10, 134, 134, 1), (300, 100, 1), (100, 392, 1), (100, 396, 1), (100, 400, 1)])
def test_the_row_tile_follows_the_header_s_rule(sizes):
    lib = _lib.lib()
    arr = (ctypes.c_int * len(sizes))(*sizes)
    for dt, esize in ((torch.float32, 4), (torch.float64, 8)):
        want = _tile(sizes, esize)
        got = lib.sgmcmc_bnn_predict_row_tile(arr, len(sizes) - 1, esize)
        if want is None:
            assert got == EINVAL and lib.sgmcmc_last_error().startswith(b"bnn_predict_row_tile: "), (sizes, esize, got)
            with pytest.raises(_lib.SgmcmcLibraryError, match="LDS"):
                kernels.bnn_predict_row_tile(sizes, dt)
        else:
            assert got == want == kernels.bnn_predict_row_tile(sizes, dt), (sizes, esize, got, want)
    assert lib.sgmcmc_bnn_predict_row_tile(arr, len(sizes) - 1, 2) == EINVAL
    assert b"element_size must be 4 or 8" in lib.sgmcmc_last_error()


def test_the_default_net_gets_32_rows_and_the_sizes_the_tile_shrinks_at():
    assert _tile((1, 50, 50, 50, 1), 4) == 32 and _tile((1, 50, 50, 50, 1), 8) == 32
    assert _tile((10, 190, 190, 1), 4) == 4 and _tile((10, 190, 190, 1), 8) is None
    assert _tile((100, 392, 1), 4) == 1 and _tile((100, 396, 1), 4) is None and _tile((300, 100, 1), 4) == 16


# ---- Python: refusals that must not reach the library -------------------------------------------------------------------

def _no_library():
    raise AssertionError("the library was asked for")


def test_posterior_predictive_refuses_before_touching_the_library(monkeypatch):
    monkeypatch.setattr(kernels, "lib", _no_library)
    X = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="different widths"):
        posterior_predictive([torch.zeros(4, 147), torch.zeros(4, 148)], X, SIZES)
    with pytest.raises(ValueError, match="different numbers of samples"):
        posterior_predictive([DeviceTrace(147, 4, "cpu"), torch.zeros(4, 147)], X, SIZES)     # an empty trace and a full one
    with pytest.raises(ValueError, match="146 wide, layer sizes .* need 147"):
        posterior_predictive(torch.zeros(4, 146), X, SIZES)
    with pytest.raises(ValueError, match="146 wide"):
        posterior_predictive(torch.zeros(2, 4, 146), X, SIZES)
    with pytest.raises(ValueError, match=r"X must be an \(N, 3\) tensor"):
        posterior_predictive(torch.zeros(4, 147), torch.zeros(5, 4), SIZES)
    with pytest.raises(ValueError, match=r"X must be an \(N, 3\) tensor"):
        posterior_predictive(torch.zeros(4, 147), np.zeros((5, 3)), SIZES)
    with pytest.raises(ValueError, match="layer_sizes"):
        posterior_predictive(torch.zeros(4, 147), X, [3])
    with pytest.raises(ValueError, match="at most 64 separate chains"):
        posterior_predictive([torch.zeros(4, 147)] * 65, X, SIZES)
    with pytest.raises(ValueError, match=r"\(n, P\) or \(m, n, P\)"):
        posterior_predictive(torch.zeros(147), X, SIZES)
    # a CPU tensor: no host path exists, and none is substituted
    for traces in (torch.zeros(4, 147), torch.zeros(2, 4, 147), [torch.zeros(4, 147)] * 3, torch.zeros(4, 150)):
        with pytest.raises(TypeError, match="live on cpu"):
            posterior_predictive(traces, X, SIZES)
    full = DeviceTrace(147, 4, "cpu")
    full.advance(4, 1)
    with pytest.raises(TypeError, match="live on cpu"):
        posterior_predictive(full, X, SIZES, return_individual_predictions=True)


def test_the_thin_binding_refuses_host_tensors_loudly():
    with pytest.raises(_lib.SgmcmcLibraryError, match="no CPU fallback"):
        kernels.bnn_predict(torch.zeros(4, 147), SIZES, torch.zeros(5, 3), torch.zeros(4, 5))


# ---- BayesianNeuralNetwork.predict: the default is the path it was ----------------------------------------------------------

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
def test_predict_without_on_device_is_the_host_path_it_was(monkeypatch, normalize):
    from pysgmcmc_amd.models import predictive
    monkeypatch.setattr(predictive, "posterior_predictive", lambda *a, **k: _no_library())
    bnn = _tiny_ensemble(normalize)
    X = np.random.RandomState(0).randn(11, 3)
    # the parent's predict, written out: the batched outputs, then numpy on the host
    x = (X - bnn.x_mean) / bnn.x_std if normalize else X
    out = bnn._network_outputs(x)
    means, noise = out[:, :, 0], np.exp(out[:, :, 1])
    em = means.mean(axis=0)
    ev = ((means - em) ** 2).mean(axis=0)
    if normalize:
        means, noise = means * bnn.y_std + bnn.y_mean, noise * bnn.y_std ** 2
        em, ev = em * bnn.y_std + bnn.y_mean, ev * bnn.y_std ** 2
    for kw in ({}, {"on_device": False}):
        got_m, got_v = bnn.predict(X, **kw)
        assert np.array_equal(got_m, em) and np.array_equal(got_v, ev)
        got_f, got_n = bnn.predict(X, return_individual_predictions=True, **kw)
        assert got_f.shape == got_n.shape == (5, 11)
        assert np.array_equal(got_f, means) and np.array_equal(got_n, noise)
    # and those are the networks' outputs, one by one
    with torch.no_grad():
        ref = np.stack([mlp_forward(net, torch.as_tensor(x)).numpy() for net in bnn.samples])
    assert np.allclose(out, ref, rtol=1e-13, atol=1e-13)
    assert bnn._kept_matrix is None                     # nothing was flattened for the device


def test_predict_on_device_has_no_host_fallback():
    bnn = _tiny_ensemble(False)
    with pytest.raises(TypeError, match="live on cpu"):
        bnn.predict(np.zeros((4, 3)), on_device=True)
    flat, sizes = bnn._kept_networks_matrix()
    assert sizes == [3, 8, 5, 1] and tuple(flat.shape) == (5, kernels._bnn_n_params(sizes))
    # a row is W1 (in, out), b1, ..., log_var -- and the matrix is kept until the next train()
    net = bnn.samples[2]
    assert torch.equal(flat[2], torch.cat([p.reshape(-1) for p in net]))
    assert bnn._kept_networks_matrix()[0] is flat
