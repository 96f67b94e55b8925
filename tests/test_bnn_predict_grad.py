"""The predictive-gradient add-on (include/sgmcmc_hip_predict_grad.h) without a GPU: the header's symbols and its version,
the ctypes declarations, every refusal of the entry before any launch, ``sgmcmc_bnn_predict_grad_row_tile`` against a Python
restatement of the footprint rule, the Python-side refusals of ``models.predictive_gradients`` before the library is reached,
the two statements the kernel is pinned to on the GPU (the backward sweep, the derivative of the variance) against torch
autograd in float64, and the host path of ``BayesianNeuralNetwork.predictive_gradients`` against central differences of
``predict``. What the kernels compute is checked on the GPU (tests/test_bnn_predict_grad_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import predict_grad_cases as C
from pysgmcmc_amd import _lib, kernels
from pysgmcmc_amd.diagnostics.device_trace import DeviceTrace
from pysgmcmc_amd.models import BayesianNeuralNetwork, PredictiveGradients, predictive_gradients
from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params, mlp_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_predict_grad.h")
EINVAL = -1


def _declared_symbols(path=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", text)))


def test_the_header_declares_four_exported_symbols_and_version_1():
    handle = ctypes.CDLL(_lib.build())
    syms = _declared_symbols()
    assert syms == ["sgmcmc_bnn_predict_grad_f32", "sgmcmc_bnn_predict_grad_f64", "sgmcmc_bnn_predict_grad_row_tile",
                    "sgmcmc_predict_grad_abi_version"], syms
    for name in syms:
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    text = open(HEADER).read()
    assert re.search(r"#define\s+SGMCMC_PREDICT_GRAD_ABI_VERSION\s+1\s", text)
    assert re.search(r"#define\s+SGMCMC_PREDICT_GRAD_MAX_CHAINS\s+64\s", text)
    assert _lib.lib().sgmcmc_predict_grad_abi_version() == _lib.PREDICT_GRAD_ABI_VERSION == 1
    # the boundary header and the other add-ons are what they were
    for name in ("sgmcmc_hip.h", "sgmcmc_hip_predict.h", "sgmcmc_hip_score.h", "sgmcmc_hip_chains.h", "sgmcmc_hip_diag.h",
                 "sgmcmc_hip_fused.h", "sgmcmc_hip_fused_trace.h"):
        assert "predict_grad" not in open(os.path.join(ROOT, "include", name)).read().lower(), name
    # the grid rule a GPU test depends on is written down
    assert "grid.y = min(n_tiles, ceil(4096 / S), 65535)" in text


def test_both_new_files_are_build_dependencies():
    deps = [os.path.basename(p) for p in _lib.build_dependencies()]
    assert "sgmcmc_bnn_predict_grad.hip" in deps and "sgmcmc_hip_predict_grad.h" in deps
    makefile = open(os.path.join(ROOT, "pysgmcmc_amd", "csrc", "Makefile")).read()
    assert "sgmcmc_bnn_predict_grad.hip" in makefile and "sgmcmc_hip_predict_grad.h" in makefile


def test_the_entries_are_declared_with_the_header_s_argument_types():
    lib = _lib.lib()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    # the header's prototypes, argument by argument: pointers -> void *, except the two HOST arrays the entry reads
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def wanted(name):
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
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
        return want

    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_bnn_predict_grad_" + sfx)
        want = wanted("sgmcmc_bnn_predict_grad_" + sfx)
        assert len(want) == 15 and list(f.argtypes) == want, sfx
        assert f.restype is ci
    assert list(lib.sgmcmc_bnn_predict_grad_row_tile.argtypes) == wanted("sgmcmc_bnn_predict_grad_row_tile") == [
        ctypes.POINTER(ci), ci, sz]
    assert lib.sgmcmc_bnn_predict_grad_row_tile.restype is ci
    assert lib.sgmcmc_predict_grad_abi_version.restype is ci


# ---- the C entry's refusals: host checks first, the dummy device pointers are never dereferenced --------------------------

SIZES = (3, 7, 13, 1)                                   # 147 parameters
REQUIRED = ("X", "means", "grads")
ENSEMBLE = ("ens_mean", "ens_var", "dmean", "dvar")


def _call(sfx, m=1, n=7, ld=147, sizes=SIZES, n_layers=None, chains="dummy", n_rows=5, **ptrs):
    lib = _lib.lib()
    arr = None if sizes is None else (ctypes.c_int * len(sizes))(*sizes)
    if chains == "dummy":                               # a real HOST array (it is read) of dummy DEVICE pointers (never read)
        chains = (ctypes.c_void_p * 64)(*[4096 * (c + 1) for c in range(64)])
    p = dict({name: 4096 for name in REQUIRED}, **{name: None for name in ENSEMBLE})
    p.update(ptrs)
    f = getattr(lib, "sgmcmc_bnn_predict_grad_" + sfx)
    rc = f(chains, m, n, ld, arr, (len(sizes) - 1) if n_layers is None else n_layers, p["X"], n_rows, p["means"], p["grads"],
           p["ens_mean"], p["ens_var"], p["dmean"], p["dvar"], None)
    return rc, lib.sgmcmc_last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_entry_refuses_bad_arguments_before_any_launch(sfx):
    def refused(text, **kw):
        rc, msg = _call(sfx, **kw)
        assert rc == EINVAL and msg.startswith(b"bnn_predict_grad: ") and text in msg, (kw, rc, msg)

    for m in (0, -1, 65):
        refused(b"chains, must be 1 .. 64", m=m)
    refused(b"chains is NULL", chains=None)
    refused(b"layer_sizes is NULL", sizes=None, n_layers=3)
    for name in REQUIRED:
        refused(name.encode() + b" is NULL", **{name: None})
    # the four ensemble outputs: all, or none
    for given in range(1, 15):
        some = {name: 4096 for k, name in enumerate(ENSEMBLE) if given >> k & 1}
        refused(b"go together", **some)
    holes = (ctypes.c_void_p * 64)(4096, None, 8192)
    refused(b"chains[1] is NULL", chains=holes, m=3)
    refused(b"ld = 146 is smaller than n_params = 147", ld=146)
    refused(b"ld = 0 is smaller", ld=0)
    refused(b"must be < 2^31", m=64, n=2 ** 31 // 64)
    refused(b"must be < 2^31", m=2, n=2 ** 63)                             # no wrap-around
    refused(b"is too large for one launch", n_rows=64 * (2 ** 31 - 1) + 1)
    refused(b"is too large for one launch", n_rows=2 ** 64 - 1)            # no wrap-around
    refused(b"n_rows * D0", sizes=(5, 1), n_rows=256 * (2 ** 31 - 1) // 5 + 1)      # n_rows itself would do
    assert _call(sfx, n_rows=0)[0] == 0
    # K11's net rules in K11's wording
    for text, sizes in ((b"1..8 layers", (3,) + (4,) * 8 + (1,)), (b"1..8 layers", (3,)), (b"bad layer size", (3, 0, 1)),
                        (b"the last layer must have one unit", (3, 7, 2))):
        refused(text, sizes=sizes, ld=10 ** 6)
    esize = 4 if sfx == "f32" else 8
    refused(b"the parameters alone need more than 160 KiB of LDS", sizes=(200, 840 // esize, 1), ld=10 ** 6)
    refused(b"ONE test row need", sizes=(100, 1600 // esize, 1), ld=10 ** 6)
    refused(b"ld = 1000000 is smaller than n_params", sizes=(2 ** 31 - 1,) * 8 + (1,), ld=10 ** 6)      # nothing wraps
    # the ensemble outputs change nothing about the refusals
    refused(b"ld = 146 is smaller", ld=146, **{name: 4096 for name in ENSEMBLE})
    # an earlier check wins over a later one: m, the NULLs in the header's order, all-or-none, the net, chains[c], ld, m * n,
    # n_rows, the LDS
    refused(b"chains, must be", m=0, X=None)
    refused(b"chains is NULL", chains=None, sizes=None, n_layers=3)
    refused(b"layer_sizes is NULL", sizes=None, n_layers=3, X=None)
    refused(b"X is NULL", X=None, means=None)
    refused(b"means is NULL", means=None, grads=None)
    refused(b"grads is NULL", grads=None, dvar=4096)
    refused(b"go together", dvar=4096, sizes=(3, 7, 2))
    refused(b"the last layer must have one unit", sizes=(3, 7, 2), chains=holes, m=3)
    refused(b"chains[1] is NULL", chains=holes, m=3, ld=0)
    refused(b"ld = 0 is smaller", ld=0, m=64, n=2 ** 31 // 64)
    refused(b"must be < 2^31", m=64, n=2 ** 31 // 64, n_rows=2 ** 63)
    refused(b"is too large for one launch", n_rows=2 ** 63, sizes=(100, 1600 // esize, 1), ld=10 ** 6)
    # nothing to do is a successful no-op, whatever else is passed
    assert _call(sfx, n_rows=0, m=0, X=None)[0] == 0
    assert _call(sfx, n=0, means=None, grads=None, sizes=(3, 7, 2), dvar=4096)[0] == 0


# ---- the row tile against the footprint rule --------------------------------------------------------------------------------

def _row_tile(sizes, esize):
    return _lib.lib().sgmcmc_bnn_predict_grad_row_tile((ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, esize)


def test_the_row_tile_follows_the_footprint_rule():
    seen = set()
    nets = C.NETS + [[1, 40, 40, 40, 1],                # 32 rows in f32; the tile halves in f64
                     [2, 180, 180, 1],                  # 130 KiB of parameters in f32: 8 rows; f64: refused
                     [2, 197, 197, 1]]                  # 155 KiB of parameters in f32: one row is all that fits; f64: refused
    for sizes in nets:
        for esize in (4, 8):
            want = C.row_tile_rule(sizes, esize)
            got = _row_tile(sizes, esize)
            assert got == (want if want is not None else EINVAL), (sizes, esize, got, want)
            seen.add(want)
            if want is not None:
                dt = {4: torch.float32, 8: torch.float64}[esize]
                assert kernels.bnn_predict_grad_row_tile(sizes, dt) == want
    # worked by hand for the default net: 5252 parameters (a multiple of 4); at 16 rows the X tile is 16 elements, three
    # activation buffers and two delta buffers of 16 * 50 = 800 each: 9268 elements
    assert C.footprint_bytes([1, 50, 50, 50, 1], 4, 16) == 4 * (5252 + 16 + 5 * 800) == 37072
    assert C.footprint_bytes([1, 50, 50, 50, 1], 4, 32) == 4 * (5252 + 32 + 5 * 1600) > 2 * 4 * 5252 > 40 * 1024
    assert _row_tile([1, 50, 50, 50, 1], 4) == 16 and _row_tile([1, 50, 50, 50, 1], 8) == 16
    assert _row_tile([1, 40, 40, 40, 1], 4) == 32 and _row_tile([1, 40, 40, 40, 1], 8) == 16
    assert _row_tile([2, 180, 180, 1], 4) == 8
    assert _row_tile([5, 1], 4) == _row_tile([5, 1], 8) == 32
    # one row only: the parameters exceed half the LDS, so the budget is all 160 KiB, and two rows do not fit
    assert _row_tile([2, 197, 197, 1], 4) == 1
    assert C.footprint_bytes([2, 197, 197, 1], 4, 2) > 160 * 1024 >= C.footprint_bytes([2, 197, 197, 1], 4, 1)
    assert {1, 8, 16, 32, None} <= seen
    # refused: by the LDS, by the net rules, by the element size
    assert _row_tile([2, 197, 197, 1], 8) == EINVAL and _lib.lib().sgmcmc_last_error().startswith(b"bnn_predict_grad_row_tile: ")
    assert _row_tile([100, 1600 // 4, 1], 4) == EINVAL and b"ONE test row" in _lib.lib().sgmcmc_last_error()
    assert C.row_tile_rule([100, 1600 // 4, 1], 4) is None
    assert _row_tile([3, 7, 2], 4) == EINVAL and _row_tile([3, 0, 1], 4) == EINVAL
    for esize in (0, 2, 16):
        assert _row_tile([3, 7, 1], esize) == EINVAL
    with pytest.raises(_lib.SgmcmcLibraryError, match="160 KiB"):
        kernels.bnn_predict_grad_row_tile([2, 197, 197, 1], torch.float64)


# ---- Python: refusals that must not reach the library -------------------------------------------------------------------

def _no_library(*args, **kwargs):
    raise AssertionError("the library was asked for")


def test_predictive_gradients_refuses_before_touching_the_library(monkeypatch):
    monkeypatch.setattr(kernels, "bnn_predict_grad", _no_library)
    monkeypatch.setattr(kernels, "lib", _no_library)
    X = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="different widths"):
        predictive_gradients([torch.zeros(4, 147), torch.zeros(4, 148)], X, SIZES)
    with pytest.raises(ValueError, match="predictive_gradients: the traces are 146 wide, layer sizes .* need 147"):
        predictive_gradients(torch.zeros(4, 146), X, SIZES)
    with pytest.raises(ValueError, match="146 wide"):
        predictive_gradients(torch.zeros(2, 4, 146), X, SIZES)
    with pytest.raises(ValueError, match=r"X must be an \(N, 3\) tensor"):
        predictive_gradients(torch.zeros(4, 147), torch.zeros(5, 4), SIZES)
    with pytest.raises(ValueError, match=r"X must be an \(N, 3\) tensor"):
        predictive_gradients(torch.zeros(4, 147), torch.zeros(5), SIZES)
    with pytest.raises(ValueError, match=r"X must be an \(N, 3\) tensor"):
        predictive_gradients(torch.zeros(4, 147), np.zeros((5, 3)), SIZES)
    with pytest.raises(ValueError, match="layer_sizes"):
        predictive_gradients(torch.zeros(4, 147), X, [3])
    with pytest.raises(ValueError, match="at most 64 separate chains"):
        predictive_gradients([torch.zeros(4, 147)] * 65, X, SIZES)
    # a CPU tensor: no host path exists, and none is substituted
    for traces in (torch.zeros(4, 147), torch.zeros(2, 4, 147), [torch.zeros(4, 147)] * 3, torch.zeros(4, 150)):
        for individual in (False, True):
            with pytest.raises(TypeError, match="predictive_gradients: the traces live on cpu"):
                predictive_gradients(traces, X, SIZES, return_individual=individual)
    full = DeviceTrace(147, 4, "cpu")
    full.advance(4, 1)
    with pytest.raises(TypeError, match="live on cpu"):
        predictive_gradients(full, X, SIZES)
    meta = torch.zeros(4, 147, device="meta")
    assert meta.is_cuda is False
    with pytest.raises(TypeError, match="live on meta"):
        predictive_gradients(meta, torch.zeros(5, 3, device="meta"), SIZES)
    assert PredictiveGradients._fields == ("mean", "var", "dmean", "dvar")


class _DeviceLike(torch.Tensor):
    """A host tensor that says it lives on the device: lets the dtype, device and emptiness refusals be reached without a GPU."""
    is_cuda = True


def test_predictive_gradients_refuses_a_mismatched_x_and_empty_traces(monkeypatch):
    monkeypatch.setattr(kernels, "bnn_predict_grad", _no_library)
    monkeypatch.setattr(kernels, "lib", _no_library)
    traces = torch.zeros(4, 147).as_subclass(_DeviceLike)
    with pytest.raises(TypeError, match="X must be a torch.float32 tensor on cpu"):
        predictive_gradients(traces, torch.zeros(5, 3, dtype=torch.float64), SIZES)
    with pytest.raises(TypeError, match="X must be a torch.float32 tensor on cpu"):
        predictive_gradients(traces, torch.zeros(5, 3, device="meta"), SIZES)
    with pytest.raises(ValueError, match="the traces hold no samples"):
        predictive_gradients(torch.zeros(0, 147).as_subclass(_DeviceLike), torch.zeros(5, 3), SIZES)
    with pytest.raises(ValueError, match="the traces hold no samples"):
        predictive_gradients(torch.zeros(3, 0, 147).as_subclass(_DeviceLike), torch.zeros(5, 3), SIZES)


def test_the_thin_binding_refuses_host_tensors_loudly():
    with pytest.raises(_lib.SgmcmcLibraryError, match="no CPU fallback"):
        kernels.bnn_predict_grad(torch.zeros(4, 147), SIZES, torch.zeros(5, 3), torch.zeros(4, 5), torch.zeros(4, 5, 3))
    assert "bnn_predict_grad" in kernels.__all__ and "bnn_predict_grad_row_tile" in kernels.__all__


# ---- the two statements the kernel is pinned to, against torch autograd in float64 ---------------------------------------

def test_the_statement_of_dvar_is_the_derivative_of_the_population_variance():
    rng = np.random.RandomState(0)
    for S, N, D in ((1, 3, 2), (7, 5, 3), (40, 4, 1)):
        # f_s(x) = a_s . tanh(B_s x): any smooth function with a known gradient will do
        A, B = rng.randn(S, 6), rng.randn(S, 6, D)
        x = torch.tensor(rng.randn(N, D), requires_grad=True)
        f = torch.einsum("sk,snk->sn", torch.tensor(A), torch.tanh(torch.einsum("skd,nd->snk", torch.tensor(B), x)))
        g = np.stack([torch.autograd.grad(f[s].sum(), x, retain_graph=True)[0].numpy() for s in range(S)])
        want_dvar = torch.autograd.grad(((f - f.mean(0)) ** 2).mean(0).sum(), x, retain_graph=True)[0].numpy()
        want_dmean = torch.autograd.grad(f.mean(0).sum(), x)[0].numpy()
        fn = f.detach().numpy()
        dmean, dvar = C.ensemble_statement(fn, g, fn.mean(axis=0))
        plain = 2.0 * ((fn - fn.mean(axis=0))[:, :, None] * g).sum(axis=0) / S
        for got, want in ((dvar, want_dvar), (plain, want_dvar), (dmean, want_dmean)):
            assert got.shape == (N, D)
            assert np.all(np.abs(got - want) <= 1e-13 * np.maximum(1.0, np.abs(want))), (S, np.abs(got - want).max())
        if S == 1:
            assert np.all(dvar == 0.0) and np.array_equal(dmean, g[0])


@pytest.mark.parametrize("sizes", C.NETS, ids=C.NET_IDS)
def test_the_backward_statement_is_autograd_of_mlp_forward(sizes):
    rng = np.random.RandomState(len(sizes) * 131 + sizes[0])
    P = C.n_params(sizes)
    base = torch.cat([p.reshape(-1) for p in init_mlp_params(sizes[0], hidden=sizes[1:-1], seed=5)]).numpy()
    X = rng.uniform(-1.0, 1.0, size=(9, sizes[0]))
    worst = 0.0
    for s in range(4):
        theta = base + 0.1 * rng.randn(P)
        params = C.split(theta, sizes)
        mean, grad = C.backward_statement(params, X)
        x = torch.tensor(X, requires_grad=True)
        out = mlp_forward([torch.from_numpy(p.copy()) for p in params], x)[:, 0]
        want = torch.autograd.grad(out.sum(), x)[0].numpy()
        assert grad.shape == want.shape == X.shape and grad.dtype == np.float64
        assert np.all(np.abs(mean - out.detach().numpy()) <= 1e-13)
        worst = max(worst, float(np.abs(grad - want).max()))
        if len(sizes) == 2:
            assert np.array_equal(grad, np.repeat(params[0][:, 0][None, :], 9, axis=0))
    assert worst <= 1e-13, worst


# ---- BayesianNeuralNetwork.predictive_gradients: the host path -----------------------------------------------------------

def _tiny_ensemble(normalize_input, normalize_output):
    bnn = BayesianNeuralNetwork(session="cpu", dtype=torch.float64, n_nets=5, normalize_input=normalize_input,
                                normalize_output=normalize_output)
    bnn.is_trained = True
    for k in range(5):
        net = init_mlp_params(3, hidden=(8, 5), seed=k, dtype=torch.float64)
        net[1].normal_(generator=torch.Generator().manual_seed(k))
        net[-1].fill_(-2.0 - 0.1 * k)
        bnn.samples.append(net)
    if normalize_input:
        bnn.x_mean, bnn.x_std = np.array([0.1, -0.2, 0.3]), np.array([1.5, 0.5, 2.0])
    if normalize_output:
        bnn.y_mean, bnn.y_std = 0.7, 1.9
    return bnn


@pytest.mark.parametrize("normalize_input, normalize_output", [(False, False), (True, True), (True, False), (False, True)])
def test_the_host_path_is_the_derivative_of_predict_in_the_caller_s_units(monkeypatch, normalize_input, normalize_output):
    from pysgmcmc_amd.models import predictive
    monkeypatch.setattr(predictive, "predictive_gradients", _no_library)
    bnn = _tiny_ensemble(normalize_input, normalize_output)
    X = np.random.RandomState(0).randn(11, 3)
    dmean, dvar = bnn.predictive_gradients(X)
    assert dmean.shape == dvar.shape == (11, 3) and dmean.dtype == dvar.dtype == np.float64
    h = 1e-5
    for d in range(3):
        step = np.zeros(3)
        step[d] = h
        (m_hi, v_hi), (m_lo, v_lo) = bnn.predict(X + step), bnn.predict(X - step)
        for got, want in ((dmean[:, d], (m_hi - m_lo) / (2 * h)), (dvar[:, d], (v_hi - v_lo) / (2 * h))):
            assert np.all(np.abs(got - want) <= 1e-6 * np.maximum(1.0, np.abs(got))), (d, np.abs(got - want).max())
    # the chunking of the rows changes nothing: one row per pass
    monkeypatch.setattr(BayesianNeuralNetwork, "PREDICT_ACTIVATION_BYTES", 1)
    again = bnn.predictive_gradients(X)
    assert np.allclose(again[0], dmean, rtol=1e-14, atol=0.0) and np.allclose(again[1], dvar, rtol=1e-13, atol=1e-16)
    assert bnn._kept_matrix is None                     # nothing was flattened for the device
    if normalize_input and normalize_output:
        # the same networks in their own units
        plain = _tiny_ensemble(False, False)
        raw = plain.predictive_gradients((X - bnn.x_mean) / bnn.x_std)
        assert np.allclose(dmean, 1.9 * raw[0] / bnn.x_std, rtol=1e-14, atol=0.0)
        assert np.allclose(dvar, 1.9 ** 2 * raw[1] / bnn.x_std, rtol=1e-14, atol=0.0)


def test_predictive_gradients_refuses_what_it_cannot_differentiate():
    bnn = _tiny_ensemble(False, False)
    with pytest.raises(TypeError, match="live on cpu"):                     # no host fallback behind on_device=True
        bnn.predictive_gradients(np.zeros((4, 3)), on_device=True)
    bnn.is_trained = False
    with pytest.raises(ValueError, match="untrained"):
        bnn.predictive_gradients(np.zeros((4, 3)))
