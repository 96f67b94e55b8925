"""The all-parameter effective sample size without a GPU: the diagnostics add-on header (include/sgmcmc_hip_diag.h) and what
the library exports for it, the host-side argument checks of sgmcmc_ess_variogram_*, the wrapper's refusal of CPU tensors,
``DeviceTrace`` bookkeeping on CPU tensors and the argument errors of ``effective_n_all``. The kernel itself is tested on
the device in test_device_ess_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_diag.h")
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip.h")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", text)))


def test_diag_header_is_an_add_on_and_the_library_exports_it():
    from pysgmcmc_amd import _lib
    assert _declared(DIAG_HEADER) == ["sgmcmc_diag_abi_version", "sgmcmc_ess_variogram_f32", "sgmcmc_ess_variogram_f64"]
    handle = ctypes.CDLL(_lib.build())
    for name in _declared(DIAG_HEADER):
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    opening = open(DIAG_HEADER).read().split("*/")[0]
    assert "OPTIONAL diagnostics add-on" in opening and "OUTSIDE" in opening and "8(b)" in opening
    # the boundary header keeps its declared set: nothing of the add-on leaked into it
    boundary = _declared(HEADER)
    assert len(boundary) == 71
    assert not [n for n in boundary if "ess" in n.split("_") or "diag" in n]
    lib = _lib.lib()
    assert lib.sgmcmc_abi_version() == 6
    assert lib.sgmcmc_diag_abi_version() == _lib.DIAG_ABI_VERSION == 1
    assert "#define SGMCMC_DIAG_ABI_VERSION 1" in open(DIAG_HEADER).read()


def test_diag_version_is_checked_at_load(monkeypatch):
    from pysgmcmc_amd import _lib
    _lib.build()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "DIAG_ABI_VERSION", 2)
    with pytest.raises(_lib.SgmcmcLibraryError, match="diagnostics ABI"):
        _lib.lib()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_invalid_arguments_are_refused_before_any_launch(sfx):
    """Dummy pointers that are never dereferenced: every call fails (or is a no-op) on the host."""
    from pysgmcmc_amd import _lib
    _lib.build()
    lib = _lib.lib()
    f = getattr(lib, "sgmcmc_ess_variogram_" + sfx)
    dummy = ctypes.c_void_p(4096)
    table = (ctypes.c_void_p * 65)(*([4096] * 65))

    def call(chains=table, m=2, n=10, P=8, ld=8, ess=dummy, staging=0, launch=None):
        return f(chains, m, n, P, ld, ess, None, None, staging, launch, None)

    for kw, text in (({"m": 0}, b"m = 0"), ({"m": 65}, b"m = 65"), ({"m": -1}, b"m = -1"),
                     ({"n": 0}, b"n = 0"), ({"n": 1}, b"n = 1"), ({"n": 1 << 31}, b"n = 2147483648"),
                     ({"ld": 7}, b"ld = 7"), ({"ess": None}, b"non-NULL"), ({"chains": None}, b"non-NULL"),
                     ({"staging": 3}, b"staging"), ({"staging": 1, "n": 100000}, b"does not fit the LDS"),
                     ({"launch": ctypes.byref(_lib.LaunchStruct(100, 0, 0, -1))}, b"block_threads")):
        assert call(**kw) == -1, kw
        assert text in lib.sgmcmc_last_error(), (kw, lib.sgmcmc_last_error())
    holed = (ctypes.c_void_p * 2)(4096, None)
    assert call(chains=holed) == -1 and b"chains[1] is NULL" in lib.sgmcmc_last_error()
    # P = 0 is a successful no-op, whatever else is passed
    assert call(P=0, ld=0) == 0
    assert call(P=0, ld=0, ess=None, chains=None) == 0


def test_wrapper_refuses_cpu_tensors():
    from pysgmcmc_amd import diagnostics, kernels
    from pysgmcmc_amd._lib import SgmcmcLibraryError
    x = torch.zeros(2, 10, 4)
    with pytest.raises(SgmcmcLibraryError):
        kernels.ess_variogram(x, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(SgmcmcLibraryError):
        diagnostics.effective_n_all(x)
    t = diagnostics.DeviceTrace(4, 10, "cpu")
    for _ in range(3):
        t.append(torch.zeros(4))
    with pytest.raises(SgmcmcLibraryError):
        diagnostics.effective_n_all([t, t])


def test_device_trace_bookkeeping():
    from pysgmcmc_amd.diagnostics import DeviceTrace
    t = DeviceTrace(3, 4, "cpu", torch.float64)
    assert len(t) == 0 and t.values().shape == (0, 3) and t.capacity == 4 and t.n_params == 3
    assert t.dtype == torch.float64 and t.device.type == "cpu"
    src = torch.arange(3, dtype=torch.float64)
    for k in range(4):
        t.append(src + k)
        src_before = src.clone()
        assert len(t) == k + 1
        assert torch.equal(src, src_before)
    v = t.values()
    assert v.shape == (4, 3) and torch.equal(v, torch.arange(3, dtype=torch.float64)[None] + torch.arange(4.0, dtype=torch.float64)[:, None])
    assert v.data_ptr() == t.buffer.data_ptr()                 # a view, not a copy
    with pytest.raises(IndexError):
        t.append(src)
    assert len(t) == 4
    with pytest.raises(ValueError):
        DeviceTrace(3, 4, "cpu").append(torch.zeros(4))
    t.reset()
    assert len(t) == 0 and t.values().shape == (0, 3)
    t.append(torch.full((3, 1), 7.0, dtype=torch.float64))     # any shape with n_params elements
    assert torch.equal(t.values(), torch.full((1, 3), 7.0, dtype=torch.float64))


class _FakeArena(object):
    def __init__(self):
        self.theta = torch.zeros(5)
        self.shapes, self.sizes, self.offsets = [(2, 2), (1,)], [4, 1], [0, 4]

    def row(self, name):
        assert name == "theta"
        return self.theta


class _FakeSampler(object):
    def __init__(self, fail_at=None):
        self.arena = _FakeArena()
        self.sample_format = "numpy"
        self.param_names = ["w", "b"]
        self.steps, self.fail_at, self.formats = 0, fail_at, []

    def __next__(self):
        if self.fail_at is not None and self.steps == self.fail_at:
            raise RuntimeError("step failed")
        self.steps += 1
        self.formats.append(self.sample_format)
        self.arena.theta += 1.0
        return None, None


def test_record_keeps_every_kth_step_and_restores_the_sample_format():
    from pysgmcmc_amd.diagnostics import DeviceTrace
    s = _FakeSampler()
    t = DeviceTrace.record(s, 4, keep_every=3)
    assert s.steps == 12 and s.sample_format == "numpy" and set(s.formats) == {"view"}
    assert len(t) == 4 and t.capacity == 4
    assert torch.equal(t.values(), torch.tensor([3.0, 6.0, 9.0, 12.0])[:, None].expand(4, 5))
    assert t.param_names == ["w", "b"] and t.param_shapes == [(2, 2), (1,)]
    s = _FakeSampler(fail_at=5)
    s.sample_format = "device"
    with pytest.raises(RuntimeError, match="step failed"):
        DeviceTrace.record(s, 4, keep_every=2)
    assert s.sample_format == "device"
    with pytest.raises(ValueError):
        DeviceTrace.record(_FakeSampler(), 4, keep_every=0)


def test_effective_n_all_argument_errors():
    from pysgmcmc_amd.diagnostics import DeviceTrace, effective_n_all, effective_sample_sizes_of

    def trace(n, P):
        t = DeviceTrace(P, 8, "cpu")
        for _ in range(n):
            t.append(torch.zeros(P))
        return t

    with pytest.raises(ValueError, match="different numbers of samples"):
        effective_n_all([trace(4, 3), trace(5, 3)])
    with pytest.raises(ValueError, match="different widths"):
        effective_n_all([trace(4, 3), trace(4, 2)])
    with pytest.raises(ValueError, match="at least 2 samples"):
        effective_n_all(trace(1, 3))
    with pytest.raises(ValueError, match="at most 64 chains"):
        effective_n_all(torch.zeros(65, 4, 3))
    with pytest.raises(ValueError, match=r"\(n, P\) or \(m, n, P\)"):
        effective_n_all(torch.zeros(7))
    with pytest.raises(ValueError, match="no traces"):
        effective_n_all([])
    with pytest.raises(TypeError):
        effective_n_all([trace(4, 3), "nope"])
    with pytest.raises(TypeError):
        effective_n_all(3)
    with pytest.raises(ValueError, match="param_shapes"):
        effective_sample_sizes_of(trace(4, 3))
    with pytest.raises(ValueError, match="names"):
        effective_sample_sizes_of(trace(4, 3), param_shapes=[(3,)], names=["a", "b"])


def test_new_names_are_exported_next_to_the_reference_s():
    from pysgmcmc_amd import diagnostics, kernels
    for name in ("DeviceTrace", "effective_n_all", "effective_sample_sizes_of", "effective_sample_sizes", "gelman_rubin",
                 "PYSGMCMCTrace", "pymc3_multitrace"):
        assert name in diagnostics.__all__ and hasattr(diagnostics, name)
    assert "ess_variogram" in kernels.__all__
