"""K12, R-hat and effective sample size of every parameter from a strided trace of up to 4096 chains, without a GPU: the
many-chains diagnostics add-on header (include/sgmcmc_hip_chains.h) and what the library exports for it, the host-side
argument checks of sgmcmc_chain_diag_*, the wrapper's and the public functions' refusal of CPU tensors, and the argument
errors of ``chain_diagnostics_all`` / ``gelman_rubin_all``. The kernel itself is tested on the device in
test_chain_diag_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS_HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_chains.h")
DIAG_HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_diag.h")
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip.h")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", text)))


def test_chains_header_is_an_add_on_and_the_library_exports_it():
    from pysgmcmc_amd import _lib
    assert _declared(CHAINS_HEADER) == ["sgmcmc_chain_diag_f32", "sgmcmc_chain_diag_f64", "sgmcmc_chains_abi_version"]
    handle = ctypes.CDLL(_lib.build())
    for name in _declared(CHAINS_HEADER):
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    text = open(CHAINS_HEADER).read()
    opening = text.split("*/")[0]
    assert "OPTIONAL" in opening and "add-on" in opening and "OUTSIDE" in opening and "8(b)" in opening
    assert "#define SGMCMC_CHAINS_ABI_VERSION 1" in text and "#define SGMCMC_CHAINS_MAX_CHAINS 4096" in text
    # the boundary header and the diagnostics add-on keep their declared sets: nothing of this add-on leaked into them
    boundary = _declared(HEADER)
    assert len(boundary) == 71
    assert not [n for n in boundary if "chain_diag" in n or "chains_abi" in n]
    assert _declared(DIAG_HEADER) == ["sgmcmc_diag_abi_version", "sgmcmc_ess_variogram_f32", "sgmcmc_ess_variogram_f64"]
    lib = _lib.lib()
    assert lib.sgmcmc_abi_version() == 6 and lib.sgmcmc_diag_abi_version() == 1
    assert lib.sgmcmc_chains_abi_version() == _lib.CHAINS_ABI_VERSION == 1
    assert _lib.CHAINS_MAX_CHAINS == 4096
    # the sources and the header are among what build() watches
    deps = [os.path.basename(d) for d in _lib.build_dependencies()]
    assert "sgmcmc_chain_diag.hip" in deps and "sgmcmc_hip_chains.h" in deps


def test_chains_version_is_checked_at_load(monkeypatch):
    from pysgmcmc_amd import _lib
    _lib.build()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "CHAINS_ABI_VERSION", 2)
    with pytest.raises(_lib.SgmcmcLibraryError, match="chains ABI"):
        _lib.lib()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_invalid_arguments_are_refused_before_any_launch(sfx):
    """Dummy pointers that are never dereferenced: every call fails (or is a no-op) on the host."""
    from pysgmcmc_amd import _lib
    _lib.build()
    lib = _lib.lib()
    f = getattr(lib, "sgmcmc_chain_diag_" + sfx)
    dummy = ctypes.c_void_p(4096)

    def call(trace=dummy, m=20, n=10, P=8, ld=8, chain_stride=80, rhat=dummy, ess=dummy, raw=None, stop_lag=None, waves=0):
        return f(trace, m, n, P, ld, chain_stride, rhat, ess, raw, stop_lag, waves, None)

    for kw, text in (({"m": 0}, b"m = 0"), ({"m": -1}, b"m = -1"), ({"m": 4097}, b"m = 4097"),
                     ({"n": 0}, b"n = 0"), ({"n": 1}, b"n = 1"), ({"n": 1 << 31}, b"n = 2147483648"),
                     ({"ld": 7}, b"ld = 7"), ({"chain_stride": 79}, b"chain_stride = 79"),
                     ({"ld": 9, "chain_stride": 88}, b"chain_stride = 88"),           # needs 9 * 9 + 8 = 89
                     ({"ld": 1 << 62, "chain_stride": 1 << 63}, b"overflows"),
                     ({"m": 4096, "chain_stride": 1 << 62}, b"overflows"),
                     ({"trace": None}, b"trace must be non-NULL"),
                     ({"rhat": None, "ess": None}, b"at least one of rhat, ess, raw and stop_lag"),
                     ({"waves": 3}, b"waves = 3"), ({"waves": 32}, b"waves = 32"), ({"waves": -1}, b"waves = -1")):
        assert call(**kw) == -1, kw
        assert text in lib.sgmcmc_last_error(), (kw, lib.sgmcmc_last_error())
    # P = 0 is a successful no-op, whatever else is passed
    assert call(P=0, ld=0, chain_stride=0) == 0
    assert call(P=0, ld=0, chain_stride=0, trace=None, rhat=None, ess=None, m=0, n=0, waves=7) == 0


def test_wrapper_and_public_functions_refuse_cpu_tensors():
    from pysgmcmc_amd import diagnostics, kernels
    from pysgmcmc_amd._lib import SgmcmcLibraryError
    x = torch.zeros(20, 10, 4)
    with pytest.raises(SgmcmcLibraryError, match="no CPU fallback"):
        kernels.chain_diag(x, rhat=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(SgmcmcLibraryError):
        kernels.chain_diag(x[0], ess=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(SgmcmcLibraryError):
        diagnostics.chain_diagnostics_all(x)
    with pytest.raises(SgmcmcLibraryError):
        diagnostics.chain_diagnostics_all(x, details=True)
    with pytest.raises(SgmcmcLibraryError):
        diagnostics.gelman_rubin_all(x)
    t = diagnostics.DeviceTrace(4, 10, "cpu")
    for _ in range(3):
        t.append(torch.zeros(4))
    with pytest.raises(SgmcmcLibraryError):
        diagnostics.chain_diagnostics_all([t, t])
    with pytest.raises(SgmcmcLibraryError):
        diagnostics.gelman_rubin_all(t)


def test_wrapper_argument_errors():
    from pysgmcmc_amd import kernels
    with pytest.raises(TypeError):
        kernels.chain_diag([torch.zeros(4, 3)], rhat=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\(m, n, P\) or \(n, P\)"):
        kernels.chain_diag(torch.zeros(7), rhat=torch.zeros(7, dtype=torch.float64))


@pytest.mark.parametrize("name", ["chain_diagnostics_all", "gelman_rubin_all"])
def test_public_argument_errors(name):
    from pysgmcmc_amd import diagnostics
    from pysgmcmc_amd.diagnostics import DeviceTrace
    fn = getattr(diagnostics, name)

    def trace(n, P):
        t = DeviceTrace(P, 8, "cpu")
        for _ in range(n):
            t.append(torch.zeros(P))
        return t

    with pytest.raises(ValueError, match=name + ".*different numbers of samples"):
        fn([trace(4, 3), trace(5, 3)])
    with pytest.raises(ValueError, match="different widths"):
        fn([trace(4, 3), trace(4, 2)])
    with pytest.raises(ValueError, match="at least 2 samples"):
        fn(trace(1, 3))
    with pytest.raises(ValueError, match="at least 2 samples"):
        fn(torch.zeros(3, 1, 5))
    with pytest.raises(ValueError, match="at most 4096 chains, got 4097"):
        fn(torch.zeros(4097, 2, 3))
    with pytest.raises(ValueError, match=r"\(n, P\) or \(m, n, P\)"):
        fn(torch.zeros(7))
    with pytest.raises(ValueError, match="no traces"):
        fn([])
    with pytest.raises(TypeError):
        fn([trace(4, 3), "nope"])
    with pytest.raises(TypeError):
        fn(3)


def test_effective_n_all_still_stops_at_64_chains():
    from pysgmcmc_amd.diagnostics import effective_n_all
    with pytest.raises(ValueError, match="effective_n_all: at most 64 chains"):
        effective_n_all(torch.zeros(65, 4, 3))


def test_new_names_are_exported():
    from pysgmcmc_amd import diagnostics, kernels
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    for name in ("chain_diagnostics_all", "gelman_rubin_all", "effective_n_all", "DeviceTrace", "gelman_rubin"):
        assert name in diagnostics.__all__ and hasattr(diagnostics, name)
    assert "chain_diag" in kernels.__all__ and "ess_variogram" in kernels.__all__
    assert callable(FusedBNNChains.diagnose)
    assert "diagnose" in FusedBNNChains.collect.__doc__ and "64" in FusedBNNChains.collect.__doc__
