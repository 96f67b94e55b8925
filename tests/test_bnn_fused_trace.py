"""The thinned-trace add-on of the whole-step BNN kernel (include/sgmcmc_hip_fused_trace.h) without a GPU: the header's
three symbols and its version, every refusal of the new entry point before any launch, the Python-side refusals of
``kernels.bnn_fused_steps(trace=...)`` / ``fused_bnn_steps(trace=...)`` / ``DeviceTrace.record(fused=True)`` before the
library is reached, and the thinning arithmetic of ``DeviceTrace`` over successive chunks. What a traced launch writes is
checked on the GPU (tests/test_bnn_fused_trace_gpu.py)."""
import ctypes
import os
import re

import pytest
import torch

from pysgmcmc_amd import _lib, kernels
from pysgmcmc_amd.diagnostics.device_trace import DeviceTrace
from pysgmcmc_amd.samplers._fused_bnn import FusedBNNStepsMixin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_fused_trace.h")


def _declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", text)))


def test_the_header_declares_three_exported_symbols_and_version_1():
    handle = ctypes.CDLL(_lib.build())
    syms = _declared_symbols()
    assert syms == ["sgmcmc_bnn_fused_trace_steps_f32", "sgmcmc_bnn_fused_trace_steps_f64",
                    "sgmcmc_fused_trace_abi_version"], syms
    for name in syms:
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    assert re.search(r"#define\s+SGMCMC_FUSED_TRACE_ABI_VERSION\s+1\s", open(HEADER).read())
    assert _lib.lib().sgmcmc_fused_trace_abi_version() == _lib.FUSED_TRACE_ABI_VERSION == 1
    # no experiment knobs, no process-wide setters (tests/test_boundary.py's rules)
    assert not [n for n in syms if "set_" in n or "get_" in n or "probe" in n]


# ---- the C entry's refusals: host checks first, the dummy pointers are never dereferenced --------------------------------

KINDS = {0: (7, 3), 1: (6, 3), 2: (3, 5)}      # kind -> (rows, scalars)


def _call(sfx, kind=0, n_rows=None, n_scalars=None, rows="dummy", n_chains=1, n_steps=13, trace=4096, stride=0, capacity=7,
          row=2, every=4, phase=0, theta=4096):
    lib = _lib.lib()
    real = ctypes.c_float if sfx == "f32" else ctypes.c_double
    nr, ns = KINDS.get(kind, (7, 3))
    sizes = (ctypes.c_int * 4)(3, 7, 13, 1)
    d = ctypes.c_void_p(4096)
    net = (147, 148, n_chains, sizes, 3, d, d, 40, d, 5, 5.0, 40.0, 1.0, 1e-6, 0.01)
    rows_arr = (ctypes.c_void_p * nr)(theta, *[4096] * (nr - 1))
    scalars = (real * 5)(1e-3, 40.0, 0.05, 1.0, 0.0)
    f = getattr(lib, "sgmcmc_bnn_fused_trace_steps_" + sfx)
    rc = f(kind, rows_arr if rows == "dummy" else rows, nr if n_rows is None else n_rows, *net, scalars,
           ns if n_scalars is None else n_scalars, None, 0, n_steps, 0, 0, None, d, trace, stride, capacity, row, every, phase,
           None)
    return rc, lib.sgmcmc_last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_entry_refuses_bad_arguments_before_any_launch(sfx):
    head = b"bnn_fused_trace_steps: "

    def refused(text, **kw):
        rc, msg = _call(sfx, **kw)
        assert rc == -1 and msg.startswith(head) and text in msg, (kw, rc, msg)

    refused(b"kind must be", kind=3)
    refused(b"kind must be", kind=-1)
    for kind, (nr, ns) in KINDS.items():
        refused(b"rows, not", kind=kind, n_rows=nr + 1)
        refused(b"scalars, not", kind=kind, n_scalars=ns - 1)
    refused(b"has 7 rows, not 6", kind=0, n_rows=6)            # SGLD's count under SGHMC's kind
    # the shared checks of the untraced entries, under the new entry's name
    for kind in KINDS:
        refused(b"NULL argument", kind=kind, theta=None)
        refused(b"16-B aligned", kind=kind, theta=4100)
        # the trace arguments, after them
        refused(b"trace is NULL", kind=kind, trace=None)
        refused(b"trace_every must be >= 1", kind=kind, every=0)
        refused(b"trace_phase must be < trace_every", kind=kind, phase=4)
        refused(b"trace_phase must be < trace_every", kind=kind, every=1, phase=1)
    # 13 steps, every 4th: phase 0 keeps 3 rows (2 + 3 <= 5), phase 3 keeps 4 (2 + 4 > 5)
    refused(b"trace_capacity", capacity=4)
    refused(b"trace_capacity", capacity=5, phase=3)
    refused(b"trace_capacity", capacity=7, row=5)
    refused(b"trace_capacity", capacity=7, row=2 ** 64 - 1)       # no wrap-around
    refused(b"trace_capacity", capacity=7, n_steps=2 ** 64 - 1, every=2 ** 63, phase=2 ** 63 - 1, row=6)
    refused(b"trace_chain_stride", n_chains=3, stride=7 * 147 - 1)
    refused(b"trace_chain_stride", n_chains=3, stride=0)
    # an earlier check wins over a later one
    refused(b"NULL argument", theta=None, trace=None)
    refused(b"trace is NULL", trace=None, every=0)
    # n_steps = 0 is a successful no-op, whatever else is passed
    assert _call(sfx, n_steps=0, trace=None, every=0)[0] == 0
    assert _call(sfx, n_steps=0, kind=3)[0] == 0


# ---- Python: refusals that must not reach the library -------------------------------------------------------------------

def _no_library():
    raise AssertionError("the library was asked for")


def _steps(trace, n_chains=1, **kw):
    theta = torch.zeros(148 * n_chains)
    starts = torch.zeros(13 * n_chains, dtype=torch.int32)
    return kernels.bnn_fused_steps("sghmc", (theta,) * 7, [3, 7, 13, 1], torch.zeros(40, 3), torch.zeros(40), starts, 5, 5.0,
                                   40.0, 1.0, 1e-6, 0.01, (1e-3, 40.0, 0.05), 0, 13, 0, 0, torch.zeros(13 * n_chains),
                                   n_chains=n_chains, chain_stride=148, trace=trace, **kw)


def test_bnn_fused_steps_refuses_a_wrong_trace_before_touching_the_library(monkeypatch):
    monkeypatch.setattr(kernels, "lib", _no_library)
    with pytest.raises(TypeError, match="step's dtype"):
        _steps(torch.zeros(7, 147, dtype=torch.float64))
    with pytest.raises(TypeError, match="step's dtype"):
        _steps([[0.0] * 147] * 7)
    with pytest.raises(TypeError, match="lives on"):
        _steps(torch.zeros(7, 147, device="meta"))
    for bad in (torch.zeros(7, 148), torch.zeros(7 * 147), torch.zeros(2, 7, 147), torch.zeros(147, 7).t()):
        with pytest.raises(TypeError, match=r"contiguous \(capacity, 147\)"):
            _steps(bad)
    with pytest.raises(TypeError, match=r"\(3, capacity, 147\)"):
        _steps(torch.zeros(7, 147), n_chains=3)
    with pytest.raises(TypeError, match=r"\(3, capacity, 147\)"):
        _steps(torch.zeros(2, 7, 147), n_chains=3)
    for kw in (dict(trace_every=0), dict(trace_every=4, trace_phase=4), dict(trace_phase=-1), dict(trace_row=-1)):
        with pytest.raises(ValueError, match="trace_every must be >= 1"):
            _steps(torch.zeros(7, 147), **kw)


class _Arena(object):
    n = 147
    shapes = [(3, 7), (7,), (7, 13), (13,), (13, 1), (1,), (1, 1)]
    offsets = [0, 21, 28, 119, 132, 145, 146]

    def row(self, key):
        return torch.zeros(147)


class _Chain(FusedBNNStepsMixin):
    """The mixin over a chain that would fit the kernel: everything after the refusals reaches the library."""
    arena = _Arena()
    _torch_dtype = torch.float32
    device = torch.device("cpu")
    param_names = ["w1", "b1", "w2", "b2", "w3", "b3", "log_var"]

    def fused_bnn_available(self):
        return True

    def _fused_stepsizes(self, n_steps):
        raise AssertionError("the schedule was drawn from before the trace was checked")


def test_fused_bnn_steps_refuses_before_drawing_or_launching(monkeypatch):
    monkeypatch.setattr(kernels, "lib", _no_library)
    s = _Chain()
    trace = DeviceTrace(147, 3, "cpu")
    for k in (0, -2):
        with pytest.raises(ValueError, match="keep_every must be >= 1"):
            s.fused_bnn_steps(13, trace, keep_every=k)
    with pytest.raises(ValueError, match="the trace holds"):
        s.fused_bnn_steps(13, DeviceTrace(148, 3, "cpu"))
    with pytest.raises(ValueError, match="the trace holds"):
        s.fused_bnn_steps(13, DeviceTrace(147, 3, "cpu", dtype=torch.float64))
    with pytest.raises(IndexError, match="capacity of 3 samples exhausted"):
        s.fused_bnn_steps(16, trace, keep_every=4)              # would keep 4
    with pytest.raises(IndexError, match="capacity of 3 samples exhausted"):
        s.fused_bnn_steps(4, trace, keep_every=1)
    trace.steps_since_kept = 3
    with pytest.raises(IndexError):
        s.fused_bnn_steps(13, trace, keep_every=4)              # 3 + 13 = 16 steps: 4 kept
    with pytest.raises(ValueError, match="cannot continue"):
        s.fused_bnn_steps(1, trace, keep_every=2)               # a trace 3 steps past its last kept sample
    assert len(trace) == 0 and trace.steps_since_kept == 3 and trace.param_shapes is None
    # append raises the same error as the launch path
    full = DeviceTrace(147, 0, "cpu")
    with pytest.raises(IndexError, match="capacity of 0 samples exhausted"):
        full.append(torch.zeros(147))
    # a trace that fits reaches the schedule (and would then launch); its parameter description is filled in on the way
    with pytest.raises(AssertionError, match="the schedule was drawn"):
        s.fused_bnn_steps(12, DeviceTrace(147, 3, "cpu"), keep_every=4)


def test_record_fused_needs_a_sampler_that_fits_the_kernel(monkeypatch):
    monkeypatch.setattr(kernels, "lib", _no_library)

    class NoFit(_Chain):
        def fused_bnn_available(self):
            return False

    with pytest.raises(ValueError, match="fused=True needs"):
        DeviceTrace.record(NoFit(), 12, keep_every=2, fused=True)
    with pytest.raises(ValueError, match="fused=True needs"):
        DeviceTrace.record(object(), 12, fused=True)
    with pytest.raises(ValueError, match="keep_every >= 1"):
        DeviceTrace.record(_Chain(), 12, keep_every=0, fused=True)
    t = DeviceTrace.record(_Chain(), 0, keep_every=2, fused=True)        # nothing to keep: nothing launched
    assert len(t) == 0 and t.param_names == _Chain.param_names and t.param_offsets == _Arena.offsets
    assert [tuple(s) for s in t.param_shapes] == _Arena.shapes


def test_chain_group_refuses_a_trace_that_is_no_3d_tensor():
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    group = FusedBNNChains.__new__(FusedBNNChains)
    group.samplers = [_Chain()]
    for bad in (torch.zeros(7, 147), DeviceTrace(147, 7, "cpu")):
        with pytest.raises(TypeError, match=r"\(n_chains, capacity, n_params\)"):
            group.steps(13, trace=bad, keep_every=4)


# ---- the thinning arithmetic over chunks ----------------------------------------------------------------------------------

def test_steps_since_kept_over_chunks():
    """Chunks of 5, 7, 1 steps at keep_every = 4: steps 4 | 8, 12 | none are kept."""
    t = DeviceTrace(3, 3, "cpu")
    assert t.steps_since_kept == 0 and len(t) == 0
    seen = []
    for n in (5, 7, 1):
        assert t.kept_rows(n, 4) == (t.steps_since_kept + n) // 4
        seen.append((t.advance(n, 4), t.steps_since_kept, len(t)))
    assert seen == [(1, 1, 1), (2, 0, 3), (0, 1, 3)]
    # one chunk of 13 ends in the same place
    u = DeviceTrace(3, 3, "cpu")
    assert u.advance(13, 4) == 3 and (len(u), u.steps_since_kept) == (3, 1)
    # a full trace refuses the next kept sample and stays as it was
    with pytest.raises(IndexError, match="capacity of 3 samples exhausted"):
        u.advance(3, 4)
    assert (len(u), u.steps_since_kept) == (3, 1)
    assert u.advance(2, 4) == 0 and u.steps_since_kept == 3
    u.reset()
    assert (len(u), u.steps_since_kept) == (0, 0)
    with pytest.raises(ValueError):
        u.advance(4, 0)
