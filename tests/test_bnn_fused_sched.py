"""The whole-step add-on (include/sgmcmc_hip_fused.h) without a GPU: every declared symbol is exported, the add-on has
its own version, and the HOST table builders -- one block of five derived scalars per step of a stepsize schedule -- give
what the samplers' formulas give (``pysgmcmc/samplers/sghmc.py:111-117,211-217``, ``sgld.py:106-108``,
``relativistic_sghmc.py:105-106,117-125``). Bit equality with the device block of ``sgmcmc_*_scalars_*`` and with the
by-value launches is checked on the GPU (tests/test_bnn_fused_sched_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pysgmcmc_amd import _lib, kernels
from pysgmcmc_amd.stepsize_schedules import BurnInRampStepsizeSchedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_fused.h")

# the samplers' other scalars, in the order of kernels.step_scalars_table
OTHER = {"sghmc": (100.0, 0.05), "sgld": (1.0, 100.0), "rsghmc": (1.5, 0.7, 1.0, 0.25)}


def _declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_of_the_add_on_header():
    handle = ctypes.CDLL(_lib.build())
    syms = _declared_symbols()
    assert len(syms) == 1 + 6 + 4 + 2, syms
    for name in syms:
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    for kind in ("sghmc", "sgld", "rsghmc"):
        assert "sgmcmc_%s_scalars_steps_f32" % kind in syms and "sgmcmc_%s_scalars_steps_f64" % kind in syms
    assert "sgmcmc_bnn_fused_rsghmc_steps_f64" in syms and "sgmcmc_bnn_fused_sgld_sched_steps_f32" in syms
    assert _lib.lib().sgmcmc_fused_abi_version() == _lib.FUSED_ABI_VERSION == 1
    # the add-on carries no experiment knobs and no process-wide setters either (tests/test_boundary.py's rules)
    assert not [n for n in syms if "set_" in n or "get_" in n or "probe" in n]


def _restated(kind, eps, other):
    """The five scalars in float64 numpy, op for op as the samplers state them."""
    eps = np.float64(eps)
    two = np.float64(2.0)
    if kind == "sghmc":
        scale_grad, mdecay = (np.float64(v) for v in other)
        eps_s = eps / np.sqrt(scale_grad)
        return [np.power(eps, two), (two * np.power(eps_s, two)) * mdecay, two * np.power(eps_s, np.float64(3.0)),
                np.power(eps_s, np.float64(4.0)), mdecay]
    if kind == "sgld":
        A, scale_grad = (np.float64(v) for v in other)
        sc = np.float64(1e-16)
        return [eps, A, A - np.float64(0.0), two * eps, scale_grad + ((two * np.sign(scale_grad)) * sc + sc)]
    mass, c, D, b_hat = (np.float64(v) for v in other)
    return [eps, mass, D, (mass * mass) * (c * c), np.sqrt(eps * ((two * D) - (eps * b_hat)))]


@pytest.mark.parametrize("kind", ["sghmc", "sgld", "rsghmc"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_equal_stepsizes_give_identical_rows(kind, dt):
    table = kernels.step_scalars_table(kind, [0.0037] * 9, *OTHER[kind], dtype=dt, device="cpu")
    assert table.shape == (9, 5) and table.dtype == dt and torch.isfinite(table).all()
    for t in range(1, 9):
        assert torch.equal(table[t], table[0])
    one = kernels.step_scalars_table(kind, [0.0037], *OTHER[kind], dtype=dt, device="cpu")
    assert torch.equal(one[0], table[0])
    assert kernels.step_scalars_table(kind, [], *OTHER[kind], dtype=dt, device="cpu").shape == (0, 5)


@pytest.mark.parametrize("kind", ["sghmc", "sgld", "rsghmc"])
def test_ramp_rows_are_the_samplers_formulas_to_one_ulp(kind):
    ramp = BurnInRampStepsizeSchedule(1e-4, 1e-2, burn_in_steps=9)
    eps = [next(ramp) for _ in range(12)]
    assert len(set(eps)) == 10 and eps[-1] == 1e-2
    table = kernels.step_scalars_table(kind, eps, *OTHER[kind], dtype=torch.float64, device="cpu").numpy()
    for t, e in enumerate(eps):
        want = np.array(_restated(kind, e, OTHER[kind]), dtype=np.float64)
        assert (np.abs(table[t] - want) <= np.spacing(np.abs(want))).all(), (kind, t, table[t], want)
    # the stepsize itself travels unrounded where the operator reads it as is
    if kind != "sghmc":
        assert (table[:, 0] == np.array(eps)).all()


def test_table_builders_check_their_arguments_and_need_no_device():
    lib = _lib.lib()
    eps = (ctypes.c_double * 3)(0.01, 0.02, 0.03)
    block = (ctypes.c_double * 15)()
    assert lib.sgmcmc_sghmc_scalars_steps_f64(eps, 3, 100.0, 0.05, block) == 0
    assert block[0] == 0.01 ** 2 or abs(block[0] - 1e-4) < 1e-19
    assert lib.sgmcmc_sghmc_scalars_steps_f64(None, 3, 100.0, 0.05, block) == -1
    assert b"sghmc_scalars_steps" in lib.sgmcmc_last_error()
    assert lib.sgmcmc_rsghmc_scalars_steps_f64(eps, 3, 1.0, 1.0, 1.0, 0.0, None) == -1
    assert b"rsghmc_scalars_steps" in lib.sgmcmc_last_error()
    assert lib.sgmcmc_sgld_scalars_steps_f64(None, 0, 1.0, 100.0, None) == 0          # nothing to fill


def test_whole_step_entries_refuse_null_arguments_before_any_launch():
    """Host checks run first: callable without a device, the dummy pointers are never dereferenced."""
    lib = _lib.lib()
    sizes = (ctypes.c_int * 4)(3, 7, 13, 1)
    d = ctypes.c_void_p(4096)
    net = (147, 148, 1, sizes, 3, d, d, 40, d, 5, 5.0, 40.0, 1.0, 1e-6, 0.01)
    # a NULL theta: every one of the ten entries, through the argtypes _lib declares for it
    table = {"steps": (1e-3,), "sched_steps": (d,)}
    refused = 0
    for sfx in ("f32", "f64"):
        for kind, n_rows, other in (("sghmc", 7, (40.0, 0.05)), ("sgld", 6, (40.0, 1.0))):
            for variant, first in table.items():
                f = getattr(lib, "sgmcmc_bnn_fused_%s_%s_%s" % (kind, variant, sfx))
                rc = f(None, *[d] * (n_rows - 1), *net, *first, *other, 0, 1, 0, 0, None, d, None)
                assert rc == -1 and b"NULL argument" in lib.sgmcmc_last_error(), (kind, variant, sfx)
                assert lib.sgmcmc_last_error().startswith(b"bnn_fused_%s_%s: " % (kind.encode(), variant.encode()))
                refused += 1
        f = getattr(lib, "sgmcmc_bnn_fused_rsghmc_steps_" + sfx)
        assert f(None, d, d, *net, 1e-3, 1.0, 1.0, 1.0, 0.0, None, 0, 1, 0, None, d, None) == -1
        assert lib.sgmcmc_last_error().startswith(b"bnn_fused_rsghmc_steps: NULL argument")
        refused += 1
    assert refused == 10
    assert lib.sgmcmc_bnn_fused_sgld_steps_f32(None, d, d, d, d, d, *net, 1e-3, 40.0, 1.0, 0, 1, 0, 0, None, d, None) == -1
    assert lib.sgmcmc_last_error().startswith(b"bnn_fused_sgld_steps")
    rc = lib.sgmcmc_bnn_fused_sghmc_sched_steps_f32(d, d, d, d, d, d, d, *net, None, 40.0, 0.05, 0, 1, 0, 0, None, d, None)
    assert rc == -1 and b"scalars_steps is NULL" in lib.sgmcmc_last_error()
    rc = lib.sgmcmc_bnn_fused_sgld_sched_steps_f64(d, d, d, d, d, d, *net, None, 40.0, 1.0, 0, 1, 0, 0, None, d, None)
    assert rc == -1 and b"scalars_steps is NULL" in lib.sgmcmc_last_error()
    rc = lib.sgmcmc_bnn_fused_rsghmc_steps_f32(d, None, d, *net, 1e-3, 1.0, 1.0, 1.0, 0.0, None, 0, 1, 0, None, d, None)
    assert rc == -1 and b"NULL argument" in lib.sgmcmc_last_error()
    rc = lib.sgmcmc_bnn_fused_rsghmc_steps_f32(d, ctypes.c_void_p(4100), d, *net, 1e-3, 1.0, 1.0, 1.0, 0.0, None, 0, 1, 0, None,
                                               d, None)
    assert rc == -1 and b"16-B aligned" in lib.sgmcmc_last_error()
    rc = lib.sgmcmc_bnn_fused_rsghmc_steps_f32(d, d, d, *net, 1e-3, 1.0, 1.0, 1.0, 0.0, None, 0, 1, 0, d, d, None)
    assert rc == -1 and b"n_params % 4 == 0" in lib.sgmcmc_last_error()


def test_bnn_fused_steps_refuses_an_unknown_kind_before_touching_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(kernels, "lib", no_library)
    with pytest.raises(ValueError, match="kind must be one of rsghmc, sghmc, sgld"):
        kernels.bnn_fused_steps("svgd", (), [1, 1], None, None, None, 1, 1.0, 1.0, 1.0, 1e-6, 0.01, (1e-3,), 0, 1, 0, 0, None)
