"""The particle-gradient add-on (include/sgmcmc_hip_particles.h, kernel K15) without a GPU: the header's symbols and its
version, the ctypes declarations, ``sgmcmc_bnn_particles_lds_bytes`` against a Python restatement of the footprint rule,
every refusal of the entry before any launch in the documented order, ``BNNParticleCost.__call__`` plus autograd against the
oracle's analytic cost and gradient in float64, ``bnn_particles`` against ``init_mlp_params``, and an ``SVGDSampler`` with a
plain cost left as it was. What the kernel computes is checked on the GPU (tests/test_bnn_particles_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pysgmcmc_amd import _lib, kernels
from pysgmcmc_amd.data_batches import Placeholder
from pysgmcmc_amd.models import BNNParticleCost, bnn_particles
from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params
from pysgmcmc_amd.samplers import SVGDSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_particles.h")
EINVAL = -1
DEFAULT = [1, 50, 50, 50, 1]


def _prototypes():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_header_declares_four_exported_symbols_and_version_1():
    handle = ctypes.CDLL(_lib.build())
    syms = sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", _prototypes())))
    assert syms == ["sgmcmc_bnn_particles_cost_grad_f32", "sgmcmc_bnn_particles_cost_grad_f64",
                    "sgmcmc_bnn_particles_lds_bytes", "sgmcmc_particles_abi_version"], syms
    for name in syms:
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    assert re.search(r"#define\s+SGMCMC_PARTICLES_ABI_VERSION\s+1\s", open(HEADER).read())
    assert _lib.lib().sgmcmc_particles_abi_version() == _lib.PARTICLES_ABI_VERSION == 1
    assert "bnn_particles_cost_grad" in kernels.__all__ and "bnn_particles_lds_bytes" in kernels.__all__


def test_both_new_files_are_build_dependencies():
    deps = [os.path.basename(p) for p in _lib.build_dependencies()]
    assert "sgmcmc_bnn_particles.hip" in deps and "sgmcmc_hip_particles.h" in deps
    makefile = open(os.path.join(ROOT, "pysgmcmc_amd", "csrc", "Makefile")).read()
    assert "sgmcmc_bnn_particles.hip" in makefile and "sgmcmc_hip_particles.h" in makefile


def test_the_entries_are_declared_with_the_header_s_argument_types():
    lib = _lib.lib()
    vp, sz, ci, cd = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
    text = _prototypes()

    def wanted(ret, name):
        proto = re.search(r"%s\s+%s\s*\((.*?)\)\s*;" % (ret, name), text, flags=re.S).group(1)
        want = []
        for arg in (a.strip() for a in proto.split(",")):
            if arg == "const int *layer_sizes":
                want.append(ctypes.POINTER(ci))
            elif "*" in arg or arg.startswith("sgmcmc_stream_t"):
                want.append(vp)
            elif arg.startswith("size_t"):
                want.append(sz)
            elif arg.startswith("double "):
                want.append(cd)
            else:
                assert arg.startswith("int "), arg
                want.append(ci)
        return want

    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_bnn_particles_cost_grad_" + sfx)
        want = wanted("int", "sgmcmc_bnn_particles_cost_grad_" + sfx)
        assert len(want) == 19 and list(f.argtypes) == want, sfx
        assert f.restype is ci
    assert list(lib.sgmcmc_bnn_particles_lds_bytes.argtypes) == wanted("size_t", "sgmcmc_bnn_particles_lds_bytes") == [
        ctypes.POINTER(ci), ci, ci, sz]
    assert lib.sgmcmc_bnn_particles_lds_bytes.restype is sz
    assert lib.sgmcmc_particles_abi_version.restype is ci


# ---- the footprint ---------------------------------------------------------------------------------------------------------

def _n_params(sizes):
    return sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1


def _rule(sizes, batch, esize):
    """The whole-step kernel's footprint rule (samplers/_fused_bnn.py), 0 where it exceeds the 160 KiB of one CU."""
    lds = 160 + ((2 * sum(sizes) + 1) * batch + _n_params(sizes) + 4) * esize
    return lds if lds <= 160 * 1024 else 0


def test_lds_bytes_is_the_whole_step_kernel_s_footprint_rule():
    nets = [DEFAULT, [3, 5, 7, 1], [2, 4, 3, 1], [4, 1], [30, 6, 1], [1, 40, 40, 40, 1], [2, 180, 180, 1], [2, 197, 197, 1],
            [8] + [16] * 7 + [1], [1, 1]]
    seen_zero = seen_fit = 0
    for sizes in nets:
        for dt, esize in ((torch.float32, 4), (torch.float64, 8)):
            for batch in (1, 2, 3, 5, 20, 49, 50, 65, 116, 117, 1000, 2 ** 31 - 1):
                want = _rule(sizes, batch, esize)
                assert kernels.bnn_particles_lds_bytes(sizes, batch, dt) == want, (sizes, batch, esize)
                seen_zero += want == 0
                seen_fit += want > 0
    assert seen_zero > 20 and seen_fit > 20
    f32, f64 = torch.float32, torch.float64
    assert kernels.bnn_particles_lds_bytes(DEFAULT, 116, f32) == 160 + (305 * 116 + 5252 + 4) * 4 == 162704 > 64 * 1024
    assert kernels.bnn_particles_lds_bytes(DEFAULT, 117, f32) == 0
    assert kernels.bnn_particles_lds_bytes(DEFAULT, 49, f64) == 160 + (305 * 49 + 5256) * 8 <= 160 * 1024
    assert kernels.bnn_particles_lds_bytes(DEFAULT, 50, f64) == 0
    # what the entry refuses has no footprint: the net rules, the batch, the element size; nothing wraps
    raw = _lib.lib().sgmcmc_bnn_particles_lds_bytes
    arr = lambda *s: (ctypes.c_int * len(s))(*s)
    assert raw(arr(3, 7, 2), 2, 4, 4) == 0 and raw(arr(3, 0, 1), 2, 4, 4) == 0 and raw(arr(3, 1), 0, 4, 4) == 0
    assert raw(arr(3, 1), 1, 0, 4) == 0 and raw(arr(3, 1), 1, -5, 4) == 0 and raw(None, 1, 4, 4) == 0
    assert raw(arr(*([3] + [4] * 8 + [1])), 9, 4, 4) == 0
    for esize in (0, 2, 16):
        assert raw(arr(3, 1), 1, 4, esize) == 0
    assert raw(arr(*([2 ** 31 - 1] * 8 + [1])), 8, 2 ** 31 - 1, 8) == 0
    assert raw(arr(3, 1), 1, 4, 4) == 160 + (9 * 4 + 5 + 4) * 4


def test_the_cost_knows_whether_the_kernel_takes_it():
    xp, yp = Placeholder(), Placeholder()
    cost = BNNParticleCost(DEFAULT, xp, yp, batch_size=20, n_examples=100)
    assert cost.n_params == 5252 and cost.use_hip_kernel is True
    assert cost.fits(torch.float32) and cost.fits(torch.float64)                 # at batch_size rows: nothing fed yet
    xp.feed(torch.zeros(117, 1))
    assert not cost.fits(torch.float32) and cost.fits(torch.float32, batch=116)
    assert not cost.fits(torch.float16)
    assert not BNNParticleCost([3] + [4] * 9 + [1], xp, yp, 20, 100).fits(torch.float32)


# ---- the C entry's refusals: host checks first, the dummy device pointers are never dereferenced --------------------------

SIZES = (3, 7, 13, 1)                                   # 147 parameters
POINTERS = ("theta", "Xb", "yb", "grad", "cost_out")


def _call(sfx, n=5, ld=147, sizes=SIZES, n_layers=None, ldx=3, batch=4, ld_grad=147, add_prior=1, **ptrs):
    lib = _lib.lib()
    arr = None if sizes is None else (ctypes.c_int * len(sizes))(*sizes)
    p = dict({name: 4096 for name in POINTERS}, **ptrs)
    f = getattr(lib, "sgmcmc_bnn_particles_cost_grad_" + sfx)
    rc = f(p["theta"], n, ld, arr, (len(sizes) - 1) if n_layers is None else n_layers, p["Xb"], ldx, p["yb"], batch, 20.0,
           100.0, 1.0, 1e-6, 0.01, add_prior, p["grad"], ld_grad, p["cost_out"], None)
    return rc, lib.sgmcmc_last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_entry_refuses_bad_arguments_before_any_launch(sfx):
    def refused(text, **kw):
        rc, msg = _call(sfx, **kw)
        assert rc == EINVAL and msg.startswith(b"bnn_particles_cost_grad: ") and text in msg, (kw, rc, msg)

    for name in POINTERS:
        refused(name.encode() + b" is NULL", **{name: None})
    refused(b"layer_sizes is NULL", sizes=None, n_layers=3)
    # the net rules under the words of the small-net core
    for text, sizes in ((b"1..8 layers", (3,) + (4,) * 8 + (1,)), (b"1..8 layers", (3,)), (b"bad layer size", (3, 0, 1)),
                        (b"the last layer must have one unit", (3, 7, 2))):
        refused(text, sizes=sizes, ld=10 ** 6, ld_grad=10 ** 6)
    for batch in (0, -3):
        refused(b"must be >= 1", batch=batch)
    refused(b"ld = 146 is smaller than n_params = 147", ld=146)
    refused(b"ld = 0 is smaller", ld=0)
    refused(b"ld_grad = 146 is smaller than n_params = 147", ld_grad=146)
    refused(b"ldx = 2 is smaller than the 3 inputs", ldx=2)
    esize = 4 if sfx == "f32" else 8
    big = dict(ld=10 ** 6, ld_grad=10 ** 6, ldx=10 ** 6)
    refused(b"the parameters alone need more than 160 KiB of LDS", sizes=(200, 840 // esize, 1), **big)
    refused(b"need more than 160 KiB of LDS at batch", sizes=[1, 50, 50, 50, 1], batch=117 if sfx == "f32" else 50, ldx=1, **{
        k: v for k, v in big.items() if k != "ldx"})
    refused(b"at batch 2147483647", batch=2 ** 31 - 1)
    refused(b"ld = 1000000 is smaller than n_params", sizes=(2 ** 31 - 1,) * 8 + (1,), **big)           # nothing wraps
    refused(b"must be < 2^31", n=2 ** 31)
    # an earlier check wins over a later one: the NULLs in the header's order, the net, batch, ld, ld_grad, ldx, the footprint,
    # n_particles
    refused(b"theta is NULL", theta=None, Xb=None)
    refused(b"Xb is NULL", Xb=None, yb=None)
    refused(b"yb is NULL", yb=None, grad=None)
    refused(b"grad is NULL", grad=None, cost_out=None)
    refused(b"cost_out is NULL", cost_out=None, sizes=None, n_layers=3)
    refused(b"layer_sizes is NULL", sizes=None, n_layers=0)
    refused(b"the last layer must have one unit", sizes=(3, 7, 2), batch=0)
    refused(b"must be >= 1", batch=0, ld=0)
    refused(b"ld = 0 is smaller", ld=0, ld_grad=0)
    refused(b"ld_grad = 0 is smaller", ld_grad=0, ldx=0)
    refused(b"ldx = 0 is smaller", ldx=0, batch=2 ** 31 - 1)
    refused(b"at batch 2147483647", batch=2 ** 31 - 1, n=2 ** 31)
    # nothing to do is a successful no-op, whatever else is passed
    assert _call(sfx, n=0)[0] == 0
    assert _call(sfx, n=0, theta=None, sizes=(3, 7, 2), batch=0)[0] == 0


def test_the_thin_binding_refuses_host_tensors_loudly():
    z = torch.zeros
    with pytest.raises(_lib.SgmcmcLibraryError, match="no CPU fallback"):
        kernels.bnn_particles_cost_grad(z(2 * 147), 2, 147, SIZES, z(4, 3), z(4), z(2 * 147), 147, z(2), 20, 100, 1.0, 1e-6,
                                        0.01)
    with pytest.raises(ValueError, match="too short"):
        kernels.bnn_particles_cost_grad(z(2 * 147 - 1), 2, 147, SIZES, z(4, 3), z(4), z(2 * 147), 147, z(2), 20, 100, 1.0,
                                        1e-6, 0.01)
    with pytest.raises(ValueError, match=r"Xb must be a \(B, 3\) matrix"):
        kernels.bnn_particles_cost_grad(z(2 * 147), 2, 147, SIZES, z(4, 6)[:, ::2], z(4), z(2 * 147), 147, z(2), 20, 100, 1.0,
                                        1e-6, 0.01)
    with pytest.raises(TypeError, match="yb must be a torch.float32 tensor"):
        kernels.bnn_particles_cost_grad(z(2 * 147), 2, 147, SIZES, z(4, 3), z(4, dtype=torch.float64), z(2 * 147), 147, z(2),
                                        20, 100, 1.0, 1e-6, 0.01)


# ---- the torch cost of one flat particle --------------------------------------------------------------------------------

@pytest.mark.parametrize("wdecay", [1.0, 0.0])
@pytest.mark.parametrize("sizes", [[3, 6, 5, 1], [4, 1], DEFAULT], ids=["3-6-5-1", "4-1", "default"])
def test_the_particle_cost_and_autograd_equal_the_oracle(oracle, sizes, wdecay):
    rng = np.random.default_rng(len(sizes) * 17 + sizes[0])
    params = init_mlp_params(sizes[0], hidden=sizes[1:-1], seed=4, dtype=torch.float64)
    for p in params[1::2]:
        p.normal_(generator=torch.Generator().manual_seed(9))
    B = 20
    X, Y = rng.normal(size=(B, sizes[0])), rng.normal(size=(B, 1))
    xp, yp = Placeholder().feed(torch.tensor(X)), Placeholder().feed(torch.tensor(Y))
    cost = BNNParticleCost(sizes, xp, yp, batch_size=B, n_examples=100, wdecay=wdecay)
    flat = torch.cat([p.reshape(-1) for p in params]).requires_grad_(True)
    assert flat.numel() == cost.n_params == _n_params(sizes)
    for view, p in zip(cost.views(flat), params):
        assert view.shape == p.shape and torch.equal(view.detach(), p)
    nll = cost(flat)
    grad, = torch.autograd.grad(nll, flat)
    c_np, g_np = oracle.bnn_cost_and_grad([p.numpy() for p in params], X, Y, B, 100, wdecay=wdecay)
    assert np.isclose(float(nll.detach()), c_np, rtol=1e-13)
    assert np.allclose(grad.numpy(), np.concatenate([np.asarray(g).reshape(-1) for g in g_np]), rtol=1e-10, atol=1e-14)
    # the statements are BNNCost.negative_log_likelihood's: the same bits, in float32 too
    from pysgmcmc_amd.models.bayesian_neural_network import BNNCost
    for dt in (torch.float64, torch.float32):
        ps = [p.to(dt) for p in params]
        xp.feed(torch.tensor(X, dtype=dt)), yp.feed(torch.tensor(Y, dtype=dt))
        want_nll, want_mse = BNNCost(xp, yp, B, 100, wdecay=wdecay).negative_log_likelihood(ps, xp.value, yp.value)
        got = cost(torch.cat([p.reshape(-1) for p in ps]))
        assert got.dtype == dt and torch.equal(got, want_nll) and torch.equal(cost.last_mse, want_mse)
    xp.feed(torch.tensor(X)), yp.feed(torch.tensor(Y))
    # a (B,) target is the same minibatch
    yp.feed(torch.tensor(Y[:, 0]))
    assert float(cost(flat.detach())) == float(nll.detach())


def test_bnn_particles_are_the_rows_init_mlp_params_gives():
    for dt in (torch.float32, torch.float64):
        rows = bnn_particles(3, 2, hidden=(5, 4), seed=11, dtype=dt)
        assert len(rows) == 3
        for i, row in enumerate(rows):
            want = torch.cat([p.reshape(-1) for p in init_mlp_params(2, hidden=(5, 4), seed=11 + i, dtype=dt)])
            assert row.dtype == dt and row.dim() == 1 and torch.equal(row, want)
        assert not torch.equal(rows[0], rows[1])
    assert bnn_particles(2, 1, seed=0)[0].numel() == 5252 and bnn_particles(0, 1) == []
    assert len(bnn_particles(2, 1)) == 2                                          # unseeded draws


# ---- an SVGD sampler with any other cost is what it was --------------------------------------------------------------------

def test_a_sampler_with_a_plain_cost_never_reaches_the_kernel(monkeypatch):
    calls = []
    monkeypatch.setattr(kernels, "bnn_particles_cost_grad", lambda *a, **k: calls.append(a))
    monkeypatch.setattr(kernels, "bnn_particles_lds_bytes", lambda *a, **k: calls.append(a))
    parts = [torch.tensor([0.5 * i, -0.25 * i, 1.0]) for i in range(4)]
    s = SVGDSampler(parts, lambda p: (p * p).sum(), session="cpu", dtype=torch.float64)
    for name in ("_particles_kernel_fits", "_cost_and_grad_particles"):
        monkeypatch.setattr(SVGDSampler, name, lambda *a, **k: calls.append(name))
    assert "_particle_costs" not in vars(s) and s._particle_costs is None
    before = dict(vars(s))
    cost = s._cost_and_grad()                                                     # vmap or loop, as before
    assert calls == [] and "_particle_costs" not in vars(s)
    assert set(vars(s)) == set(before)
    want = torch.stack([(p.double() ** 2).sum() for p in parts])
    assert torch.allclose(cost, want, rtol=1e-14)
    g = s._matrix("grad")
    assert torch.allclose(g, 2.0 * torch.stack(parts).double(), rtol=1e-14)
    # a BNNParticleCost on the CPU keeps to autograd as well: the kernel route needs a GPU
    xp, yp = Placeholder().feed(torch.zeros(4, 2, dtype=torch.float64)), Placeholder().feed(torch.ones(4, 1, dtype=torch.float64))
    monkeypatch.undo()
    monkeypatch.setattr(kernels, "bnn_particles_cost_grad", lambda *a, **k: calls.append(a))
    bc = BNNParticleCost([2, 3, 1], xp, yp, 4, 10)
    s2 = SVGDSampler(bnn_particles(3, 2, hidden=(3,), seed=1), bc, session="cpu", dtype=torch.float64)
    costs = s2._cost_and_grad()
    assert calls == [] and costs.shape == (3,)
    for i, p in enumerate(bnn_particles(3, 2, hidden=(3,), seed=1)):
        assert np.isclose(float(costs[i]), float(bc(p)), rtol=1e-13)
