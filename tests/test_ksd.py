"""The kernel Stein discrepancy add-on K16 (include/sgmcmc_hip_ksd.h, csrc/sgmcmc_ksd.hip) without a GPU: the header's symbols
and version, the ctypes declarations, the workspace size, every refusal of the entry before any launch in the documented
order, the launch plan against the case table of ``ksd_cases.py``, the ``C`` constants of the entrywise bar; the host
statement ``diagnostics.stein`` against the definition of the Stein kernel by double autograd, its symmetry, diagonal and sum
order, known behaviour on Gaussian draws; and ``models.bnn_posterior_scores`` on the CPU. What the kernels compute is checked
on the GPU (tests/test_ksd_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pysgmcmc_amd import _lib, diagnostics, kernels, models
from pysgmcmc_amd.data_batches import Placeholder
from pysgmcmc_amd.diagnostics import stein

import ksd_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_ksd.h")
EINVAL = -1
MEAN, GRAM, REDUCE, PAIR, FINISH = M.MEAN, M.GRAM, M.REDUCE, M.PAIR, M.FINISH


def _prototypes():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- symbols and calls ------------------------------------------------------------------------------------------------------

def test_the_header_declares_six_exported_symbols_and_version_1():
    handle = ctypes.CDLL(_lib.build())
    syms = sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", _prototypes())))
    assert syms == ["sgmcmc_ksd_abi_version", "sgmcmc_ksd_f32", "sgmcmc_ksd_f64", "sgmcmc_ksd_max_samples",
                    "sgmcmc_ksd_plan", "sgmcmc_ksd_workspace_bytes"], syms
    for name in syms:
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    assert re.search(r"#define\s+SGMCMC_KSD_ABI_VERSION\s+1\s", open(HEADER).read())
    assert _lib.lib().sgmcmc_ksd_abi_version() == _lib.KSD_ABI_VERSION == 1
    for name in ("ksd_max_samples", "ksd_workspace", "ksd_plan", "ksd"):
        assert name in kernels.__all__ and callable(getattr(kernels, name))
    ids = dict(re.findall(r"#define\s+SGMCMC_KSD_([A-Z]+)\s+(\d+)\s", open(HEADER).read()))
    launches = {k.lower(): int(v) for k, v in ids.items() if k not in ("ABI", "IMQ", "RBF")}
    assert launches == {v: k for k, v in kernels.KSD_IDS.items()}
    assert {"imq": int(ids["IMQ"]), "rbf": int(ids["RBF"])} == kernels.KSD_KINDS == {"imq": 0, "rbf": 1}
    assert '#include "sgmcmc_hip_ksd.h"' not in open(os.path.join(ROOT, "include", "sgmcmc_hip.h")).read()


def test_both_new_files_are_build_dependencies():
    deps = [os.path.basename(p) for p in _lib.build_dependencies()]
    assert "sgmcmc_ksd.hip" in deps and "sgmcmc_hip_ksd.h" in deps
    makefile = open(os.path.join(ROOT, "pysgmcmc_amd", "csrc", "Makefile")).read()
    assert "sgmcmc_ksd.hip" in makefile and "sgmcmc_hip_ksd.h" in makefile and "-ffp-contract=off" in makefile


def test_the_entries_are_declared_with_the_header_s_argument_types():
    lib = _lib.lib()
    vp, sz, ci, cd, cf = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_float
    text = _prototypes()

    def wanted(ret, name):
        proto = re.search(r"%s\s+%s\s*\((.*?)\)\s*;" % (ret, name), text, flags=re.S).group(1)
        want = []
        for arg in (" ".join(a.split()) for a in proto.split(",")):
            if arg == "int *out":
                want.append(ctypes.POINTER(ci))
            elif "*" in arg or arg.startswith("sgmcmc_stream_t"):
                want.append(vp)
            elif arg.startswith("size_t"):
                want.append(sz)
            elif arg.startswith("double "):
                want.append(cd)
            elif arg.startswith("float "):
                want.append(cf)
            else:
                assert arg.startswith("int "), arg
                want.append(ci)
        return want

    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_ksd_" + sfx)
        want = wanted("int", "sgmcmc_ksd_" + sfx)
        assert len(want) == 16 and list(f.argtypes) == want, sfx
        assert want[7:10] == [cd, cd, cd] and f.restype is ci            # c, beta and h2 are doubles in both entries
    assert list(lib.sgmcmc_ksd_workspace_bytes.argtypes) == wanted("size_t", "sgmcmc_ksd_workspace_bytes") == [sz, sz]
    assert lib.sgmcmc_ksd_workspace_bytes.restype is sz
    assert list(lib.sgmcmc_ksd_plan.argtypes) == wanted("int", "sgmcmc_ksd_plan")
    assert lib.sgmcmc_ksd_max_samples.restype is ci and lib.sgmcmc_ksd_abi_version.restype is ci


def test_workspace_bytes_depends_on_the_sample_count_alone():
    raw = _lib.lib().sgmcmc_ksd_workspace_bytes
    assert kernels.ksd_max_samples() == 4096 == stein.MAX_SAMPLES
    for esize in (4, 8):
        for n in (0, 1, 4097, 2 ** 31, 2 ** 40):
            assert raw(n, esize) == 0
        sizes = [raw(n, esize) for n in range(2, 4097)]
        assert all(s > 0 and s % 128 == 0 for s in sizes)
        for n in (2, 64, 129, 1024, 4096):
            blocks = -(-n // 64)
            pairs = blocks * (blocks + 1) // 2
            parts = max(1, 512 // pairs) * pairs * 4 * 4096
            lower = (3 * n * n + 65536 + parts) * esize + 2 * n * 8       # A, B, C, the means, the blocks; row sums, diagonal
            assert lower <= raw(n, esize) <= lower + 8 * 128
    for esize in (0, 1, 2, 16):
        assert raw(129, esize) == 0
    assert len(raw.argtypes) == 2                                         # no dim in the signature
    with pytest.raises(ValueError, match="2..4096"):
        kernels.ksd_workspace(4097, torch.zeros(4))
    with pytest.raises(ValueError, match="2..4096"):
        kernels.ksd_workspace(1, torch.zeros(4))
    with pytest.raises(_lib.SgmcmcLibraryError, match="no CPU fallback"):
        kernels.ksd_workspace(129, torch.zeros(4))
    with pytest.raises(_lib.SgmcmcLibraryError, match="no CPU fallback"):
        kernels.ksd(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(8))


# ---- refusals: host checks first, the dummy device pointers are never dereferenced ----------------------------------------

def _call(sfx, n=129, dim=7, ld_x=8, ld_s=9, kind=0, c=1.0, beta=-0.5, h2=1.0, ld_m=129, **ptrs):
    lib = _lib.lib()
    p = dict(dict(samples=4096, scores=4096, workspace=4096, matrix=4096, rows=4096, stats=4096), **ptrs)
    rc = getattr(lib, "sgmcmc_ksd_" + sfx)(p["samples"], ld_x, p["scores"], ld_s, n, dim, kind, c, beta, h2, p["workspace"],
                                           p["matrix"], ld_m, p["rows"], p["stats"], None)
    return rc, lib.sgmcmc_last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_entry_refuses_bad_arguments_in_the_stated_order(sfx):
    def refused(text, **kw):
        rc, msg = _call(sfx, **kw)
        assert rc == EINVAL and msg.startswith(b"ksd: ") and text in msg, (kw, rc, msg)

    for name in ("samples", "scores", "workspace", "stats"):
        refused(b"null pointer", **{name: None})
    for n in (0, 1, 4097, 2 ** 40):
        refused(b"outside [2, 4096]", n=n)
    refused(b"dim < 1", dim=0, ld_x=0, ld_s=0)
    refused(b"ld_x < dim", ld_x=6)
    refused(b"ld_s < dim", ld_s=6)
    for kind in (-1, 2):
        refused(b"kind", kind=kind)
    for c, beta in ((0.0, -0.5), (-1.0, -0.5), (float("nan"), -0.5), (1.0, 0.0), (1.0, -1.0), (1.0, 0.5), (1.0, float("nan"))):
        refused(b"IMQ", c=c, beta=beta)
    for h2 in (0.0, -1.0, float("nan")):
        refused(b"RBF", kind=1, h2=h2)
    refused(b"ld_m < n", ld_m=128)
    refused(b"32-byte aligned", workspace=4096 + 16)
    refused(b"dim above 2^34", dim=2 ** 34 + 1, ld_x=2 ** 35, ld_s=2 ** 35)
    # an earlier check wins over a later one
    refused(b"null pointer", scores=None, n=1)
    refused(b"outside [2, 4096]", n=1, dim=0)
    refused(b"dim < 1", dim=0, ld_x=0, ld_s=0, kind=7)
    refused(b"ld_x < dim", ld_x=6, ld_s=6)
    refused(b"ld_s < dim", ld_s=6, kind=7)
    refused(b"kind", kind=7, c=0.0, h2=0.0)
    refused(b"IMQ", c=0.0, ld_m=1)
    refused(b"RBF", kind=1, h2=0.0, ld_m=1)
    refused(b"ld_m < n", ld_m=1, workspace=4096 + 8)
    refused(b"32-byte aligned", workspace=4096 + 8, dim=2 ** 34 + 1, ld_x=2 ** 35, ld_s=2 ** 35)
    # what a kind does not read is not checked; outputs that are not asked for are not checked
    refused(b"32-byte aligned", kind=1, c=0.0, beta=3.0, workspace=4096 + 8)
    refused(b"32-byte aligned", kind=0, h2=-1.0, workspace=4096 + 8)
    refused(b"32-byte aligned", matrix=None, rows=None, ld_m=0, workspace=4096 + 8)


def test_the_plan_refuses_what_the_entry_refuses():
    raw = _lib.lib().sgmcmc_ksd_plan
    out = (ctypes.c_int * 64)()
    for n, dim, esize in ((1, 5, 4), (4097, 5, 4), (129, 0, 4), (129, 5, 2), (129, 2 ** 34 + 1, 8)):
        assert raw(n, dim, esize, out, 64) == EINVAL and _lib.lib().sgmcmc_last_error().startswith(b"ksd_plan: ")
    assert raw(129, 5, 4, None, 0) == 5 and raw(4096, 5, 8, None, 0) == 5             # counts without a buffer
    assert raw(129, 65536, 4, None, 0) == 5 and raw(129, 65537, 4, None, 0) == 7      # a pair of launches per phase
    assert raw(129, 2 ** 34, 4, None, 0) == 2 * 2 ** 18 + 3
    assert raw(129, 65537, 4, out, 8) == 7 and list(out[:8]) == [MEAN, 32, 2048, 0, GRAM, 32, 510, 85]   # what fits
    with pytest.raises(_lib.SgmcmcLibraryError):
        kernels.ksd_plan(4097, 5, torch.float32)


# ---- the plan ---------------------------------------------------------------------------------------------------------------

DTYPES = ((M.F32, torch.float32), (M.F64, torch.float64))


def _all_cases(np_dtype):
    return list(M.TABLE) + M.walk_cases(np_dtype) + M.phase_cases(np_dtype) + M.CLAMP_CASES


@pytest.mark.parametrize("np_dtype,dtype", DTYPES, ids=["f32", "f64"])
def test_the_plan_covers_dim_and_the_walk_cases_walk(np_dtype, dtype):
    esize = np.dtype(np_dtype).itemsize
    tile = 32 if esize == 4 else 16
    for n, d in _all_cases(np_dtype) + [(1024, 5253), (4096, 5253), (4096, 1_000_003)]:
        plan = kernels.ksd_plan(n, d, dtype)
        ids = [l.id for l in plan]
        phases = -(-d // M.PHASE_COLS)
        assert ids == [MEAN, GRAM] * phases + [REDUCE, PAIR, FINISH], (n, d, ids)
        by_id = {l.id: l for l in plan}
        gram = by_id[GRAM]
        blocks = -(-n // 64)
        pairs = blocks * (blocks + 1) // 2
        assert gram.tile == tile and gram.cap == max(1, 512 // pairs)
        n_tiles = -(-min(d, M.PHASE_COLS) // gram.tile)                               # of the widest phase
        assert gram.grid == min(n_tiles, gram.cap) * pairs and gram.grid <= max(512, pairs)
        grams, means = [l for l in plan if l.id == GRAM], [l for l in plan if l.id == MEAN]
        assert all(l == gram for l in grams) and M.PHASE_COLS % gram.tile == 0        # phases start on a tile edge
        assert all(l.tile == 32 and l.cap == 0 for l in means)
        assert sum(l.grid * 32 for l in means) >= d > sum(l.grid * 32 for l in means) - 32 - 32 * (phases - 1)
        assert [l.grid for l in means[:-1]] == [M.PHASE_COLS // 32] * (phases - 1)
        assert by_id[PAIR].grid == n and by_id[FINISH].grid == 1 and by_id[REDUCE].grid * 256 >= pairs * 4 * 4096
        assert all(l.grid >= 1 for l in plan)
        # the partial blocks of the largest grid fit the workspace
        assert gram.cap * pairs * 4 * 4096 * esize < _lib.lib().sgmcmc_ksd_workspace_bytes(n, esize)
    for n, d in M.walk_cases(np_dtype):
        gram = [l for l in kernels.ksd_plan(n, d, dtype) if l.id == GRAM][0]
        assert d == gram.cap * gram.tile + gram.tile + 3 and -(-d // gram.tile) == gram.cap + 2 > gram.cap
        assert d % gram.tile == 3 and d % 2 == 1 and d < M.PHASE_COLS
    for n, d in M.phase_cases(np_dtype):
        gram = [l for l in kernels.ksd_plan(n, d, dtype) if l.id == GRAM]
        assert len(gram) == 2 and d == M.PHASE_COLS + gram[0].tile + 3 and d % 2 == 1
        assert M.PHASE_COLS // gram[0].tile > gram[0].cap                            # the first phase walks as well
    for n, d in M.CLAMP_CASES:
        gram = [l for l in kernels.ksd_plan(n, d, dtype) if l.id == GRAM][0]
        assert gram.cap == 1 and gram.grid == -(-n // 64) * (-(-n // 64) + 1) // 2 > 512 and -(-d // gram.tile) > 1   # and it walks
    for n, d in M.TABLE:
        gram = [l for l in kernels.ksd_plan(n, d, dtype) if l.id == GRAM][0]
        assert -(-d // gram.tile) <= gram.cap                                       # the table proper never walks GRAM


def test_the_table_is_the_issue_s():
    assert M.TABLE == [(2, 1), (63, 5), (64, 64), (65, 67), (129, 40), (257, 3)]
    assert M.walk_cases(M.F32) == [(2, 512 * 32 + 32 + 3), (257, 34 * 32 + 32 + 3)]
    assert M.walk_cases(M.F64) == [(2, 512 * 16 + 16 + 3), (257, 34 * 16 + 16 + 3)]
    assert M.phase_cases(M.F32) == [(129, 65536 + 32 + 3)] and M.phase_cases(M.F64) == [(129, 65536 + 16 + 3)]
    assert [k["kernel"] for k in M.KERNELS.values()] == ["imq", "imq", "rbf"]
    assert M.KERNELS["imq"] == dict(kernel="imq", c=1.0, beta=-0.5)                  # the default kernel
    X, S = M.inputs(63, 5, M.F32)
    rng = np.random.default_rng([63, 5, 4])
    assert np.array_equal(X, (0.3 + rng.normal(size=(63, 5)) / np.sqrt(5)).astype(np.float32))
    assert np.array_equal(S, rng.normal(size=(63, 5)).astype(np.float32))


# ---- the C of the entrywise bar -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("np_dtype", [M.F32, M.F64], ids=["f32", "f64"])
def test_c_is_eight_times_the_host_statement_s_own_worst_error(np_dtype):
    name = np.dtype(np_dtype).name
    rows = {k: v for k, v in M.ORACLE_UNITS.items() if k[2] == name}
    assert sorted((n, d) for n, d, _ in rows) == sorted(M.TABLE)
    (wn, wd, wkern), worst = M.WORST[np_dtype]
    assert worst == max(max(v) for v in rows.values()) == rows[(wn, wd, name)][list(M.KERNELS).index(wkern)]
    assert M.C[np_dtype] == 8 * worst
    if np_dtype == M.F64 and not M.LONG_DOUBLE_IS_WIDER:
        return                                                   # nothing wider than f64 to measure against here
    got = M.narrow_against_wide(wn, wd, np_dtype, wkern)
    print("%s host statement against the wider one at %r: %.3f units" % (name, (wn, wd, wkern), got))
    assert abs(got - worst) <= 5e-4 * worst + 5e-4               # the table holds three decimals


# ---- the host statement -----------------------------------------------------------------------------------------------------

def _definition(X, S, phi):
    """k_p = s_x . s_y k + s_x . grad_y k + s_y . grad_x k + tr grad_x grad_y k by double autograd"""
    n, d = X.shape
    K = torch.zeros(n, n, dtype=torch.float64)
    for i in range(n):
        for j in range(n):
            x, y = X[i].clone().requires_grad_(True), X[j].clone().requires_grad_(True)
            k = phi(torch.sum((x - y) ** 2))
            gx, = torch.autograd.grad(k, x, create_graph=True)
            gy, = torch.autograd.grad(k, y, create_graph=True)
            tr = sum(torch.autograd.grad(gx[a], y, retain_graph=True)[0][a] for a in range(d))
            K[i, j] = (S[i] @ S[j] * k + S[i] @ gy + S[j] @ gx + tr).detach()
    return K.numpy()


@pytest.mark.parametrize("kw,phi", [
    (dict(kernel="imq", c=1.0, beta=-0.5), lambda r2: (1.0 + r2) ** -0.5),
    (dict(kernel="imq", c=0.7, beta=-0.3), lambda r2: (0.49 + r2) ** -0.3),
    (dict(kernel="rbf", bandwidth=0.8), lambda r2: torch.exp(-r2 / 1.6)),
], ids=["imq", "imq_pow", "rbf"])
def test_the_host_statement_is_the_definition_of_the_stein_kernel(kw, phi):
    rng = np.random.default_rng(7)
    X, S = 0.3 + rng.normal(size=(6, 3)), rng.normal(size=(6, 3))
    want = _definition(torch.as_tensor(X), torch.as_tensor(S), phi)
    for order in ("library", "k"):                            # numpy's matrix product, and column by column
        got = stein.stein_kernel_matrix(X, S, order=order, **kw)
        assert got.dtype == np.float64 and np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
    with pytest.raises(ValueError, match="order"):
        stein.stein_kernel_matrix(X, S, order="rows", **kw)


@pytest.mark.parametrize("kern", list(M.KERNELS))
@pytest.mark.parametrize("np_dtype", [M.F32, M.F64], ids=["f32", "f64"])
def test_the_host_statement_is_symmetric_with_an_exact_diagonal(np_dtype, kern):
    n, d = 65, 67
    X, S = M.inputs(n, d, np_dtype)
    kw = M.KERNELS[kern]
    K, p = stein.stein_kernel_matrix(X, S, dtype=np_dtype, details=True, **kw)
    assert K.dtype == np.float64 and np.array_equal(K, K.T)
    assert np.all(np.diag(p["r2"]) == 0.0) and np.all(np.diag(p["t"]) == 0.0)
    phi0 = np.diag(p["phi"])[0]                                                      # phi(0): one value on the whole diagonal
    assert np.all(np.diag(p["phi"]) == phi0)
    if kw["kernel"] == "imq":
        u = kw["c"] * kw["c"]
        assert phi0 == 1.0 / np.sqrt(u) if kw["beta"] == -0.5 else abs(phi0 - u ** kw["beta"]) <= 2e-16 * phi0
        d1 = (kw["beta"] * phi0) / u
    else:
        assert phi0 == 1.0
        d1 = -1.0 / (2.0 * kw["bandwidth"])
    assert np.array_equal(np.diag(K), phi0 * np.diag(p["B"]) - (2.0 * d) * d1)       # phi(0) B_ii - 2 d phi'(0)


def test_the_sums_follow_the_stated_order():
    rng = np.random.default_rng(3)
    K = rng.normal(size=(600, 600)) * 10.0 ** rng.integers(-6, 6, size=(600, 600))

    def lanes(v):                                             # the header's words, one scalar at a time
        red = [0.0] * 256
        for j, x in enumerate(v):
            red[j % 256] = red[j % 256] + float(x)
        off = 128
        while off:
            for t in range(off):
                red[t] = red[t] + red[t + off]
            off //= 2
        return red[0]

    rows, total, trace = stein.stein_sums(K)
    want = np.array([lanes(K[i]) for i in range(600)])
    assert np.array_equal(rows, want) and total == lanes(want) and trace == lanes(np.diag(K))
    assert not np.array_equal(rows, K.sum(axis=1))            # the order matters at this spread of magnitudes


def test_a_cpu_call_takes_the_host_statement():
    X, S = M.inputs(63, 5, M.F64)
    for kern, kw in M.KERNELS.items():
        ref = M.reference(63, 5, M.F64, kern)
        for conv in (np.asarray, torch.as_tensor):
            r = diagnostics.kernel_stein_discrepancy(conv(X), conv(S), return_matrix=True, **kw)
            assert isinstance(r, diagnostics.SteinDiscrepancy) and r.thinning == 1
            assert r._fields[:5] == ("ksd", "v_statistic", "u_statistic", "row_sums", "matrix")
            assert np.array_equal(np.asarray(r.matrix), ref.K) and np.array_equal(np.asarray(r.row_sums), ref.rows)
            assert float(r.v_statistic) == ref.v and float(r.u_statistic) == ref.u
            assert float(r.ksd) == np.sqrt(max(ref.v, 0.0))
        assert diagnostics.kernel_stein_discrepancy(X, S, **kw).matrix is None
    chains = diagnostics.kernel_stein_discrepancy(X[:60].reshape(3, 20, 5), S[:60].reshape(3, 20, 5))
    flat = diagnostics.kernel_stein_discrepancy(X[:60], S[:60])
    assert chains.v_statistic == flat.v_statistic
    with pytest.raises(ValueError, match="4096.*thin"):
        diagnostics.kernel_stein_discrepancy(np.zeros((4097, 2)), np.zeros((4097, 2)))
    with pytest.raises(ValueError, match="bandwidth"):
        diagnostics.kernel_stein_discrepancy(X, S, kernel="rbf")
    with pytest.raises(ValueError, match="beta"):
        diagnostics.kernel_stein_discrepancy(X, S, beta=0.5)


# ---- known behaviour ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [2, 50])
def test_u_of_gaussian_draws_is_below_u_of_the_shifted_draws(d):
    x = np.random.default_rng(1).normal(size=(400, d))
    on = diagnostics.kernel_stein_discrepancy(x, -x)                  # the score of N(0, I) at x
    off = diagnostics.kernel_stein_discrepancy(x + 0.5, -(x + 0.5))   # the same draws shifted, scored by N(0, I)
    print("d = %d: U = %.4g on target, %.4g shifted by 0.5" % (d, on.u_statistic, off.u_statistic))
    assert on.u_statistic < 0.1 * off.u_statistic and off.u_statistic > 0.1
    assert on.ksd < off.ksd


# ---- bnn_posterior_scores on the CPU --------------------------------------------------------------------------------------

def test_bnn_posterior_scores_on_the_cpu_is_autograd_of_the_full_data_cost():
    sizes, N = [2, 5, 4, 1], 23
    rng = np.random.default_rng(11)
    X = torch.as_tensor(rng.normal(size=(N, 2)))
    y = torch.as_tensor(rng.normal(size=N))
    P = 2 * 5 + 5 + 5 * 4 + 4 + 4 + 1 + 1
    theta = torch.as_tensor(0.3 * rng.normal(size=(2, 3, P)))
    got = models.bnn_posterior_scores(theta, sizes, X, y, wdecay=0.7, prior_mean=1e-3, prior_var=0.02)
    assert got.shape == (6, P) and got.dtype == torch.float64
    xp, yp = Placeholder().feed(X), Placeholder().feed(y)
    cost = models.BNNParticleCost(sizes, xp, yp, N, N, wdecay=0.7, prior_mean=1e-3, prior_var=0.02)
    for i, row in enumerate(theta.reshape(6, P)):
        row = row.clone().requires_grad_(True)
        g, = torch.autograd.grad(cost(row), row)
        assert torch.equal(got[i], g * (-float(N)))
        # the score is the gradient of log p = -N cost: a central difference along one direction
        v = torch.as_tensor(rng.normal(size=P))
        v = v / v.norm()
        with torch.no_grad():
            fd = (-N * cost(row + 1e-5 * v) + N * cost(row - 1e-5 * v)) / 2e-5
        assert abs(float(fd) - float(got[i] @ v)) <= 1e-6 * max(1.0, abs(float(fd)))
    out = torch.empty(6, P, dtype=torch.float64)
    assert models.bnn_posterior_scores(theta, sizes, X, y, 0.7, 1e-3, 0.02, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError, match="parameters"):
        models.bnn_posterior_scores(theta[..., :-1], sizes, X, y)


def test_the_existing_exports_are_unchanged():
    assert diagnostics.__all__[:9] == ("PYSGMCMCTrace", "pymc3_multitrace", "effective_sample_sizes", "gelman_rubin",
                                       "DeviceTrace", "effective_n_all", "effective_sample_sizes_of", "chain_diagnostics_all",
                                       "gelman_rubin_all")
    assert models.__all__[:10] == ("BayesianNeuralNetwork", "log_variance_prior_log_like", "weight_prior_log_like",
                                   "posterior_predictive", "heldout_score", "HeldOutScore", "predictive_gradients",
                                   "PredictiveGradients", "BNNParticleCost", "bnn_particles")
    for name in ("stein", "SteinDiscrepancy", "kernel_stein_discrepancy", "stein_kernel_matrix"):
        assert name in diagnostics.__all__ and hasattr(diagnostics, name)
    assert "bnn_posterior_scores" in models.__all__ and callable(models.bnn_posterior_scores)
    assert set(("SteinDiscrepancy", "kernel_stein_discrepancy", "stein_kernel_matrix")) <= set(stein.__all__)
    from pysgmcmc_amd.samplers.fused_chains import FusedBNNChains
    assert callable(FusedBNNChains.stein_discrepancy)
