"""The many-particle SVGD add-on (include/sgmcmc_hip_svgd_many.h, csrc/sgmcmc_svgd_many.hip) without a GPU: the header's
symbols and version, the ctypes declarations, the workspace size, every refusal of the entries before any launch in the
documented order, the launch plan against the case table of ``svgd_many_cases.py``, the ``c`` constants of the displacement
bar, and the register-resident path left as it was. What the kernels compute is checked on the GPU
(tests/test_svgd_many_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pysgmcmc_amd import _lib, kernels
from pysgmcmc_amd.samplers import SVGDSampler

import svgd_many_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip_svgd_many.h")
EINVAL = -1
GRAM, REDUCE, DIST, SELECT, NEXT, BANDWIDTH, KMATRIX, UPDATE, KGRAD, COPY, MEAN = range(1, 12)


def _prototypes():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_header_declares_eight_exported_symbols_and_version_1():
    handle = ctypes.CDLL(_lib.build())
    syms = sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", _prototypes())))
    assert syms == ["sgmcmc_svgd_many_abi_version", "sgmcmc_svgd_many_kernel_f32", "sgmcmc_svgd_many_kernel_f64",
                    "sgmcmc_svgd_many_max_particles", "sgmcmc_svgd_many_plan", "sgmcmc_svgd_many_step_f32",
                    "sgmcmc_svgd_many_step_f64", "sgmcmc_svgd_many_workspace_bytes"], syms
    for name in syms:
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    assert re.search(r"#define\s+SGMCMC_SVGD_MANY_ABI_VERSION\s+1\s", open(HEADER).read())
    assert _lib.lib().sgmcmc_svgd_many_abi_version() == _lib.SVGD_MANY_ABI_VERSION == 1
    for name in ("svgd_many_max_particles", "svgd_many_workspace", "svgd_many_step", "svgd_many_kernel", "svgd_many_plan"):
        assert name in kernels.__all__ and callable(getattr(kernels, name))
    ids = dict(re.findall(r"#define\s+SGMCMC_SVGD_MANY_([A-Z]+)\s+(\d+)\s", open(HEADER).read()))
    assert {k.lower(): int(v) for k, v in ids.items() if k != "ABI"} == {v: k for k, v in kernels.SVGD_MANY_IDS.items()}


def test_both_new_files_are_build_dependencies():
    deps = [os.path.basename(p) for p in _lib.build_dependencies()]
    assert "sgmcmc_svgd_many.hip" in deps and "sgmcmc_hip_svgd_many.h" in deps
    makefile = open(os.path.join(ROOT, "pysgmcmc_amd", "csrc", "Makefile")).read()
    assert "sgmcmc_svgd_many.hip" in makefile and "sgmcmc_hip_svgd_many.h" in makefile


def test_the_entries_are_declared_with_the_header_s_argument_types():
    lib = _lib.lib()
    vp, sz, ci, cd, cf = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_float
    text = _prototypes()

    def wanted(ret, name):
        proto = re.search(r"%s\s+%s\s*\((.*?)\)\s*;" % (ret, name), text, flags=re.S).group(1)
        want = []
        for arg in (a.strip() for a in proto.split(",")):
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
        for entry, old, n_args in (("step", "sgmcmc_svgd_step_", 12), ("kernel", "sgmcmc_svgd_kernel_", 10)):
            f = getattr(lib, "sgmcmc_svgd_many_%s_%s" % (entry, sfx))
            want = wanted("int", "sgmcmc_svgd_many_%s_%s" % (entry, sfx))
            assert len(want) == n_args and list(f.argtypes) == want, (entry, sfx)
            assert list(f.argtypes) == list(getattr(lib, old + sfx).argtypes)     # the argument lists of the namesakes
            assert f.restype is ci
    assert list(lib.sgmcmc_svgd_many_workspace_bytes.argtypes) == wanted("size_t", "sgmcmc_svgd_many_workspace_bytes") == [sz, sz]
    assert lib.sgmcmc_svgd_many_workspace_bytes.restype is sz
    assert list(lib.sgmcmc_svgd_many_plan.argtypes) == wanted("int", "sgmcmc_svgd_many_plan")
    assert lib.sgmcmc_svgd_many_max_particles.restype is ci and lib.sgmcmc_svgd_many_abi_version.restype is ci


def test_workspace_bytes_depends_on_the_particle_count_alone():
    raw = _lib.lib().sgmcmc_svgd_many_workspace_bytes
    assert kernels.svgd_many_max_particles() == 1024
    for esize in (4, 8):
        for n in (0, 1, 1025, 2 ** 31, 2 ** 40):
            assert raw(n, esize) == 0
        sizes = [raw(n, esize) for n in range(2, 1025)]
        assert all(s > 0 and s % 128 == 0 for s in sizes)
        for n in (2, 64, 129, 1024):
            np16 = (n + 15) // 16 * 16
            assert raw(n, esize) >= (16 + n * n + np16 * np16 + np16 + 65536) * esize  # header, D, K, row sums, means
        assert raw(1024, esize) <= 4 * 1024 * 1024 * esize                              # and a bounded number of blocks
    for esize in (0, 1, 2, 16):
        assert raw(129, esize) == 0
    assert len(raw.argtypes) == 2                                                       # no dim in the signature
    with pytest.raises(ValueError, match="2..1024"):
        kernels.svgd_many_workspace(1025, torch.zeros(4))
    with pytest.raises(ValueError, match="2..1024"):
        kernels.svgd_many_workspace(1, torch.zeros(4))
    with pytest.raises(_lib.SgmcmcLibraryError, match="no CPU fallback"):
        kernels.svgd_many_workspace(129, torch.zeros(4))


# ---- refusals: host checks first, the dummy device pointers are never dereferenced ----------------------------------------

def _step(sfx, n=129, dim=7, ld=8, sign=-1, **ptrs):
    lib = _lib.lib()
    p = dict(dict(particles=4096, grad=4096, hist_grad=4096, workspace=4096), **ptrs)
    rc = getattr(lib, "sgmcmc_svgd_many_step_" + sfx)(p["particles"], p["grad"], p["hist_grad"], n, dim, ld, 0.1, 0.9, 1e-6,
                                                      sign, p["workspace"], None)
    return rc, lib.sgmcmc_last_error()


def _kernel(sfx, n=129, dim=7, ld=8, kgrad_ld=7, **ptrs):
    lib = _lib.lib()
    p = dict(dict(particles=4096, workspace=4096, kernel_out=4096, kgrad=4096, bw=4096), **ptrs)
    rc = getattr(lib, "sgmcmc_svgd_many_kernel_" + sfx)(p["particles"], n, dim, ld, p["workspace"], p["kernel_out"],
                                                        p["kgrad"], kgrad_ld, p["bw"], None)
    return rc, lib.sgmcmc_last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_step_entry_refuses_bad_arguments_in_the_stated_order(sfx):
    def refused(text, **kw):
        rc, msg = _step(sfx, **kw)
        assert rc == EINVAL and msg.startswith(b"svgd_many_step: ") and text in msg, (kw, rc, msg)

    for name in ("particles", "grad", "hist_grad", "workspace"):
        refused(b"null pointer", **{name: None})
    for n in (0, 1, 1025, 2 ** 40):
        refused(b"outside [2, 1024]", n=n)
    refused(b"dim < 1", dim=0, ld=0)
    refused(b"ld < dim", ld=6)
    for sign in (0, 2, -2):
        refused(b"repulsion_sign", sign=sign)
    refused(b"32-byte aligned", workspace=4096 + 16)
    refused(b"dim above 2^34", dim=2 ** 34 + 1, ld=2 ** 35)
    # an earlier check wins over a later one
    refused(b"null pointer", grad=None, n=1)
    refused(b"outside [2, 1024]", n=1, dim=0)
    refused(b"dim < 1", dim=0, ld=0, sign=0)
    refused(b"ld < dim", ld=6, sign=0)
    refused(b"repulsion_sign", sign=0, workspace=4096 + 8)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_kernel_entry_refuses_bad_arguments_in_the_stated_order(sfx):
    def refused(text, **kw):
        rc, msg = _kernel(sfx, **kw)
        assert rc == EINVAL and msg.startswith(b"svgd_many_kernel: ") and text in msg, (kw, rc, msg)

    refused(b"null pointer", particles=None)
    refused(b"null pointer", workspace=None)
    for n in (0, 1, 1025):
        refused(b"outside [2, 1024]", n=n)
    refused(b"dim < 1", dim=0, ld=0)
    refused(b"ld < dim", ld=6)
    refused(b"kgrad_ld < dim", kgrad_ld=6)
    refused(b"32-byte aligned", workspace=4096 + 16)
    refused(b"null pointer", workspace=None, n=1)
    refused(b"outside [2, 1024]", n=1025, dim=0)
    refused(b"dim < 1", dim=0, ld=0, kgrad_ld=0)
    refused(b"ld < dim", ld=6, kgrad_ld=6)
    refused(b"kgrad_ld < dim", kgrad_ld=6, workspace=4096 + 16)


def test_the_plan_refuses_what_the_step_refuses():
    raw = _lib.lib().sgmcmc_svgd_many_plan
    out = (ctypes.c_int * 64)()
    for n, dim, esize in ((1, 5, 4), (1025, 5, 4), (129, 0, 4), (129, 5, 2), (129, 2 ** 34 + 1, 8)):
        assert raw(n, dim, esize, out, 64) == EINVAL and _lib.lib().sgmcmc_last_error().startswith(b"svgd_many_plan: ")
    assert raw(129, 5, 4, None, 0) == 11 and raw(130, 5, 8, None, 0) == 16          # counts without a buffer
    assert raw(129, 65536, 4, None, 0) == 11 and raw(129, 65537, 4, None, 0) == 13  # a pair of launches per phase
    assert raw(129, 2 ** 34, 4, None, 0) == 2 * 2 ** 18 + 9
    assert raw(129, 65537, 4, out, 8) == 13 and list(out[:8]) == [MEAN, 32, 2048, 0, GRAM, 64, 510, 85]   # what fits
    with pytest.raises(_lib.SgmcmcLibraryError):
        kernels.svgd_many_plan(1025, 5, torch.float32)


# ---- the plan ---------------------------------------------------------------------------------------------------------------

DTYPES = ((M.F32, torch.float32), (M.F64, torch.float64))


def _all_cases(np_dtype):
    return list(M.TABLE) + M.walk_cases(np_dtype) + M.phase_cases(np_dtype)


@pytest.mark.parametrize("np_dtype,dtype", DTYPES, ids=["f32", "f64"])
def test_the_plan_covers_dim_and_the_walk_cases_walk(np_dtype, dtype):
    esize = np.dtype(np_dtype).itemsize
    seen = set()
    for n, d in _all_cases(np_dtype) + [(2, 1), (64, 100), (128, 5252), (1024, 1_000_003)]:
        plan = kernels.svgd_many_plan(n, d, dtype)
        ids = [l.id for l in plan]
        even = (n * n) % 2 == 0
        phases = -(-d // M.PHASE_COLS)
        assert ids == [MEAN, GRAM] * phases + [REDUCE, DIST] + [SELECT] * esize + [NEXT] * even + [
            BANDWIDTH, KMATRIX, UPDATE], (n, d, ids)
        by_id = {l.id: l for l in plan}
        gram, update = by_id[GRAM], by_id[UPDATE]
        blocks = -(-n // 64)
        pairs = blocks * (blocks + 1) // 2
        assert gram.tile == (64 if esize == 4 else 32) and gram.cap == max(1, 512 // pairs)
        n_tiles = -(-min(d, M.PHASE_COLS) // gram.tile)                               # of the widest phase
        assert gram.grid == min(n_tiles, gram.cap) * pairs and gram.grid <= max(512, pairs)
        assert (gram.grid // pairs) * gram.tile >= min(d, M.PHASE_COLS) or n_tiles > gram.cap   # one round, or walks
        grams, means = [l for l in plan if l.id == GRAM], [l for l in plan if l.id == MEAN]
        assert all(l == gram for l in grams) and M.PHASE_COLS % gram.tile == 0        # phases start on a tile edge
        assert all(l.tile == 32 and l.cap == 0 for l in means)
        assert sum(l.grid * 32 for l in means) >= d > sum(l.grid * 32 for l in means) - 32 - 32 * (phases - 1)
        assert [l.grid for l in means[:-1]] == [M.PHASE_COLS // 32] * (phases - 1)
        assert update.tile == 16 and update.cap == 0 and update.grid * 16 >= d > (update.grid - 1) * 16
        assert by_id[KMATRIX].grid == (n + 15) // 16 * 16 and by_id[BANDWIDTH].grid == 1
        assert by_id[DIST].grid * 256 >= n * n and by_id[REDUCE].grid * 256 >= pairs * 4096
        assert all(l.grid >= 1 for l in plan)
        # the partial blocks of the largest grid fit the workspace
        assert gram.cap * pairs * 4096 * esize < _lib.lib().sgmcmc_svgd_many_workspace_bytes(n, esize)
        seen.update(ids)
    for n, d in M.walk_cases(np_dtype):
        gram = [l for l in kernels.svgd_many_plan(n, d, dtype) if l.id == GRAM][0]
        assert d == gram.cap * gram.tile + gram.tile + 3 and -(-d // gram.tile) == gram.cap + 2 > gram.cap
        assert d % gram.tile == 3 and d % 2 == 1 and d < M.PHASE_COLS
        assert n * (d + 1) * esize < 64e6
    for n, d in M.phase_cases(np_dtype):
        plan = kernels.svgd_many_plan(n, d, dtype)
        gram = [l for l in plan if l.id == GRAM]
        assert len(gram) == 2 and d == M.PHASE_COLS + gram[0].tile + 3 and d % 2 == 1
        assert M.PHASE_COLS // gram[0].tile > gram[0].cap                            # the first phase walks as well
    for n, d in M.TABLE:
        gram = [l for l in kernels.svgd_many_plan(n, d, dtype) if l.id == GRAM][0]
        assert -(-d // gram.tile) <= gram.cap                                       # the table proper never walks GRAM
    # every launch of a step the dispatch can pick is reached by some case of the table (odd and even n * n)
    table_ids = set()
    for n, d in _all_cases(np_dtype):
        table_ids.update(l.id for l in kernels.svgd_many_plan(n, d, dtype))
    assert table_ids == set(range(GRAM, UPDATE + 1)) | {MEAN} == seen


def test_the_table_is_the_issue_s():
    assert M.TABLE == [(129, 1), (129, 40), (130, 64), (161, 257), (257, 3), (512, 70), (1024, 3), (1024, 65)]
    assert M.walk_cases(M.F32) == [(129, 85 * 64 + 64 + 3), (1024, 3 * 64 + 64 + 3)]
    assert M.walk_cases(M.F64) == [(129, 85 * 32 + 32 + 3), (1024, 3 * 32 + 32 + 3)]
    assert M.TOL[M.F32] == dict(rtol=3e-5, atol=3e-6) and M.TOL[M.F64] == dict(rtol=1e-10, atol=1e-12)
    assert M.SWEEP_RTOL == {M.F32: 3e-5, M.F64: 1e-10} and (M.EPS, M.ALPHA, M.FUDGE) == (0.05, 0.9, 1e-6)


# ---- the c of the displacement bar ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("np_dtype", [M.F32, M.F64], ids=["f32", "f64"])
def test_c_is_eight_times_the_oracle_s_own_worst_error(np_dtype):
    name = np.dtype(np_dtype).name
    rows = {k: v for k, v in M.ORACLE_UNITS.items() if k[2] == name}
    assert sorted((n, d) for n, d, _ in rows) == sorted(M.TABLE)
    (wn, wd, wsign), worst = M.WORST[np_dtype]
    assert worst == max(max(v) for v in rows.values()) == max(rows[(wn, wd, name)][0 if wsign == 1 else 2:][:2])
    assert M.C[np_dtype] == 8 * worst
    assert M.C[M.F32] == 8 * 3.912
    if np_dtype == M.F64 and not M.LONG_DOUBLE_IS_WIDER:
        return                                                   # nothing wider than f64 to measure against here
    rx, rh = M.narrow_against_wide(M.Case(wn, wd, np_dtype, wsign))
    print("%s oracle against the wider one at %r: %.3f (X), %.3f (H) units" % (name, (wn, wd, wsign), rx, rh))
    assert abs(max(rx, rh) - worst) <= 5e-4 * worst + 5e-4      # the table holds three decimals


# ---- the register-resident path and the sampler's dispatch ------------------------------------------------------------------

def test_the_register_resident_path_keeps_its_limit():
    assert kernels.svgd_max_particles() == 128
    assert _lib.lib().sgmcmc_svgd_workspace_bytes(129, 4) == 0
    with pytest.raises(ValueError, match=r"1\.\.128"):
        kernels.svgd_workspace(129, torch.zeros(4))


def test_the_sampler_picks_the_path_by_particle_count_and_names_both_limits():
    assert not SVGDSampler._many(128) and SVGDSampler._many(129) and SVGDSampler._many(1024)
    with pytest.raises(ValueError, match=r"1024.*128|128.*1024"):
        SVGDSampler._workspace_for(1025, torch.zeros(4))
    with pytest.raises(_lib.SgmcmcLibraryError, match="no CPU fallback"):
        SVGDSampler._workspace_for(129, torch.zeros(4))
    with pytest.raises(_lib.SgmcmcLibraryError, match="no CPU fallback"):
        SVGDSampler._workspace_for(128, torch.zeros(4))
