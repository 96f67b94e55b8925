"""The drop-in boundary (CPU, no GPU compute): the C-ABI library loads and exports
every symbol include/sgmcmc_hip.h declares; the product never touches oracle/;
the extension is required (no silent fallback)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgmcmc_hip.h")


def _declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sgmcmc_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_expected_entry_points():
    syms = _declared_symbols()
    for name in ("sgmcmc_sghmc_step_f32", "sgmcmc_sghmc_step_f64", "sgmcmc_sgld_step_f32", "sgmcmc_sgld_step_f64",
                 "sgmcmc_rsghmc_step_f32", "sgmcmc_rsghmc_step_f64", "sgmcmc_philox_normal_f32",
                 "sgmcmc_moments_update_f32", "sgmcmc_rhat_pack_f32", "sgmcmc_rhat_finish_f32",
                 "sgmcmc_rhat_pack_f64", "sgmcmc_rhat_finish_f64",
                 "sgmcmc_summary_f32", "sgmcmc_last_error", "sgmcmc_abi_version"):
        assert name in syms


def test_library_loads_and_exports_every_declared_symbol():
    from pysgmcmc_amd import _lib
    _lib.build()
    handle = ctypes.CDLL(_lib.lib_path())
    for name in _declared_symbols():
        assert hasattr(handle, name), "libsgmcmc_hip.so does not export %s" % name
    lib = _lib.lib()
    assert lib.sgmcmc_abi_version() == _lib.ABI_VERSION == 6
    assert lib.sgmcmc_summary_workspace_bytes() >= 1024 * 32
    # the per-call launch geometry is validated on the host before anything is launched: checkable without a
    # GPU (the output pointer is a dummy that is never dereferenced because the call fails first)
    bad = _lib.LaunchStruct(100, 0, 0, -1)
    rc = lib.sgmcmc_philox_normal_f32(ctypes.c_void_p(4096), 8, 1, 0, None, ctypes.byref(bad), None)
    assert rc == -1 and b"block_threads" in lib.sgmcmc_last_error()
    bad = _lib.LaunchStruct(0, 3, 0, -1)
    rc = lib.sgmcmc_moments_update_f32(ctypes.c_void_p(4096), ctypes.c_void_p(4096), ctypes.c_void_p(4096), 8, 1,
                                       ctypes.byref(bad), None)
    assert rc == -1 and b"quads_per_thread" in lib.sgmcmc_last_error()


def _contract_map():
    text = open(HEADER).read()
    block = text[text.index("---- Contract map"):text.index("---- end of the contract map")]
    groups, cur = {}, None
    for line in block.splitlines():
        m = re.match(r"\s*\*\s*\[([a-z-]+)\]", line)
        if m:
            cur = groups.setdefault(m.group(1), [])
        if cur is not None:
            cur.extend(re.findall(r"\bsgmcmc_[a-z0-9_]+\b(?![*_])", line))
    return groups


def test_contract_map_partitions_the_declared_entry_points():
    """the header says which entry points are the SURVEY 8(b) boundary and which are the cost path's
    internals; the map names every declared entry point exactly once, and nothing that is not declared (or not exported)."""
    from pysgmcmc_amd import _lib
    groups = _contract_map()
    assert sorted(groups) == ["boundary", "cost-path", "svgd", "whole-step"]
    named = [n for g in groups.values() for n in g]
    assert len(named) == len(set(named)), sorted(n for n in set(named) if named.count(n) > 1)
    assert sorted(named) == _declared_symbols()
    handle = ctypes.CDLL(_lib.build())
    assert all(hasattr(handle, n) for n in named)
    # the five step functions, moments, R-hat pack / finish, Philox, statistics: the boundary section 8(b) asked for
    for name in ("sgmcmc_sghmc_step_f32", "sgmcmc_sgld_step_f64", "sgmcmc_rsghmc_step_f32", "sgmcmc_moments_update_f32",
                 "sgmcmc_rhat_pack_f32", "sgmcmc_rhat_finish_f64", "sgmcmc_philox_normal_f32", "sgmcmc_step_stats_finish"):
        assert name in groups["boundary"]
    assert not [n for n in groups["boundary"] if "bnn" in n or "tanh" in n or "svgd" in n]
    assert not hasattr(handle, "sgmcmc_tanh_rowdot_f32")        # superseded by sgmcmc_bias_tanh_rowdot_*, dropped in ABI v6
    assert len(named) == 71


def test_abi_exports_no_experiment_knobs():
    """the ABI a maintainer binds must not carry experiment switches. v4 dropped the hand-written GEMM entry
    points (tile-variant / timing-probe / de-phasing arguments); they were removed with the experiments in round 5."""
    from pysgmcmc_amd import _lib
    handle = ctypes.CDLL(_lib.build())
    header = open(HEADER).read()
    assert not [name for name in _declared_symbols() if "gemm" in name]
    for name in ("sgmcmc_gemm_tn_f32", "sgmcmc_gemm_tn_sghmc_f32", "sgmcmc_gemm_tn_sghmc_blocks"):
        assert not hasattr(handle, name)
    for word in ("phase_counters", "phase_sleep", "int variant", "probe"):
        assert word not in header, "include/sgmcmc_hip.h mentions %r" % word


def test_abi_holds_no_process_wide_state():
    """no global mutable state. The launch-geometry setter of ABI v1 is gone; the header must not
    declare, and the library must not export, any set/get configuration entry point."""
    from pysgmcmc_amd import _lib
    handle = ctypes.CDLL(_lib.build())
    for name in ("sgmcmc_set_launch_config", "sgmcmc_get_launch_config"):
        assert name not in _declared_symbols()
        assert not hasattr(handle, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    # exported data symbols (B/D = bss/data) would be process-wide state; the one allowed is the THREAD-LOCAL
    # error text behind sgmcmc_last_error() (sgmcmc_host::g_err, a TLS symbol)
    data = [l for l in nm.splitlines() if l.split()[1:2] and l.split()[1] in ("B", "D") and "sgmcmc" in l.lower()
            and "g_err" not in l]
    assert not data, data


def test_library_contains_gfx950_code_object():
    from pysgmcmc_amd import _lib
    out = subprocess.run(["strings", "-n", "6", _lib.lib_path()], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_build_dependencies_cover_every_file_the_makefile_names():
    """``_lib.build()`` rebuilds when a dependency is newer than the library: every translation unit and header the Makefile
    compiles from (SRCS, HDRS) must be one, or editing it would leave a stale library in place."""
    from pysgmcmc_amd import _lib
    text = open(os.path.join(ROOT, "pysgmcmc_amd", "csrc", "Makefile")).read().replace("\\\n", " ")
    named = []
    for var in ("SRCS", "HDRS"):
        named += re.search(r"^%s\s*:=(.*)$" % var, text, re.M).group(1).split()
    assert len(named) >= 15, named
    deps = _lib.build_dependencies()
    assert all(os.path.isfile(d) for d in deps), deps
    have = {os.path.basename(d) for d in deps}
    missing = [n for n in named if os.path.basename(n) not in have]
    assert not missing, missing
    assert {"sgmcmc_bnn_gw.hip", "sgmcmc_bnn_cost.hip", "Makefile"} <= have


def test_every_internal_header_a_translation_unit_includes_is_a_makefile_dependency():
    """The objects depend on HDRS and on nothing else: an ``#include "sgmcmc_*.hpp"`` in a ``csrc/*.hip`` that HDRS does not
    list would leave stale objects in place when that header is edited."""
    import glob
    csrc = os.path.join(ROOT, "pysgmcmc_amd", "csrc")
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    hdrs = set(re.search(r"^HDRS\s*:=(.*)$", text, re.M).group(1).split())
    units = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    included = {(os.path.basename(u), h) for u in units for h in re.findall(r'#include\s+"(sgmcmc_\w+\.hpp)"', open(u).read())}
    assert len(units) >= 15 and ("sgmcmc_bnn_predict.hip", "sgmcmc_bnn_small_net.hpp") in included
    missing = sorted((u, h) for u, h in included if h not in hdrs or not os.path.isfile(os.path.join(csrc, h)))
    assert not missing, missing
    # and a header one of those headers includes
    nested = {h2 for _, h in included for h2 in re.findall(r'#include\s+"(sgmcmc_\w+\.hpp)"', open(os.path.join(csrc, h)).read())}
    assert nested <= hdrs, sorted(nested - hdrs)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "pysgmcmc_amd")
    offenders = []
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b|sgmcmc_oracle|oracle_shim|libsgmcmc_oracle", text, re.M):
                    offenders.append(os.path.join(dirpath, f))
    assert not offenders, offenders


def test_missing_extension_fails_loudly(monkeypatch, tmp_path):
    from pysgmcmc_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.SgmcmcLibraryError):
        _lib.lib()


def test_cpu_tensor_is_refused():
    """No CPU fallback: stepping a sampler whose state is on the CPU raises."""
    import torch
    from pysgmcmc_amd import kernels
    from pysgmcmc_amd._lib import SgmcmcLibraryError
    t = torch.zeros(8)
    with pytest.raises(SgmcmcLibraryError):
        kernels.sghmc_step(t, t.clone(), t.clone(), t.clone(), t.clone(), t.clone(), t.clone(), None,
                           0.01, 1.0, 0.05, True)


def test_plain_graph_launch_is_a_call_not_a_default(monkeypatch):
    """The HIP-runtime setting that helps device-bound chains and hurts host-bound ones is never set by importing the package."""
    import pysgmcmc_amd
    monkeypatch.delenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", raising=False)
    assert pysgmcmc_amd.runtime_env() == {"DEBUG_CLR_GRAPH_PACKET_CAPTURE": None}
    import importlib
    importlib.reload(pysgmcmc_amd)
    assert pysgmcmc_amd.runtime_env() == {"DEBUG_CLR_GRAPH_PACKET_CAPTURE": None}
    in_time = pysgmcmc_amd.prefer_plain_graph_launch()
    assert pysgmcmc_amd.runtime_env() == {"DEBUG_CLR_GRAPH_PACKET_CAPTURE": "0"}
    import torch
    assert in_time == (not torch.cuda.is_initialized())
    monkeypatch.delenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", raising=False)
    # under a profiler's preloaded tool library the HIP runtime is up before Python runs: setting the variable here is too late ...
    monkeypatch.setattr(pysgmcmc_amd, "_PLAIN_LAUNCH_SET_IN_TIME", False)
    monkeypatch.setenv("LD_PRELOAD", "/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so")
    assert pysgmcmc_amd.prefer_plain_graph_launch() is False
    # ... and stays too late: the variable that call left in the environment is not mistaken for the caller's
    assert pysgmcmc_amd.runtime_env() == {"DEBUG_CLR_GRAPH_PACKET_CAPTURE": "0"}
    assert pysgmcmc_amd.prefer_plain_graph_launch() is False
    assert pysgmcmc_amd.configure_for_device_bound_chains(gemm_tuning=False)["plain_graph_launch"] is False
    # ... unless whoever started the process exported it (recorded when the package was imported)
    monkeypatch.setattr(pysgmcmc_amd, "_PLAIN_LAUNCH_EXPORTED_AT_IMPORT", True)
    assert pysgmcmc_amd.prefer_plain_graph_launch() is True
    monkeypatch.delenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", raising=False)
    monkeypatch.setenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
    importlib.reload(pysgmcmc_amd)
    assert pysgmcmc_amd._PLAIN_LAUNCH_EXPORTED_AT_IMPORT is True
    monkeypatch.delenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", raising=False)
    importlib.reload(pysgmcmc_amd)
    assert pysgmcmc_amd._PLAIN_LAUNCH_EXPORTED_AT_IMPORT is False


def test_device_bound_switch_reports_what_took_effect(monkeypatch):
    """``configure_for_device_bound_chains()`` is the one documented call behind bench.py's `value`: it returns what took effect
    (the graph launch path only before the first HIP call; GEMM tuning only where TunableOp exists -- not on a box without a
    device, where it must not raise either)."""
    import pysgmcmc_amd
    import torch
    monkeypatch.delenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", raising=False)
    try:
        took = pysgmcmc_amd.configure_for_device_bound_chains()
        assert took["plain_graph_launch"] == (not torch.cuda.is_initialized()) and set(took) == {"gemm_tuning", "plain_graph_launch"}
        assert took["gemm_tuning"] or not torch.cuda.is_available()
        assert pysgmcmc_amd.runtime_env() == {"DEBUG_CLR_GRAPH_PACKET_CAPTURE": "0"}
        monkeypatch.delenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", raising=False)
        assert pysgmcmc_amd.configure_for_device_bound_chains(gemm_tuning=False, plain_graph_launch=False) == {
            "gemm_tuning": False, "plain_graph_launch": False}
        assert pysgmcmc_amd.runtime_env() == {"DEBUG_CLR_GRAPH_PACKET_CAPTURE": None}
    finally:
        if torch.cuda.is_available():
            from pysgmcmc_amd.models.bayesian_neural_network import enable_gemm_tuning
            enable_gemm_tuning(False)


def test_dense_layer_column_plan_without_a_device():
    """``sgmcmc_bnn_dense_tanh_dot_parts`` is host arithmetic (which columns of an M x N layer run as 32 x 64 tiles and which as
    half tiles): without a device it assumes 256 compute units, MI355X's count."""
    from pysgmcmc_amd import _lib
    lib = _lib.lib()
    parts = lib.sgmcmc_bnn_dense_tanh_dot_parts
    assert parts(256, 2048) == 32                                # one tile per CU: 32 column tiles of 64
    assert parts(512, 2048) == 32                                # two full rounds
    assert parts(256, 4864) == 64 + 24                           # configs[4]: 512 full tiles + the last 12 column tiles as 24 half tiles
    assert parts(256, 4096 + 64 * 20) == (4096 + 64 * 20) // 64  # a last round more than half full stays on full tiles
    assert parts(20, 2048) == 0 and parts(256, 100) == 0         # shapes the launch refuses


# state pointers / by-value scalars (eps first) of sgmcmc_<kind>_step_*; the burn-in kinds take an adapt flag behind grad_decay
_STEP_ENTRIES = {"sghmc": (8, 3), "sgld": (7, 3), "rsghmc": (3, 5)}


def _step_call(lib, kind, sfx, rows, n=4, adapt=0, stats_ws=None, opts=None, launch=None):
    n_rows, n_scalars = _STEP_ENTRIES[kind]
    rows = [4096 * (k + 1) for k in range(n_rows)] if rows is None else rows        # never dereferenced: the call fails first
    flag = [] if kind == "rsghmc" else [adapt]
    f = getattr(lib, "sgmcmc_%s_step_%s" % (kind, sfx))
    return f(*rows, n, *[0.01] * (n_scalars + 1), *flag, None, 1, 0, None, stats_ws, opts, launch, None)


def test_step_entries_refuse_bad_arguments_before_any_launch():
    """The per-step entries validate on the host, in a fixed order, before the first HIP call: return code and
    ``sgmcmc_last_error()`` text of every refusal (the texts an integrator's logs carry), on a machine without a device."""
    from pysgmcmc_amd import _lib
    lib = _lib.lib()
    required = {"sghmc": b"sghmc_step: theta, V, grad and minv must be non-NULL",
                "sgld": b"sgld_step: theta, grad and minv must be non-NULL",
                "rsghmc": b"rsghmc_step: theta, p and grad_cost must be non-NULL"}
    needs = {"sghmc": b"sghmc_step: adapt=1 needs tau, g and v_hat", "sgld": b"sgld_step: adapt=1 needs tau, g and v_hat"}
    gather = dict(gather_x=4096, gather_y=8192, gather_x_out=12288, gather_y_out=16384, gather_batch=32, gather_x_out_ld=16)
    bad_opts = [
        (dict(first_element=2), None, b"%s_step: opts.first_element must be a multiple of 4 (slices start on a quad)"),
        (dict(stats_select=7), None, b"%s_step: opts.stats_select must be 0 (all) or SGMCMC_STATS_THETA_SQ"),
        (dict(stats_record_total=1), None, b"%s_step: opts.stats_record_* without a stats workspace"),
        (dict(moments_mean=4096), None, b"%s_step: opts.moments_mean and opts.moments_m2 go together"),
        (dict(moments_mean=4096, moments_m2=8192, moments_count=0), None, b"%s_step: opts.moments_count must be >= 1"),
        (dict(gather_dim=0, **gather), None,
         b"%s_step: opts.gather_* needs X, y, both outputs, batch > 0, dim > 0 and x_out_ld >= dim"),
        (None, _lib.LaunchStruct(100, 0, 0, -1), b"launch.block_threads must be 64, 128, 192, 256, 0 (default) or -1 (auto)"),
    ]
    for sfx in ("f32", "f64"):
        for kind, (n_rows, n_scalars) in _STEP_ENTRIES.items():
            assert _step_call(lib, kind, sfx, [None] * n_rows) == -1
            assert lib.sgmcmc_last_error() == required[kind]
            # n == 0 returns before the NULL checks and leaves the previous error text in place
            assert _step_call(lib, kind, sfx, [None] * n_rows, n=0, adapt=1) == 0
            assert lib.sgmcmc_last_error() == required[kind]
            if kind in needs:
                rows = [4096 * (k + 1) for k in range(n_rows)]
                for k in range(n_rows - 5, n_rows - 2):                             # tau, g, v_hat
                    assert _step_call(lib, kind, sfx, rows[:k] + [None] + rows[k + 1:], adapt=1) == -1
                    assert lib.sgmcmc_last_error() == needs[kind]
            for fields, launch, text in bad_opts:
                opts = None if fields is None else ctypes.byref(_lib.StepOptsStruct(**fields))
                assert _step_call(lib, kind, sfx, None, opts=opts, launch=None if launch is None else ctypes.byref(launch)) == -1
                assert lib.sgmcmc_last_error() == (text % kind.encode() if b"%s" in text else text)
            scalars = getattr(lib, "sgmcmc_%s_scalars_%s" % (kind, sfx))
            assert scalars(*[0.01] * n_scalars, None, None) == -1
            assert lib.sgmcmc_last_error() == b"%s_scalars: scalars_dev is NULL" % kind.encode()


def test_step_entries_are_declared_with_the_header_s_argument_types():
    """``_lib._declare`` builds the twelve per-step declarations from one table: the lists it must produce, written out."""
    from pysgmcmc_amd import _lib
    lib = _lib.lib()
    vp, sz, ci, u64, op, lp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64, _lib._op, _lib._lp
    for sfx, real in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        want = {
            "sgmcmc_sghmc_step_": [vp, vp, vp, vp, vp, vp, vp, vp, sz, real, real, real, real, ci, vp, u64, u64, vp, vp, op, lp, vp],
            "sgmcmc_sgld_step_": [vp, vp, vp, vp, vp, vp, vp, sz, real, real, real, real, ci, vp, u64, u64, vp, vp, op, lp, vp],
            "sgmcmc_rsghmc_step_": [vp, vp, vp, sz, real, real, real, real, real, real, vp, u64, u64, vp, vp, op, lp, vp],
            "sgmcmc_sghmc_scalars_": [real, real, real, vp, vp],
            "sgmcmc_sgld_scalars_": [real, real, real, vp, vp],
            "sgmcmc_rsghmc_scalars_": [real, real, real, real, real, vp, vp],
        }
        for name, argtypes in want.items():
            f = getattr(lib, name + sfx)
            assert list(f.argtypes) == argtypes and f.restype is ci, name + sfx
