"""ctypes binding of ``libsgmcmc_hip.so`` (C ABI in ``include/sgmcmc_hip.h``).

This is the only way the package reaches the GPU update kernels. There is no
CPU fallback: if the shared library is missing or a call fails, a
``SgmcmcLibraryError`` is raised.
"""
import ctypes
import os

__all__ = ["SgmcmcLibraryError", "lib", "lib_path", "check", "build", "build_dependencies"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
# PYSGMCMC_AMD_LIB: load an alternative build of the same ABI (kernel experiments)
_LIB_PATH = os.environ.get("PYSGMCMC_AMD_LIB") or os.path.join(_CSRC, "libsgmcmc_hip.so")


class SgmcmcLibraryError(RuntimeError):
    """libsgmcmc_hip.so is missing, failed to load, or a call into it failed."""


def lib_path():
    return _LIB_PATH


def build_dependencies():
    """Every file the library is built from, as found on disk: the translation units, their headers and the Makefile in
    ``csrc/``, and the public headers in ``include/``. ``build()`` rebuilds when one of them is newer than the library."""
    import glob
    include = os.path.join(os.path.dirname(_HERE), "include")
    return sorted(glob.glob(os.path.join(_CSRC, "*.hip")) + glob.glob(os.path.join(_CSRC, "*.hpp"))
                  + [os.path.join(_CSRC, "Makefile")] + glob.glob(os.path.join(include, "*.h")))


def build(force=False):
    """Compile ``csrc/libsgmcmc_hip.so`` for gfx950 with hipcc (no GPU needed)."""
    import subprocess
    deps = build_dependencies()
    stale = (not os.path.exists(_LIB_PATH)
             or os.path.getmtime(_LIB_PATH) < max(os.path.getmtime(d) for d in deps))
    if force or stale:
        subprocess.check_call(["make", "-s", "-j4", "-C", _CSRC, "libsgmcmc_hip.so"])
    return _LIB_PATH


_lib = None
ABI_VERSION = 6               # SGMCMC_ABI_VERSION of include/sgmcmc_hip.h
DIAG_ABI_VERSION = 1          # SGMCMC_DIAG_ABI_VERSION of include/sgmcmc_hip_diag.h (the diagnostics add-on)
FUSED_ABI_VERSION = 1         # SGMCMC_FUSED_ABI_VERSION of include/sgmcmc_hip_fused.h (the whole-step add-on)
FUSED_TRACE_ABI_VERSION = 1   # SGMCMC_FUSED_TRACE_ABI_VERSION of include/sgmcmc_hip_fused_trace.h (the thinned-trace add-on)
PREDICT_ABI_VERSION = 1       # SGMCMC_PREDICT_ABI_VERSION of include/sgmcmc_hip_predict.h (the posterior-predictive add-on)
CHAINS_ABI_VERSION = 1        # SGMCMC_CHAINS_ABI_VERSION of include/sgmcmc_hip_chains.h (the many-chains diagnostics add-on)
SCORE_ABI_VERSION = 1         # SGMCMC_SCORE_ABI_VERSION of include/sgmcmc_hip_score.h (the held-out-score add-on)
PREDICT_GRAD_ABI_VERSION = 1  # SGMCMC_PREDICT_GRAD_ABI_VERSION of include/sgmcmc_hip_predict_grad.h (the predictive-gradient add-on)
PARTICLES_ABI_VERSION = 1     # SGMCMC_PARTICLES_ABI_VERSION of include/sgmcmc_hip_particles.h (the particle-gradient add-on)
SVGD_MANY_ABI_VERSION = 1     # SGMCMC_SVGD_MANY_ABI_VERSION of include/sgmcmc_hip_svgd_many.h (SVGD with up to 1024 particles)
KSD_ABI_VERSION = 1           # SGMCMC_KSD_ABI_VERSION of include/sgmcmc_hip_ksd.h (the kernel Stein discrepancy, K16)
THIN_ABI_VERSION = 1          # SGMCMC_THIN_ABI_VERSION of include/sgmcmc_hip_thin.h (Stein thinning, K17)
RANK_ABI_VERSION = 1          # SGMCMC_RANK_ABI_VERSION of include/sgmcmc_hip_rank.h (rank normalisation, K18)
PSIS_ABI_VERSION = 1          # SGMCMC_PSIS_ABI_VERSION of include/sgmcmc_hip_psis.h (PSIS-LOO, K19)
CALIB_ABI_VERSION = 1         # SGMCMC_CALIB_ABI_VERSION of include/sgmcmc_hip_calib.h (PIT, coverage and CRPS, K20)
ESS_STAGING_AUTO, ESS_STAGING_LDS, ESS_STAGING_GLOBAL = 0, 1, 2
ESS_MAX_CHAINS = 64
PREDICT_MAX_CHAINS = 64
CHAINS_MAX_CHAINS = 4096
RANK_MAX_CHAINS = 2048        # SGMCMC_RANK_MAX_CHAINS: the 2 m split chains must fit K12
RANK_MAX_POOLED = 8192        # SGMCMC_RANK_MAX_POOLED: pooled draws of one parameter, N = 2 m (n // 2)
PSIS_MAX_DRAWS = 8192         # SGMCMC_PSIS_MAX_DRAWS: draws of one observation column
CALIB_MAX_DRAWS = 4096        # SGMCMC_CALIB_MAX_DRAWS: draws of one predictive mixture
CALIB_MAX_LEVELS = 16         # SGMCMC_CALIB_MAX_LEVELS
CALIB_MAX_BINS = 64           # SGMCMC_CALIB_MAX_BINS
SCORE_MAX_CHAINS = 64
PREDICT_GRAD_MAX_CHAINS = 64

_u64 = ctypes.c_uint64
_sz = ctypes.c_size_t
_ci = ctypes.c_int
_vp = ctypes.c_void_p


class LaunchStruct(ctypes.Structure):
    """``sgmcmc_launch_t``: per-call launch geometry (0 / -1 = default)."""
    _fields_ = [("block_threads", _ci), ("quads_per_thread", _ci), ("max_blocks", _ci), ("nontemporal", _ci),
                ("start_event", _vp), ("stop_event", _vp)]


_lp = ctypes.POINTER(LaunchStruct)


class StepOptsStruct(ctypes.Structure):
    """``sgmcmc_step_opts_t``: optional extras of one step call (slices, statistics selection, fused moments, ...)."""
    _fields_ = [("first_element", ctypes.c_uint64), ("stats_record_base", ctypes.c_uint32),
                ("stats_record_total", ctypes.c_uint32), ("stats_select", ctypes.c_int), ("flags", ctypes.c_uint),
                ("moments_mean", ctypes.c_void_p), ("moments_m2", ctypes.c_void_p), ("moments_count", ctypes.c_uint64),
                ("scalars_dev", ctypes.c_void_p),
                ("gather_x", ctypes.c_void_p), ("gather_y", ctypes.c_void_p), ("gather_x_out", ctypes.c_void_p),
                ("gather_y_out", ctypes.c_void_p), ("gather_start", ctypes.c_uint64), ("gather_batch", ctypes.c_uint32),
                ("gather_dim", ctypes.c_uint32), ("gather_x_out_ld", ctypes.c_uint32), ("reserved0", ctypes.c_uint32)]


_op = ctypes.POINTER(StepOptsStruct)
STATS_THETA_SQ = 1
STEP_HBM_RESIDENT = 1
STEP_SKIP_MINV_STORE = 2


def _declare(lib):
    lib.sgmcmc_abi_version.restype = _ci
    lib.sgmcmc_last_error.restype = ctypes.c_char_p
    lib.sgmcmc_device_count.restype = _ci
    lib.sgmcmc_event_create.argtypes = [ctypes.POINTER(_vp)]
    lib.sgmcmc_event_create.restype = _ci
    lib.sgmcmc_event_destroy.argtypes = [_vp]
    lib.sgmcmc_event_destroy.restype = _ci
    lib.sgmcmc_event_elapsed_ms.argtypes = [_vp, _vp, ctypes.POINTER(ctypes.c_float)]
    lib.sgmcmc_event_elapsed_ms.restype = _ci
    lib.sgmcmc_event_synchronize.argtypes = [_vp]
    lib.sgmcmc_event_synchronize.restype = _ci
    # The per-step update entries (sgmcmc_hip.h [boundary]): state pointers, n, the kind's by-value scalars (eps first),
    # grad_decay, [adapt,] xi, seed, step, step_dev, stats_ws, opts, launch, stream; their scalars twins: the same scalars,
    # scalars_dev, stream. kind: (state pointers, by-value scalars, adapt flag)
    per_step = {"sghmc": (8, 3, True), "sgld": (7, 3, True), "rsghmc": (3, 5, False)}
    for sfx, real in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        for kind, (n_rows, n_scalars, adapt) in per_step.items():
            f = getattr(lib, "sgmcmc_%s_step_%s" % (kind, sfx))
            f.argtypes = ([_vp] * n_rows + [_sz] + [real] * (n_scalars + 1) + ([_ci] if adapt else [])
                          + [_vp, _u64, _u64, _vp, _vp, _op, _lp, _vp])
            f.restype = _ci
            f = getattr(lib, "sgmcmc_%s_scalars_%s" % (kind, sfx))
            f.argtypes = [real] * n_scalars + [_vp, _vp]
            f.restype = _ci
        f = getattr(lib, "sgmcmc_toy_chains_" + sfx)
        f.argtypes = [_ci, _ci, ctypes.POINTER(ctypes.c_double), _ci] + [_vp] * 6 + [_sz, _ci, ctypes.POINTER(ctypes.c_double),
                      _vp, _u64, _u64, ctypes.c_int64, _u64, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_philox_normal_" + sfx)
        f.argtypes = [_vp, _sz, _u64, _u64, _vp, _lp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_moments_update_" + sfx)
        f.argtypes = [_vp, _vp, _vp, _sz, _u64, _lp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_rhat_pack_" + sfx)
        f.argtypes = [_vp, _vp, _sz, _u64, _sz, _sz, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_rhat_finish_" + sfx)
        f.argtypes = [_vp, _sz, _sz, _ci, _u64, _vp, _vp, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_bnn_head_" + sfx)
        f.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _sz] + [ctypes.c_double] * 6 + [_ci, _vp, _vp, _vp, _vp, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_bnn_last_layer_backward_" + sfx)
        f.argtypes = [_vp, _vp, _vp, _sz, _sz, _vp, real, _vp, _vp, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_tanh_backward_colsum_" + sfx)
        f.argtypes = [_vp, _vp, _sz, _sz, _vp, real, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_tanh_backward_" + sfx)
        f.argtypes = [_vp, _vp, _sz, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_bias_tanh_rowdot_" + sfx)
        f.argtypes = [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_bias_tanh_" + sfx)
        f.argtypes = [_vp, _vp, _sz, _sz, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_bnn_head_last_layer_backward_" + sfx)
        f.argtypes = ([_vp, _sz] + [_vp] * 4 + [_sz, _sz] + [ctypes.c_double] * 6 + [_ci, _vp, _vp, _vp, real] + [_vp] * 7 + [_vp])
        f.restype = _ci
        f = getattr(lib, "sgmcmc_window_gather_" + sfx)
        f.argtypes = [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_svgd_step_" + sfx)
        f.argtypes = [_vp, _vp, _vp, _sz, _sz, _sz, real, ctypes.c_double, real, _ci, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_svgd_kernel_" + sfx)
        f.argtypes = [_vp, _sz, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_summary_" + sfx)
        f.argtypes = [_vp, _sz, _vp, _vp, _vp]
        f.restype = _ci
    lib.sgmcmc_bnn_dense_tanh_f32.argtypes = [_vp] * 4 + [_ci] * 6 + [_vp] * 5
    lib.sgmcmc_bnn_dense_tanh_f32.restype = _ci
    lib.sgmcmc_bnn_dense_tanh_dot_parts.argtypes = [_ci, _ci]
    lib.sgmcmc_bnn_dense_tanh_dot_parts.restype = _ci
    lib.sgmcmc_bnn_dense_tanh_backward_f32.argtypes = [_vp] * 5 + [_ci] * 7 + [_vp, _ci, _ci, _vp, ctypes.c_float, _vp, _vp]
    lib.sgmcmc_bnn_dense_tanh_backward_f32.restype = _ci
    lib.sgmcmc_colsum_finish_f32.argtypes = [_vp, _ci, _ci, _vp, ctypes.c_float, _vp, _vp]
    lib.sgmcmc_colsum_finish_f32.restype = _ci
    lib.sgmcmc_bnn_planes_bytes.argtypes = [_ci, _ci]
    lib.sgmcmc_bnn_planes_bytes.restype = _sz
    lib.sgmcmc_bnn_split_planes_f32.argtypes = [_vp, _ci, _sz, _ci, _ci, _ci, _vp, _sz, _vp]
    lib.sgmcmc_bnn_split_planes_f32.restype = _ci
    lib.sgmcmc_bnn_gw_planes_f32.argtypes = [_vp, _sz, _vp, _sz, _vp, _sz, _ci, _ci, _ci, _ci, _ci, _vp]
    lib.sgmcmc_bnn_gw_planes_f32.restype = _ci
    lib.sgmcmc_philox_bits_u32.argtypes = [_vp, _sz, _u64, _u64, _vp, _vp]
    lib.sgmcmc_counter_add_u64.argtypes = [_vp, _u64, _vp]
    lib.sgmcmc_counter_add_u64.restype = _ci
    lib.sgmcmc_philox_bits_u32.restype = _ci
    lib.sgmcmc_summary_workspace_bytes.restype = _sz
    lib.sgmcmc_svgd_workspace_bytes.argtypes = [_sz, _sz]
    lib.sgmcmc_svgd_workspace_bytes.restype = _sz
    lib.sgmcmc_svgd_max_particles.restype = _ci
    lib.sgmcmc_step_stats_workspace_bytes.argtypes = [_sz]
    lib.sgmcmc_step_stats_workspace_bytes.restype = _sz
    lib.sgmcmc_step_stats_records.argtypes = [_sz, _lp]
    lib.sgmcmc_step_stats_records.restype = _sz
    lib.sgmcmc_step_stats_records_sized.argtypes = [_sz, _sz, _lp]
    lib.sgmcmc_step_stats_records_sized.restype = _sz
    lib.sgmcmc_step_stats_finish.argtypes = [_vp, _vp, _vp]
    lib.sgmcmc_step_stats_finish.restype = _ci
    # include/sgmcmc_hip_diag.h
    lib.sgmcmc_diag_abi_version.restype = _ci
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_ess_variogram_" + sfx)
        f.argtypes = [ctypes.POINTER(_vp), _ci, _sz, _sz, _sz, _vp, _vp, _vp, _ci, _lp, _vp]
        f.restype = _ci
    # include/sgmcmc_hip_fused.h
    lib.sgmcmc_fused_abi_version.restype = _ci
    # The whole-step BNN kernel's entry points (sgmcmc_hip.h [whole-step] and sgmcmc_hip_fused.h): state rows, the net run
    # n_params .. prior_var, the kind's by-value scalars (eps first), first_step, n_steps, [burn_in_steps,] seed_base, xi,
    # cost_out, stream. A `sched` twin takes a required table where eps was; the relativistic entry an optional one after
    # its scalars. kind: (rows, by-value scalars, burn_in_steps argument, sched twin)
    net = [_sz, _sz, _ci, ctypes.POINTER(_ci), _ci, _vp, _vp, _sz, _vp, _ci] + [ctypes.c_double] * 5
    whole_step = {"sghmc": (7, 3, True, True), "sgld": (6, 3, True, True), "rsghmc": (3, 5, False, False)}
    for sfx, real in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        for kind, (n_rows, n_scalars, burn_in, sched) in whole_step.items():
            f = getattr(lib, "sgmcmc_%s_scalars_steps_%s" % (kind, sfx))        # host pointers, nothing launched
            f.argtypes = [ctypes.POINTER(real), _sz] + [real] * (n_scalars - 1) + [ctypes.POINTER(real)]
            f.restype = _ci
            tail = [_u64] * (4 if burn_in else 3) + [_vp, _vp, _vp]
            f = getattr(lib, "sgmcmc_bnn_fused_%s_steps_%s" % (kind, sfx))
            f.argtypes = [_vp] * n_rows + net + [real] * n_scalars + ([] if sched else [_vp]) + tail
            f.restype = _ci
            if sched:
                f = getattr(lib, "sgmcmc_bnn_fused_%s_sched_steps_%s" % (kind, sfx))
                f.argtypes = [_vp] * n_rows + net + [_vp] + [real] * (n_scalars - 1) + tail
                f.restype = _ci
    # include/sgmcmc_hip_fused_trace.h: kind, host array of rows, the net run, host array of scalars, table, first_step,
    # n_steps, burn_in_steps, seed_base, xi, cost_out, trace, its chain stride, capacity, row, every, phase, stream
    lib.sgmcmc_fused_trace_abi_version.restype = _ci
    for sfx, real in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        f = getattr(lib, "sgmcmc_bnn_fused_trace_steps_" + sfx)
        f.argtypes = ([_ci, ctypes.POINTER(_vp), _ci] + net + [ctypes.POINTER(real), _ci, _vp] + [_u64] * 4
                      + [_vp, _vp, _vp, _sz] + [_u64] * 4 + [_vp])
        f.restype = _ci
    # include/sgmcmc_hip_predict.h: host array of chain matrices, m, n, ld, layer sizes, n_layers, X, n_rows, means, noise_var,
    # ens_mean, ens_var, stream
    lib.sgmcmc_predict_abi_version.restype = _ci
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_bnn_predict_" + sfx)
        f.argtypes = [ctypes.POINTER(_vp), _ci, _sz, _sz, ctypes.POINTER(_ci), _ci, _vp, _sz, _vp, _vp, _vp, _vp, _vp]
        f.restype = _ci
    lib.sgmcmc_bnn_predict_row_tile.argtypes = [ctypes.POINTER(_ci), _ci, _sz]
    lib.sgmcmc_bnn_predict_row_tile.restype = _ci
    # include/sgmcmc_hip_chains.h: trace, m, n, P, ld, chain_stride, rhat, ess, raw, stop_lag, waves, stream
    lib.sgmcmc_chains_abi_version.restype = _ci
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_chain_diag_" + sfx)
        f.argtypes = [_vp, _ci, _sz, _sz, _sz, _sz, _vp, _vp, _vp, _vp, _ci, _vp]
        f.restype = _ci
    # include/sgmcmc_hip_score.h: host array of chain matrices, m, n, ld, layer sizes, n_layers, X, y, n_rows, means, row_lppd,
    # row_pwaic, ens_mean, ens_var, loglik, sample_loglik, summary, stream
    lib.sgmcmc_score_abi_version.restype = _ci
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_bnn_score_" + sfx)
        f.argtypes = [ctypes.POINTER(_vp), _ci, _sz, _sz, ctypes.POINTER(_ci), _ci, _vp, _vp, _sz] + [_vp] * 8 + [_vp]
        f.restype = _ci
    # include/sgmcmc_hip_predict_grad.h: host array of chain matrices, m, n, ld, layer sizes, n_layers, X, n_rows, means, grads,
    # ens_mean, ens_var, dmean, dvar, stream
    lib.sgmcmc_predict_grad_abi_version.restype = _ci
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_bnn_predict_grad_" + sfx)
        f.argtypes = [ctypes.POINTER(_vp), _ci, _sz, _sz, ctypes.POINTER(_ci), _ci, _vp, _sz] + [_vp] * 6 + [_vp]
        f.restype = _ci
    lib.sgmcmc_bnn_predict_grad_row_tile.argtypes = [ctypes.POINTER(_ci), _ci, _sz]
    lib.sgmcmc_bnn_predict_grad_row_tile.restype = _ci
    # include/sgmcmc_hip_particles.h: theta, n_particles, ld, layer sizes, n_layers, Xb, ldx, yb, batch, batch_size, n_examples,
    # wdecay, prior_mean, prior_var, add_prior, grad, ld_grad, cost_out, stream
    lib.sgmcmc_particles_abi_version.restype = _ci
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_bnn_particles_cost_grad_" + sfx)
        f.argtypes = ([_vp, _sz, _sz, ctypes.POINTER(_ci), _ci, _vp, _sz, _vp, _ci] + [ctypes.c_double] * 5
                      + [_ci, _vp, _sz, _vp, _vp])
        f.restype = _ci
    lib.sgmcmc_bnn_particles_lds_bytes.argtypes = [ctypes.POINTER(_ci), _ci, _ci, _sz]
    lib.sgmcmc_bnn_particles_lds_bytes.restype = _sz
    # include/sgmcmc_hip_svgd_many.h: the argument lists of sgmcmc_svgd_step_* / sgmcmc_svgd_kernel_* above
    lib.sgmcmc_svgd_many_abi_version.restype = _ci
    lib.sgmcmc_svgd_many_max_particles.restype = _ci
    lib.sgmcmc_svgd_many_workspace_bytes.argtypes = [_sz, _sz]
    lib.sgmcmc_svgd_many_workspace_bytes.restype = _sz
    lib.sgmcmc_svgd_many_plan.argtypes = [_sz, _sz, _sz, ctypes.POINTER(_ci), _ci]
    lib.sgmcmc_svgd_many_plan.restype = _ci
    for sfx, real in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        f = getattr(lib, "sgmcmc_svgd_many_step_" + sfx)
        f.argtypes = [_vp, _vp, _vp, _sz, _sz, _sz, real, ctypes.c_double, real, _ci, _vp, _vp]
        f.restype = _ci
        f = getattr(lib, "sgmcmc_svgd_many_kernel_" + sfx)
        f.argtypes = [_vp, _sz, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp]
        f.restype = _ci
    # include/sgmcmc_hip_ksd.h: samples, ld_x, scores, ld_s, n, dim, kind, c, beta, h2, workspace, matrix_out, ld_m,
    # row_sums_out, stats_out, stream
    lib.sgmcmc_ksd_abi_version.restype = _ci
    lib.sgmcmc_ksd_max_samples.restype = _ci
    lib.sgmcmc_ksd_workspace_bytes.argtypes = [_sz, _sz]
    lib.sgmcmc_ksd_workspace_bytes.restype = _sz
    lib.sgmcmc_ksd_plan.argtypes = [_sz, _sz, _sz, ctypes.POINTER(_ci), _ci]
    lib.sgmcmc_ksd_plan.restype = _ci
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_ksd_" + sfx)
        f.argtypes = [_vp, _sz, _vp, _sz, _sz, _sz, _ci] + [ctypes.c_double] * 3 + [_vp, _vp, _sz, _vp, _vp, _vp]
        f.restype = _ci
    # include/sgmcmc_hip_thin.h: matrix, ld_m, n, m, batch, batch_stride, flags, indices_out, path_out, stream
    lib.sgmcmc_stein_thin_abi_version.restype = _ci
    lib.sgmcmc_stein_thin_max_samples.restype = _ci
    lib.sgmcmc_stein_thin_plan.argtypes = [_sz, _sz, _sz, ctypes.POINTER(_ci), _ci]
    lib.sgmcmc_stein_thin_plan.restype = _ci
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_stein_thin_" + sfx)
        f.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, _ci, _vp, _vp, _vp]
        f.restype = _ci
    # include/sgmcmc_hip_rank.h: trace, m, n, P, ld, chain_stride, z, z_folded, tail_lo, tail_hi, ld_out, chain_stride_out, stream
    lib.sgmcmc_rank_abi_version.restype = _ci
    lib.sgmcmc_rank_max_pooled.restype = _ci
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_rank_normalize_" + sfx)
        f.argtypes = [_vp, _ci, _sz, _sz, _sz, _sz, _vp, _vp, _vp, _vp, _sz, _sz, _vp]
        f.restype = _ci
    # include/sgmcmc_hip_psis.h: loglik, ld, S, n_rows, r_eff, elpd_loo, khat, n_tail, row_lppd, log_weights, ld_w, summary, stream
    lib.sgmcmc_psis_abi_version.restype = _ci
    lib.sgmcmc_psis_max_draws.restype = _ci
    lib.sgmcmc_psis_loo.argtypes = [_vp, _sz, _sz, _sz, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]
    lib.sgmcmc_psis_loo.restype = _ci
    # include/sgmcmc_hip_calib.h: means, ld, S, n_rows, var, y, levels, n_levels, n_bins, pit, crps, summary, stream
    lib.sgmcmc_calib_abi_version.restype = _ci
    lib.sgmcmc_calib_max_draws.restype = _ci
    for sfx in ("f32", "f64"):
        f = getattr(lib, "sgmcmc_mixture_calibration_" + sfx)
        f.argtypes = [_vp, _sz, _sz, _sz, _vp, _vp, ctypes.POINTER(ctypes.c_double), _ci, _ci, _vp, _vp, _vp, _vp]
        f.restype = _ci


def lib():
    """The loaded library (argtypes declared). Raises SgmcmcLibraryError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise SgmcmcLibraryError(
            "pysgmcmc_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C pysgmcmc_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback." % _LIB_PATH)
    try:
        handle = ctypes.CDLL(_LIB_PATH)
    except OSError as exc:
        raise SgmcmcLibraryError("pysgmcmc_amd: cannot load %s: %s" % (_LIB_PATH, exc))
    _declare(handle)
    if handle.sgmcmc_abi_version() != ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_diag_abi_version() != DIAG_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: diagnostics ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_fused_abi_version() != FUSED_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: whole-step add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_fused_trace_abi_version() != FUSED_TRACE_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: thinned-trace add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_predict_abi_version() != PREDICT_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: posterior-predictive add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_chains_abi_version() != CHAINS_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: many-chains diagnostics add-on (chains ABI) version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_score_abi_version() != SCORE_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: held-out-score add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_predict_grad_abi_version() != PREDICT_GRAD_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: predictive-gradient add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_particles_abi_version() != PARTICLES_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: particle-gradient add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_svgd_many_abi_version() != SVGD_MANY_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: many-particle SVGD add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_ksd_abi_version() != KSD_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: kernel Stein discrepancy add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_stein_thin_abi_version() != THIN_ABI_VERSION:
        raise SgmcmcLibraryError("pysgmcmc_amd: Stein thinning add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_rank_abi_version() != RANK_ABI_VERSION or handle.sgmcmc_rank_max_pooled() != RANK_MAX_POOLED:
        raise SgmcmcLibraryError("pysgmcmc_amd: rank normalisation add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_psis_abi_version() != PSIS_ABI_VERSION or handle.sgmcmc_psis_max_draws() != PSIS_MAX_DRAWS:
        raise SgmcmcLibraryError("pysgmcmc_amd: PSIS-LOO add-on ABI version mismatch in %s" % _LIB_PATH)
    if handle.sgmcmc_calib_abi_version() != CALIB_ABI_VERSION or handle.sgmcmc_calib_max_draws() != CALIB_MAX_DRAWS:
        raise SgmcmcLibraryError("pysgmcmc_amd: calibration add-on ABI version mismatch in %s" % _LIB_PATH)
    _lib = handle
    return handle


def check(rc, what):
    """Turn a non-zero return code into an exception carrying sgmcmc_last_error()."""
    if rc != 0:
        msg = lib().sgmcmc_last_error()
        raise SgmcmcLibraryError("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else "?"))
