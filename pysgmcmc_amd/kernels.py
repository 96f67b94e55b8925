"""Thin torch-tensor front end of the C ABI (``include/sgmcmc_hip.h``).

Every function takes flat, contiguous device tensors, passes their raw
pointers to ``libsgmcmc_hip.so`` and launches on torch's *current* HIP stream
(so ``torch.cuda.Event`` timing, stream ordering with the autograd kernels and
``torch.cuda.graph`` capture all see the launch). PyTorch is plumbing here:
device memory and streams only.

No CPU path exists: a CPU tensor raises ``SgmcmcLibraryError``.
"""
import collections
import ctypes

import torch

from pysgmcmc_amd._lib import CALIB_MAX_BINS, CALIB_MAX_DRAWS, CALIB_MAX_LEVELS, PSIS_MAX_DRAWS, RANK_MAX_CHAINS, RANK_MAX_POOLED, SgmcmcLibraryError, check, lib

__all__ = [
    "sghmc_step", "sgld_step", "rsghmc_step", "update_step", "philox_normal", "philox_bits",
    "moments_update", "rhat_pack", "rhat_finish", "summary",
    "LaunchConfig", "KernelEvents", "StepOpts", "step_stats_records", "step_scalars", "toy_chains", "set_launch_config", "get_launch_config", "summary_workspace", "counter_add", "StepStats", "bnn_head", "bnn_dense_tanh_backward", "bnn_dense_tanh_backward_fits", "colsum_finish", "tanh_backward", "tanh_backward_colsum", "bnn_last_layer_backward", "bnn_fused_sghmc_steps", "step_stats_finish",
    "bnn_fused_sgld_steps", "bnn_fused_rsghmc_steps", "bnn_fused_steps", "step_scalars_table", "window_gather", "tanh_rowdot", "bias_tanh", "bnn_dense_tanh", "bnn_dense_tanh_fits", "bnn_head_last_layer_backward", "svgd_workspace", "svgd_step", "svgd_kernel", "svgd_max_particles",
    "ess_variogram", "bnn_predict", "bnn_predict_row_tile", "chain_diag", "bnn_score",
    "bnn_predict_grad", "bnn_predict_grad_row_tile", "bnn_particles_cost_grad", "bnn_particles_lds_bytes",
    "svgd_many_max_particles", "svgd_many_workspace", "svgd_many_step", "svgd_many_kernel", "svgd_many_plan",
    "ksd_max_samples", "ksd_workspace", "ksd_plan", "ksd",
    "stein_thin_max_samples", "stein_thin_plan", "stein_thin",
    "rank_normalize", "rank_max_pooled",
    "psis_loo", "psis_max_draws",
    "mixture_calibration", "calib_max_draws",
]

_SFX = {torch.float32: "f32", torch.float64: "f64"}


def _sfx(t):
    try:
        return _SFX[t.dtype]
    except KeyError:
        raise TypeError("pysgmcmc_amd kernels support float32/float64, got %s" % t.dtype)


def _ptr(t, like=None):
    """Raw device pointer of a flat contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise SgmcmcLibraryError(
            "pysgmcmc_amd: tensor lives on %s; the SG-MCMC update path runs only as HIP kernels on an "
            "AMD GPU (no CPU fallback)." % t.device)
    if not t.is_contiguous():
        raise ValueError("pysgmcmc_amd: kernel arguments must be contiguous")
    if like is not None:
        if t.dtype != like.dtype:
            raise TypeError("pysgmcmc_amd: dtype mismatch %s vs %s" % (t.dtype, like.dtype))
        if t.numel() != like.numel():
            raise ValueError("pysgmcmc_amd: length mismatch %d vs %d" % (t.numel(), like.numel()))
        if t.device != like.device:
            raise ValueError("pysgmcmc_amd: device mismatch %s vs %s" % (t.device, like.device))
    return t.data_ptr()


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _ctr(step_dev):
    """Device step counter (int64 tensor with one element) -> pointer, or NULL."""
    if step_dev is None:
        return None
    if step_dev.dtype != torch.int64 or step_dev.numel() != 1:
        raise TypeError("step_dev must be a one-element int64 device tensor")
    return _ptr(step_dev)


class StepStats(object):
    """Device buffers for the statistics a step kernel reduces on the fly:
    ``out`` = float64[4] {sum theta'^2, sum V'^2 (p'^2), sum minv, sum minv^2}."""

    def __init__(self, n, device):
        self.out = torch.zeros(4, dtype=torch.float64, device=device)
        self.workspace = torch.empty(max(lib().sgmcmc_step_stats_workspace_bytes(int(n)), 32),
                                     dtype=torch.uint8, device=device)


def _stats(stats):
    return (None,) if stats is None else (_ptr(stats.workspace),)


def step_stats_finish(stats):
    """K7: reduce the per-block partials the last step kernel left in ``stats.workspace`` into ``stats.out``."""
    with _on(stats.out):
        rc = lib().sgmcmc_step_stats_finish(_ptr(stats.workspace), _ptr(stats.out), _stream(stats.out))
    check(rc, "sgmcmc_step_stats_finish")
    return stats.out


def counter_add(counter, inc=1):
    """counter += inc on the current stream (graph-capturable)."""
    with _on(counter):
        rc = lib().sgmcmc_counter_add_u64(_ctr(counter), int(inc), _stream(counter))
    check(rc, "sgmcmc_counter_add_u64")


def _on(t):
    """Device guard for the launch; refuses CPU tensors (there is no CPU update path)."""
    _ptr(t)
    return torch.cuda.device(t.device)


class LaunchConfig(object):
    """Launch geometry of the streaming kernels (``sgmcmc_launch_t``; performance only, results never depend
    on it). Pass one as ``launch=`` to a kernel call, or hang it on a sampler (``sampler.launch``). ``None``
    everywhere = the library's measured defaults. There is no process-wide setting in the C ABI; the
    module-level default below exists for the sweep tools and is plain Python state of the caller."""

    __slots__ = ("_c", "events")

    def __init__(self, block_threads=0, quads_per_thread=0, max_blocks=0, nontemporal=-1, events=None):
        from pysgmcmc_amd._lib import LaunchStruct
        # events: a KernelEvents pair that receives the kernel's own start/stop timestamps (hipExtLaunchKernel)
        self.events = events
        self._c = LaunchStruct(int(block_threads), int(quads_per_thread), int(max_blocks), int(nontemporal),
                               None if events is None else events.start, None if events is None else events.stop)

    def as_dict(self):
        c = self._c
        return {"block_threads": c.block_threads, "quads_per_thread": c.quads_per_thread,
                "max_blocks": c.max_blocks, "nontemporal": c.nontemporal}



class KernelEvents(object):
    """A pair of HIP events that a launch fills with the KERNEL's own start and stop timestamps (the duration
    rocprofv3 reports for the kernel), via ``LaunchConfig(events=...)``. ``elapsed_us()`` after a synchronise."""

    def __init__(self, device=None):
        """``device``: the device whose launches the events will time (default: the current device)."""
        import ctypes
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
            check(lib().sgmcmc_event_create(ctypes.byref(a)), "sgmcmc_event_create")
            check(lib().sgmcmc_event_create(ctypes.byref(b)), "sgmcmc_event_create")
        self.start, self.stop = a.value, b.value

    def elapsed_us(self):
        import ctypes
        ms = ctypes.c_float()
        check(lib().sgmcmc_event_elapsed_ms(self.start, self.stop, ctypes.byref(ms)), "sgmcmc_event_elapsed_ms")
        return float(ms.value) * 1e3

    def us_until(self, later):
        """Microseconds from the end of this kernel to the end of the kernel ``later`` timed."""
        import ctypes
        ms = ctypes.c_float()
        check(lib().sgmcmc_event_elapsed_ms(self.stop, later.stop, ctypes.byref(ms)), "sgmcmc_event_elapsed_ms")
        return float(ms.value) * 1e3

    def synchronize(self):
        """Block the host until the kernel has finished."""
        check(lib().sgmcmc_event_synchronize(self.stop), "sgmcmc_event_synchronize")

    def __del__(self):
        try:
            lib().sgmcmc_event_destroy(self.start)
            lib().sgmcmc_event_destroy(self.stop)
        except Exception:                     # interpreter shutdown
            pass


_default_launch = None


def set_launch_config(block_threads=0, quads_per_thread=0, max_blocks=0, nontemporal=-1):
    """Python-side default ``LaunchConfig`` for calls that pass no ``launch=`` (sweep tools). Validated by the
    library at the next launch. ``set_launch_config()`` with no arguments restores the library defaults."""
    global _default_launch
    cfg = LaunchConfig(block_threads, quads_per_thread, max_blocks, nontemporal)
    _default_launch = None if cfg.as_dict() == LaunchConfig().as_dict() else cfg


def get_launch_config():
    """The effective defaults: the library's (block_threads -1 = auto, 1 quad per lane, uncapped grid,
    nontemporal 2 = auto) overlaid with the Python-side default."""
    out = {"block_threads": -1, "quads_per_thread": 1, "max_blocks": 1 << 20, "nontemporal": 2}
    if _default_launch is not None:
        d = _default_launch.as_dict()
        out.update({k: v for k, v in d.items() if v != (-1 if k == "nontemporal" else 0)})
    return out


def _launch(launch):
    import ctypes
    cfg = launch if launch is not None else _default_launch
    return None if cfg is None else ctypes.byref(cfg._c)


class StepOpts(object):
    """Optional extras of one step call (``sgmcmc_step_opts_t``; see ``include/sgmcmc_hip.h``):

    ``first_element``  this launch covers the slice of the chain's parameter vector that starts there (multiple of 4);
    ``stats_base`` / ``stats_total``  statistics record slot of block 0 / record count of the whole step;
    ``theta_sq_only``  reduce only sum theta'^2;  ``hbm_resident``  geometry hint for slices of a large arena;
    ``skip_minv_store``  burn-in step that does not write minv;
    ``moments`` = (mean, m2, count)  fold theta' into the Welford moments in the same pass (K4 fused);
    ``scalars_dev``  device block from :func:`step_scalars` that overrides the by-value scalars;
    ``gather`` = (X, y, start, x_out, y_out)  the NEXT step's minibatch window as a side job of the launch (what
    :func:`window_gather` does, without a launch of its own; see :func:`gather_fits_step_launch`)."""

    __slots__ = ("_c", "_keep")

    def __init__(self, first_element=0, stats_base=0, stats_total=0, theta_sq_only=False, hbm_resident=False,
                 skip_minv_store=False, moments=None, scalars_dev=None, gather=None, like=None):
        from pysgmcmc_amd import _lib
        flags = (_lib.STEP_HBM_RESIDENT if hbm_resident else 0) | (_lib.STEP_SKIP_MINV_STORE if skip_minv_store else 0)
        mean = m2 = None
        count = 0
        if moments is not None:
            mean, m2, count = moments
            if like is not None:
                for t in (mean, m2):
                    if t.dtype != like.dtype or t.numel() != like.numel() or t.device != like.device:
                        raise TypeError("pysgmcmc_amd: fused moments must match theta in dtype, length and device")
        if scalars_dev is not None and like is not None and (scalars_dev.dtype != like.dtype or scalars_dev.numel() < 5):
            raise TypeError("pysgmcmc_amd: scalars_dev must hold 5 elements of the step's dtype")
        gx = gy = gxo = gyo = None
        gstart = gbatch = gdim = gld = 0
        if gather is not None:
            gx, gy, gstart, gxo, gyo = gather
            if not gather_fits_step_launch(gx, gy, gstart, gxo, gyo) or (like is not None and (gx.dtype != like.dtype or gx.device != like.device)):
                raise ValueError("pysgmcmc_amd: this window cannot ride in a step launch (see kernels.gather_fits_step_launch)")
            gbatch, gdim, gld = int(gxo.shape[0]), int(gx.shape[1]), int(gxo.stride(0))
        self._keep = (mean, m2, scalars_dev, gx, gy, gxo, gyo)
        self._c = _lib.StepOptsStruct(int(first_element), int(stats_base), int(stats_total),
                                      _lib.STATS_THETA_SQ if theta_sq_only else 0, flags, _ptr(mean), _ptr(m2), int(count),
                                      _ptr(scalars_dev), *[None if t is None else t.data_ptr() for t in (gx, gy, gxo, gyo)],     # (x_out is a pitched view)
                                      int(gstart), gbatch, gdim, gld, 0)


def gather_fits_step_launch(X, y, start, x_out, y_out):
    """True when the window ``X[start:start + B]``, ``y[start:start + B]`` -> ``x_out [B, D]`` (row pitch ``x_out.stride(0)``),
    ``y_out [B]`` can be gathered as the side job of a step launch (``StepOpts(gather=...)``): one dtype and device, contiguous
    dataset, rows of a multiple of 16 bytes, 16-byte aligned source window and destination."""
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dim() == 2 and X.is_contiguous() and y.is_contiguous() and y.dim() == 1):
        return False
    if not (X.dtype == y.dtype == x_out.dtype == y_out.dtype and X.device == y.device == x_out.device == y_out.device):
        return False
    if X.dtype not in (torch.float32, torch.float64) or x_out.dim() != 2 or x_out.stride(1) != 1 or not y_out.is_contiguous():
        return False
    B, D, es = int(x_out.shape[0]), int(X.shape[1]), X.element_size()
    if x_out.shape[1] != D or y_out.numel() != B or B == 0 or start < 0 or start + B > X.shape[0] or y.numel() != X.shape[0]:
        return False
    return ((D * es) % 16 == 0 and (x_out.stride(0) * es) % 16 == 0 and (X.data_ptr() + start * D * es) % 16 == 0
            and x_out.data_ptr() % 16 == 0 and y_out.data_ptr() % 4 == 0)


def _opts(opts, like):
    import ctypes
    if opts is None:
        return None
    if not isinstance(opts, StepOpts):
        opts = StepOpts(like=like, **opts)
    return ctypes.byref(opts._c)


def step_stats_records(n, launch, dtype=torch.float32):
    """Number of blocks (= statistics records) a vector-path step launch of ``n`` elements of ``dtype`` uses under ``launch``
    (a :class:`LaunchConfig` with an explicit ``block_threads``). A float64 launch streams one quad per lane whatever
    ``quads_per_thread`` says, so its count differs from the float32 one there."""
    import ctypes
    if dtype not in _SFX:
        raise TypeError("pysgmcmc_amd kernels support float32/float64, got %s" % dtype)
    blocks = int(lib().sgmcmc_step_stats_records_sized(int(n), 4 if dtype == torch.float32 else 8, ctypes.byref(launch._c)))
    if blocks == 0:
        check(-1, "sgmcmc_step_stats_records")
    return blocks


def step_scalars(kind, out, *scalars):
    """Fill the device block ``out`` (>= 5 elements of the step's dtype) with the derived scalars of a step, for
    ``StepOpts(scalars_dev=out)``: kind "sghmc" (eps, scale_grad, mdecay), "sgld" (eps, A, scale_grad) or "rsghmc"
    (eps, mass, c, D, b_hat)."""
    f = getattr(lib(), "sgmcmc_%s_scalars_%s" % (kind, _sfx(out)))
    if out.numel() < 5:
        raise ValueError("pysgmcmc_amd: the scalars block needs 5 elements")
    with _on(out):
        rc = f(*[float(v) for v in scalars], _ptr(out), _stream(out))
    check(rc, "sgmcmc_%s_scalars" % kind)
    return out


def update_step(kind, rows, scalars, adapt=None, xi=None, seed=0, step=0, step_dev=None, stats=None, grad_decay=0.0, launch=None,
                opts=None):
    """``sgmcmc_<kind>_step_*``, one update launch in place: the state ``rows`` in the entry's order (theta first), its by-value
    ``scalars`` (eps first), the ``adapt`` flag of a burn-in kind (None: the kind has none), then what all kinds take."""
    theta = rows[0]
    f = getattr(lib(), "sgmcmc_%s_step_%s" % (kind, _sfx(theta)))
    with _on(theta):
        rc = f(*[_ptr(t, theta) for t in rows], theta.numel(), *[float(v) for v in scalars], float(grad_decay),
               *(() if adapt is None else (int(bool(adapt)),)), _ptr(xi, theta), int(seed), int(step), _ctr(step_dev),
               *_stats(stats), _opts(opts, theta), _launch(launch), _stream(theta))
    check(rc, "sgmcmc_%s_step" % kind)


def sghmc_step(theta, V, grad, tau, g, v_hat, minv, r, eps, scale_grad, mdecay, adapt, xi=None, seed=0, step=0, step_dev=None,
               stats=None, grad_decay=0.0, launch=None, opts=None):
    """K1, one fused SGHMC step in place (pysgmcmc/samplers/sghmc.py:165-251)."""
    update_step("sghmc", (theta, V, grad, tau, g, v_hat, minv, r), (eps, scale_grad, mdecay), adapt, xi, seed, step, step_dev,
                stats, grad_decay, launch, opts)


def sgld_step(theta, grad, tau, g, v_hat, minv, r, eps, A, scale_grad, adapt, xi=None, seed=0, step=0, step_dev=None,
              stats=None, grad_decay=0.0, launch=None, opts=None):
    """K2, one fused SGLD step in place (pysgmcmc/samplers/sgld.py:149-211)."""
    update_step("sgld", (theta, grad, tau, g, v_hat, minv, r), (eps, A, scale_grad), adapt, xi, seed, step, step_dev,
                stats, grad_decay, launch, opts)


def rsghmc_step(theta, p, grad_cost, eps, mass, c, D, b_hat, xi=None, seed=0, step=0, step_dev=None,
                stats=None, grad_decay=0.0, launch=None, opts=None):
    """K3, one fused relativistic SGHMC step (pysgmcmc/samplers/relativistic_sghmc.py:120-140)."""
    update_step("rsghmc", (theta, p, grad_cost), (eps, mass, c, D, b_hat), None, xi, seed, step, step_dev,
                stats, grad_decay, launch, opts)


def toy_chains(sampler, target, target_params, theta, mom, tau, g, v_hat, minv, scalars, seeds, first_step, n_steps,
               burn_in_steps, keep_every=1, kept=None):
    """``n_steps`` steps of ``theta.shape[0]`` independent chains on a built-in toy target in one launch
    (``sgmcmc_toy_chains_*``, see include/sgmcmc_hip.h). ``theta`` etc.: ``[n_chains, dim]`` device tensors;
    ``seeds``: int64 device tensor ``[n_chains]``; ``kept``: ``[ceil(n_steps / keep_every), n_chains, dim]`` or None."""
    import ctypes
    f = getattr(lib(), "sgmcmc_toy_chains_" + _sfx(theta))
    n_chains, dim = int(theta.shape[0]), int(theta.shape[1])
    tp = [float(v) for v in target_params]
    k = {0: len(tp) // 3, 2: len(tp) // 2}.get(int(target), 0)        # an unknown target is the library's to refuse
    if seeds.dtype != torch.int64 or seeds.numel() != n_chains:
        raise TypeError("seeds must be an int64 device tensor with one entry per chain")
    if int(keep_every) < 1:
        raise ValueError("keep_every must be >= 1")
    if int(n_steps) < 0 or int(first_step) < 0:
        raise ValueError("first_step and n_steps are unsigned step counts")
    n_kept = (int(n_steps) + int(keep_every) - 1) // int(keep_every)
    if kept is not None and (kept.numel() != n_kept * n_chains * dim or kept.dtype != theta.dtype):
        raise ValueError("kept must hold ceil(n_steps / keep_every) x n_chains x dim elements of theta's dtype")
    arr = (ctypes.c_double * max(len(tp), 1))(*tp)
    sc = (ctypes.c_double * 5)(*([float(v) for v in scalars] + [0.0] * (5 - len(scalars))))
    with _on(theta):
        rc = f(int(sampler), int(target), arr, k, _ptr(theta), _ptr(mom, theta), _ptr(tau, theta), _ptr(g, theta),
               _ptr(v_hat, theta), _ptr(minv, theta), n_chains, dim, sc, _ptr(seeds), int(first_step), int(n_steps),
               int(burn_in_steps), int(keep_every), _ptr(kept), _stream(theta))
    check(rc, "sgmcmc_toy_chains")
    return kept


def philox_normal(out, seed, step, step_dev=None, launch=None):
    """K5, out[i] = xi(seed, step, i)."""
    f = getattr(lib(), "sgmcmc_philox_normal_" + _sfx(out))
    with _on(out):
        rc = f(_ptr(out), out.numel(), int(seed), int(step), _ctr(step_dev), _launch(launch), _stream(out))
    check(rc, "sgmcmc_philox_normal")
    return out


def philox_bits(out, seed, step, step_dev=None):
    if out.dtype not in (torch.int32, torch.uint32):
        raise TypeError("philox_bits wants a 32-bit integer tensor")
    with _on(out):
        rc = lib().sgmcmc_philox_bits_u32(_ptr(out), out.numel(), int(seed), int(step), _ctr(step_dev), _stream(out))
    check(rc, "sgmcmc_philox_bits_u32")
    return out


def moments_update(theta, mean, m2, count, launch=None):
    """K4, Welford update of (mean, m2) with the sample theta; count includes it."""
    f = getattr(lib(), "sgmcmc_moments_update_" + _sfx(theta))
    with _on(theta):
        rc = f(_ptr(theta), _ptr(mean, theta), _ptr(m2, theta), theta.numel(), int(count), _launch(launch), _stream(theta))
    check(rc, "sgmcmc_moments_update")


def rhat_pack(mean, m2, count, out3, n_shards=1, shard_len=None):
    """This chain's contribution to the R-hat exchange: ``[mean | mean^2 | m2 / (count - 1)]``, either as one
    ``3 n`` buffer (``n_shards = 1``: all-reduce) or as ``n_shards`` chunks of ``[3][shard_len]`` (reduce-scatter:
    chunk ``s`` = the rows of parameters ``[s * shard_len, (s + 1) * shard_len)``, zero beyond ``n``)."""
    n = mean.numel()
    shard_len = n if shard_len is None else int(shard_len)
    if out3.numel() != 3 * int(n_shards) * shard_len:
        raise ValueError("out3 must hold 3 * n_shards * shard_len elements")
    if out3.dtype != mean.dtype or m2.dtype != mean.dtype:
        # the kernel is picked from mean.dtype: an f64 pack into an f32 buffer of equal length would write past its end
        raise TypeError("rhat_pack: mean, m2 and out3 must share a dtype (got %s, %s, %s)" % (mean.dtype, m2.dtype, out3.dtype))
    if out3.device != mean.device:
        raise ValueError("rhat_pack: out3 lives on %s, the moments on %s" % (out3.device, mean.device))
    f = getattr(lib(), "sgmcmc_rhat_pack_" + _sfx(mean))
    with _on(mean):
        rc = f(_ptr(mean), _ptr(m2, mean), n, int(count), int(n_shards), shard_len, _ptr(out3), _stream(mean))
    check(rc, "sgmcmc_rhat_pack")


def rhat_finish(sum3, n, m_chains, count, rhat, summary_out4=None, summary_workspace=None, ld=None):
    """R-hat of ``n`` parameters from the chain-summed rows ``sum3 = [S_mean | S_sq | S_var]`` (row pitch ``ld``,
    default ``n``). With ``summary_out4`` (float64[4] device tensor) and ``summary_workspace`` the K6 summary
    {sum, sum^2, min, max} of R-hat is left on the device (no host sync)."""
    f = getattr(lib(), "sgmcmc_rhat_finish_" + _sfx(sum3))
    if rhat.dtype != sum3.dtype:
        raise TypeError("rhat and sum3 must share a dtype")
    if summary_out4 is not None and summary_out4.dtype != torch.float64:
        raise TypeError("summary_out4 must be float64")
    ld = int(n if ld is None else ld)
    if sum3.numel() < 2 * ld + int(n) or rhat.numel() < int(n):
        raise ValueError("rhat_finish: buffers shorter than n / ld say")
    with _on(sum3):
        rc = f(_ptr(sum3), int(n), ld, int(m_chains), int(count), _ptr(rhat), _ptr(summary_out4), _ptr(summary_workspace),
               _stream(sum3))
    check(rc, "sgmcmc_rhat_finish")


_ESS_STAGING = {"auto": 0, "lds": 1, "global": 2}


def ess_variogram(chains, ess, raw=None, stop_lag=None, ld=None, staging="auto", launch=None):
    """K10 (``include/sgmcmc_hip_diag.h``): effective sample size of every parameter from the traces of ``m`` chains.

    ``chains``: one ``(m, n, P)`` device tensor, one ``(n, P)`` tensor (a single chain), or a sequence of ``m``
    ``(n, P)`` tensors that live in buffers of their own. Rows must be dense (stride 1 along P) and all chains share
    the row pitch ``ld`` (default: the tensors' own row stride), so views of wider buffers pass without a copy.
    ``ess``: int64[P]; ``raw``: float64[P] or None; ``stop_lag``: int32[P] or None. ``staging``: ``"auto"``,
    ``"lds"`` or ``"global"`` (where the slab lives while the lags are walked; same bits). ``launch``: a
    ``LaunchConfig`` (``block_threads`` = parameters per workgroup, and the timestamp events)."""
    import ctypes
    if torch.is_tensor(chains):
        if chains.dim() == 2:
            mats = [chains]
        elif chains.dim() == 3:
            mats = list(chains.unbind(0))
        else:
            raise ValueError("ess_variogram: chains must be (n, P), (m, n, P) or a sequence of (n, P) tensors")
    else:
        mats = list(chains)
    if not mats:
        raise ValueError("ess_variogram: no chains")
    first = mats[0]
    for x in mats:
        if not x.is_cuda:
            raise SgmcmcLibraryError("pysgmcmc_amd: trace lives on %s; the effective sample size of all parameters runs "
                                     "only as a HIP kernel on an AMD GPU (no CPU fallback)." % x.device)
        if x.dim() != 2 or x.shape != first.shape:
            raise ValueError("ess_variogram: every chain must be an (n, P) matrix of the same shape")
        if x.dtype != first.dtype or x.device != first.device:
            raise TypeError("ess_variogram: the chains must share a dtype and a device")
    f = getattr(lib(), "sgmcmc_ess_variogram_" + _sfx(first))
    n, P = int(first.shape[0]), int(first.shape[1])
    if ld is None:
        ld = int(first.stride(0)) if n > 1 else P
    ld = int(ld)
    for x in mats:
        if (P > 1 and x.stride(1) != 1) or (n > 1 and x.stride(0) != ld):
            raise ValueError("ess_variogram: rows must be dense and %d elements apart in every chain" % ld)
    for out, dt, name in ((ess, torch.int64, "ess"), (raw, torch.float64, "raw"), (stop_lag, torch.int32, "stop_lag")):
        if out is None:
            if name == "ess":
                raise ValueError("ess_variogram: ess is required")
            continue
        if out.dtype != dt:
            raise TypeError("ess_variogram: %s must be %s" % (name, dt))
        if out.numel() != P or out.device != first.device:
            raise ValueError("ess_variogram: %s must hold P = %d elements on %s" % (name, P, first.device))
    try:
        stage = _ESS_STAGING[staging]
    except KeyError:
        raise ValueError("ess_variogram: staging must be 'auto', 'lds' or 'global'")
    table = (ctypes.c_void_p * len(mats))(*[x.data_ptr() for x in mats])
    with torch.cuda.device(first.device):
        rc = f(table, len(mats), n, P, ld, _ptr(ess), _ptr(raw), _ptr(stop_lag), stage, _launch(launch), _stream(first))
    check(rc, "sgmcmc_ess_variogram")
    return ess


def chain_diag(trace, rhat=None, ess=None, raw=None, stop_lag=None, waves=None):
    """K12 (``include/sgmcmc_hip_chains.h``): R-hat and the effective sample size of every parameter from ONE strided
    trace of up to 4096 chains, in one launch.

    ``trace``: an ``(m, n, P)`` device tensor, or ``(n, P)`` for a single chain. Rows must be dense (stride 1 along P);
    ``ld = stride(1)`` and ``chain_stride = stride(0)``, so views of wider or longer buffers pass without a copy.
    ``rhat``: float64[P] or None; ``ess``: int64[P] or None; ``raw``: float64[P] or None; ``stop_lag``: int32[P] or None;
    at least one of the four. With ``ess``, ``raw`` and ``stop_lag`` all None the launch takes the moments only (R-hat).
    ``waves``: None (auto) or 1, 2, 4, 8, 16, the waves of a workgroup that share a parameter's chains (same bits).
    Returns ``(rhat, ess, raw, stop_lag)`` as passed."""
    if not torch.is_tensor(trace):
        raise TypeError("chain_diag: trace must be an (m, n, P) or (n, P) device tensor")
    if trace.dim() == 2:
        trace = trace.unsqueeze(0)
    if trace.dim() != 3:
        raise ValueError("chain_diag: trace must be (m, n, P) or (n, P), got %s" % (tuple(trace.shape),))
    if not trace.is_cuda:
        raise SgmcmcLibraryError("pysgmcmc_amd: trace lives on %s; the chain diagnostics of all parameters run only as a "
                                 "HIP kernel on an AMD GPU (no CPU fallback)." % trace.device)
    f = getattr(lib(), "sgmcmc_chain_diag_" + _sfx(trace))
    m, n, P = (int(v) for v in trace.shape)
    if P > 1 and trace.stride(2) != 1:
        raise ValueError("chain_diag: rows must be dense (stride 1 along the parameters)")
    ld = int(trace.stride(1)) if n > 1 else P
    chain_stride = int(trace.stride(0)) if m > 1 else max((n - 1) * ld + P, 0)
    if ld < 0 or chain_stride < 0:
        raise ValueError("chain_diag: negative strides are not supported")
    outs = ((rhat, torch.float64, "rhat"), (ess, torch.int64, "ess"), (raw, torch.float64, "raw"),
            (stop_lag, torch.int32, "stop_lag"))
    if all(out is None for out, _, _ in outs):
        raise ValueError("chain_diag: at least one of rhat, ess, raw and stop_lag is required")
    for out, dt, name in outs:
        if out is None:
            continue
        if out.dtype != dt:
            raise TypeError("chain_diag: %s must be %s" % (name, dt))
        if out.numel() != P or out.device != trace.device:
            raise ValueError("chain_diag: %s must hold P = %d elements on %s" % (name, P, trace.device))
    with torch.cuda.device(trace.device):
        rc = f(trace.data_ptr(), m, n, P, ld, chain_stride, _ptr(rhat), _ptr(ess), _ptr(raw), _ptr(stop_lag),
               0 if waves is None else int(waves), _stream(trace))
    check(rc, "sgmcmc_chain_diag")
    return rhat, ess, raw, stop_lag


def _bnn_n_params(sizes):
    return sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1


def _bnn_row_tile(entry, layer_sizes, dtype):
    import ctypes
    sizes = [int(v) for v in layer_sizes]
    esize = {torch.float32: 4, torch.float64: 8}[dtype]
    tile = getattr(lib(), entry)((ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, esize)
    if tile < 1:
        check(tile, entry)
    return tile


def bnn_predict_row_tile(layer_sizes, dtype=torch.float32):
    """Test rows per tile of ``bnn_predict``'s forward launch for this net and dtype (``sgmcmc_bnn_predict_row_tile``:
    host arithmetic, nothing launched). Performance only; the results do not depend on it."""
    return _bnn_row_tile("sgmcmc_bnn_predict_row_tile", layer_sizes, dtype)


def _bnn_trace_arguments(what, noun, chains, layer_sizes, X):
    """The chain handling ``bnn_predict`` and ``bnn_score`` share: ``(f, mats, sizes, n, ld)`` -- the entry
    ``sgmcmc_<what>_<dtype>``, the chain matrices that go into its pointer table (a 3-D tensor whose chains lie back to back
    is ONE matrix), the layer sizes, the rows per matrix and their pitch -- after the checks of the chains and of ``X``."""
    if torch.is_tensor(chains):
        if chains.dim() == 2:
            mats = [chains]
        elif chains.dim() == 3:
            m3, n3, P3 = (int(v) for v in chains.shape)
            if m3 >= 1 and n3 >= 1 and (m3 == 1 or chains.stride(0) == n3 * chains.stride(1)):
                # the chains lie back to back at one row pitch: one matrix of m * n rows, no pointer table
                mats = [chains.as_strided((m3 * n3, P3), (chains.stride(1), chains.stride(2)), chains.storage_offset())]
            else:
                mats = list(chains.unbind(0))
        else:
            raise ValueError(what + ": chains must be (n, P), (m, n, P) or a sequence of (n, P) tensors")
    else:
        mats = list(chains)
    if not mats:
        raise ValueError(what + ": no chains")
    first = mats[0]
    for x in mats:
        if not x.is_cuda:
            raise SgmcmcLibraryError("pysgmcmc_amd: trace lives on %s; %s runs "
                                     "only as a HIP kernel on an AMD GPU (no CPU fallback)." % (x.device, noun))
        if x.dim() != 2 or x.shape != first.shape:
            raise ValueError(what + ": every chain must be an (n, P) matrix of the same shape")
        if x.dtype != first.dtype or x.device != first.device:
            raise TypeError(what + ": the chains must share a dtype and a device")
    f = getattr(lib(), "sgmcmc_" + what + "_" + _sfx(first))
    sizes = [int(v) for v in layer_sizes]
    n, P = int(first.shape[0]), int(first.shape[1])
    if len(sizes) < 2 or P < _bnn_n_params(sizes):
        raise ValueError(what + ": the traces are %d wide, layer sizes %s need %d parameters" % (
            P, sizes, _bnn_n_params(sizes) if len(sizes) >= 2 else -1))
    ld = int(first.stride(0)) if n > 1 else P
    for x in mats:
        if (P > 1 and x.stride(1) != 1) or (n > 1 and x.stride(0) != ld):
            raise ValueError(what + ": rows must be dense and %d elements apart in every chain" % ld)
    if not torch.is_tensor(X) or X.dtype != first.dtype or X.device != first.device:
        raise TypeError(what + ": X must be a %s tensor on %s" % (first.dtype, first.device))
    if X.dim() != 2 or int(X.shape[1]) != sizes[0] or not X.is_contiguous():
        raise ValueError(what + ": X must be a contiguous (N, %d) matrix, got %s" % (sizes[0], tuple(X.shape)))
    return f, mats, sizes, n, ld


def _bnn_check_outputs(what, device, outputs):
    """``outputs``: ``(tensor, dtype, numel, name, required)`` each; a tensor that is given must be one of that dtype holding
    ``numel`` elements on ``device``."""
    for out, dt, numel, name, required in outputs:
        if out is None:
            if required:
                raise ValueError("%s: %s is required" % (what, name))
            continue
        if not torch.is_tensor(out) or out.dtype != dt:
            raise TypeError("%s: %s must be a %s tensor" % (what, name, dt))
        if out.numel() != numel or out.device != device:
            raise ValueError("%s: %s must hold %d elements on %s" % (what, name, numel, device))


def bnn_predict(chains, layer_sizes, X, means, noise_var=None, ens_mean=None, ens_var=None):
    """K11 (``include/sgmcmc_hip_predict.h``): the outputs of ``S`` sampled networks of a small tanh-MLP BNN at the rows
    of ``X``, read from device traces, and their ensemble moments, in one call without host synchronisation.

    ``chains``: one ``(m, n, P)`` device tensor, one ``(n, P)`` tensor, or a sequence of ``m <= 64`` ``(n, P)`` tensors
    that live in buffers of their own; sample ``s = c * n + i`` is row ``i`` of chain ``c``, a flat parameter vector in
    the whole-step kernel's order (``P >= n_params``; what lies behind ``n_params`` is not read). Rows must be dense and
    all chains share one row pitch, as for ``ess_variogram``; a 3-D tensor whose chains lie back to back goes down as ONE
    matrix of ``m * n`` rows, so it may hold more than 64 chains. ``X``: ``(N, layer_sizes[0])``, contiguous, the chains'
    dtype. ``means``: ``(S, N)`` of that dtype, required (also the reduction's only scratch). ``noise_var``: ``(S,)`` of
    that dtype or None. ``ens_mean``, ``ens_var``: float64 ``(N,)``, both or neither. Returns ``means``."""
    import ctypes
    f, mats, sizes, n, ld = _bnn_trace_arguments("bnn_predict", "the posterior predictive of device traces", chains,
                                                 layer_sizes, X)
    first = mats[0]
    S, N = len(mats) * n, int(X.shape[0])
    for out, dt, numel, name in ((means, first.dtype, S * N, "means"), (noise_var, first.dtype, S, "noise_var"),
                                 (ens_mean, torch.float64, N, "ens_mean"), (ens_var, torch.float64, N, "ens_var")):
        if out is None:
            if name == "means":
                raise ValueError("bnn_predict: means is required")
            continue
        if out.dtype != dt:
            raise TypeError("bnn_predict: %s must be %s" % (name, dt))
        if out.numel() != numel or out.device != first.device:
            raise ValueError("bnn_predict: %s must hold %d elements on %s" % (name, numel, first.device))
    if (ens_mean is None) != (ens_var is None):
        raise ValueError("bnn_predict: ens_mean and ens_var go together")
    table = (ctypes.c_void_p * len(mats))(*[x.data_ptr() for x in mats])
    with torch.cuda.device(first.device):
        rc = f(table, len(mats), n, ld, (ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, _ptr(X), N, _ptr(means),
               _ptr(noise_var), _ptr(ens_mean), _ptr(ens_var), _stream(first))
    check(rc, "sgmcmc_bnn_predict")
    return means


def bnn_score(chains, layer_sizes, X, y, means, row_lppd, row_pwaic, ens_mean, ens_var, loglik=None, sample_loglik=None,
              summary=None):
    """K13 (``include/sgmcmc_hip_score.h``): the held-out score of ``S`` sampled networks of a small tanh-MLP BNN at the
    rows of ``X`` against the targets ``y``, read from device traces, in one call without host synchronisation.

    ``chains``, ``layer_sizes``, ``X``: as for :func:`bnn_predict`. ``y``: ``(N,)`` of the chains' dtype, in the units the
    networks work in. ``means``: ``(S, N)`` of that dtype, required: K11's output, the reductions' input. ``row_lppd``,
    ``row_pwaic``, ``ens_mean``, ``ens_var``: float64 ``(N,)``, required: per row the log pointwise predictive density, the
    sample variance over the networks of the pointwise log density, and K11's ensemble moments. Optional, float64:
    ``loglik`` ``(S, N)``, the pointwise log densities; ``sample_loglik`` ``(S,)``, their sums over the rows; ``summary``
    ``(3,)``: ``sum(row_lppd)``, ``sum(row_pwaic)``, ``sum((ens_mean - y)^2)``. Returns ``row_lppd``."""
    import ctypes
    f, mats, sizes, n, ld = _bnn_trace_arguments("bnn_score", "the held-out score of device traces", chains, layer_sizes, X)
    first = mats[0]
    S, N = len(mats) * n, int(X.shape[0])
    f64 = torch.float64
    _bnn_check_outputs("bnn_score", first.device, (
        (y, first.dtype, N, "y", True), (means, first.dtype, S * N, "means", True), (row_lppd, f64, N, "row_lppd", True),
        (row_pwaic, f64, N, "row_pwaic", True), (ens_mean, f64, N, "ens_mean", True), (ens_var, f64, N, "ens_var", True),
        (loglik, f64, S * N, "loglik", False), (sample_loglik, f64, S, "sample_loglik", False),
        (summary, f64, 3, "summary", False)))
    table = (ctypes.c_void_p * len(mats))(*[x.data_ptr() for x in mats])
    with torch.cuda.device(first.device):
        rc = f(table, len(mats), n, ld, (ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, _ptr(X), _ptr(y), N, _ptr(means),
               _ptr(row_lppd), _ptr(row_pwaic), _ptr(ens_mean), _ptr(ens_var), _ptr(loglik), _ptr(sample_loglik),
               _ptr(summary), _stream(first))
    check(rc, "sgmcmc_bnn_score")
    return row_lppd


def bnn_predict_grad_row_tile(sizes, dtype=torch.float32):
    """Test rows per tile of ``bnn_predict_grad``'s forward + backward launch for this net and dtype
    (``sgmcmc_bnn_predict_grad_row_tile``: host arithmetic, nothing launched). Performance only; the results do not depend
    on it."""
    return _bnn_row_tile("sgmcmc_bnn_predict_grad_row_tile", sizes, dtype)


def bnn_predict_grad(chains, layer_sizes, X, means, grads, ens_mean=None, ens_var=None, dmean=None, dvar=None):
    """K14 (``include/sgmcmc_hip_predict_grad.h``): the outputs of ``S`` sampled networks of a small tanh-MLP BNN at the
    rows of ``X`` AND their gradients with respect to those rows, read from device traces, with the input gradients of the
    ensemble mean and variance, in one call without host synchronisation.

    ``chains``, ``layer_sizes``, ``X``: as for :func:`bnn_predict`; ``D0 = layer_sizes[0]``. ``means``: ``(S, N)`` of the
    chains' dtype, required: K11's bits. ``grads``: ``(S, N, D0)`` of that dtype, required: ``grads[s, r, d]`` is the
    derivative of ``means[s, r]`` with respect to ``X[r, d]``. ``ens_mean``, ``ens_var``: float64 ``(N,)``; ``dmean``,
    ``dvar``: float64 ``(N, D0)``, the derivatives of ``ens_mean[r]`` and ``ens_var[r]`` with respect to ``X[r, d]``: all
    four or none. Returns ``grads``."""
    import ctypes
    f, mats, sizes, n, ld = _bnn_trace_arguments("bnn_predict_grad", "the predictive gradients of device traces", chains,
                                                 layer_sizes, X)
    first = mats[0]
    S, N, D0 = len(mats) * n, int(X.shape[0]), sizes[0]
    f64 = torch.float64
    _bnn_check_outputs("bnn_predict_grad", first.device, (
        (means, first.dtype, S * N, "means", True), (grads, first.dtype, S * N * D0, "grads", True),
        (ens_mean, f64, N, "ens_mean", False), (ens_var, f64, N, "ens_var", False),
        (dmean, f64, N * D0, "dmean", False), (dvar, f64, N * D0, "dvar", False)))
    if len({out is None for out in (ens_mean, ens_var, dmean, dvar)}) != 1:
        raise ValueError("bnn_predict_grad: ens_mean, ens_var, dmean and dvar go together")
    table = (ctypes.c_void_p * len(mats))(*[x.data_ptr() for x in mats])
    with torch.cuda.device(first.device):
        rc = f(table, len(mats), n, ld, (ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, _ptr(X), N, _ptr(means),
               _ptr(grads), _ptr(ens_mean), _ptr(ens_var), _ptr(dmean), _ptr(dvar), _stream(first))
    check(rc, "sgmcmc_bnn_predict_grad")
    return grads


def bnn_particles_lds_bytes(layer_sizes, batch, dtype=torch.float32):
    """Dynamic LDS of one workgroup of ``bnn_particles_cost_grad`` for this net, minibatch and dtype, in bytes
    (``sgmcmc_bnn_particles_lds_bytes``: the whole-step kernel's footprint rule; host arithmetic, nothing launched), or 0
    when the kernel does not take the call: the footprint exceeds 160 KiB, or the net is none it runs."""
    import ctypes
    sizes = [int(v) for v in layer_sizes]
    esize = {torch.float32: 4, torch.float64: 8}[dtype]
    if len(sizes) < 2:
        return 0
    return int(lib().sgmcmc_bnn_particles_lds_bytes((ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, int(batch), esize))


def bnn_particles_cost_grad(theta, n, ld, layer_sizes, Xb, yb, grad, ld_grad, costs, batch_size, n_examples, wdecay,
                            prior_mean, prior_var, add_prior=True):
    """K15 (``include/sgmcmc_hip_particles.h``): the cost of each of ``n`` particles of a small tanh-MLP BNN on one
    minibatch and its gradient with respect to the particle's parameters, in one launch without host synchronisation.

    ``theta``: flat device tensor, particle ``p`` the ``n_params`` elements from ``p * ld`` on, in the whole-step kernel's
    parameter order, at any alignment. ``Xb``: ``(B, layer_sizes[0])`` of that dtype with dense rows, possibly a pitched
    view (``ldx = Xb.stride(0)``); ``yb``: its ``B`` targets, contiguous. ``grad``: flat, row ``p`` written from
    ``p * ld_grad`` on, nothing behind ``n_params``; ``costs``: ``n`` elements. ``add_prior=False`` leaves the weight-prior
    term ``coef * theta`` out, which gives the gradient row of the whole-step kernel. Returns ``costs``."""
    import ctypes
    sizes = [int(v) for v in layer_sizes]
    what = "bnn_particles_cost_grad"
    if len(sizes) < 2:
        raise ValueError(what + ": layer_sizes needs at least two entries")
    n, ld, ld_grad, n_params = int(n), int(ld), int(ld_grad), _bnn_n_params(sizes)
    f = getattr(lib(), "sgmcmc_bnn_particles_cost_grad_" + _sfx(theta))
    for t, name in ((Xb, "Xb"), (yb, "yb"), (grad, "grad"), (costs, "costs")):
        if not torch.is_tensor(t) or t.dtype != theta.dtype or t.device != theta.device:
            raise TypeError("%s: %s must be a %s tensor on %s" % (what, name, theta.dtype, theta.device))
    if Xb.dim() != 2 or int(Xb.shape[1]) != sizes[0] or (sizes[0] > 1 and Xb.stride(1) != 1):
        raise ValueError("%s: Xb must be a (B, %d) matrix with dense rows, got %s" % (what, sizes[0], tuple(Xb.shape)))
    B = int(Xb.shape[0])
    ldx = int(Xb.stride(0)) if B > 1 else max(int(Xb.stride(0)), sizes[0])
    if yb.numel() != B:
        raise ValueError("%s: yb must hold the %d targets of Xb" % (what, B))
    if n > 0 and (theta.numel() < (n - 1) * ld + n_params or grad.numel() < (n - 1) * ld_grad + n_params
                  or costs.numel() < n or min(ld, ld_grad) < n_params):
        raise ValueError("%s: theta, grad or costs is too short for %d particles of %d parameters at pitches %d and %d"
                         % (what, n, n_params, ld, ld_grad))
    with _on(theta):
        rc = f(_ptr(theta), n, ld, (ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, Xb.data_ptr(), ldx, _ptr(yb), B,
               float(batch_size), float(n_examples), float(wdecay), float(prior_mean), float(prior_var), int(bool(add_prior)),
               _ptr(grad), ld_grad, _ptr(costs), _stream(theta))
    check(rc, "sgmcmc_bnn_particles_cost_grad")
    return costs


def summary_workspace(device):
    return torch.empty(lib().sgmcmc_summary_workspace_bytes(), dtype=torch.uint8, device=device)


def summary(x, out4=None, workspace=None):
    """K6, deterministic {sum, sum of squares, min, max} of a flat array -> float64[4] device tensor."""
    f = getattr(lib(), "sgmcmc_summary_" + _sfx(x))
    if out4 is None:
        out4 = torch.empty(4, dtype=torch.float64, device=x.device)
    if workspace is None:
        workspace = torch.empty(lib().sgmcmc_summary_workspace_bytes(), dtype=torch.uint8, device=x.device)
    with _on(x):
        rc = f(_ptr(x), x.numel(), _ptr(out4), _ptr(workspace), _stream(x))
    check(rc, "sgmcmc_summary")
    return out4


def bnn_head(mean, y, log_var, theta_sumsq, batch_size, n_examples, n_params, wdecay, prior_mean, prior_var,
             delta, cost_out, grad_log_var_out, mse_out, fold_prior_grad=False, stats_workspace=None,
             last_bias=None, grad_last_bias_out=None, add_last_bias=False):
    """Loss head of the BNN cost path in one launch (see include/sgmcmc_hip.h). ``theta_sumsq`` is a
    float64 device scalar, or None when ``stats_workspace`` (a StepStats.workspace) is given."""
    f = getattr(lib(), "sgmcmc_bnn_head_" + _sfx(mean))
    if theta_sumsq is not None and theta_sumsq.dtype != torch.float64:
        raise TypeError("theta_sumsq must be a float64 device scalar")
    with _on(mean):
        rc = f(_ptr(mean), _ptr(y, mean), _ptr(log_var), _ptr(theta_sumsq), _ptr(stats_workspace), _ptr(last_bias),
               mean.numel(), float(batch_size), float(n_examples), float(n_params), float(wdecay), float(prior_mean),
               float(prior_var), int(bool(fold_prior_grad)) | (2 if add_last_bias else 0), _ptr(delta, mean), _ptr(cost_out),
               _ptr(grad_log_var_out), _ptr(grad_last_bias_out), _ptr(mse_out), _stream(mean))
    check(rc, "sgmcmc_bnn_head")


def tanh_backward(delta, h):
    """delta *= 1 - h^2 in place."""
    f = getattr(lib(), "sgmcmc_tanh_backward_" + _sfx(delta))
    with _on(delta):
        rc = f(_ptr(delta), _ptr(h, delta), delta.numel(), _stream(delta))
    check(rc, "sgmcmc_tanh_backward")


def tanh_backward_colsum(delta, h, colsum, bias=None, beta=0.0):
    """delta *= 1 - h^2 in place on a row-major (rows, cols) matrix and colsum[c] = sum_r delta[r, c]
    (+ beta * bias[c]): tanh backward fused with the bias gradient of that layer."""
    f = getattr(lib(), "sgmcmc_tanh_backward_colsum_" + _sfx(delta))
    rows, cols = delta.shape
    with _on(delta):
        rc = f(_ptr(delta), _ptr(h, delta), rows, cols, _ptr(bias), float(beta), _ptr(colsum), _stream(delta))
    check(rc, "sgmcmc_tanh_backward_colsum")


def bnn_last_layer_backward(dvec, w, h, delta_prev, colsum, gw, bias_prev=None, beta=0.0):
    """Backward of a single-output last layer fused with the tanh backward of the layer below
    (see include/sgmcmc_hip.h): fills delta_prev (rows, cols), colsum (cols,), gw (cols,)."""
    f = getattr(lib(), "sgmcmc_bnn_last_layer_backward_" + _sfx(h))
    rows, cols = h.shape
    with _on(h):
        rc = f(_ptr(dvec), _ptr(w), _ptr(h), rows, cols, _ptr(bias_prev), float(beta), _ptr(delta_prev, h),
               _ptr(colsum), _ptr(gw), _stream(h))
    check(rc, "sgmcmc_bnn_last_layer_backward")


def step_scalars_table(kind, eps_list, *scalars, dtype, device):
    """Device table ``[len(eps_list), 5]`` of a whole-step launch's per-step scalars (``scalars_steps=``): row ``t`` is the
    block ``step_scalars`` makes for stepsize ``eps_list[t]``. ``scalars`` are the sampler's other scalars in the order of
    ``step_scalars``: kind "sghmc" (scale_grad, mdecay), "sgld" (A, scale_grad), "rsghmc" (mass, c, D, b_hat). The rows are
    derived on the host by the library (``sgmcmc_*_scalars_steps_*``, no launch); this does the one upload."""
    import ctypes
    import numpy as np
    npdt = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
    real = ctypes.c_float if dtype == torch.float32 else ctypes.c_double
    eps = np.ascontiguousarray(np.asarray(eps_list, dtype=npdt).reshape(-1))
    block = np.empty((eps.size, 5), dtype=npdt)
    f = getattr(lib(), "sgmcmc_%s_scalars_steps_%s" % (kind, _SFX[dtype]))
    rc = f(eps.ctypes.data_as(ctypes.POINTER(real)), eps.size, *[float(v) for v in scalars],
           block.ctypes.data_as(ctypes.POINTER(real)))
    check(rc, "sgmcmc_%s_scalars_steps" % kind)
    return torch.from_numpy(block).to(device)


# kind -> (where the C entry's scalars after eps stand in the sampler's ``scalars``; a burn-in sampler's entry, which has a
# ``burn_in_steps`` argument and a ``sched`` twin for a table, where the relativistic entry takes the table as an option)
_FUSED_KINDS = {"sghmc": ((1, 2), True), "sgld": ((2, 1), True), "rsghmc": ((1, 2, 3, 4), False)}
_FUSED_KIND_INDEX = {"sghmc": 0, "sgld": 1, "rsghmc": 2}      # `kind` of sgmcmc_bnn_fused_trace_steps_*


def bnn_fused_steps(kind, rows, layer_sizes, X, y, window_starts, batch, batch_size, n_examples, wdecay, prior_mean,
                    prior_var, scalars, first_step, n_steps, burn_in_steps, seed_base, cost_out, xi=None, n_chains=1,
                    chain_stride=None, scalars_steps=None, trace=None, trace_every=1, trace_row=0, trace_phase=0):
    """``n_steps`` complete steps of a small tanh-MLP BNN per chain in one launch, whichever the update: ``kind`` "sghmc",
    "sgld" or "rsghmc", ``rows`` the kind's state rows in the entry's order, ``scalars`` the sampler's scalars in the order
    of ``step_scalars`` (``eps`` first). ``scalars_steps`` (``step_scalars_table(kind, ...)``) replaces ``eps`` step by
    step; ``burn_in_steps`` is ignored for "rsghmc". The one caller of ``sgmcmc_bnn_fused_*_steps_*``.

    ``trace``: a contiguous device tensor ``(capacity, n_params)`` (one chain) or ``(n_chains, capacity, n_params)`` of
    the step's dtype. The launch then keeps theta after every ``trace_every``-th step in it, from row ``trace_row`` on
    (``sgmcmc_bnn_fused_trace_steps_*``, include/sgmcmc_hip_fused_trace.h): step ``t`` of the launch is kept iff
    ``(trace_phase + t + 1) % trace_every == 0``, where ``trace_phase < trace_every`` counts the steps taken since the
    last kept one. The chain and its costs are those of the untraced launch, bit for bit."""
    import ctypes
    if kind not in _FUSED_KINDS:
        raise ValueError("bnn_fused_steps: kind must be one of %s, not %r" % (", ".join(sorted(_FUSED_KINDS)), kind))
    order, burn_in = _FUSED_KINDS[kind]
    theta, sched = rows[0], burn_in and scalars_steps is not None
    if trace is not None:
        _fused_trace_check(trace, theta, layer_sizes, n_chains, trace_every, trace_row, trace_phase)
    name = "sgmcmc_bnn_fused_%s_%ssteps" % (kind, "sched_" if sched else "")
    f = getattr(lib(), "%s_%s" % (name, _sfx(theta)))
    sizes = [int(v) for v in layer_sizes]
    n_params = sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1
    if chain_stride is None:
        chain_stride = theta.numel() if n_chains == 1 else theta.numel() // n_chains
    if window_starts.dtype != torch.int32 or window_starts.numel() != n_chains * n_steps:
        raise TypeError("window_starts must be an int32 device tensor of n_chains * n_steps entries")
    if scalars_steps is not None and (scalars_steps.dtype != theta.dtype or scalars_steps.numel() != 5 * int(n_steps)):
        raise TypeError("scalars_steps must hold n_steps x 5 elements of the step's dtype (kernels.step_scalars_table)")
    other = [float(scalars[i]) for i in order]
    if trace is not None:
        return _bnn_fused_trace_steps(kind, rows, sizes, n_params, X, y, window_starts, batch, batch_size, n_examples, wdecay,
                                      prior_mean, prior_var, [float(scalars[0])] + other, first_step, n_steps, burn_in_steps,
                                      seed_base, cost_out, xi, n_chains, chain_stride, scalars_steps, trace, trace_every,
                                      trace_row, trace_phase)
    by_value = [_ptr(scalars_steps)] + other if sched else [float(scalars[0])] + other
    with _on(theta):
        rc = f(*[_ptr(r) for r in rows], n_params, int(chain_stride), int(n_chains), (ctypes.c_int * len(sizes))(*sizes),
               len(sizes) - 1, _ptr(X), _ptr(y), int(X.shape[0]), _ptr(window_starts), int(batch), float(batch_size),
               float(n_examples), float(wdecay), float(prior_mean), float(prior_var), *by_value,
               *([] if burn_in else [_ptr(scalars_steps)]), int(first_step), int(n_steps),
               *([int(burn_in_steps)] if burn_in else []), int(seed_base), _ptr(xi), _ptr(cost_out), _stream(theta))
    check(rc, name)
    return cost_out


def _fused_trace_check(trace, theta, layer_sizes, n_chains, trace_every, trace_row, trace_phase):
    """The Python-side refusals of a traced ``bnn_fused_steps``, before the library is reached."""
    sizes = [int(v) for v in layer_sizes]
    n_params = sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1
    if not torch.is_tensor(trace) or trace.dtype != theta.dtype:
        raise TypeError("trace must be a device tensor of the step's dtype (%s)" % theta.dtype)
    if trace.device != theta.device:
        raise TypeError("trace lives on %s, the chain on %s" % (trace.device, theta.device))
    if not trace.is_contiguous() or not (
            (trace.dim() == 2 and n_chains == 1 and trace.shape[1] == n_params)
            or (trace.dim() == 3 and trace.shape[0] == n_chains and trace.shape[2] == n_params)):
        raise TypeError("trace must be a contiguous (capacity, %d) tensor for one chain or (%d, capacity, %d) for the "
                        "launch's chains, got %s" % (n_params, n_chains, n_params, tuple(trace.shape)))
    if int(trace_every) < 1 or not 0 <= int(trace_phase) < int(trace_every) or int(trace_row) < 0:
        raise ValueError("trace_every must be >= 1, 0 <= trace_phase < trace_every and trace_row >= 0")


def _bnn_fused_trace_steps(kind, rows, sizes, n_params, X, y, window_starts, batch, batch_size, n_examples, wdecay, prior_mean,
                           prior_var, entry_scalars, first_step, n_steps, burn_in_steps, seed_base, cost_out, xi, n_chains,
                           chain_stride, scalars_steps, trace, trace_every, trace_row, trace_phase):
    """The traced launch of ``bnn_fused_steps``; ``entry_scalars``: the kind's scalars in the order of its C entry."""
    import ctypes
    theta = rows[0]
    capacity = int(trace.shape[-2])
    real = ctypes.c_float if theta.dtype == torch.float32 else ctypes.c_double
    f = getattr(lib(), "sgmcmc_bnn_fused_trace_steps_" + _sfx(theta))
    with _on(theta):
        rc = f(_FUSED_KIND_INDEX[kind], (ctypes.c_void_p * len(rows))(*[_ptr(r) for r in rows]), len(rows), n_params,
               int(chain_stride), int(n_chains), (ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, _ptr(X), _ptr(y),
               int(X.shape[0]), _ptr(window_starts), int(batch), float(batch_size), float(n_examples), float(wdecay),
               float(prior_mean), float(prior_var), (real * len(entry_scalars))(*entry_scalars), len(entry_scalars),
               _ptr(scalars_steps), int(first_step), int(n_steps), int(burn_in_steps), int(seed_base), _ptr(xi),
               _ptr(cost_out), _ptr(trace), capacity * n_params, capacity, int(trace_row), int(trace_every),
               int(trace_phase), _stream(theta))
    check(rc, "sgmcmc_bnn_fused_trace_steps")
    return cost_out


def bnn_fused_sghmc_steps(theta, V, grad, tau, g, v_hat, minv, layer_sizes, X, y, window_starts, batch,
                          batch_size, n_examples, wdecay, prior_mean, prior_var, eps, scale_grad, mdecay,
                          first_step, n_steps, burn_in_steps, seed_base, cost_out, xi=None, n_chains=1,
                          chain_stride=None, scalars_steps=None):
    """``n_steps`` complete SGHMC steps of a small tanh-MLP BNN per chain in one launch (see
    include/sgmcmc_hip.h). Rows are ``(n_chains * chain_stride,)`` or, for one chain, ``(n_params,)``.
    ``scalars_steps`` (``step_scalars_table("sghmc", ...)``): a stepsize per step instead of ``eps``
    (``sgmcmc_bnn_fused_sghmc_sched_steps_*``, include/sgmcmc_hip_fused.h)."""
    return bnn_fused_steps("sghmc", (theta, V, grad, tau, g, v_hat, minv), layer_sizes, X, y, window_starts, batch,
                           batch_size, n_examples, wdecay, prior_mean, prior_var, (eps, scale_grad, mdecay), first_step,
                           n_steps, burn_in_steps, seed_base, cost_out, xi, n_chains, chain_stride, scalars_steps)


def bnn_fused_sgld_steps(theta, grad, tau, g, v_hat, minv, layer_sizes, X, y, window_starts, batch,
                         batch_size, n_examples, wdecay, prior_mean, prior_var, eps, scale_grad, A,
                         first_step, n_steps, burn_in_steps, seed_base, cost_out, xi=None, n_chains=1,
                         chain_stride=None, scalars_steps=None):
    """The fused small-model kernel with the preconditioned-SGLD update (``sgmcmc_bnn_fused_sgld_steps_*``;
    with ``scalars_steps`` from ``step_scalars_table("sgld", ...)``: ``sgmcmc_bnn_fused_sgld_sched_steps_*``)."""
    return bnn_fused_steps("sgld", (theta, grad, tau, g, v_hat, minv), layer_sizes, X, y, window_starts, batch,
                           batch_size, n_examples, wdecay, prior_mean, prior_var, (eps, A, scale_grad), first_step,
                           n_steps, burn_in_steps, seed_base, cost_out, xi, n_chains, chain_stride, scalars_steps)


def bnn_fused_rsghmc_steps(theta, p, grad, layer_sizes, X, y, window_starts, batch, batch_size, n_examples, wdecay,
                           prior_mean, prior_var, eps, mass, c, D, b_hat, first_step, n_steps, seed_base, cost_out,
                           xi=None, n_chains=1, chain_stride=None, scalars_steps=None):
    """The fused small-model kernel with the relativistic SGHMC update (``sgmcmc_bnn_fused_rsghmc_steps_*``,
    include/sgmcmc_hip_fused.h): rows ``theta, p, grad``, no burn-in switch. ``scalars_steps``
    (``step_scalars_table("rsghmc", ...)``) replaces the by-value stepsize step by step."""
    return bnn_fused_steps("rsghmc", (theta, p, grad), layer_sizes, X, y, window_starts, batch, batch_size, n_examples,
                           wdecay, prior_mean, prior_var, (eps, mass, c, D, b_hat), first_step, n_steps, 0, seed_base,
                           cost_out, xi, n_chains, chain_stride, scalars_steps)


def bias_tanh(a, bias):
    """``a = tanh(a + bias)`` in place (``a``: contiguous ``[rows, cols]``, ``bias``: ``[cols]``): a hidden layer's activation
    after a plain forward GEMM."""
    rows, cols = int(a.shape[0]), int(a.shape[1])
    if bias.numel() != cols or bias.dtype != a.dtype or not a.is_contiguous() or not bias.is_contiguous():
        raise ValueError("pysgmcmc_amd: bias_tanh shapes / dtypes do not match")
    with _on(a):
        rc = getattr(lib(), "sgmcmc_bias_tanh_" + _sfx(a))(_ptr(a), _ptr(bias), rows, cols, _stream(a))
    check(rc, "sgmcmc_bias_tanh")
    return a


def bnn_dense_tanh_fits(h, W, out):
    """Can :func:`bnn_dense_tanh` take this layer? f32 device tensors, batch a multiple of 32, fan-out a multiple of 64, fan-in a
    multiple of 16 and >= 64, 16-byte aligned rows. Any number of 32 x 64 output tiles: more than one per compute unit run in
    rounds, a thin last round as half tiles (``include/sgmcmc_hip.h``)."""
    if not (h.is_cuda and h.dtype == W.dtype == out.dtype == torch.float32 and h.dim() == W.dim() == out.dim() == 2):
        return False
    M, K, N = int(h.shape[0]), int(h.shape[1]), int(W.shape[1])
    if W.shape[0] != K or tuple(out.shape) != (M, N) or M % 32 or N % 64 or K % 16 or K < 64:
        return False
    for t in (h, W, out):
        if t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
            return False
    return True


def bnn_dense_tanh_dot_parts(M, N, device):
    """Rows of the ``dot_parts`` buffer :func:`bnn_dense_tanh` fills for an ``M x N`` layer on ``device`` (one per column tile:
    64 columns, or 32 where the launch uses half tiles)."""
    with torch.cuda.device(device):
        n = int(lib().sgmcmc_bnn_dense_tanh_dot_parts(int(M), int(N)))
    if n <= 0:
        raise ValueError("pysgmcmc_amd: bnn_dense_tanh_dot_parts: M %% 32 == 0 and N %% 64 == 0 required, got %d x %d" % (M, N))
    return n


def bnn_dense_tanh(h, W, bias, out, w_next=None, dot_parts=None, stats_workspace=None, tsq_parts=None):
    """``out = tanh(h @ W + bias)`` in ONE launch on the fp32 matrix cores (``sgmcmc_bnn_dense_tanh_f32``; shapes as
    :func:`bnn_dense_tanh_fits` demands). With ``w_next [N]`` and ``dot_parts [bnn_dense_tanh_dot_parts(M, N), M]`` the launch also
    leaves the per-column-tile partial dot products of ``out`` with ``w_next`` (the single output unit); with ``stats_workspace`` and
    ``tsq_parts`` it adds up the sum(theta^2) records like :func:`tanh_rowdot`."""
    M, K = int(h.shape[0]), int(h.shape[1])
    N = int(W.shape[1])
    if not bnn_dense_tanh_fits(h, W, out) or bias.numel() != N or bias.dtype != h.dtype:
        raise ValueError("pysgmcmc_amd: bnn_dense_tanh: shapes / dtypes / alignment do not fit the kernel (see bnn_dense_tanh_fits)")
    if dot_parts is not None and (w_next is None or w_next.numel() != N or not dot_parts.is_contiguous()
                                  or dot_parts.numel() != bnn_dense_tanh_dot_parts(M, N, h.device) * M):
        raise ValueError("pysgmcmc_amd: bnn_dense_tanh needs w_next [N] and dot_parts [bnn_dense_tanh_dot_parts(M, N), M]")
    if tsq_parts is not None and (tsq_parts.dtype != torch.float64 or tsq_parts.numel() < 16 or (M // 32) * (N // 64) < 16):
        raise ValueError("pysgmcmc_amd: bnn_dense_tanh: tsq_parts must be float64[16] and the launch needs >= 16 output tiles")
    with torch.cuda.device(h.device):                          # (h may be a pitched view: rows are what must be contiguous)
        rc = lib().sgmcmc_bnn_dense_tanh_f32(h.data_ptr(), W.data_ptr(), _ptr(bias), out.data_ptr(), M, N, K, h.stride(0),
                                             W.stride(0), out.stride(0), _ptr(w_next), _ptr(dot_parts), _ptr(stats_workspace),
                                             _ptr(tsq_parts), _stream(h))
    check(rc, "sgmcmc_bnn_dense_tanh_f32")
    return out


def bnn_dense_tanh_backward_fits(delta, W, act, out):
    """Can :func:`bnn_dense_tanh_backward` take this layer? ``delta [M, K]``, ``W [N, K]`` (the weights of the layer above, fan-in
    N), ``act`` / ``out [M, N]``: the limits of :func:`bnn_dense_tanh_fits` with the roles of W's two axes swapped."""
    if not (delta.is_cuda and delta.dtype == W.dtype == act.dtype == out.dtype == torch.float32
            and delta.dim() == W.dim() == act.dim() == out.dim() == 2):
        return False
    M, K, N = int(delta.shape[0]), int(delta.shape[1]), int(W.shape[0])
    if W.shape[1] != K or tuple(out.shape) != (M, N) or tuple(act.shape) != (M, N) or M % 32 or N % 64 or K % 16 or K < 64:
        return False
    for t in (delta, W, act, out):
        if t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
            return False
    return True


def bnn_dense_tanh_backward(delta, W, act, out, colsum_parts=None, finish=None):
    """``out = (delta @ W.T) * (1 - act ** 2)`` in ONE launch on the fp32 matrix cores (``sgmcmc_bnn_dense_tanh_backward_f32``):
    the backward step through a hidden tanh layer, d cost / d pre-activation of the layer below from the one above.
    ``colsum_parts [M // 32, N]`` (optional) receives the column sums of ``out`` per 32-row tile -- the bias gradient once its
    rows are added up, which the NEXT launch does on the side when handed ``finish = (parts, colsum, bias, beta)``
    (``colsum[:] = parts.sum(0) + beta * bias``, rows added in order), or :func:`colsum_finish`. Deterministic."""
    M, K = int(delta.shape[0]), int(delta.shape[1])
    N = int(W.shape[0])
    if not bnn_dense_tanh_backward_fits(delta, W, act, out):
        raise ValueError("pysgmcmc_amd: bnn_dense_tanh_backward: shapes / dtypes / alignment do not fit the kernel "
                         "(see bnn_dense_tanh_backward_fits)")
    if colsum_parts is not None and (colsum_parts.dtype != delta.dtype or colsum_parts.numel() != (M // 32) * N
                                     or not colsum_parts.is_contiguous() or colsum_parts.device != delta.device):
        raise ValueError("pysgmcmc_amd: bnn_dense_tanh_backward: colsum_parts must be a contiguous [M // 32, N] tensor")
    fin = _colsum_finish_args(finish, delta)
    if fin[0] is not None and colsum_parts is not None and fin[0] == colsum_parts.data_ptr():
        raise ValueError("pysgmcmc_amd: bnn_dense_tanh_backward: the finish job needs partial sums other than this launch's own")
    with torch.cuda.device(delta.device):
        rc = lib().sgmcmc_bnn_dense_tanh_backward_f32(
            delta.data_ptr(), W.data_ptr(), act.data_ptr(), out.data_ptr(), _ptr(colsum_parts), M, N, K, delta.stride(0),
            W.stride(0), act.stride(0), out.stride(0), *fin, _stream(delta))
    check(rc, "sgmcmc_bnn_dense_tanh_backward_f32")
    return out


def _colsum_finish_args(finish, like):
    """(parts ptr, rows, n, bias ptr, beta, colsum ptr) of a ``finish = (parts [rows, n], colsum [n], bias [n] | None, beta)`` job."""
    if finish is None:
        return (None, 0, 0, None, 0.0, None)
    parts, colsum, bias, beta = finish
    n = int(colsum.numel())
    if (parts.dim() != 2 or parts.shape[1] != n or not parts.is_contiguous() or not colsum.is_contiguous()
            or parts.dtype != like.dtype or colsum.dtype != like.dtype or parts.device != like.device or colsum.device != like.device
            or (beta != 0.0 and (bias is None or bias.numel() != n or bias.dtype != like.dtype or not bias.is_contiguous()))):
        raise ValueError("pysgmcmc_amd: column-sum finish job: parts [rows, n], colsum [n] (and bias [n] with beta != 0) of the launch's dtype / device")
    return (parts.data_ptr(), int(parts.shape[0]), n, bias.data_ptr() if beta != 0.0 else None, float(beta), colsum.data_ptr())


def colsum_finish(parts, colsum, bias=None, beta=0.0):
    """``colsum[:] = parts.sum(0) (+ beta * bias)``, the rows of ``parts`` added in order: the second half of
    :func:`bnn_dense_tanh_backward`'s bias gradient as a launch of its own (``sgmcmc_colsum_finish_f32``)."""
    if parts.dtype != torch.float32 or not parts.is_cuda:
        raise TypeError("pysgmcmc_amd: colsum_finish takes float32 device tensors")
    fin = _colsum_finish_args((parts, colsum, bias, beta), parts)
    with torch.cuda.device(parts.device):
        rc = lib().sgmcmc_colsum_finish_f32(*fin, _stream(parts))
    check(rc, "sgmcmc_colsum_finish_f32")
    return colsum


def bnn_planes_bytes(M, N):
    """Bytes of one set of three bf16 planes of an ``[M, N]`` float32 matrix (``sgmcmc_bnn_planes_bytes``; 0: invalid shape)."""
    return int(lib().sgmcmc_bnn_planes_bytes(int(M), int(N)))


def _stack_stride(ts):
    """Elements between consecutive tensors of ``ts`` (equal shapes, row-major with one row pitch, equally spaced), or raise."""
    t0 = ts[0]
    if any(t.shape != t0.shape or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1
           or t.stride(0) != t0.stride(0) for t in ts):
        raise ValueError("pysgmcmc_amd: a batch of equally shaped float32 [rows, cols] device matrices with one row pitch is expected")
    gaps = {ts[k + 1].data_ptr() - ts[k].data_ptr() for k in range(len(ts) - 1)}
    if len(gaps) > 1 or any(g <= 0 or g % 4 for g in gaps):
        raise ValueError("pysgmcmc_amd: the matrices of a batch must lie at one constant, positive stride")
    return gaps.pop() // 4 if gaps else 0


def bnn_split_planes(mats, planes):
    """Write every ``[M, N]`` float32 matrix of ``mats`` (equally spaced) as three exact bf16 planes into the uint8 buffer
    ``planes`` (``len(mats) * bnn_planes_bytes(M, N)`` bytes; layout: include/sgmcmc_hip.h) -- the operands of
    :func:`bnn_gw_planes`. One launch (``sgmcmc_bnn_split_planes_f32``)."""
    stride = _stack_stride(mats)
    M, N = int(mats[0].shape[0]), int(mats[0].shape[1])
    one = bnn_planes_bytes(M, N)
    if one == 0 or planes.dtype != torch.uint8 or not planes.is_cuda or planes.numel() < one * len(mats) or planes.data_ptr() % 16:
        raise ValueError("pysgmcmc_amd: bnn_split_planes needs M %% 16 == 0 and a 16-byte aligned uint8 device buffer of "
                         "len(mats) * bnn_planes_bytes(M, N) bytes")
    with torch.cuda.device(planes.device):
        rc = lib().sgmcmc_bnn_split_planes_f32(mats[0].data_ptr(), len(mats), stride, M, N, int(mats[0].stride(0)), planes.data_ptr(),
                                               one, _stream(planes))
    check(rc, "sgmcmc_bnn_split_planes_f32")
    return planes


def bnn_gw_planes(a_planes, b_planes, outs, M):
    """``outs[z][nA, nB] = A_z^T B_z`` for the plane sets written by :func:`bnn_split_planes` (``a_planes``: ``len(outs)`` sets of
    ``[M, nA]`` matrices, ``b_planes``: of ``[M, nB]``) -- the weight gradients ``h^T delta`` of equally shaped layers as ONE launch
    on the bf16 matrix pipe at fp32 accuracy (``sgmcmc_bnn_gw_planes_f32``). ``outs``: equally spaced float32 device views."""
    stride = _stack_stride(outs)
    nA, nB = int(outs[0].shape[0]), int(outs[0].shape[1])
    sa, sb = bnn_planes_bytes(M, nA), bnn_planes_bytes(M, nB)
    if (sa == 0 or a_planes.dtype != torch.uint8 or b_planes.dtype != torch.uint8 or a_planes.numel() < sa * len(outs)
            or b_planes.numel() < sb * len(outs) or a_planes.device != outs[0].device or b_planes.device != outs[0].device):
        raise ValueError("pysgmcmc_amd: bnn_gw_planes needs M %% 16 == 0 and plane buffers of len(outs) sets each on the outputs' device")
    with torch.cuda.device(outs[0].device):
        rc = lib().sgmcmc_bnn_gw_planes_f32(a_planes.data_ptr(), sa, b_planes.data_ptr(), sb, outs[0].data_ptr(), stride, len(outs),
                                            int(M), nA, nB, int(outs[0].stride(0)), _stream(outs[0]))
    check(rc, "sgmcmc_bnn_gw_planes_f32")
    return outs


def tanh_rowdot(a, w, out, stats_workspace=None, tsq_parts=None, bias=None):
    """``a = tanh(a [+ bias])`` in place (``[rows, cols]``) and ``out[r] = a[r] . w`` in one launch. With ``stats_workspace``
    (a ``StepStats.workspace``) and ``tsq_parts`` (float64[16] device tensor) the launch also adds up the
    sum(theta^2) partials into 16 slices for :func:`bnn_head_last_layer_backward`."""
    f = getattr(lib(), "sgmcmc_bias_tanh_rowdot_" + _sfx(a))
    rows, cols = int(a.shape[0]), int(a.shape[1])
    if w.numel() != cols or out.numel() != rows or (bias is not None and (bias.numel() != cols or bias.dtype != a.dtype)):
        raise ValueError("pysgmcmc_amd: tanh_rowdot shapes do not match")
    if tsq_parts is not None and (tsq_parts.dtype != torch.float64 or tsq_parts.numel() < 16):
        raise TypeError("tsq_parts must be a float64 device tensor of 16 elements")
    with _on(a):
        rc = f(_ptr(a), _ptr(bias), _ptr(w), rows, cols, _ptr(out), _ptr(stats_workspace), _ptr(tsq_parts), _stream(a))
    check(rc, "sgmcmc_tanh_rowdot")


def bnn_head_last_layer_backward(mean, y, log_var, tsq_parts, last_bias, batch_size, n_examples, n_params, wdecay,
                                 prior_mean, prior_var, w, h, bias_prev, beta, cost_out, grad_log_var_out,
                                 grad_last_bias_out, mse_out, delta_prev, colsum, gw, fold_prior_grad=False,
                                 add_last_bias=True):
    """Loss head + backward of the single-output last layer (+ tanh backward and bias gradient of the layer below) in
    ONE launch; see ``include/sgmcmc_hip.h``. ``mean`` = the pre-bias outputs of :func:`tanh_rowdot` (``[rows]``), or the
    per-column-tile partial dot products of :func:`bnn_dense_tanh` (``[n_parts, rows]``, added in the launch)."""
    f = getattr(lib(), "sgmcmc_bnn_head_last_layer_backward_" + _sfx(h))
    rows, cols = h.shape
    n_parts = mean.numel() // rows
    if (n_parts * rows != mean.numel() or y.numel() != rows or not mean.is_contiguous()
            or not (mean.dim() == 1 or (mean.dim() == 2 and mean.shape[1] == rows))):
        raise ValueError("pysgmcmc_amd: bnn_head_last_layer_backward: mean must be a contiguous [rows] or [n_parts, rows] tensor, y [rows]")
    if y.dtype != h.dtype or y.device != h.device or mean.dtype != h.dtype or mean.device != h.device:
        raise TypeError("pysgmcmc_amd: bnn_head_last_layer_backward: mean and y must have the dtype and device of h")
    with _on(h):
        rc = f(_ptr(mean), n_parts, _ptr(y), _ptr(log_var), _ptr(tsq_parts), _ptr(last_bias), rows, cols, float(batch_size),
               float(n_examples), float(n_params), float(wdecay), float(prior_mean), float(prior_var),
               int(bool(fold_prior_grad)) | (2 if add_last_bias else 0), _ptr(w), _ptr(h), _ptr(bias_prev), float(beta),
               _ptr(cost_out), _ptr(grad_log_var_out), _ptr(grad_last_bias_out), _ptr(mse_out), _ptr(delta_prev, h),
               _ptr(colsum), _ptr(gw), _stream(h))
    check(rc, "sgmcmc_bnn_head_last_layer_backward")


def window_gather(X, y, start, x_out, y_out):
    """``x_out[:] = X[start:start + B]``, ``y_out[:] = y[start:start + B]`` in one launch (B = rows of x_out; ``x_out`` may be a
    pitched view -- rows contiguous, any row stride)."""
    f = getattr(lib(), "sgmcmc_window_gather_" + _sfx(X))
    batch = int(x_out.shape[0])
    dim = int(X.numel() // X.shape[0])
    if x_out.numel() != batch * dim or y_out.numel() != batch or x_out.dim() != 2 or x_out.stride(1) != 1 or x_out.stride(0) < dim:
        raise ValueError("pysgmcmc_amd: window_gather output shapes do not match the window")
    if x_out.dtype != X.dtype or y_out.dtype != X.dtype or x_out.device != X.device or not y_out.is_contiguous():
        raise TypeError("pysgmcmc_amd: window_gather outputs must have the dataset's dtype and device")
    with torch.cuda.device(X.device):
        rc = f(_ptr(X), _ptr(y), int(X.shape[0]), int(start), batch, dim, x_out.data_ptr(), int(x_out.stride(0)), _ptr(y_out), _stream(X))
    check(rc, "sgmcmc_window_gather")


def svgd_max_particles():
    return int(lib().sgmcmc_svgd_max_particles())


def svgd_workspace(n_particles, like):
    """Device workspace of the SVGD kernels for ``n_particles`` particles in ``like``'s dtype/device."""
    nbytes = int(lib().sgmcmc_svgd_workspace_bytes(int(n_particles), like.element_size()))
    if nbytes == 0:
        raise ValueError("pysgmcmc_amd: SVGD supports 1..%d particles, got %d" % (svgd_max_particles(), n_particles))
    if not like.is_cuda:
        _ptr(like)                       # raises the no-CPU-path error
    return torch.empty(nbytes // like.element_size(), dtype=like.dtype, device=like.device)


def svgd_step(particles, grad, hist_grad, n_particles, dim, eps, alpha, fudge_factor, workspace, ld=None,
              repulsion_sign=1):
    """One SVGD step in place on the ``[n_particles x ld]`` matrices (``sgmcmc_svgd_step_*``)."""
    f = getattr(lib(), "sgmcmc_svgd_step_" + _sfx(particles))
    ld = int(dim if ld is None else ld)
    for t in (particles, grad, hist_grad):
        if t.numel() < (n_particles - 1) * ld + dim:
            raise ValueError("pysgmcmc_amd: SVGD matrix shorter than (n_particles - 1) * ld + dim")
    with _on(particles):
        rc = f(_ptr(particles), _ptr(grad), _ptr(hist_grad), int(n_particles), int(dim), ld, float(eps), float(alpha),
               float(fudge_factor), int(repulsion_sign), _ptr(workspace), _stream(particles))
    check(rc, "sgmcmc_svgd_step")


def svgd_kernel(particles, n_particles, dim, workspace, ld=None, kernel_gradients=True):
    """``svgd_kernel(particles)`` of the reference: returns (kernel_matrix [n, n], kernel_gradients [n, dim]
    or None, bandwidth tensor {median, h, h^2}) as fresh device tensors."""
    f = getattr(lib(), "sgmcmc_svgd_kernel_" + _sfx(particles))
    ld = int(dim if ld is None else ld)
    n = int(n_particles)
    K = torch.empty((n, n), dtype=particles.dtype, device=particles.device)
    kg = torch.empty((n, int(dim)), dtype=particles.dtype, device=particles.device) if kernel_gradients else None
    bw = torch.empty(3, dtype=particles.dtype, device=particles.device)
    with _on(particles):
        rc = f(_ptr(particles), n, int(dim), ld, _ptr(workspace), _ptr(K), _ptr(kg), int(dim), _ptr(bw),
               _stream(particles))
    check(rc, "sgmcmc_svgd_kernel")
    return K, kg, bw


# ---- SVGD with up to 1024 particles (include/sgmcmc_hip_svgd_many.h, csrc/sgmcmc_svgd_many.hip) ----
SvgdManyLaunch = collections.namedtuple("SvgdManyLaunch", "id tile grid cap")
SVGD_MANY_IDS = {1: "gram", 2: "reduce", 3: "dist", 4: "select", 5: "next", 6: "bandwidth", 7: "kmatrix", 8: "update",
                 9: "kgrad", 10: "copy", 11: "mean"}


def svgd_many_max_particles():
    return int(lib().sgmcmc_svgd_many_max_particles())


def svgd_many_workspace(n_particles, like):
    """Device workspace of the many-particle SVGD kernels for ``n_particles`` particles in ``like``'s dtype/device."""
    nbytes = int(lib().sgmcmc_svgd_many_workspace_bytes(int(n_particles), like.element_size()))
    if nbytes == 0:
        raise ValueError("pysgmcmc_amd: the many-particle SVGD path supports 2..%d particles in float32/float64, got %d"
                         % (svgd_many_max_particles(), n_particles))
    if not like.is_cuda:
        _ptr(like)                       # raises the no-CPU-path error
    return torch.empty(nbytes // like.element_size(), dtype=like.dtype, device=like.device)


def svgd_many_plan(n_particles, dim, like):
    """The launches of one ``svgd_many_step`` call: a list of ``SvgdManyLaunch(id, tile, grid, cap)`` (host arithmetic;
    ``like`` is a tensor or a dtype and gives the element size)."""
    esize = like.element_size() if torch.is_tensor(like) else torch.empty((), dtype=like).element_size()
    k = int(lib().sgmcmc_svgd_many_plan(int(n_particles), int(dim), esize, None, 0))
    check(0 if k > 0 else k, "sgmcmc_svgd_many_plan")
    out = (ctypes.c_int * (4 * k))()
    lib().sgmcmc_svgd_many_plan(int(n_particles), int(dim), esize, out, 4 * k)
    return [SvgdManyLaunch(*out[4 * i:4 * i + 4]) for i in range(k)]


def svgd_many_step(particles, grad, hist_grad, n_particles, dim, eps, alpha, fudge_factor, workspace, ld=None,
                   repulsion_sign=1):
    """One SVGD step in place on the ``[n_particles x ld]`` matrices (``sgmcmc_svgd_many_step_*``, 2..1024 particles)."""
    f = getattr(lib(), "sgmcmc_svgd_many_step_" + _sfx(particles))
    ld = int(dim if ld is None else ld)
    for t in (particles, grad, hist_grad):
        if t.numel() < (n_particles - 1) * ld + dim:
            raise ValueError("pysgmcmc_amd: SVGD matrix shorter than (n_particles - 1) * ld + dim")
    with _on(particles):
        rc = f(_ptr(particles), _ptr(grad), _ptr(hist_grad), int(n_particles), int(dim), ld, float(eps), float(alpha),
               float(fudge_factor), int(repulsion_sign), _ptr(workspace), _stream(particles))
    check(rc, "sgmcmc_svgd_many_step")


def svgd_many_kernel(particles, n_particles, dim, workspace, ld=None, kernel_gradients=True):
    """``svgd_kernel`` for 2..1024 particles: (kernel_matrix [n, n], kernel_gradients [n, dim] or None, bandwidth tensor
    {median, h, h^2}) as fresh device tensors."""
    f = getattr(lib(), "sgmcmc_svgd_many_kernel_" + _sfx(particles))
    ld = int(dim if ld is None else ld)
    n = int(n_particles)
    if particles.numel() < (n - 1) * ld + dim:
        raise ValueError("pysgmcmc_amd: SVGD matrix shorter than (n_particles - 1) * ld + dim")
    K = torch.empty((n, n), dtype=particles.dtype, device=particles.device)
    kg = torch.empty((n, int(dim)), dtype=particles.dtype, device=particles.device) if kernel_gradients else None
    bw = torch.empty(3, dtype=particles.dtype, device=particles.device)
    with _on(particles):
        rc = f(_ptr(particles), n, int(dim), ld, _ptr(workspace), _ptr(K), _ptr(kg), int(dim), _ptr(bw),
               _stream(particles))
    check(rc, "sgmcmc_svgd_many_kernel")
    return K, kg, bw


# ---- K16: kernel Stein discrepancy of up to 4096 samples (include/sgmcmc_hip_ksd.h, csrc/sgmcmc_ksd.hip) ----
KsdLaunch = collections.namedtuple("KsdLaunch", "id tile grid cap")
KSD_IDS = {1: "mean", 2: "gram", 3: "reduce", 4: "pair", 5: "finish"}
KSD_KINDS = {"imq": 0, "rbf": 1}


def ksd_max_samples():
    return int(lib().sgmcmc_ksd_max_samples())


def ksd_workspace(n, like):
    """Device workspace of ``ksd`` for ``n`` samples in ``like``'s dtype/device; it does not depend on the width."""
    nbytes = int(lib().sgmcmc_ksd_workspace_bytes(int(n), like.element_size()))
    if nbytes == 0:
        raise ValueError("pysgmcmc_amd: the kernel Stein discrepancy supports 2..%d samples in float32/float64, got %d"
                         % (ksd_max_samples(), n))
    if not like.is_cuda:
        _ptr(like)                       # raises the no-CPU-path error
    return torch.empty(nbytes // like.element_size(), dtype=like.dtype, device=like.device)


def ksd_plan(n, dim, like):
    """The launches of one ``ksd`` call: a list of ``KsdLaunch(id, tile, grid, cap)`` (host arithmetic; ``like`` is a tensor
    or a dtype and gives the element size)."""
    esize = like.element_size() if torch.is_tensor(like) else torch.empty((), dtype=like).element_size()
    k = int(lib().sgmcmc_ksd_plan(int(n), int(dim), esize, None, 0))
    check(0 if k > 0 else k, "sgmcmc_ksd_plan")
    out = (ctypes.c_int * (4 * k))()
    lib().sgmcmc_ksd_plan(int(n), int(dim), esize, out, 4 * k)
    return [KsdLaunch(*out[4 * i:4 * i + 4]) for i in range(k)]


def ksd(samples, scores, workspace, kind="imq", c=1.0, beta=-0.5, h2=None, matrix=None, row_sums=None, stats=None):
    """K16 (``sgmcmc_ksd_*``): the Stein kernel matrix of the ``(n, dim)`` device matrices ``samples`` and ``scores`` (dense
    rows, any row pitch) and its sums, on the current stream without host synchronisation. ``kind``: ``"imq"``
    (``(c^2 + r^2)^beta``) or ``"rbf"`` (``exp(-r^2 / (2 h2))``, ``h2`` required). ``matrix``: ``(n, n)`` of the samples'
    dtype with dense rows, or None; ``row_sums``: ``n`` float64, or None; ``stats``: 4 float64 ``{V, U, total, trace}``,
    allocated when None. Returns ``stats``."""
    what = "ksd"
    f = getattr(lib(), "sgmcmc_ksd_" + _sfx(samples))
    if kind not in KSD_KINDS:
        raise ValueError("%s: kind must be 'imq' or 'rbf', got %r" % (what, kind))
    if kind == "rbf" and h2 is None:
        raise ValueError("%s: the RBF kernel needs h2" % what)
    if not torch.is_tensor(scores) or scores.dtype != samples.dtype or scores.device != samples.device:
        raise TypeError("%s: scores must be a %s tensor on %s" % (what, samples.dtype, samples.device))
    if samples.dim() != 2 or scores.shape != samples.shape:
        raise ValueError("%s: samples and scores must be (n, dim) matrices of one shape" % what)
    n, dim = int(samples.shape[0]), int(samples.shape[1])
    for t, name in ((samples, "samples"), (scores, "scores")):
        if (dim > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < dim):
            raise ValueError("%s: %s must have dense rows that do not overlap" % (what, name))
    if not samples.is_cuda:
        _ptr(samples)                    # raises the no-CPU-path error
    need = int(lib().sgmcmc_ksd_workspace_bytes(n, samples.element_size()))
    if need and (not torch.is_tensor(workspace) or workspace.numel() * workspace.element_size() < need):
        raise ValueError("%s: the workspace is shorter than ksd_workspace(%d, samples): %d bytes" % (what, n, need))
    ld_x, ld_s = (int(t.stride(0)) if n > 1 else dim for t in (samples, scores))
    ld_m = 0
    if matrix is not None:
        if matrix.dtype != samples.dtype or matrix.device != samples.device or tuple(matrix.shape) != (n, n) \
                or matrix.stride(1) != 1 or matrix.stride(0) < n:
            raise ValueError("%s: matrix must be (n, n) of the samples' dtype with dense rows that do not overlap" % what)
        ld_m = int(matrix.stride(0))
    for t, name, size in ((row_sums, "row_sums", n), (stats, "stats", 4)):
        if t is not None and (t.dtype != torch.float64 or t.device != samples.device or t.numel() != size
                              or not t.is_contiguous()):
            raise ValueError("%s: %s must be %d contiguous float64 elements on %s" % (what, name, size, samples.device))
    if stats is None:
        stats = torch.empty(4, dtype=torch.float64, device=samples.device)
    with torch.cuda.device(samples.device):
        rc = f(samples.data_ptr(), ld_x, scores.data_ptr(), ld_s, n, dim, KSD_KINDS[kind], float(c), float(beta),
               float(0.0 if h2 is None else h2), _ptr(workspace), None if matrix is None else matrix.data_ptr(), ld_m,
               _ptr(row_sums), _ptr(stats), _stream(samples))
    check(rc, "sgmcmc_ksd")
    return stats


# ---- K17: greedy Stein thinning from a Stein kernel matrix (include/sgmcmc_hip_thin.h, csrc/sgmcmc_stein_thin.hip) ----
SteinThinLaunch = collections.namedtuple("SteinThinLaunch", "block columns_per_thread grid waves")
STEIN_THIN_DISTINCT = 1


def stein_thin_max_samples():
    return int(lib().sgmcmc_stein_thin_max_samples())


def stein_thin_plan(n, m, batch=1):
    """The launch of one ``stein_thin`` call: ``SteinThinLaunch(block, columns_per_thread, grid, waves)`` (host arithmetic)."""
    out = (ctypes.c_int * 4)()
    rc = int(lib().sgmcmc_stein_thin_plan(int(n), int(m), int(batch), out, 4))
    check(0 if rc > 0 else rc, "sgmcmc_stein_thin_plan")
    return SteinThinLaunch(*out)


def stein_thin(matrix, m, indices=None, path=None, distinct=False, n=None, batch=1, batch_stride=0):
    """K17 (``sgmcmc_stein_thin_*``): greedy Stein thinning, ``m`` picks from each of ``batch`` blocks of ``n x n`` elements of
    the device matrix ``matrix`` (two-dimensional, dense rows, any row pitch; what ``ksd`` writes as ``matrix``), in one launch
    on the current stream without host synchronisation. Block ``p`` starts ``p * batch_stride`` elements behind the first
    element, ``batch_stride = n * matrix.stride(0) + n`` walks diagonal blocks; ``n`` defaults to the number of rows (one block:
    the whole matrix). ``distinct``: a picked row is not picked again (``m <= n``). ``indices``: ``batch * m`` int32,
    ``path``: ``batch * m`` float64 (the V-statistic of the first ``t`` picks), both contiguous, allocated when None as
    ``(m,)``, or ``(batch, m)`` when ``batch > 1``. Returns ``(indices, path)``; the indices are local to their block."""
    what = "stein_thin"
    f = getattr(lib(), "sgmcmc_stein_thin_" + _sfx(matrix))
    if matrix.dim() != 2:
        raise ValueError("%s: matrix must be two-dimensional" % what)
    rows, cols = int(matrix.shape[0]), int(matrix.shape[1])
    if (cols > 1 and matrix.stride(1) != 1) or (rows > 1 and matrix.stride(0) < cols):
        raise ValueError("%s: matrix must have dense rows that do not overlap" % what)
    n = rows if n is None else int(n)
    m, batch, batch_stride = int(m), int(batch), int(batch_stride)
    ld = int(matrix.stride(0)) if rows > 1 else cols
    if n < 1 or m < 1 or batch < 1 or batch_stride < 0:
        raise ValueError("%s: n, m and batch must be positive and batch_stride non-negative" % what)
    # the last block, like every block before it, must lie inside the matrix
    r0, c0 = divmod((batch - 1) * batch_stride, max(ld, 1))
    if r0 + n > rows or c0 + n > cols:
        raise ValueError("%s: block %d of %d x %d elements at offset %d does not lie inside the %d x %d matrix"
                         % (what, batch - 1, n, n, (batch - 1) * batch_stride, rows, cols))
    shape = (m,) if batch == 1 else (batch, m)
    for t, name, dt in ((indices, "indices", torch.int32), (path, "path", torch.float64)):
        if t is not None and (t.dtype != dt or t.device != matrix.device or t.numel() != batch * m or not t.is_contiguous()):
            raise ValueError("%s: %s must be %d contiguous %s elements on %s" % (what, name, batch * m, dt, matrix.device))
    if not matrix.is_cuda:
        _ptr(matrix)                     # raises the no-CPU-path error
    if indices is None:
        indices = torch.empty(shape, dtype=torch.int32, device=matrix.device)
    if path is None:
        path = torch.empty(shape, dtype=torch.float64, device=matrix.device)
    with torch.cuda.device(matrix.device):
        rc = f(matrix.data_ptr(), ld, n, m, batch, batch_stride, STEIN_THIN_DISTINCT if distinct else 0, _ptr(indices),
               _ptr(path), _stream(matrix))
    check(rc, "sgmcmc_stein_thin")
    return indices, path


def rank_max_pooled():
    """The largest pooled count ``N = 2 m (n // 2)`` of one ``rank_normalize`` call (``SGMCMC_RANK_MAX_POOLED``)."""
    return RANK_MAX_POOLED


def rank_normalize(trace, z=None, z_folded=None, tail_lo=None, tail_hi=None):
    """K18 (``include/sgmcmc_hip_rank.h``): the rank normalisation of every parameter of ONE strided trace, in one launch on
    the current stream: the draws of the ``2 m`` split chains pooled, ranked with average ranks over ties and mapped through
    the inverse normal CDF (``z``), the same for ``|x - median|`` (``z_folded``), and the indicators of the lower and upper
    5 % tails (``tail_lo``, ``tail_hi``). K12 (``chain_diag``) turns them into rank-normalised R-hat, bulk and tail ESS.

    ``trace``: an ``(m, n, P)`` device tensor, or ``(n, P)`` for a single chain, float32 or float64, dense rows;
    ``ld = stride(1)``, ``chain_stride = stride(0)`` as for ``chain_diag``. ``n >= 4``, ``m <= 2048`` and
    ``2 m (n // 2) <= rank_max_pooled()``. The outputs, at least one, are float64 ``(2 m, n // 2, P)`` tensors on the trace's
    device with dense rows and COMMON strides (column blocks of one ``(2 m, n // 2, 4 P)`` buffer, say). Shapes and dtypes
    are checked before a device is touched. Returns ``(z, z_folded, tail_lo, tail_hi)`` as passed."""
    what = "rank_normalize"
    if not torch.is_tensor(trace):
        raise TypeError("%s: trace must be an (m, n, P) or (n, P) device tensor" % what)
    if trace.dim() == 2:
        trace = trace.unsqueeze(0)
    if trace.dim() != 3:
        raise ValueError("%s: trace must be (m, n, P) or (n, P), got %s" % (what, tuple(trace.shape)))
    sfx = _sfx(trace)
    m, n, P = (int(v) for v in trace.shape)
    if m < 1 or m > RANK_MAX_CHAINS:
        raise ValueError("%s: m = %d chains, must be 1 .. %d" % (what, m, RANK_MAX_CHAINS))
    if n < 4:
        raise ValueError("%s: needs at least 4 samples per chain, got n = %d" % (what, n))
    half = n // 2
    if 2 * m * half > RANK_MAX_POOLED:
        raise ValueError("%s: N = 2 * %d * %d = %d pooled draws, at most %d" % (what, m, half, 2 * m * half, RANK_MAX_POOLED))
    if P > 1 and trace.stride(2) != 1:
        raise ValueError("%s: rows must be dense (stride 1 along the parameters)" % what)
    ld = int(trace.stride(1))
    chain_stride = int(trace.stride(0)) if m > 1 else (n - 1) * ld + P
    if ld < 0 or chain_stride < 0:
        raise ValueError("%s: negative strides are not supported" % what)
    outs = ((z, "z"), (z_folded, "z_folded"), (tail_lo, "tail_lo"), (tail_hi, "tail_hi"))
    if all(out is None for out, _ in outs):
        raise ValueError("%s: at least one of z, z_folded, tail_lo and tail_hi is required" % what)
    ld_out = chain_stride_out = None
    for out, name in outs:
        if out is None:
            continue
        if not torch.is_tensor(out) or out.dtype != torch.float64:
            raise TypeError("%s: %s must be a float64 tensor" % (what, name))
        if tuple(out.shape) != (2 * m, half, P):
            raise ValueError("%s: %s must be of shape (2 m, n // 2, P) = %s, got %s" % (what, name, (2 * m, half, P),
                                                                                        tuple(out.shape)))
        if out.device != trace.device:
            raise ValueError("%s: %s must live on %s" % (what, name, trace.device))
        if P > 1 and out.stride(2) != 1:
            raise ValueError("%s: the rows of %s must be dense" % (what, name))
        strides = (int(out.stride(1)) if half > 1 else P, int(out.stride(0)))
        if ld_out is None:
            ld_out, chain_stride_out = strides
        elif strides != (ld_out, chain_stride_out):
            raise ValueError("%s: the outputs must share their strides, %s has %s against %s" % (
                what, name, strides, (ld_out, chain_stride_out)))
    if ld_out < P or chain_stride_out < (half - 1) * ld_out + P:
        raise ValueError("%s: the outputs' rows or chains overlap (strides %s)" % (what, (chain_stride_out, ld_out)))
    if not trace.is_cuda:
        raise SgmcmcLibraryError("pysgmcmc_amd: trace lives on %s; the rank normalisation runs only as a HIP kernel on an "
                                 "AMD GPU (no CPU fallback)." % trace.device)
    f = getattr(lib(), "sgmcmc_rank_normalize_" + sfx)
    with torch.cuda.device(trace.device):
        rc = f(trace.data_ptr(), m, n, P, ld, chain_stride, *[None if out is None else out.data_ptr() for out, _ in outs],
               ld_out, chain_stride_out, _stream(trace))
    check(rc, "sgmcmc_rank_normalize")
    return z, z_folded, tail_lo, tail_hi


def psis_max_draws():
    """The largest number of draws ``S`` of one ``psis_loo`` call (``SGMCMC_PSIS_MAX_DRAWS``)."""
    return PSIS_MAX_DRAWS


def psis_loo(loglik, r_eff=1.0, elpd_loo=None, khat=None, n_tail=None, row_lppd=None, log_weights=None, summary=None):
    """K19 (``include/sgmcmc_hip_psis.h``): Pareto-smoothed importance-sampling leave-one-out of every observation column
    of the pointwise log densities ``loglik``, in one launch on the current stream (and a second small one for ``summary``).

    ``loglik``: a float64 ``(S, n_rows)`` device tensor with dense rows (``ld = stride(0)``, a view of a wider buffer is
    fine), ``2 <= S <= psis_max_draws()``: what ``bnn_score`` leaves in its ``loglik``. ``r_eff``: the relative efficiency of
    the draws, a positive finite number. ``elpd_loo``, ``khat`` (float64) and ``n_tail`` (int32) ``(n_rows,)`` are allocated
    when they are missing; optional: ``row_lppd`` float64 ``(n_rows,)``, ``log_weights`` float64 ``(S, n_rows)`` with dense
    rows (the normalised smoothed log weights), ``summary`` float64 ``(4,)`` = ``{sum elpd_loo, sum row_lppd, rows with khat
    > 0.7, rows holding a NaN or an infinity}``. Sizes, ``r_eff``, shapes and dtypes are checked before a device is touched,
    in the order of the header's refusals. Returns ``(elpd_loo, khat, n_tail)``."""
    what = "psis_loo"
    if not torch.is_tensor(loglik):
        raise TypeError("%s: loglik must be an (S, n_rows) float64 device tensor" % what)
    if loglik.dim() != 2:
        raise ValueError("%s: loglik must be (S, n_rows), got %s" % (what, tuple(loglik.shape)))
    S, n_rows = (int(v) for v in loglik.shape)
    if S < 2 or S > PSIS_MAX_DRAWS:
        raise ValueError("%s: S = %d draws, must be 2 .. %d" % (what, S, PSIS_MAX_DRAWS))
    r_eff = float(r_eff)
    if not (r_eff > 0.0 and r_eff != float("inf")):
        raise ValueError("%s: r_eff = %g, must be a positive finite number" % (what, r_eff))
    if loglik.dtype != torch.float64:
        raise TypeError("%s: loglik must be a float64 tensor, got %s" % (what, loglik.dtype))
    if n_rows > 1 and loglik.stride(1) != 1:
        raise ValueError("%s: the rows of loglik must be dense (stride 1 along the observations)" % what)
    ld = int(loglik.stride(0))
    if ld < n_rows:
        raise ValueError("%s: ld = %d is smaller than n_rows = %d" % (what, ld, n_rows))
    dev = loglik.device
    for out, dt, name in ((elpd_loo, torch.float64, "elpd_loo"), (khat, torch.float64, "khat"), (n_tail, torch.int32, "n_tail"),
                          (row_lppd, torch.float64, "row_lppd")):
        if out is None:
            continue
        if not torch.is_tensor(out) or out.dtype != dt:
            raise TypeError("%s: %s must be a %s tensor" % (what, name, dt))
        if tuple(out.shape) != (n_rows,) or out.device != dev or not out.is_contiguous():
            raise ValueError("%s: %s must be a contiguous (n_rows,) = (%d,) tensor on %s" % (what, name, n_rows, dev))
    ld_w = 0
    if log_weights is not None:
        if not torch.is_tensor(log_weights) or log_weights.dtype != torch.float64:
            raise TypeError("%s: log_weights must be a %s tensor" % (what, torch.float64))
        if tuple(log_weights.shape) != (S, n_rows) or log_weights.device != dev:
            raise ValueError("%s: log_weights must be of shape (S, n_rows) = %s on %s, got %s" % (
                what, (S, n_rows), dev, tuple(log_weights.shape)))
        if n_rows > 1 and log_weights.stride(1) != 1:
            raise ValueError("%s: the rows of log_weights must be dense" % what)
        ld_w = int(log_weights.stride(0))
        if ld_w < n_rows:
            raise ValueError("%s: ld_w = %d is smaller than n_rows = %d" % (what, ld_w, n_rows))
    if summary is not None:
        if not torch.is_tensor(summary) or summary.dtype != torch.float64:
            raise TypeError("%s: summary must be a %s tensor" % (what, torch.float64))
        if summary.numel() != 4 or summary.device != dev or not summary.is_contiguous():
            raise ValueError("%s: summary must hold 4 contiguous elements on %s" % (what, dev))
    if n_rows >= 2 ** 31:
        raise ValueError("%s: n_rows = %d is too large for one launch" % (what, n_rows))
    if not loglik.is_cuda:
        raise SgmcmcLibraryError("pysgmcmc_amd: loglik lives on %s; PSIS-LOO runs only as a HIP kernel on an AMD GPU (no CPU "
                                 "fallback; diagnostics.psis.psis_loo_host is the host statement)." % dev)
    if elpd_loo is None:
        elpd_loo = torch.empty(n_rows, dtype=torch.float64, device=dev)
    if khat is None:
        khat = torch.empty(n_rows, dtype=torch.float64, device=dev)
    if n_tail is None:
        n_tail = torch.empty(n_rows, dtype=torch.int32, device=dev)
    opt = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        rc = lib().sgmcmc_psis_loo(loglik.data_ptr(), ld, S, n_rows, r_eff, elpd_loo.data_ptr(), khat.data_ptr(),
                                   n_tail.data_ptr(), opt(row_lppd), opt(log_weights), ld_w, opt(summary), _stream(loglik))
    check(rc, "sgmcmc_psis_loo")
    return elpd_loo, khat, n_tail


def calib_max_draws():
    """The largest number of draws ``S`` of one ``mixture_calibration`` call (``SGMCMC_CALIB_MAX_DRAWS``)."""
    return CALIB_MAX_DRAWS


def mixture_calibration(means, var, y, levels=(), n_bins=0, pit=None, crps=None, summary=None):
    """K20 (``include/sgmcmc_hip_calib.h``): the probability integral transform and the closed-form CRPS of every target
    ``y[r]`` under the equal-weight mixture of the ``S`` Gaussians ``N(means[s][r], var[s])``, in one launch on the current
    stream (and a second small one for ``summary``).

    ``means``: a float32 or float64 ``(S, n_rows)`` device tensor with dense rows (``ld = stride(0)``, a view of a wider
    buffer is fine), ``1 <= S <= calib_max_draws()``: what ``bnn_predict`` and ``bnn_score`` leave in their ``means``. ``var``:
    float64 ``(S,)``, the variance of every draw's Gaussian. ``y``: ``(n_rows,)`` of ``means``' dtype. ``levels``: up to 16
    host numbers in (0, 1), the central intervals whose coverage is counted; ``n_bins``: 0 .. 64 bins of the PIT histogram.
    ``pit`` and ``crps`` float64 ``(n_rows,)`` are allocated when they are missing; optional: ``summary`` float64 ``(2 +
    len(levels) + n_bins,)`` = ``{the fixed-order sum of crps, rows holding a NaN, the rows in each interval, the rows in each
    bin}``. Sizes, levels, shapes and dtypes are checked before a device is touched, in the order of the header's refusals.
    Returns ``(pit, crps)``."""
    what = "mixture_calibration"
    if not torch.is_tensor(means):
        raise TypeError("%s: means must be an (S, n_rows) float32 or float64 device tensor" % what)
    if means.dim() != 2:
        raise ValueError("%s: means must be (S, n_rows), got %s" % (what, tuple(means.shape)))
    S, n_rows = (int(v) for v in means.shape)
    if S < 1 or S > CALIB_MAX_DRAWS:
        raise ValueError("%s: S = %d draws, must be 1 .. %d" % (what, S, CALIB_MAX_DRAWS))
    levels = [float(v) for v in levels]
    n_levels, n_bins = len(levels), int(n_bins)
    if n_levels > CALIB_MAX_LEVELS:
        raise ValueError("%s: n_levels = %d, must be 0 .. %d" % (what, n_levels, CALIB_MAX_LEVELS))
    if n_bins < 0 or n_bins > CALIB_MAX_BINS:
        raise ValueError("%s: n_bins = %d, must be 0 .. %d" % (what, n_bins, CALIB_MAX_BINS))
    for k, v in enumerate(levels):
        if not (0.0 < v < 1.0):
            raise ValueError("%s: levels[%d] = %g, must lie in (0, 1)" % (what, k, v))
    if means.dtype not in _SFX:
        raise TypeError("%s: means must be a float32 or float64 tensor, got %s" % (what, means.dtype))
    dev = means.device
    if not torch.is_tensor(var) or var.dtype != torch.float64:
        raise TypeError("%s: var must be a %s tensor" % (what, torch.float64))
    if tuple(var.shape) != (S,) or var.device != dev or not var.is_contiguous():
        raise ValueError("%s: var must be a contiguous (S,) = (%d,) tensor on %s" % (what, S, dev))
    if not torch.is_tensor(y) or y.dtype != means.dtype:
        raise TypeError("%s: y must be a %s tensor, like means" % (what, means.dtype))
    if tuple(y.shape) != (n_rows,) or y.device != dev or not y.is_contiguous():
        raise ValueError("%s: y must be a contiguous (n_rows,) = (%d,) tensor on %s" % (what, n_rows, dev))
    for out, name in ((pit, "pit"), (crps, "crps")):
        if out is None:
            continue
        if not torch.is_tensor(out) or out.dtype != torch.float64:
            raise TypeError("%s: %s must be a %s tensor" % (what, name, torch.float64))
        if tuple(out.shape) != (n_rows,) or out.device != dev or not out.is_contiguous():
            raise ValueError("%s: %s must be a contiguous (n_rows,) = (%d,) tensor on %s" % (what, name, n_rows, dev))
    if summary is not None:
        if not torch.is_tensor(summary) or summary.dtype != torch.float64:
            raise TypeError("%s: summary must be a %s tensor" % (what, torch.float64))
        if summary.numel() != 2 + n_levels + n_bins or summary.device != dev or not summary.is_contiguous():
            raise ValueError("%s: summary must hold 2 + n_levels + n_bins = %d contiguous elements on %s" % (
                what, 2 + n_levels + n_bins, dev))
    if n_rows > 1 and means.stride(1) != 1:
        raise ValueError("%s: the rows of means must be dense (stride 1 along the observations)" % what)
    ld = int(means.stride(0)) if S > 1 else max(int(means.stride(0)), n_rows)
    if ld < n_rows:
        raise ValueError("%s: ld = %d is smaller than n_rows = %d" % (what, ld, n_rows))
    if n_rows >= 2 ** 31:
        raise ValueError("%s: n_rows = %d is too large for one launch" % (what, n_rows))
    if not means.is_cuda:
        raise SgmcmcLibraryError("pysgmcmc_amd: means lives on %s; the calibration kernel runs only as a HIP kernel on an AMD "
                                 "GPU (no CPU fallback; diagnostics.mixture_calibration_host is the host statement)." % dev)
    if pit is None:
        pit = torch.empty(n_rows, dtype=torch.float64, device=dev)
    if crps is None:
        crps = torch.empty(n_rows, dtype=torch.float64, device=dev)
    lv = (ctypes.c_double * max(n_levels, 1))(*levels)
    with torch.cuda.device(dev):
        f = getattr(lib(), "sgmcmc_mixture_calibration_" + _SFX[means.dtype])
        rc = f(means.data_ptr(), ld, S, n_rows, var.data_ptr(), y.data_ptr(), lv, n_levels, n_bins, pit.data_ptr(),
               crps.data_ptr(), None if summary is None else summary.data_ptr(), _stream(means))
    check(rc, "sgmcmc_mixture_calibration")
    return pit, crps
