"""Device-resident traces of whole parameter vectors, and the effective sample size of EVERY parameter from them.

The reference's ``effective_sample_sizes`` (``pysgmcmc/diagnostics/sampler_diagnostics.py:47-82``) returns one ESS
per parameter dimension from traces that are Python lists of host arrays; ``sampler_diagnostics.effective_n`` restates
its estimator for ONE scalar (an FFT and a host read per call). Here the trace never leaves the device:

  ``DeviceTrace``                 a preallocated ``(capacity, n_params)`` matrix; ``append`` is one stream-ordered
                                  device copy, ``record`` steps a sampler and keeps its flat ``theta`` row; with
                                  ``fused=True`` the whole-step BNN kernel K8 writes the kept rows itself, in ONE launch
                                  (``sampler.fused_bnn_steps(n, trace, keep_every)``)
  ``effective_n_all``             one launch of K10 (``kernels.ess_variogram``) -> int64 ESS of all P parameters, on the
                                  device, no host synchronisation
  ``chain_diagnostics_all``       one launch of K12 (``kernels.chain_diag``) -> float64 R-hat AND int64 ESS of all P
                                  parameters from up to 4096 chains (K10 stops at 64); ``gelman_rubin_all`` is its
                                  R-hat-only launch
  ``rank_diagnostics_all``        one launch of K18 (``kernels.rank_normalize``) and two of K12 -> the rank-normalised split
                                  R-hat and the bulk and tail ESS of all P parameters
  ``effective_sample_sizes_of``   the reference's ``{name: array shaped like the parameter}`` cut from that vector

Scope: chains that share a device (``ConcurrentChains``, sequential chains as in ``multitrace``, the stacked state of
``FusedBNNChains``) and a single chain. Chains on different ranks are OUT of scope: the stop rule needs the cross-chain
``rho_t`` lag by lag, so an all-parameter ESS across ranks would take a collective per lag or an all-gather of whole
traces; ``sampler_diagnostics.ess_across_ranks`` stays the multi-rank path, for a few scalars.
"""
import torch

from pysgmcmc_amd import kernels

__all__ = ["DeviceTrace", "effective_n_all", "effective_sample_sizes_of", "chain_diagnostics_all", "gelman_rubin_all",
           "rank_diagnostics_all"]


class DeviceTrace(object):
    """``capacity`` samples of an ``n_params``-long parameter vector in one preallocated device matrix."""

    def __init__(self, n_params, capacity, device, dtype=torch.float32):
        self.n_params = int(n_params)
        self.capacity = int(capacity)
        if self.n_params < 0 or self.capacity < 0:
            raise ValueError("DeviceTrace: n_params and capacity must be >= 0")
        self.buffer = torch.empty(self.capacity, self.n_params, dtype=dtype, device=device)
        self._len = 0
        # steps a whole-step launch (``fused_bnn_steps(n, trace, keep_every)``) took after the last sample it kept: the next
        # chunk continues the thinning from here
        self.steps_since_kept = 0
        # set by record(): how to cut a flat vector into the sampler's parameters
        self.param_names = None
        self.param_shapes = None
        self.param_offsets = None

    @property
    def device(self):
        return self.buffer.device

    @property
    def dtype(self):
        return self.buffer.dtype

    def __len__(self):
        return self._len

    def append(self, theta_flat):
        """Copy one flat parameter vector into the next row (asynchronous on the current stream; no host sync)."""
        if self._len >= self.capacity:
            raise IndexError("DeviceTrace: capacity of %d samples exhausted" % self.capacity)
        if theta_flat.numel() != self.n_params:
            raise ValueError("DeviceTrace.append: %d elements, the trace is %d wide" % (theta_flat.numel(), self.n_params))
        self.buffer[self._len].copy_(theta_flat.detach().reshape(-1), non_blocking=True)
        self._len += 1

    def values(self):
        """The ``(len, n_params)`` view of the samples recorded so far (aliases the buffer)."""
        return self.buffer[:self._len]

    def reset(self):
        self._len = 0
        self.steps_since_kept = 0

    def describe(self, sampler):
        """Take the names, shapes and offsets of ``sampler``'s parameters (what ``effective_sample_sizes_of`` cuts by)."""
        arena = sampler.arena
        self.param_names = list(getattr(sampler, "param_names", [str(i) for i in range(len(arena.shapes))]))
        self.param_shapes = list(arena.shapes)
        self.param_offsets = list(arena.offsets)

    def kept_rows(self, n_steps, keep_every):
        """How many of the next ``n_steps`` steps a run that keeps every ``keep_every``-th one would keep, counted from
        the last kept sample."""
        return (self.steps_since_kept + int(n_steps)) // int(keep_every)

    def advance(self, n_steps, keep_every):
        """Account for ``n_steps`` steps whose every ``keep_every``-th sample something else wrote into the next rows of
        ``buffer`` (a whole-step launch): the length grows by the kept count, which is returned, and
        ``steps_since_kept`` moves on. ``IndexError`` if the rows do not exist."""
        n_steps, keep_every = int(n_steps), int(keep_every)
        if n_steps < 0 or keep_every < 1:
            raise ValueError("DeviceTrace.advance: n_steps must be >= 0 and keep_every >= 1")
        kept = self.kept_rows(n_steps, keep_every)
        if self._len + kept > self.capacity:
            raise IndexError("DeviceTrace: capacity of %d samples exhausted" % self.capacity)
        self._len += kept
        self.steps_since_kept = (self.steps_since_kept + n_steps) % keep_every
        return kept

    @classmethod
    def record(cls, sampler, n_samples, keep_every=1, fused=False):
        """Step ``sampler`` ``n_samples * keep_every`` times and keep ``sampler.arena.row("theta")`` after every
        ``keep_every``-th step. The sampler's ``sample_format`` is ``"view"`` for the duration (no per-step host
        copy) and restored afterwards, also when a step raises. The chain itself is untouched: the appends only read
        theta, in stream order after the step that produced it.

        ``fused=True``: the same samples of a chain that fits the whole-step BNN kernel
        (``sampler.fused_bnn_available()``, else ``ValueError``) in ONE launch that writes the kept rows itself:
        ``sampler.fused_bnn_steps(n_samples * keep_every, trace, keep_every)``."""
        n_samples, keep_every = int(n_samples), int(keep_every)
        if n_samples < 0 or keep_every < 1:
            raise ValueError("DeviceTrace.record: n_samples must be >= 0 and keep_every >= 1")
        if fused and not (hasattr(sampler, "fused_bnn_available") and sampler.fused_bnn_available()):
            raise ValueError("DeviceTrace.record: fused=True needs a sampler whose fused_bnn_available() is true")
        arena = sampler.arena
        theta = arena.row("theta")
        trace = cls(theta.numel(), n_samples, theta.device, theta.dtype)
        trace.describe(sampler)
        if fused:
            if n_samples:
                sampler.fused_bnn_steps(n_samples * keep_every, trace, keep_every)
            return trace
        fmt = sampler.sample_format
        sampler.sample_format = "view"
        try:
            for _ in range(n_samples):
                for _ in range(keep_every):
                    next(sampler)
                trace.append(sampler.arena.row("theta"))
        finally:
            sampler.sample_format = fmt
        return trace


def _chain_matrices(traces, who="effective_n_all"):
    """``traces`` of effective_n_all (or of ``who``) -> list of (n, P) tensors, one per chain."""
    if isinstance(traces, DeviceTrace):
        return [traces.values()]
    if torch.is_tensor(traces):
        if traces.dim() == 2:
            return [traces]
        if traces.dim() == 3:
            return list(traces.unbind(0))
        raise ValueError("%s: a tensor of traces must be (n, P) or (m, n, P), got %s" % (who, tuple(traces.shape),))
    try:
        items = list(traces)
    except TypeError:
        raise TypeError("%s: traces must be a DeviceTrace, a sequence of them or a device tensor" % who)
    if not items:
        raise ValueError("%s: no traces" % who)
    mats = []
    for t in items:
        if isinstance(t, DeviceTrace):
            mats.append(t.values())
        elif torch.is_tensor(t) and t.dim() == 2:
            mats.append(t)
        else:
            raise TypeError("%s: every chain must be a DeviceTrace or an (n, P) tensor" % who)
    first = mats[0]
    for x in mats[1:]:
        if x.shape[0] != first.shape[0]:
            raise ValueError("%s: the chains hold different numbers of samples (%d and %d)" % (who, first.shape[0], x.shape[0]))
        if x.shape[1] != first.shape[1]:
            raise ValueError("%s: the chains are of different widths (%d and %d)" % (who, first.shape[1], x.shape[1]))
    return mats


def effective_n_all(traces, details=False, staging="auto", launch=None):
    """Effective sample size of each of the P parameters (variogram estimate, the arithmetic of
    ``sampler_diagnostics.effective_n``) in ONE kernel launch on the traces' device.

    ``traces``: a ``DeviceTrace`` (one chain), a sequence of them (one per chain; equal lengths and widths, else
    ``ValueError``), or a device tensor ``(n, P)`` / ``(m, n, P)``. At most 64 chains, at least 2 samples each.
    Returns the int64 device tensor of P values; with ``details=True`` the tuple ``(ess, raw, stop_lag)``: the
    untruncated float64 estimate and the lag T at which each parameter's sum stopped. A parameter whose traces are
    constant (Vhat = 0) gets ``ess = 0``, ``raw = NaN``, ``stop_lag = 1`` where the scalar function raises. Nothing here
    waits for the host. Chains on different ranks are out of scope (see the module docstring)."""
    mats = _chain_matrices(traces)
    first = mats[0]
    if first.shape[0] < 2:
        raise ValueError("effective_n_all: needs at least 2 samples per chain, got %d" % first.shape[0])
    if len(mats) > 64:
        raise ValueError("effective_n_all: at most 64 chains, got %d" % len(mats))
    P, dev = int(first.shape[1]), first.device
    ess = torch.empty(P, dtype=torch.int64, device=dev)
    raw = torch.empty(P, dtype=torch.float64, device=dev) if details else None
    stop = torch.empty(P, dtype=torch.int32, device=dev) if details else None
    kernels.ess_variogram(mats, ess, raw, stop, staging=staging, launch=launch)
    return (ess, raw, stop) if details else ess


def _stacked_trace(traces, who):
    """``traces`` of chain_diagnostics_all -> one (m, n, P) tensor: a tensor goes through as it is, a sequence is stacked."""
    mats = None if torch.is_tensor(traces) and traces.dim() == 3 else _chain_matrices(traces, who)
    m, n = (traces.shape[0], traces.shape[1]) if mats is None else (len(mats), mats[0].shape[0])
    if m < 1:
        raise ValueError("%s: no traces" % who)
    if n < 2:
        raise ValueError("%s: needs at least 2 samples per chain, got %d" % (who, n))
    if m > 4096:
        raise ValueError("%s: at most 4096 chains, got %d" % (who, m))
    if mats is None:
        return traces
    return mats[0].unsqueeze(0) if m == 1 else torch.stack(mats)


def gelman_rubin_all(traces):
    """Gelman-Rubin R-hat of each of the P parameters, ``sqrt(Vhat / W)``, as a float64 ``(P,)`` device tensor: the
    R-hat-only launch of K12 (``kernels.chain_diag``), which takes the chain moments and walks no lag. ``traces`` as for
    :func:`chain_diagnostics_all`. NaN where a parameter's ``Vhat`` is zero or not finite, ``+inf`` where every chain is
    constant at a value of its own; with ONE chain the formula gives ``sqrt((n - 1) / n)``. Nothing waits for the host."""
    x = _stacked_trace(traces, "gelman_rubin_all")
    rhat = torch.empty(int(x.shape[2]), dtype=torch.float64, device=x.device)
    kernels.chain_diag(x, rhat=rhat)
    return rhat


def chain_diagnostics_all(traces, details=False):
    """R-hat and effective sample size of each of the P parameters across up to 4096 chains, in ONE launch of K12
    (``kernels.chain_diag``) on the traces' device: ``(rhat, ess)``, float64 and int64 ``(P,)`` device tensors; with
    ``details=True`` ``(rhat, ess, raw, stop_lag)`` as :func:`effective_n_all` gives them.

    ``traces``: what :func:`effective_n_all` accepts. A device tensor ``(m, n, P)`` (what ``FusedBNNChains.collect``
    returns, or a view of a wider or longer buffer with dense rows) goes down as it is, without a copy and with any
    ``m <= 4096``; an ``(n, P)`` tensor or a ``DeviceTrace`` is one chain; a sequence of ``DeviceTrace``s or matrices that
    live in buffers of their own is stacked into one ``(m, n, P)`` tensor first -- that ONE device copy is the price of
    the kernel's single base pointer (K10, ``effective_n_all``, takes up to 64 separate buffers without it). At least 2
    samples per chain. The estimators are those of ``effective_n_all`` and ``gelman_rubin``; for up to 16 chains ``ess``,
    ``raw`` and ``stop_lag`` equal ``effective_n_all``'s bit for bit, beyond that the chains are summed in groups of 16
    (``include/sgmcmc_hip_chains.h``). Degenerate parameters: ``rhat`` NaN, ``ess`` 0, ``raw`` NaN, ``stop_lag`` 1.
    Nothing here waits for the host. Chains on different ranks are out of scope (see the module docstring)."""
    x = _stacked_trace(traces, "chain_diagnostics_all")
    P, dev = int(x.shape[2]), x.device
    rhat = torch.empty(P, dtype=torch.float64, device=dev)
    ess = torch.empty(P, dtype=torch.int64, device=dev)
    raw = torch.empty(P, dtype=torch.float64, device=dev) if details else None
    stop = torch.empty(P, dtype=torch.int32, device=dev) if details else None
    kernels.chain_diag(x, rhat, ess, raw, stop)
    return (rhat, ess, raw, stop) if details else (rhat, ess)


def rank_diagnostics_all(traces, details=False):
    """Rank-normalised split R-hat, bulk ESS and tail ESS of each of the P parameters (Vehtari, Gelman, Simpson, Carpenter,
    Buerkner 2021): ``(rhat_rank, ess_bulk, ess_tail)``, float64 / int64 / int64 ``(P,)`` device tensors. Where the classic
    R-hat of :func:`chain_diagnostics_all` compares the chains' means and needs a finite variance, this one also sees chains
    that agree in location and differ in scale, and heavy tails do not break it.

    ``traces``: what :func:`chain_diagnostics_all` accepts, with at most 2048 chains of at least 4 samples and at most
    ``kernels.rank_max_pooled()`` pooled draws ``N = 2 m (n // 2)`` per parameter. Every chain is split in two. ONE launch
    of K18 (``kernels.rank_normalize``) writes, into one ``(2 m, n // 2, 4 P)`` buffer, the normal scores ``z`` of the pooled
    ranks (average ranks over ties), the scores ``z_folded`` of ``|x - median|`` and the indicators ``tail_lo`` / ``tail_hi``
    of the pooled 5 % and 95 % order statistics; K12 (``kernels.chain_diag``) then reads column blocks of that buffer: an
    R-hat-only launch over ``[z_folded | z]`` and a full one over ``[z | tail_lo | tail_hi]``.

        rhat_rank = max(rhat(z), rhat(z_folded))     ess_bulk = ess(z)     ess_tail = min(ess(tail_lo), ess(tail_hi))

    with the maximum and the minimum taken on the device (a NaN R-hat on either side gives NaN). With ``details=True`` the
    result is the ``rank.RankDiagnostics`` tuple of device tensors: those three, then ``rhat_bulk``, ``rhat_folded``,
    ``ess_tail_lo``, ``ess_tail_hi`` and the untruncated ``raw_bulk``, ``raw_tail_lo``, ``raw_tail_hi``. A parameter with a
    NaN or an infinite sample, or a constant one, is degenerate: R-hat NaN, ESS 0. Nothing here waits for the host.

    Two deviations from ArviZ. (1) The ESS estimator is K12's variogram rule (that of ``effective_n``) applied to the
    transformed split chains, not Geyer's initial monotone sequence; the R-hat formula is the same. (2) The tail indicators
    are taken against order statistics of the POOLED SPLIT draws, so for odd ``n`` the middle draw of every chain, which the
    split drops, does not enter the quantiles either."""
    from pysgmcmc_amd.diagnostics.rank import RankDiagnostics
    who = "rank_diagnostics_all"
    x = _stacked_trace(traces, who)
    if x.dim() == 2:
        x = x.unsqueeze(0)
    m, n, P = (int(v) for v in x.shape)
    if m > 2048:
        raise ValueError("%s: at most 2048 chains, got %d" % (who, m))
    if n < 4:
        raise ValueError("%s: needs at least 4 samples per chain, got %d" % (who, n))
    dev, half = x.device, n // 2
    buf = torch.empty(2 * m, half, 4 * P, dtype=torch.float64, device=dev)
    zf, z, lo, hi = (buf[:, :, k * P:(k + 1) * P] for k in range(4))
    kernels.rank_normalize(x, z=z, z_folded=zf, tail_lo=lo, tail_hi=hi)
    rhat2 = torch.empty(2 * P, dtype=torch.float64, device=dev)
    ess3 = torch.empty(3 * P, dtype=torch.int64, device=dev)
    raw3 = torch.empty(3 * P, dtype=torch.float64, device=dev) if details else None
    if P:
        kernels.chain_diag(buf[:, :, :2 * P], rhat=rhat2)
        kernels.chain_diag(buf[:, :, P:], ess=ess3, raw=raw3)
    rhat_f, rhat_z = rhat2[:P], rhat2[P:]
    ess_bulk, ess_lo, ess_hi = ess3[:P], ess3[P:2 * P], ess3[2 * P:]
    rhat = torch.maximum(rhat_z, rhat_f)
    ess_tail = torch.minimum(ess_lo, ess_hi)
    if not details:
        return rhat, ess_bulk, ess_tail
    return RankDiagnostics(rhat, ess_bulk, ess_tail, rhat_z, rhat_f, ess_lo, ess_hi, raw3[:P], raw3[P:2 * P], raw3[2 * P:])


def effective_sample_sizes_of(samplers_or_traces, param_shapes=None, names=None):
    """ESS per parameter dimension, ``{name: int64 device tensor shaped like the parameter}``: what the reference's
    ``effective_sample_sizes`` returns, from device traces.

    ``samplers_or_traces``: what :func:`effective_n_all` accepts. Traces made by ``DeviceTrace.record`` know their
    sampler's parameter shapes and ``param_names``; otherwise pass ``param_shapes`` (dense, in order) and optionally
    ``names`` (default ``"0", "1", ...`` as the samplers name their parameters)."""
    src = samplers_or_traces
    probe = src if isinstance(src, DeviceTrace) else (src[0] if isinstance(src, (list, tuple)) and src else None)
    offsets = None
    if param_shapes is None:
        if not isinstance(probe, DeviceTrace) or probe.param_shapes is None:
            raise ValueError("effective_sample_sizes_of: param_shapes is needed unless the traces come from DeviceTrace.record")
        param_shapes, offsets = probe.param_shapes, probe.param_offsets
        if names is None:
            names = probe.param_names
    shapes = [tuple(s) for s in param_shapes]
    sizes = []
    for shp in shapes:
        k = 1
        for d in shp:
            k *= int(d)
        sizes.append(k)
    if offsets is None:
        offsets, off = [], 0
        for k in sizes:
            offsets.append(off)
            off += k
    if names is None:
        names = [str(i) for i in range(len(shapes))]
    names = list(names)
    if len(names) != len(shapes):
        raise ValueError("effective_sample_sizes_of: %d names for %d parameters" % (len(names), len(shapes)))
    ess = effective_n_all(src)
    if offsets and offsets[-1] + sizes[-1] > ess.numel():
        raise ValueError("effective_sample_sizes_of: the parameters hold %d elements, the traces are %d wide" % (
            offsets[-1] + sizes[-1], ess.numel()))
    return {name: ess[o:o + k].view(shp) for name, o, k, shp in zip(names, offsets, sizes, shapes)}
