"""Whole steps of a small BNN in one kernel (csrc/sgmcmc_bnn_fused.hip), shared by the samplers of the hot path:
SGHMC and SGLD (the two the reference's BNN accepts, ``pysgmcmc/sampling.py:40,64``) and relativistic SGHMC.

A sampler supplies four hooks and nothing else: ``_FUSED_ROWS`` (its state rows in the kernel's order), ``_SCALARS_KIND``
(which update operator), ``_step_scalars(eps)`` (the operator's scalars, ``eps`` first) and, if it has a burn-in,
``burn_in_steps``. From there ONE path leads to the launch (``_fused_bnn_launch`` -> ``kernels.bnn_fused_steps``), for one
chain (``fused_bnn_steps``) and for a group (``fused_chains.FusedBNNChains.steps``). Either can keep every k-th sample in
a device trace inside the launch (``diagnostics.device_trace.DeviceTrace``, include/sgmcmc_hip_fused_trace.h).

The stepsize may move inside a chunk: the kernel then reads each step's derived scalars from a device table built on the
host from the schedule's values (``kernels.step_scalars_table``); a chunk at one stepsize is launched by value."""
import numpy as np
import torch

from pysgmcmc_amd import kernels

__all__ = ("FusedBNNStepsMixin",)


class FusedBNNStepsMixin(object):
    """``fused_bnn_available()`` / ``fused_bnn_steps(n)`` from the four hooks of the module docstring."""

    def fused_bnn_available(self):
        """True when whole steps can run inside ONE kernel (``sgmcmc_bnn_fused_{sghmc,sgld,rsghmc}_steps``): the cost is
        the library's MLP-BNN cost (``BNNCost``, weight prior folded), fed by a ``WindowBatches`` generator,
        the net has one output unit, at most 8 layers, and its activations fit the LDS."""
        cost, gen = self.cost_fun, self.batch_generator
        if self.device.type != "cuda" or self.noise_source is not None:
            return False
        if not (hasattr(cost, "fold_prior") and cost.fold_prior and hasattr(gen, "next_starts")):
            return False
        if gen.x_placeholder is not cost.x_placeholder or gen.y_placeholder is not cost.y_placeholder:
            return False
        sizes = self._bnn_layer_sizes()
        if sizes is None or sizes[-1] != 1 or len(sizes) - 1 > 8:
            return False
        lds = 160 + ((2 * sum(sizes) + 1) * gen.batch_size + self.arena.n + 4) * self.arena.row("theta").element_size()
        return lds <= 160 * 1024 and gen.x_dev.dtype == self._torch_dtype and gen.x_dev.is_contiguous()

    def _bnn_layer_sizes(self):
        shapes = self.arena.shapes
        if len(shapes) < 3 or len(shapes) % 2 == 0 or shapes[-1] not in ((1, 1), (1,), ()):
            return None
        sizes = [shapes[0][0]]
        for l in range((len(shapes) - 1) // 2):
            w, b = shapes[2 * l], shapes[2 * l + 1]
            if len(w) != 2 or w[0] != sizes[-1] or b != (w[1],):
                return None
            sizes.append(w[1])
        return sizes

    def _fused_scalars_table(self, eps):
        """Device table of the chunk's per-step scalars for the stepsizes ``eps``, or None when they are all equal (the
        launch then takes ``eps[0]`` by value)."""
        if all(e == eps[0] for e in eps):
            return None
        return kernels.step_scalars_table(self._SCALARS_KIND, eps, *self._step_scalars(eps[0])[1:],
                                          dtype=self._torch_dtype, device=self.device)

    def _fused_stepsizes(self, n_steps):
        """The chunk's ``n_steps`` stepsizes, drawn from the schedule up front; ``epsilon`` ends as the last one."""
        eps = [next(self.stepsize_schedule) for _ in range(n_steps)]
        self.epsilon = eps[-1]
        return eps

    def _fused_window_starts(self, n_steps):
        """The chunk's ``n_steps`` window starts (host, int32): first a window ``next(sampler)`` drew one step ahead
        (``base_classes._window_to_prefetch``) or a resumed chain carries (``load_state_dict``), then the generator's."""
        pending, self._pending_window = getattr(self, "_pending_window", None), None
        if pending is None:
            return self.batch_generator.next_starts(n_steps)
        return np.concatenate([np.asarray([pending[0]], dtype=np.int32), self.batch_generator.next_starts(n_steps - 1)])

    def _fused_bnn_launch(self, starts, costs, eps, n_steps, n_chains=1, chain_stride=None, bases=None, scalars_steps=None,
                          **trace):
        """Launch ``n_steps`` steps at stepsize ``eps`` (or the table's) on this chain's rows, or on ``bases`` for a group.
        ``trace``: the ``trace*`` keywords of ``kernels.bnn_fused_steps``, or none."""
        gen, cost, a = self.batch_generator, self.cost_fun, self.arena
        kernels.bnn_fused_steps(
            self._SCALARS_KIND, bases or [a.row(k) for k in self._FUSED_ROWS], self._bnn_layer_sizes(), gen.x_dev,
            gen.y_dev.reshape(-1), starts, gen.batch_size, cost.batch_size, cost.n_examples, cost.wdecay, cost.prior_mean,
            cost.prior_var, self._step_scalars(eps), self.n_iterations, n_steps, max(getattr(self, "burn_in_steps", 0), 0),
            self._philox_seed, costs, n_chains=n_chains, chain_stride=chain_stride, scalars_steps=scalars_steps, **trace)

    def _fused_steps_done(self, n_steps, last_cost):
        """The chain's bookkeeping after a launch that advanced it by ``n_steps``."""
        cost = self.cost_fun
        self.n_iterations += n_steps
        self._stats_valid = False                 # theta moved without the statistics workspace
        self._grad_decay = float(cost.wdecay / ((self.arena.n + 3e-16) * cost.n_examples))
        self.cost = last_cost

    def _fused_trace_args(self, trace, n_steps, keep_every):
        """What a launch of ``n_steps`` steps that keeps every ``keep_every``-th sample in the ``DeviceTrace`` ``trace``
        passes to ``kernels.bnn_fused_steps``; refuses before anything is drawn or launched."""
        keep_every = int(keep_every)
        if keep_every < 1:
            raise ValueError("fused_bnn_steps: keep_every must be >= 1, not %d" % keep_every)
        a = self.arena
        if trace.n_params != a.n or trace.dtype != self._torch_dtype or trace.device != a.row("theta").device:
            raise ValueError("fused_bnn_steps: the trace holds %s rows of %d on %s, the chain's theta is %s, %d long, on %s" % (
                trace.dtype, trace.n_params, trace.device, self._torch_dtype, a.n, a.row("theta").device))
        if trace.steps_since_kept >= keep_every:
            raise ValueError("fused_bnn_steps: the trace is %d steps past its last kept sample; keep_every = %d cannot "
                             "continue it" % (trace.steps_since_kept, keep_every))
        if len(trace) + trace.kept_rows(n_steps, keep_every) > trace.capacity:
            raise IndexError("DeviceTrace: capacity of %d samples exhausted" % trace.capacity)
        if trace.param_shapes is None:
            trace.describe(self)
        return dict(trace=trace.buffer, trace_every=keep_every, trace_row=len(trace), trace_phase=trace.steps_since_kept)

    def fused_bnn_steps(self, n_steps, trace=None, keep_every=1):
        """Advance the chain by ``n_steps`` complete steps in one launch (one workgroup; see
        ``csrc/sgmcmc_bnn_fused.hip``). Same chain as ``n_steps`` calls of ``next()`` up to the rounding of
        the matrix products (same windows, same Philox stream, same update operator). Returns the
        device tensor of the ``n_steps`` costs.

        The ``n_steps`` stepsizes are drawn from the schedule up front; ``epsilon`` ends as the last one. The schedule's
        ``update(params, cost)`` is not called inside a chunk (nor after it), so a schedule that needs that feedback per
        step has to be stepped with ``next()``.

        ``trace`` (a ``diagnostics.device_trace.DeviceTrace`` as wide as the chain's theta): the launch itself appends theta
        after every ``keep_every``-th step, counted from the trace's last kept sample (``trace.steps_since_kept``), so
        successive chunks thin as one run would. ``IndexError`` before anything is launched if the kept samples do not fit
        the trace's capacity; ``ValueError`` for ``keep_every < 1`` or a trace of another width, dtype or device. The chain
        and the costs are those of the untraced call, bit for bit."""
        if not self.fused_bnn_available():
            raise ValueError("fused_bnn_steps: this sampler/cost/batch generator does not fit the fused small-model kernel")
        n_steps = int(n_steps)
        if trace is not None:
            return self._fused_bnn_steps_traced(n_steps, trace, keep_every)
        eps = self._fused_stepsizes(n_steps)
        starts = torch.as_tensor(self._fused_window_starts(n_steps)).to(self.device)
        costs = torch.empty(n_steps, dtype=self._torch_dtype, device=self.device)
        self._fused_bnn_launch(starts, costs, eps[0], n_steps, scalars_steps=self._fused_scalars_table(eps))
        self._fused_steps_done(n_steps, costs[-1])
        return costs

    def _fused_bnn_steps_traced(self, n_steps, trace, keep_every):
        kw = self._fused_trace_args(trace, n_steps, keep_every)
        eps = self._fused_stepsizes(n_steps)
        starts = torch.as_tensor(self._fused_window_starts(n_steps)).to(self.device)
        costs = torch.empty(n_steps, dtype=self._torch_dtype, device=self.device)
        self._fused_bnn_launch(starts, costs, eps[0], n_steps, scalars_steps=self._fused_scalars_table(eps), **kw)
        trace.advance(n_steps, keep_every)
        self._fused_steps_done(n_steps, costs[-1])
        return costs
