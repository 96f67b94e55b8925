"""Posterior predictive of a small tanh-MLP BNN from device-resident traces, in one device call.

The reference's ``predict`` (``pysgmcmc/models/bayesian_neural_network.py:560-630``) evaluates the kept networks one by one
and reduces on the host. Here the samples stay where ``FusedBNNChains.collect`` / ``DeviceTrace.record`` left them:
``posterior_predictive`` hands the trace to K11 (``kernels.bnn_predict``, ``include/sgmcmc_hip_predict.h``), which runs every
sampled network at every test row out of the LDS and reduces over the samples on the device. ``predictive_gradients`` hands
it to K14 (``kernels.bnn_predict_grad``, ``include/sgmcmc_hip_predict_grad.h``), which adds the backward sweep to the inputs:
the gradients of the predictive mean and variance that an acquisition function is climbed with. Nothing here waits for the host.
"""
import collections

import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd.diagnostics.device_trace import _chain_matrices

__all__ = ["posterior_predictive", "predictive_gradients", "PredictiveGradients"]

PredictiveGradients = collections.namedtuple("PredictiveGradients", "mean var dmean dvar")
PredictiveGradients.__doc__ = """What :func:`predictive_gradients` returns, float64 device tensors: ``mean`` and ``var``
``(N,)``, the ensemble moments of :func:`posterior_predictive`; ``dmean`` and ``dvar`` ``(N, D0)``, their derivatives with
respect to the inputs, ``dmean[r, d] = d mean[r] / d X[r, d]``."""


def _trace_arguments(what, traces, X, layer_sizes, *targets):
    """The refusals ``posterior_predictive`` and ``heldout_score`` share, before the library is reached: ``(chains, sizes,
    first, S, N)`` -- what goes down to the kernel binding, the layer sizes, the first chain matrix, the number of samples and
    of test rows. ``targets``: nothing, or ``y``, which must then be ``(N,)`` of the traces' dtype and device."""
    chains = traces
    if not (torch.is_tensor(traces) and traces.dim() == 3):
        chains = _chain_matrices(traces)
        if len(chains) > 64:
            raise ValueError(what + ": at most 64 separate chains, got %d (stack them into one (m, n, P) "
                             "tensor)" % len(chains))
    mats = [chains] if torch.is_tensor(chains) else chains
    first = mats[0]
    sizes = [int(v) for v in layer_sizes]
    if len(sizes) < 2:
        raise ValueError(what + ": layer_sizes must name the inputs and at least one layer")
    n_params = kernels._bnn_n_params(sizes)
    if int(first.shape[-1]) < n_params:
        raise ValueError(what + ": the traces are %d wide, layer sizes %s need %d parameters" % (
            first.shape[-1], sizes, n_params))
    if not torch.is_tensor(X) or X.dim() != 2 or int(X.shape[1]) != sizes[0]:
        raise ValueError(what + ": X must be an (N, %d) tensor, got %s" % (
            sizes[0], tuple(X.shape) if torch.is_tensor(X) else type(X).__name__))
    if targets:
        y, N = targets[0], int(X.shape[0])
        if not torch.is_tensor(y) or tuple(y.shape) != (N,):
            raise ValueError(what + ": y must be an (N,) = (%d,) tensor, got %s" % (
                N, tuple(y.shape) if torch.is_tensor(y) else type(y).__name__))
        if y.dtype != first.dtype or y.device != first.device:
            raise TypeError(what + ": y must be a %s tensor on %s, got %s on %s" % (first.dtype, first.device, y.dtype, y.device))
    for x in mats:
        if not x.is_cuda:
            raise TypeError(what + ": the traces live on %s; they must be device tensors" % x.device)
        if x.dtype != first.dtype or x.device != first.device:
            raise TypeError(what + ": the traces must share a dtype and a device")
    if X.dtype != first.dtype or X.device != first.device:
        raise TypeError(what + ": X must be a %s tensor on %s" % (first.dtype, first.device))
    S = first.shape[0] * first.shape[1] if first.dim() == 3 else len(mats) * first.shape[0]
    if int(S) == 0:
        raise ValueError(what + ": the traces hold no samples")
    return chains, sizes, first, int(S), int(X.shape[0])


def posterior_predictive(traces, X, layer_sizes, return_individual_predictions=False):
    """Predictive moments at the rows of ``X`` of the networks sampled in ``traces``.

    ``traces``: what ``diagnostics.effective_n_all`` accepts -- a ``DeviceTrace``, a sequence of them (at most 64), or a
    device tensor ``(n, P)`` / ``(m, n, P)`` -- whose rows are flat parameter vectors in the whole-step kernel's order
    (``W1, b1, ..., WL, bL, log_var``). A 3-D tensor whose chains lie back to back goes down as one matrix, whatever ``m``.
    ``X``: contiguous ``(N, layer_sizes[0])`` device tensor of the traces' dtype, already normalised. ``layer_sizes``: ``[inputs,
    hidden..., 1]``, 1 to 8 weight layers.

    Returns device tensors, ``S`` = the number of samples: by default ``(ens_mean, ens_var)``, float64 ``(N,)``, the mean
    over the samples of the networks' outputs and their population variance; with ``return_individual_predictions``
    ``(means, noise_var)`` of the traces' dtype, ``(S, N)`` and ``(S,)``: every network's output at every row and its
    ``exp(log_var)``. Allocates its outputs and nothing else. ``ValueError`` / ``TypeError`` for traces on the host, of
    mismatched widths, narrower than the layer sizes need, or an ``X`` that does not fit them; a net the kernel refuses
    (its parameters do not fit the LDS) raises ``SgmcmcLibraryError``."""
    chains, sizes, first, S, N = _trace_arguments("posterior_predictive", traces, X, layer_sizes)
    dev = first.device
    means = torch.empty(S, N, dtype=first.dtype, device=dev)
    if return_individual_predictions:
        noise_var = torch.empty(S, dtype=first.dtype, device=dev)
        kernels.bnn_predict(chains, sizes, X, means, noise_var=noise_var)
        return means, noise_var
    ens_mean = torch.empty(N, dtype=torch.float64, device=dev)
    ens_var = torch.empty(N, dtype=torch.float64, device=dev)
    kernels.bnn_predict(chains, sizes, X, means, ens_mean=ens_mean, ens_var=ens_var)
    return ens_mean, ens_var


def predictive_gradients(traces, X, layer_sizes, return_individual=False, scratch_bytes=1 << 30):
    """Predictive moments at the rows of ``X`` of the networks sampled in ``traces`` AND their gradients with respect to
    those rows: what a Bayesian-optimisation loop needs to climb an acquisition function (K14, ``kernels.bnn_predict_grad``,
    ``include/sgmcmc_hip_predict_grad.h``).

    ``traces``, ``X``, ``layer_sizes``: what :func:`posterior_predictive` accepts, refused alike; ``D0 = layer_sizes[0]``.

    Returns device tensors, ``S`` = the number of samples: by default :class:`PredictiveGradients` ``(mean, var, dmean,
    dvar)``, float64, ``(N,), (N,), (N, D0), (N, D0)``: the mean over the samples of the networks' outputs, their population
    variance, and the derivatives of both with respect to ``X[r, d]``; with ``return_individual`` ``(means, grads)`` of the
    traces' dtype, ``(S, N)`` and ``(S, N, D0)``: every network's output at every row and its input gradient.

    The per-network gradients are ``S * N * D0`` elements. The default path therefore walks ``X`` in chunks of rows that keep
    the ``means`` and ``grads`` of one chunk within ``scratch_bytes`` (at least one row per chunk) and reuses that scratch
    from chunk to chunk on the stream; rows are independent, so the result has the same bits whatever the chunking. Nothing
    here waits for the host."""
    chains, sizes, first, S, N = _trace_arguments("predictive_gradients", traces, X, layer_sizes)
    dev, dt, D0 = first.device, first.dtype, sizes[0]
    if return_individual:
        means = torch.empty(S, N, dtype=dt, device=dev)
        grads = torch.empty(S, N, D0, dtype=dt, device=dev)
        kernels.bnn_predict_grad(chains, sizes, X, means, grads)
        return means, grads
    f64 = torch.float64
    out = PredictiveGradients(torch.empty(N, dtype=f64, device=dev), torch.empty(N, dtype=f64, device=dev),
                              torch.empty(N, D0, dtype=f64, device=dev), torch.empty(N, D0, dtype=f64, device=dev))
    per_row = S * (1 + D0) * first.element_size()
    rows = max(1, min(N, int(scratch_bytes) // per_row))
    scratch = torch.empty(S * rows * (1 + D0), dtype=dt, device=dev)
    for lo in range(0, N, rows):
        k = min(rows, N - lo)
        kernels.bnn_predict_grad(chains, sizes, X[lo:lo + k], scratch[:S * k], scratch[S * rows:S * rows + S * k * D0],
                                 *(t[lo:lo + k] for t in out))
    return out
