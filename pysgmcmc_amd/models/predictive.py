"""Posterior predictive of a small tanh-MLP BNN from device-resident traces, in one device call.

The reference's ``predict`` (``pysgmcmc/models/bayesian_neural_network.py:560-630``) evaluates the kept networks one by one
and reduces on the host. Here the samples stay where ``FusedBNNChains.collect`` / ``DeviceTrace.record`` left them:
``posterior_predictive`` hands the trace to K11 (``kernels.bnn_predict``, ``include/sgmcmc_hip_predict.h``), which runs every
sampled network at every test row out of the LDS and reduces over the samples on the device. Nothing here waits for the host.
"""
import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd.diagnostics.device_trace import _chain_matrices

__all__ = ["posterior_predictive"]


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
