"""Scores of the BNN posterior at the rows of a trace or a particle matrix, without autograd.

``bnn_posterior_scores`` returns ``grad_theta log p(theta | X, y)`` for every row of an ``(n, P)`` matrix: what a kernel
Stein discrepancy (``diagnostics.stein``) needs next to the samples. The BNN cost is ``-log p / N`` when the whole data set
is the minibatch and ``batch_size = n_examples = N``, so the score is ``-N`` times its parameter gradient, which kernel K15
(``kernels.bnn_particles_cost_grad``) gives for all rows in one launch per chunk of data rows.
"""
import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd.data_batches import Placeholder
from pysgmcmc_amd.models.particles import BNNParticleCost

__all__ = ("bnn_posterior_scores", "bnn_scores_chunk_rows")


def bnn_scores_chunk_rows(layer_sizes, n_rows, dtype, max_rows=None):
    """Data rows per K15 launch of ``bnn_posterior_scores``: the largest batch ``kernels.bnn_particles_lds_bytes`` accepts for
    this net and dtype, at most ``n_rows``, at most ``max_rows`` if given; 0 when K15 refuses the net."""
    sizes = [int(v) for v in layer_sizes]
    if dtype not in (torch.float32, torch.float64) or len(sizes) < 2 or len(sizes) - 1 > 8 or sizes[-1] != 1:
        return 0
    if kernels.bnn_particles_lds_bytes(sizes, 1, dtype) <= 0:
        return 0
    lo, hi = 1, int(n_rows)                                    # the footprint grows with the batch: bisect
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if kernels.bnn_particles_lds_bytes(sizes, mid, dtype) > 0:
            lo = mid
        else:
            hi = mid - 1
    return lo if max_rows is None else max(1, min(lo, int(max_rows)))


def _rows(samples):
    """(n, P) or (chains, n, P) -> an (n, P) matrix with dense rows (a view where the layout allows it)"""
    if samples.dim() == 3:
        samples = samples.reshape(-1, samples.shape[-1])
    if samples.dim() != 2:
        raise ValueError("bnn_posterior_scores: samples must be (n, P) or (chains, n, P), got %s" % (tuple(samples.shape),))
    if (samples.shape[1] > 1 and samples.stride(1) != 1) or (samples.shape[0] > 1 and samples.stride(0) < samples.shape[1]):
        samples = samples.contiguous()
    return samples


def bnn_posterior_scores(samples, layer_sizes, X, y, wdecay=1.0, prior_mean=1e-6, prior_var=0.01, out=None, max_rows=None):
    """``grad_theta log p(theta | X, y)`` of the MLP BNN ``layer_sizes`` for every row of ``samples``: an ``(n, P)`` or
    ``(chains, n, P)`` matrix of flat parameter vectors in trace-row order, at any row pitch. Returns ``(n, P)`` (the chains
    flattened) in the samples' dtype; ``out``: a contiguous ``(n, P)`` tensor to write into.

    On the device K15 runs once per chunk of data rows (``bnn_scores_chunk_rows``; ``max_rows`` caps the chunk), the first
    chunk with the weight prior and the others without, every chunk with ``batch_size = n_examples = N``; the chunk gradients
    are added in ascending order. K15 counts the derivative of the log-variance prior once per call, so it is taken off the
    ``log_var`` column ``chunks - 1`` times by the torch statement of that term; one multiply by ``-N`` ends it. Nothing waits
    for the host. On the CPU, and for a net K15 refuses, ``BNNParticleCost.__call__`` runs under autograd row by row."""
    sizes = [int(v) for v in layer_sizes]
    theta = _rows(samples)
    n, P = int(theta.shape[0]), int(theta.shape[1])
    X = torch.as_tensor(X, dtype=theta.dtype, device=theta.device) if not torch.is_tensor(X) else X
    y = torch.as_tensor(y, dtype=theta.dtype, device=theta.device) if not torch.is_tensor(y) else y
    X = X.reshape(X.shape[0], -1)
    y = y.reshape(-1)
    N = int(X.shape[0])
    if X.dtype != theta.dtype or y.dtype != theta.dtype or X.device != theta.device or y.device != theta.device:
        raise TypeError("bnn_posterior_scores: X and y must be %s tensors on %s" % (theta.dtype, theta.device))
    if y.numel() != N or N < 1:
        raise ValueError("bnn_posterior_scores: y must hold the %d targets of X" % N)
    xp, yp = Placeholder(), Placeholder()
    cost = BNNParticleCost(sizes, xp, yp, N, N, wdecay=wdecay, prior_mean=prior_mean, prior_var=prior_var)
    if P != cost.n_params:
        raise ValueError("bnn_posterior_scores: the rows are %d wide, the net %r has %d parameters" % (P, sizes, cost.n_params))
    if out is None:
        out = torch.empty((n, P), dtype=theta.dtype, device=theta.device)
    elif tuple(out.shape) != (n, P) or out.dtype != theta.dtype or out.device != theta.device or not out.is_contiguous():
        raise ValueError("bnn_posterior_scores: out must be a contiguous (%d, %d) %s tensor on %s"
                         % (n, P, theta.dtype, theta.device))
    chunk = bnn_scores_chunk_rows(sizes, N, theta.dtype, max_rows) if theta.is_cuda else 0
    if chunk == 0:
        xp.value, yp.value = X, y
        for i in range(n):
            row = theta[i].detach().clone().requires_grad_(True)
            (g,) = torch.autograd.grad(cost(row), row)
            out[i] = g * (-float(N))
        return out
    if n == 0:
        return out
    ld = int(theta.stride(0)) if n > 1 else P
    flat = torch.as_strided(theta, ((n - 1) * ld + P,), (1,), theta.storage_offset())
    costs = torch.empty(n, dtype=theta.dtype, device=theta.device)
    X = X if X.shape[1] < 2 or X.stride(1) == 1 else X.contiguous()
    y = y.contiguous()
    part = None
    chunks = 0
    for r0 in range(0, N, chunk):
        first = r0 == 0
        if not first and part is None:
            part = torch.empty_like(out)
        dst = out if first else part
        kernels.bnn_particles_cost_grad(flat, n, ld, sizes, X[r0:r0 + chunk], y[r0:r0 + chunk], dst.reshape(-1), P, costs,
                                        N, N, wdecay, prior_mean, prior_var, add_prior=first)
        if not first:
            out += part
        chunks += 1
    if chunks > 1:
        # d / d log_var of  -lvp / n_examples,  lvp = -(log_var - log(prior_mean))^2 / lvp_den - ...  (BNNParticleCost.__call__)
        ln_mean, lvp_den, _, _ = cost._constants(theta.dtype, theta.device)
        log_var = theta[:, P - 1]
        out[:, P - 1] -= float(chunks - 1) * ((2.0 * (log_var - ln_mean) / lvp_den) / N)
    out *= -float(N)
    return out
