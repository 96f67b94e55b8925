"""Kernel Stein discrepancy of device traces and particle sets.

R-hat and ESS measure mixing, lppd and WAIC fit to held-out data; none of them sees the bias of an SG-MCMC chain's
stationary distribution at a finite stepsize. A kernel Stein discrepancy (Gorham & Mackey, *Measuring sample quality with
kernels*; Liu, Lee & Jordan; Chwialkowski, Strathmann & Gretton) does, and needs only the samples ``x_i`` and the scores
``s_i = grad log p(x_i)``. With a base kernel ``k(x, y) = phi(r2)``, ``r2 = |x - y|^2``, the Stein kernel is

    k_p(x_i, x_j) = phi <s_i, s_j> + 2 phi' <s_j - s_i, x_i - x_j> - 2 d phi' - 4 phi'' r2          (phi, phi', phi'' at r2_ij)

and ``V = (1 / n^2) sum_ij k_p`` (the squared discrepancy of the empirical measure, a V-statistic), ``U`` the same over
``i != j`` divided by ``n (n - 1)`` (unbiased, may be negative), ``ksd = sqrt(max(V, 0))``.

  ``kernel_stein_discrepancy``   device tensors or a ``DeviceTrace``: one call of K16 (``kernels.ksd``,
                                 ``include/sgmcmc_hip_ksd.h``), nothing waits for the host; CPU tensors and numpy arrays: the
                                 host statement below
  ``stein_kernel_matrix``        the host statement of K16's arithmetic contract in numpy; the precision of the three
                                 families of sums over the columns is an argument
  ``stein_sums``                 the contract's order of the row sums, the total and the trace
  ``stein_thinning``             greedy Stein thinning (Riabiz et al., *Optimal thinning of MCMC output*): ``m`` of the rows,
                                 picked one at a time to minimise the discrepancy of the picked set. Device inputs: one call
                                 of K16 for the matrix, one of K17 (``kernels.stein_thin``, ``include/sgmcmc_hip_thin.h``)
                                 for the picks; host inputs: the two host statements
  ``stein_thinning_indices``     the host statement of K17's arithmetic contract in numpy

Base kernels: ``"imq"``, ``phi = (c^2 + r2)^beta`` with ``c > 0`` and ``-1 < beta < 0`` (the default ``c = 1``,
``beta = -1/2``: the kernel Gorham & Mackey show to detect non-convergence in more than two dimensions), and ``"rbf"``,
``phi = exp(-r2 / (2 h2))`` with ``h2`` given by the caller as ``bandwidth`` (``kernels.svgd_kernel`` returns one as the third
bandwidth word).
"""
import collections

import numpy as np
import torch

from pysgmcmc_amd import kernels
from pysgmcmc_amd.diagnostics.device_trace import DeviceTrace

__all__ = ["SteinDiscrepancy", "kernel_stein_discrepancy", "stein_kernel_matrix", "stein_sums", "MAX_SAMPLES",
           "SteinThinning", "stein_thinning", "stein_thinning_indices"]

MAX_SAMPLES = 4096            # sgmcmc_ksd_max_samples()
_LANES = 256

SteinDiscrepancy = collections.namedtuple("SteinDiscrepancy", "ksd v_statistic u_statistic row_sums matrix thinning",
                                          defaults=(1,))
SteinDiscrepancy.__doc__ = """``ksd = sqrt(max(V, 0))``, the V- and the U-statistic, the ``n`` row sums of the Stein kernel
matrix, the matrix itself (``return_matrix=True``, else None) and ``thinning``: every ``thinning``-th row of the trace was
used (1 unless an entry above thinned a trace longer than 4096 rows)."""

SteinThinning = collections.namedtuple("SteinThinning", "indices ksd_path v_path discrepancy")
SteinThinning.__doc__ = """``indices``: the ``m`` picked rows in the order they were picked (int32; ``(chains, m)`` and local to
the chain with ``per_chain=True``); ``v_path[t - 1]``: the V-statistic of the first ``t`` picks, ``ksd_path`` its clamped
square root; ``discrepancy``: the ``SteinDiscrepancy`` of the whole set, its ``matrix`` the one the picks were made from."""


def _check_kernel(kernel, c, beta, bandwidth):
    if kernel not in ("imq", "rbf"):
        raise ValueError("stein: kernel must be 'imq' or 'rbf', got %r" % (kernel,))
    if kernel == "imq" and not (c > 0 and -1.0 < beta < 0.0):
        raise ValueError("stein: the IMQ kernel needs c > 0 and -1 < beta < 0, got c = %r, beta = %r" % (c, beta))
    if kernel == "rbf" and (bandwidth is None or not bandwidth > 0):
        raise ValueError("stein: the RBF kernel needs bandwidth = h2 > 0, got %r" % (bandwidth,))


def _column_means(X):
    """Eight interleaved ascending chains over the rows, added in chain order, times 1 / n, in X's dtype."""
    n, d = X.shape
    acc = np.zeros((8, d), dtype=X.dtype)
    for r0 in range(0, n, 8):
        blk = X[r0:r0 + 8]
        acc[:blk.shape[0]] += blk
    m = acc[0].copy()
    for k in range(1, 8):
        m = m + acc[k]
    return m * (X.dtype.type(1) / X.dtype.type(n))


def _mirror(G):
    """The upper triangle of G, mirrored: exactly symmetric."""
    up = np.triu(G)
    return up + np.triu(G, 1).T


def _rounded_once(fn, x):
    """fn(x) in x's dtype. A double goes through long double where that is wider, so that the value is fn's correctly
    rounded one (but for rare double roundings) whatever vectorised pow / exp the CPU would pick for doubles."""
    if x.dtype == np.float64 and np.finfo(np.longdouble).eps < 2.0 ** -60:
        return fn(x.astype(np.longdouble)).astype(np.float64)
    return fn(x)


def _products(Xc, S, order):
    """A = X~ X~^T, B = S S^T, C = S X~^T in the operands' dtype: numpy's matrix product, or column by column."""
    if order == "library":
        return Xc @ Xc.T, S @ S.T, S @ Xc.T
    if order != "k":
        raise ValueError("stein_kernel_matrix: order must be 'library' or 'k', got %r" % (order,))
    n, d = Xc.shape
    A, B, C = (np.zeros((n, n), dtype=Xc.dtype) for _ in range(3))
    for k in range(d):
        x, s = Xc[:, k], S[:, k]
        A += x[:, None] * x[None, :]
        B += s[:, None] * s[None, :]
        C += s[:, None] * x[None, :]
    return A, B, C


def stein_kernel_matrix(samples, scores, kernel="imq", c=1.0, beta=-0.5, bandwidth=None, dtype=np.float64, details=False,
                        order="library"):
    """The ``(n, n)`` Stein kernel matrix of the ``(n, d)`` arrays ``samples`` and ``scores``: the host statement of the
    arithmetic contract of ``include/sgmcmc_hip_ksd.h``.

    The samples are centred per column (the mean in eight interleaved chains); the sums ``A = X~ X~^T``, ``B = S S^T``,
    ``C = S X~^T`` run in ``dtype`` -- ``order="library"``: numpy's matrix product, fast, its order over the columns that of
    the BLAS kernel the CPU picks; ``order="k"``: column by column in ascending order, one rounding per multiply and per add,
    the same bits on every CPU (the contract fixes the matrix cores' own order) --; then, in double (in ``dtype`` where that
    is wider),

        r2_ij = max((A_ii + A_jj) - 2 A_ij, 0)           t_ij = (C_ij + C_ji) - (C_ii + C_jj)
        k_p   = ((phi B_ij + (2 phi') t_ij) - (2 d) phi') - (4 phi'') r2_ij

    every written operation rounded once. ``details=True`` returns ``(k_p, parts)`` with ``parts`` a dict of the pieces
    (``A B C r2 t phi d1 d2 d3``, ``d3 = phi'''``) in the formula's precision."""
    _check_kernel(kernel, c, beta, bandwidth)
    dtype = np.dtype(dtype)
    X = np.ascontiguousarray(np.asarray(samples), dtype=dtype)
    S = np.ascontiguousarray(np.asarray(scores), dtype=dtype)
    if X.ndim != 2 or X.shape != S.shape:
        raise ValueError("stein_kernel_matrix: samples and scores must be (n, d) arrays of one shape")
    n, d = X.shape
    Xc = X - _column_means(X)
    wide = np.result_type(dtype, np.float64)
    A, B, C = _products(Xc, S, order)
    A, B, C = _mirror(A).astype(wide), _mirror(B).astype(wide), C.astype(wide)
    w = wide.type
    dA, dC = np.diag(A), np.diag(C)
    r2 = np.maximum((dA[:, None] + dA[None, :]) - w(2) * A, w(0))
    t = (C + C.T) - (dC[:, None] + dC[None, :])
    if kernel == "imq":
        beta_w = w(beta)
        u = w(c) * w(c) + r2
        phi = w(1) / np.sqrt(u) if beta == -0.5 else _rounded_once(lambda v: np.power(v, v.dtype.type(beta)), u)
        d1 = (beta_w * phi) / u
        d2 = ((beta_w - w(1)) * d1) / u
        d3 = ((beta_w - w(2)) * d2) / u
    else:
        tw = w(2) * w(bandwidth)
        phi = _rounded_once(np.exp, -r2 / tw)
        d1 = -phi / tw
        d2 = -d1 / tw
        d3 = -d2 / tw
    kp = ((phi * B + (w(2) * d1) * t) - (w(2) * w(d)) * d1) - (w(4) * d2) * r2
    if details:
        return kp, dict(A=A, B=B, C=C, r2=r2, t=t, phi=phi, d1=d1, d2=d2, d3=d3)
    return kp


def _lane_tree(values):
    """Sum of a vector as the contract orders it: lane t of 256 adds the elements t, t + 256, ... ascending, the lane sums are
    added by a halving tree."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    pad = (-v.size) % _LANES
    rows = np.concatenate([v, np.zeros(pad)]).reshape(-1, _LANES)
    red = np.zeros(_LANES)
    for row in rows:
        red = red + row
    off = _LANES // 2
    while off > 0:
        red[:off] = red[:off] + red[off:2 * off]
        off //= 2
    return float(red[0])


def stein_sums(matrix):
    """``(row_sums, total, trace)`` of a Stein kernel matrix in the contract's order, in double: each row by
    256 interleaved ascending lane sums and a halving tree, ``total`` over the row sums and ``trace`` over the diagonal by the
    same scheme."""
    K = np.asarray(matrix, dtype=np.float64)
    n = K.shape[0]
    pad = (-n) % _LANES
    Kp = np.concatenate([K, np.zeros((n, pad))], axis=1).reshape(n, -1, _LANES)
    red = np.zeros((n, _LANES))
    for k in range(Kp.shape[1]):
        red = red + Kp[:, k, :]
    off = _LANES // 2
    while off > 0:
        red[:, :off] = red[:, :off] + red[:, off:2 * off]
        off //= 2
    rows = red[:, 0].copy()
    return rows, _lane_tree(rows), _lane_tree(np.diag(K))


def _statistics(total, trace, n):
    nd = float(n)
    return total / (nd * nd), (total - trace) / (nd * (nd - 1.0))


def _as_matrix(a, what):
    """(n, d) or (chains, n, d) -> (chains * n, d)"""
    if isinstance(a, DeviceTrace):
        a = a.values()
    if not torch.is_tensor(a):
        a = np.asarray(a)
    if a.ndim == 3:
        a = a.reshape(-1, a.shape[-1])
    if a.ndim != 2:
        raise ValueError("kernel_stein_discrepancy: %s must be (n, d) or (chains, n, d), got %s" % (what, tuple(a.shape)))
    return a


def kernel_stein_discrepancy(samples, scores, kernel="imq", c=1.0, beta=-0.5, bandwidth=None, return_matrix=False,
                             workspace=None):
    """Kernel Stein discrepancy of ``samples`` with the scores ``scores = grad log p(samples)``: a ``SteinDiscrepancy``.

    ``samples`` / ``scores``: ``(n, d)`` or ``(chains, n, d)`` tensors (flattened over the chains) or a ``DeviceTrace``;
    2 .. 4096 rows in all, else ``ValueError`` -- thin a longer trace. Device tensors of float32 / float64 go to K16 in ONE
    call (``kernels.ksd``) and every field is a float64 device tensor (``matrix`` in the samples' dtype); nothing waits for
    the host. ``workspace``: one from ``kernels.ksd_workspace(n, samples)`` to reuse, else allocated. CPU tensors and numpy
    arrays take the host statement ``stein_kernel_matrix`` in double. ``bandwidth`` is the RBF kernel's ``h2``."""
    _check_kernel(kernel, c, beta, bandwidth)
    X, S = _as_matrix(samples, "samples"), _as_matrix(scores, "scores")
    if tuple(X.shape) != tuple(S.shape):
        raise ValueError("kernel_stein_discrepancy: samples %s and scores %s differ in shape" % (tuple(X.shape), tuple(S.shape)))
    n = int(X.shape[0])
    if n > MAX_SAMPLES:
        raise ValueError("kernel_stein_discrepancy: %d samples, the limit is %d per call: thin the trace (every k-th row)"
                         % (n, MAX_SAMPLES))
    if n < 2:
        raise ValueError("kernel_stein_discrepancy: needs at least 2 samples, got %d" % n)
    if torch.is_tensor(X) and X.is_cuda:
        if not torch.is_tensor(S) or S.device != X.device or S.dtype != X.dtype:
            raise TypeError("kernel_stein_discrepancy: scores must be a %s tensor on %s" % (X.dtype, X.device))
        X, S = (t if (t.shape[1] < 2 or t.stride(1) == 1) and t.stride(0) >= t.shape[1] else t.contiguous() for t in (X, S))
        if workspace is None:
            workspace = kernels.ksd_workspace(n, X)
        matrix = torch.empty((n, n), dtype=X.dtype, device=X.device) if return_matrix else None
        rows = torch.empty(n, dtype=torch.float64, device=X.device)
        stats = kernels.ksd(X, S, workspace, kind=kernel, c=c, beta=beta, h2=bandwidth, matrix=matrix, row_sums=rows)
        return SteinDiscrepancy(torch.sqrt(torch.clamp(stats[0], min=0.0)), stats[0], stats[1], rows, matrix)
    as_torch = torch.is_tensor(X)
    Xn, Sn = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (X, S))
    K = stein_kernel_matrix(Xn, Sn, kernel, c, beta, bandwidth, dtype=np.float64)
    rows, total, trace = stein_sums(K)
    v, u = _statistics(total, trace, n)
    out = (np.sqrt(max(v, 0.0)), v, u, rows, K if return_matrix else None)
    if as_torch:
        out = tuple(None if o is None else torch.as_tensor(o, dtype=torch.float64) for o in out)
    return SteinDiscrepancy(*out)


def stein_thinning_indices(matrix, m, distinct=False):
    """Greedy Stein thinning of the ``(n, n)`` Stein kernel matrix ``matrix``: ``(indices, path)``, ``m`` int32 row numbers in
    the order they are picked and the float64 V-statistic of the first ``t`` picks. The host statement of the arithmetic
    contract of ``include/sgmcmc_hip_thin.h``, in double, every written operation rounded once:

        h_j = 0.5 K_jj,  acc_j = 0,  S = 0;  for t = 1 .. m:
            obj_j = acc_j + h_j;   j* = the candidate with the smallest obj_j, among equal values the smallest j
            S = S + 2 obj_j*;   indices[t - 1] = j*;   path[t - 1] = S / (t t);   acc_j = acc_j + K[j*][j]  (row j*)

    Every row is a candidate at every step; with ``distinct`` a picked row is not a candidate again (``m <= n``)."""
    K = np.asarray(matrix)
    if K.ndim != 2 or K.shape[0] != K.shape[1] or K.shape[0] < 2:
        raise ValueError("stein_thinning_indices: matrix must be (n, n) with n >= 2, got %s" % (tuple(K.shape),))
    n, m = K.shape[0], int(m)
    if m < 1:
        raise ValueError("stein_thinning_indices: m must be at least 1, got %d" % m)
    if distinct and m > n:
        raise ValueError("stein_thinning_indices: distinct picks need m <= n, got m = %d, n = %d" % (m, n))
    h = 0.5 * np.diag(K).astype(np.float64)
    acc = np.zeros(n)
    free = np.ones(n, dtype=bool)
    indices, path = np.empty(m, dtype=np.int32), np.empty(m)
    S = 0.0
    for t in range(1, m + 1):
        obj = acc + h
        if distinct:
            cand = np.flatnonzero(free)
            j = int(cand[np.argmin(obj[cand])])                  # argmin: the first of equal values
            free[j] = False
        else:
            j = int(np.argmin(obj))
        S = S + 2.0 * float(obj[j])
        indices[t - 1], path[t - 1] = j, S / (float(t) * float(t))
        acc = acc + K[j].astype(np.float64)
    return indices, path


def _as_chains(a, what):
    if isinstance(a, DeviceTrace):
        a = a.values()
    if not torch.is_tensor(a):
        a = np.asarray(a)
    if a.ndim != 3:
        raise ValueError("stein_thinning: per_chain=True needs %s as (chains, n, d), got %s" % (what, tuple(a.shape)))
    return int(a.shape[0]), int(a.shape[1])


def stein_thinning(samples, scores, m, kernel="imq", c=1.0, beta=-0.5, bandwidth=None, distinct=False, per_chain=False,
                   workspace=None):
    """Greedy Stein thinning of ``samples`` with the scores ``scores = grad log p(samples)``: a ``SteinThinning`` of the ``m``
    rows that, picked one at a time, keep the kernel Stein discrepancy of the picked set smallest -- the small ensemble to
    predict with, instead of every k-th row.

    ``samples`` / ``scores``, the kernel arguments and ``workspace`` are those of ``kernel_stein_discrepancy``: ``(n, d)`` or
    ``(chains, n, d)`` or a ``DeviceTrace``, 2 .. 4096 rows in all, else ``ValueError``. ``per_chain=False`` pools the rows:
    ``indices`` is ``(m,)`` into the flattened rows. ``per_chain=True`` needs the three-dimensional form and thins each chain
    on its own diagonal block of the one pooled matrix: ``indices`` and the paths are ``(chains, m)``, the indices local to
    the chain. ``distinct``: no row is picked twice (``m`` at most the rows of a problem); without it a row may repeat, which
    weights it.

    Device tensors: one K16 call with ``return_matrix=True``, then one K17 call (``kernels.stein_thin``); every field is a
    device tensor and nothing waits for the host. CPU tensors and numpy arrays: ``stein_kernel_matrix`` and
    ``stein_thinning_indices`` in double. The particles of an SVGD sampler go through unchanged:
    ``stein_thinning(sampler.particles, models.bnn_posterior_scores(sampler.particles, ...), m)``."""
    m = int(m)
    if m < 1:
        raise ValueError("stein_thinning: m must be at least 1, got %d" % m)
    chains, rows = (_as_chains(samples, "samples") if per_chain else (1, None))
    if per_chain and _as_chains(scores, "scores") != (chains, rows):
        raise ValueError("stein_thinning: samples and scores differ in shape")
    disc = kernel_stein_discrepancy(samples, scores, kernel, c, beta, bandwidth, return_matrix=True, workspace=workspace)
    K = disc.matrix
    n = int(K.shape[0]) if rows is None else rows
    if n < 2:
        raise ValueError("stein_thinning: a chain needs at least 2 rows, got %d" % n)
    if distinct and m > n:
        raise ValueError("stein_thinning: distinct picks need m <= %d rows, got m = %d" % (n, m))
    if torch.is_tensor(K) and K.is_cuda:
        idx, v = kernels.stein_thin(K, m, distinct=distinct, n=n, batch=chains, batch_stride=n * int(K.stride(0)) + n)
        if per_chain:
            idx, v = idx.view(chains, m), v.view(chains, m)
        return SteinThinning(idx, torch.sqrt(torch.clamp(v, min=0.0)), v, disc)
    Kn = K.numpy() if torch.is_tensor(K) else K
    parts = [stein_thinning_indices(Kn[p * n:(p + 1) * n, p * n:(p + 1) * n], m, distinct) for p in range(chains)]
    idx, v = (np.stack([p[k] for p in parts]) if per_chain else parts[0][k] for k in (0, 1))
    out = (idx, np.sqrt(np.maximum(v, 0.0)), v)
    if torch.is_tensor(K):
        out = tuple(torch.as_tensor(o) for o in out)
    return SteinThinning(*out, disc)
