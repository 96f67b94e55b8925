"""Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO): the host statement, in numpy.

``psis_loo_host`` states in numpy float64 what kernel K19 (``include/sgmcmc_hip_psis.h``) computes on the device, operation
by operation and with the same order of every sum, so the two differ only through ``exp``, ``log``, ``log1p``, ``expm1`` and
``sqrt``; ``M``, ``n_tail``, the tail's membership and ``khat = +inf`` are exact. The algorithm is that of Vehtari, Gelman
and Gabry (2017) and Vehtari, Simpson, Gelman, Yao and Gabry (2024), with the generalised Pareto fit of Zhang and Stephens
(2009), as the ``loo`` package and ArviZ state it.

This module needs no GPU and no native library to import. ``psis_loo`` at its end is the device route.
"""
import numpy as np

__all__ = ["LOG_DBL_MIN", "MAX_DRAWS", "fixed_sum", "tail_length", "gpd_fit", "psis_column", "psis_loo_host"]

LOG_DBL_MIN = float.fromhex("-0x1.6232bdd7abcd2p+9")     # log(DBL_MIN), the constant the kernel carries
MAX_DRAWS = 8192                                          # SGMCMC_PSIS_MAX_DRAWS
_PARTS = 256


def fixed_sum(v, axis=-1):
    """The project's fixed-order sum along ``axis``: 256 partials, partial ``j`` adds the elements ``j, j + 256, ...``
    ascending from 0.0, then the halving tree ``h = 128 .. 1``. (A partial is never -0.0, so the zero padding adds nothing.)"""
    v = np.moveaxis(np.asarray(v, dtype=np.float64), axis, 0)
    n = v.shape[0]
    blocks = max(1, -(-n // _PARTS))
    padded = np.zeros((blocks * _PARTS,) + v.shape[1:])
    padded[:n] = v
    padded = padded.reshape((blocks, _PARTS) + v.shape[1:])
    part = np.zeros((_PARTS,) + v.shape[1:])
    for block in padded:
        part = part + block
    h = _PARTS // 2
    while h >= 1:
        part = part[:h] + part[h:2 * h]
        h //= 2
    return part[0]


def _logsumexp(v):
    m = np.max(v)
    return m + np.log(fixed_sum(np.exp(v - m)))


def tail_length(S, r_eff=1.0):
    """``M = min(ceil(0.2 S), ceil(3 sqrt(S / r_eff)))`` clamped to ``1 .. S - 1``, in double."""
    with np.errstate(over="ignore", divide="ignore"):
        m = min(np.ceil(0.2 * np.float64(S)), np.ceil(3.0 * np.sqrt(np.float64(S) / np.float64(r_eff))))
    return int(min(max(m, 1.0), float(S - 1)))


def _gpd_fit(x):
    """``(khat, sigma)`` of ascending ``x``, nothing checked: step 5 of the header."""
    n = x.shape[0]
    dn = float(n)
    root = 0
    while (root + 1) * (root + 1) <= n:
        root += 1
    G = 30 + root
    q = int(np.floor(dn / 4.0 + 0.5)) - 1
    with np.errstate(all="ignore"):
        j = np.arange(1, G + 1, dtype=np.float64)
        b = (1.0 - np.sqrt(float(G) / (j - 0.5))) / (3.0 * x[q]) + 1.0 / x[n - 1]
        k = fixed_sum(np.log1p((-b)[:, None] * x[None, :]), axis=1) / dn
        L = dn * ((np.log(-(b / k)) - k) - 1.0)
        w = 1.0 / fixed_sum(np.exp(L[None, :] - L[:, None]), axis=1)
        w[w < 10.0 * np.finfo(np.float64).eps] = 0.0
        w = w / fixed_sum(w)
        bb = fixed_sum(b * w)
        kk = fixed_sum(np.log1p((-bb) * x)) / dn
        sigma = -kk / bb
        khat = (dn * kk + 5.0) / (dn + 10.0)
    return float(khat), float(sigma)


def gpd_fit(x):
    """The generalised Pareto fit of Zhang and Stephens with the weakly informative prior on the shape that ``loo`` and
    ArviZ use: ``(khat, sigma)`` of the ascending positive excesses ``x`` (at least 5)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.shape[0] < 5:
        raise ValueError("gpd_fit: needs at least 5 values, got %d" % x.shape[0])
    if np.any(np.diff(x) < 0):
        raise ValueError("gpd_fit: x must be ascending")
    return _gpd_fit(x)


def psis_column(l, M):
    """One column: ``(lwn, khat, n_tail, elpd_loo, row_lppd)`` of the finite log densities ``l`` with the tail length ``M``."""
    S = l.shape[0]
    with np.errstate(all="ignore"):
        # 9. K13's statement: the terms added one by one in draw order
        m = np.max(l)
        Z = np.cumsum(np.exp(l - m))[-1]
        row_lppd = (m + np.log(Z)) - np.log(np.float64(S))
        # 1. - 3.
        lr = -l
        lw = lr - np.max(lr)
        order = np.argsort(lw, kind="stable")             # the strict total order (value, draw index)
        s = lw[order]
        cut = max(s[S - M - 1], LOG_DBL_MIN)
        tail = order[s > cut]
        n = tail.shape[0]
        khat = np.inf
        # 4. and 5.
        if n > 4:
            ec = np.exp(cut)
            x = np.exp(lw[tail]) - ec
            khat, sigma = _gpd_fit(x)
            if np.isfinite(khat):
                t1 = np.log1p(-((np.arange(n, dtype=np.float64) + 0.5) / float(n)))
                y = (-sigma) * t1 if khat == 0.0 else sigma * np.expm1((-khat) * t1) / khat
                lw = lw.copy()
                lw[tail] = np.log(y + ec)
        # 6. - 8.
        lw = np.minimum(lw, 0.0)
        lwn = lw - _logsumexp(lw)
        elpd = _logsumexp(lwn + l)
    return lwn, float(khat), n, float(elpd), float(row_lppd)


def psis_loo_host(loglik, r_eff=1.0):
    """PSIS-LOO of every column of the ``(S, n_rows)`` pointwise log densities ``loglik``.

    Returns a dict of arrays: ``elpd_loo``, ``khat``, ``row_lppd`` float64 ``(n_rows,)``, ``n_tail`` int32 ``(n_rows,)``,
    ``log_weights`` float64 ``(S, n_rows)`` (the normalised smoothed log weights), ``summary`` float64 ``(4,)`` = ``{sum
    elpd_loo, sum row_lppd, rows with khat > 0.7, rows holding a NaN or an infinity}`` in the fixed order, and ``M``. A column
    that holds a NaN or an infinity gets NaN and ``n_tail = -1``."""
    loglik = np.asarray(loglik, dtype=np.float64)
    if loglik.ndim != 2:
        raise ValueError("psis_loo: loglik must be (S, n_rows), got %s" % (tuple(loglik.shape),))
    S, n_rows = loglik.shape
    if S < 2 or S > MAX_DRAWS:
        raise ValueError("psis_loo: S = %d draws, must be 2 .. %d" % (S, MAX_DRAWS))
    if not (r_eff > 0.0 and np.isfinite(r_eff)):
        raise ValueError("psis_loo: r_eff = %g, must be a positive finite number" % r_eff)
    M = tail_length(S, r_eff)
    elpd, khat, lppd = (np.full(n_rows, np.nan) for _ in range(3))
    n_tail = np.full(n_rows, -1, dtype=np.int32)
    logw = np.full((S, n_rows), np.nan)
    for r in range(n_rows):
        col = np.ascontiguousarray(loglik[:, r])
        if not np.all(np.isfinite(col)):
            continue
        logw[:, r], khat[r], n_tail[r], elpd[r], lppd[r] = psis_column(col, M)
    with np.errstate(invalid="ignore"):
        summary = np.array([fixed_sum(elpd), fixed_sum(lppd), fixed_sum((khat > 0.7).astype(np.float64)),
                            fixed_sum((n_tail < 0).astype(np.float64))])
    return dict(elpd_loo=elpd, khat=khat, n_tail=n_tail, row_lppd=lppd, log_weights=logw, summary=summary, M=M)


def _psis_loo_type():
    import collections
    fields = ["elpd_loo", "p_loo", "se", "lppd", "row_elpd", "row_lppd", "khat", "n_tail", "n_bad", "log_weights", "thinning"]
    t = collections.namedtuple("PsisLoo", fields, defaults=(1,))
    t.__doc__ = """What :func:`psis_loo` returns, all device tensors; the scalars are 0-d float64.

``elpd_loo``: the sum over the observations of ``row_elpd``. ``lppd``: the sum of ``row_lppd``. ``p_loo = lppd - elpd_loo``.
``se = sqrt(n_rows * population variance of row_elpd)``. ``row_elpd``, ``row_lppd``, ``khat``: float64 ``(n_rows,)``;
``n_tail``: int32 ``(n_rows,)``, -1 where the column held a NaN or an infinity. ``n_bad``: the number of rows with ``khat >
0.7`` (``+inf`` where the tail had at most 4 draws), whose estimate is not to be trusted. ``log_weights``: float64 ``(S,
n_rows)`` or None. ``thinning``: the stride with which the draws were taken (1: all of them)."""
    return t


PsisLoo = _psis_loo_type()
__all__ += ["PsisLoo", "psis_loo"]


def psis_loo(loglik, r_eff=1.0, weights=False):
    """PSIS-LOO of the float64 ``(S, n_rows)`` device tensor ``loglik`` (``models.heldout_score(..., pointwise=True).loglik``)
    by kernel K19 (``kernels.psis_loo``): a :class:`PsisLoo` of device tensors. ``weights=True`` also returns the normalised
    smoothed log weights. Nothing waits for the host; there is no CPU route (``psis_loo_host`` is the host statement)."""
    import torch

    from pysgmcmc_amd import kernels
    if not torch.is_tensor(loglik) or loglik.dim() != 2:
        raise ValueError("psis_loo: loglik must be an (S, n_rows) device tensor")
    S, n_rows = (int(v) for v in loglik.shape)
    if n_rows == 0:
        raise ValueError("psis_loo: loglik holds no observations")
    dev, f64 = loglik.device, torch.float64
    row_lppd = torch.empty(n_rows, dtype=f64, device=dev)
    summary = torch.empty(4, dtype=f64, device=dev)
    log_weights = torch.empty(S, n_rows, dtype=f64, device=dev) if weights else None
    row_elpd, khat, n_tail = kernels.psis_loo(loglik, r_eff, row_lppd=row_lppd, log_weights=log_weights, summary=summary)
    se = torch.sqrt(n_rows * torch.var(row_elpd, unbiased=False))
    return PsisLoo(elpd_loo=summary[0], p_loo=summary[1] - summary[0], se=se, lppd=summary[1], row_elpd=row_elpd,
                   row_lppd=row_lppd, khat=khat, n_tail=n_tail, n_bad=summary[2], log_weights=log_weights)
