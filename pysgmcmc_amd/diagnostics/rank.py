"""Host statement of the rank-normalised diagnostics (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) that kernel K18
(``include/sgmcmc_hip_rank.h``) and ``diagnostics.rank_diagnostics_all`` compute on the device: numpy and the standard
library only, small inputs, one parameter column at a time. It is what the device path is tested against.

``rank_normalized_chains``  the four transformed arrays of K18 from ``(m, n, P)`` chains, by the header's definitions:
                            integer ``rank2`` (twice the average rank) and the table ``z_of_rank2``
``rank_diagnostics``        split R-hat and variogram ESS of those arrays, with the formulas of
                            ``sampler_diagnostics.gelman_rubin_from_chains`` and ``effective_n`` written out in numpy
"""
import collections
import statistics

import numpy as np

__all__ = ["split_chains", "z_of_rank2", "rank2_of", "tail_order_statistics", "rank_normalized_chains", "rank_diagnostics",
           "RankDiagnostics", "rhat_of", "effective_n_raw"]

_INV_CDF = statistics.NormalDist().inv_cdf          # Wichura's AS241 (PPND16) in double


def split_chains(chains):
    """``(m, n, P)`` (or ``(m, n)``) -> float64 ``(2 m, n // 2, P)``: split chain ``2 c + h`` holds the first (``h = 0``) or the
    last (``h = 1``) ``n // 2`` draws of chain ``c``; for odd ``n`` the middle draw is dropped."""
    x = np.asarray(chains, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError("chains must be (m, n, P) or (m, n), got %s" % (x.shape,))
    m, n, P = x.shape
    if m < 1 or n < 4:
        raise ValueError("rank normalisation needs at least one chain of at least 4 draws, got m = %d, n = %d" % (m, n))
    half = n // 2
    return np.stack([x[:, :half], x[:, n - half:]], axis=1).reshape(2 * m, half, P)


def z_of_rank2(N):
    """Table ``t`` of ``2 N + 1`` doubles with ``t[rank2] = zeta(rank2)`` for ``rank2 = 2 .. 2 N`` (``t[0] = t[1] = NaN``):
    ``Phi^-1((rank2 - 0.75) / (2 N + 0.5))`` for ``rank2 <= N + 1`` and the negated mirror image above, as the header
    states (one rounded division does not make the two halves mirror each other otherwise)."""
    N = int(N)
    D = 2.0 * N + 0.5
    t = np.full(2 * N + 1, np.nan)
    for r in range(2, N + 2):
        t[r] = _INV_CDF((r - 0.75) / D)
    for r in range(N + 2, 2 * N + 1):
        t[r] = -t[2 * N + 2 - r]
    return t


def rank2_of(column):
    """``first + last + 2`` of every element of a one-dimensional array among the sorted array (int64)."""
    v = np.asarray(column, dtype=np.float64).ravel()
    s = np.sort(v)
    return np.searchsorted(s, v, side="left") + np.searchsorted(s, v, side="right") + 1


def tail_order_statistics(N):
    """``(k_lo, k_hi)``: the positions of the order statistics that bound the 5 % tails of ``N`` pooled draws."""
    return (N - 1) // 20, (19 * (N - 1) + 19) // 20


def rank_normalized_chains(chains):
    """``(z, z_folded, tail_lo, tail_hi)``, float64 ``(2 m, n // 2, P)`` each, of ``(m, n, P)`` chains: what K18 writes. A
    column with a NaN or an infinity is NaN in all four."""
    x = split_chains(chains)
    S, half, P = x.shape
    N = S * half
    table = z_of_rank2(N)
    k_lo, k_hi = tail_order_statistics(N)
    outs = [np.empty_like(x) for _ in range(4)]
    for p in range(P):
        v = x[:, :, p].ravel() + 0.0
        if not np.all(np.isfinite(v)):
            for o in outs:
                o[:, :, p] = np.nan
            continue
        s = np.sort(v)
        med = (s[N // 2 - 1] + s[N // 2]) * 0.5
        with np.errstate(over="ignore"):
            folded = np.abs(v - med)
        outs[0][:, :, p] = table[rank2_of(v)].reshape(S, half)
        outs[1][:, :, p] = table[rank2_of(folded)].reshape(S, half)
        outs[2][:, :, p] = (v <= s[k_lo]).astype(np.float64).reshape(S, half)
        outs[3][:, :, p] = (v >= s[k_hi]).astype(np.float64).reshape(S, half)
    return tuple(outs)


def rhat_of(x):
    """Gelman-Rubin ``sqrt(Vhat / W)`` of one ``(m, n)`` array (the formula of ``gelman_rubin_from_chains``); NaN where
    ``Vhat`` is zero or not finite."""
    x = np.asarray(x, dtype=np.float64)
    m, n = x.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        B = n * np.var(x.mean(axis=1), ddof=1) if m > 1 else 0.0
        W = np.mean(np.var(x, axis=1, ddof=1))
        Vhat = W * (n - 1) / n + B / n
        if Vhat == 0.0 or not np.isfinite(Vhat):
            return float("nan")
        return float(np.sqrt(Vhat / W))


def effective_n_raw(x):
    """The variogram estimate of ``effective_n`` before truncation, ``m n / (1 + 2 sum_t rho_t)``, of one ``(m, n)`` array, lag
    by lag; NaN where ``Vhat`` is zero or not finite."""
    x = np.asarray(x, dtype=np.float64)
    m, n = x.shape
    with np.errstate(invalid="ignore"):
        B = n * np.var(x.mean(axis=1), ddof=1) if m > 1 else 0.0
        W = np.mean(np.var(x, axis=1, ddof=1))
        Vhat = W * (n - 1) / n + B / n
    if Vhat == 0.0 or not np.isfinite(Vhat):
        return float("nan")
    rho = np.ones(n)
    negative, t = False, 1
    while not negative and t < n:
        d = x[:, t:] - x[:, :n - t]
        rho[t] = 1.0 - (np.sum(d * d) / (m * (n - t))) / (2.0 * Vhat)
        if not t % 2:
            negative = (rho[t - 1] + rho[t]) < 0
        t += 1
    return float(m * n / (1.0 + 2.0 * rho[1:t].sum()))


RankDiagnostics = collections.namedtuple("RankDiagnostics", [
    "rhat_rank", "ess_bulk", "ess_tail", "rhat_bulk", "rhat_folded", "ess_tail_lo", "ess_tail_hi",
    "raw_bulk", "raw_tail_lo", "raw_tail_hi"])


def _truncated(raw):
    return np.array([int(r) if np.isfinite(r) else 0 for r in raw], dtype=np.int64)


def rank_diagnostics(chains):
    """``RankDiagnostics`` of ``(m, n, P)`` chains, arrays of ``P`` values: ``rhat_rank = max(rhat(z), rhat(z_folded))``,
    ``ess_bulk = ess(z)``, ``ess_tail = min(ess(tail_lo), ess(tail_hi))`` over the ``2 m`` split chains, then the four
    ingredients and the untruncated estimates. A NaN R-hat on either side makes ``rhat_rank`` NaN; a degenerate ESS is 0."""
    z, zf, lo, hi = rank_normalized_chains(chains)
    P = z.shape[2]
    rhat_z = np.array([rhat_of(z[:, :, p]) for p in range(P)])
    rhat_f = np.array([rhat_of(zf[:, :, p]) for p in range(P)])
    raw = [np.array([effective_n_raw(a[:, :, p]) for p in range(P)]) for a in (z, lo, hi)]
    ess = [_truncated(r) for r in raw]
    with np.errstate(invalid="ignore"):
        rhat = np.where(np.isnan(rhat_z) | np.isnan(rhat_f), np.nan, np.maximum(rhat_z, rhat_f))
    return RankDiagnostics(rhat, ess[0], np.minimum(ess[1], ess[2]), rhat_z, rhat_f, ess[1], ess[2], raw[0], raw[1], raw[2])
