"""Case builders shared by tests/test_psis_loo.py (host) and tests/test_psis_loo_gpu.py (device): columns of pointwise log
densities that reach every branch of the PSIS statement (include/sgmcmc_hip_psis.h), and the measured bounds of the device
against the host statement ``diagnostics.psis.psis_loo_host``."""
import math

import numpy as np

from pysgmcmc_amd.diagnostics import psis

# The largest difference between K19 on an MI355X and the host statement over every case of test_psis_loo_gpu.py
# (profiles/psis_loo.txt): khat absolute, the other two |d| / max(1, |ref|). The two sides differ only through the vendor's
# exp / log / log1p / expm1 against numpy's; the tests allow 4 times the measured value, the margin K18 took for that cause.
KHAT_ABS_MEASURED = 6.883e-15    # measured 6.883e-15 at S = 1000, 67 columns, r_eff = 0.3
ELPD_REL_MEASURED = 4.878e-15    # measured 4.878e-15 at S = 1000, 67 columns, r_eff = 0.3
LOGW_REL_MEASURED = 1.013e-14    # measured 1.013e-14 at S = 1000, 67 columns, r_eff = 0.3
MARGIN = 4.0
# |L_j| is at most a few thousand, so exp(L_t - L_j) rounds at the order of 1e-12: a difference above this means the two
# sides execute different statements or a different sum order, and is a bug, not a bound to widen.
SAME_STATEMENT_LIMIT = 1e-9

DRAWS = (2, 5, 16, 24, 25, 26, 63, 64, 65, 100, 255, 256, 257, 1000, 4096, 8192)
R_EFFS = (1.0, 0.3, 2.5)
LOG_2PI = math.log(2.0 * math.pi)


def rows_for(S):
    return (1, 3, 5) if S >= 4096 else (1, 3, 67)


def gaussian(S, rng):
    """Gaussian log densities of one observation under S draws of the mean."""
    mu = 0.3 + 0.4 * rng.randn(S)
    return -0.5 * LOG_2PI - 0.5 * (1.1 - mu) ** 2


def pareto_ratios(S, rng, k=0.9):
    """Log-ratios with a generalised Pareto tail of shape k: l = -log r."""
    u = rng.uniform(size=S)
    r = np.expm1(-k * np.log1p(-u)) / k                  # the GPD quantile function
    return -np.log(np.maximum(r, 1e-300))


def every_value_twice(S, rng):
    v = np.repeat(rng.randn((S + 1) // 2), 2)[:S]
    return v[rng.permutation(S)]


def few_above(S):
    """How many draws the tie and underflow columns put above the cut: below M for every r_eff in R_EFFS once S >= 25."""
    return max(1, int(math.sqrt(S)))


def ties_at_cut(S, rng, above=None):
    """`above` distinct large log-ratios, then a block of equal ones that spans the cut, then smaller ones: the tail is the
    `above` draws alone, n_tail < M."""
    above = few_above(S) if above is None else above
    above = min(above, S - 1)
    block = min(S - above, max(1, S // 2))
    lr = np.concatenate([1.0 + np.sort(rng.uniform(0.5, 3.0, size=above)), np.full(block, 1.0),
                         rng.uniform(-2.0, 0.5, size=S - above - block)])
    return -lr[rng.permutation(S)]


def constant(S, rng):
    return np.full(S, -1.25)


def underflow(S, rng):
    """lw spans more than 745: all but a few draws lie below log(DBL_MIN), so the cut is that constant."""
    above = min(few_above(S), S - 1)
    lr = np.concatenate([rng.uniform(-600.0, 0.0, size=above), rng.uniform(-1500.0, -800.0, size=S - above)])
    lr[0] = 0.0
    return -lr[rng.permutation(S)]


PATTERNS = (gaussian, pareto_ratios, every_value_twice, ties_at_cut, constant, underflow)


def matrix(S, n_rows, seed=0, first=0):
    """(S, n_rows): column r holds pattern (first + r) % len(PATTERNS), every column from a generator of its own."""
    out = np.empty((S, n_rows))
    for r in range(n_rows):
        rng = np.random.RandomState(1000 * seed + 7 * S + r)
        out[:, r] = PATTERNS[(first + r) % len(PATTERNS)](S, rng)
    return out


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def rel_or_abs(got, ref):
    """The largest |d| / max(1, |ref|) over the finite entries of ref (0.0 when there is none)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))))


def compare(got, ref):
    """The exact assertions of one result against the host statement; returns the three measured differences (khat
    absolute, elpd_loo and log_weights relative-or-absolute). `got` and `ref`: dicts with elpd_loo, khat, n_tail, and
    optionally log_weights."""
    assert np.array_equal(got["n_tail"], ref["n_tail"]), "n_tail differs: %s against %s" % (got["n_tail"], ref["n_tail"])
    bad = ref["n_tail"] < 0
    inf = np.isposinf(ref["khat"])
    assert np.array_equal(np.isposinf(got["khat"]), inf), "khat = +inf in other rows than on the host"
    assert np.array_equal(np.isnan(got["khat"]), np.isnan(ref["khat"])), "khat is NaN in other rows than on the host"
    assert np.array_equal(np.isnan(got["elpd_loo"]), bad), "elpd_loo is NaN in other rows than the non-finite columns"
    fin = np.isfinite(ref["khat"])
    d_khat = float(np.max(np.abs(got["khat"][fin] - ref["khat"][fin]))) if fin.any() else 0.0
    d_elpd = rel_or_abs(got["elpd_loo"], ref["elpd_loo"])
    d_logw = 0.0
    if got.get("log_weights") is not None:
        assert np.array_equal(np.isnan(got["log_weights"]), np.isnan(ref["log_weights"])), "NaN weights are misplaced"
        d_logw = rel_or_abs(got["log_weights"], ref["log_weights"])
    return d_khat, d_elpd, d_logw


def host(ll, r_eff=1.0):
    return psis.psis_loo_host(ll, r_eff)
