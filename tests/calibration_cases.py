"""Case builders shared by tests/test_calibration.py (host) and tests/test_calibration_gpu.py (device): ensembles of Gaussians
with their held-out targets at the shapes where K20 (include/sgmcmc_hip_calib.h) changes its path, an independent dense
statement of the CRPS, and the measured bounds of the device against the host statement
``diagnostics.calibration.mixture_calibration_host``."""
import functools

import numpy as np

from pysgmcmc_amd.diagnostics.calibration import INV_SQRTPI, SQRT2, mixture_calibration_host, summary_of

# The largest |d| / max(1, |ref|) between K20 on an MI355X and the host statement over every case of
# test_calibration_gpu.py (profiles/calibration.txt). The two sides differ only through the vendor's erf / erfc / exp against
# torch's and numpy's on the host; the tests allow 4 times the measured value, the margin K18 and K19 took for that cause.
PIT_REL_MEASURED = 2.221e-16     # measured 2.220e-16 at S = 3, 67 rows, float32
CRPS_REL_MEASURED = 3.132e-16    # measured 3.131e-16 at S = 1, 67 rows, float64
MARGIN = 4.0
# Derived, not measured: a row's pair sum holds S^2 / 2 terms of order one, so two orders of the same sum differ by about
# S^2 / 2 * eps = 9e-10 at the cap of 4096 draws. A difference above this means another statement or another order of a
# sum, and is a bug, not a bound to widen.
SAME_STATEMENT_LIMIT = 1e-8

# the sizes at which a partial or a tree level is empty, a chain pairing has a middle element, the workgroup size changes
# (128 / 256 / 512 / 1024 / 2048 draws) or the LDS class does (256 / 1024)
DRAWS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 4096)
LEVELS = (0.5, 0.8, 0.9, 0.95)
N_BINS = 10
EPS = np.finfo(np.float64).eps


def rows_for(S):
    return (1, 2) if S >= 4096 else (1, 3, 67)


def ensemble(S, n_rows, seed=0, dtype=np.float64):
    """``(means (S, n_rows) of dtype, var (S,) float64, y (n_rows,) of dtype)``: a trend over the rows, the draws spread
    around it, per-draw variances over a factor of about 20, and targets from well inside the ensemble to eight standard
    deviations outside it (so pit runs from 0 through the middle to 1)."""
    rng = np.random.RandomState(100 * seed + S)
    trend = np.sin(np.linspace(0.0, 3.0, n_rows))
    means = trend[None, :] + 0.4 * rng.randn(S, n_rows)
    var = np.exp(0.75 * rng.randn(S) - 1.5)
    y = trend + rng.randn(n_rows) * np.where(np.arange(n_rows) % 5 == 4, 4.0, 0.5)
    return means.astype(dtype), var, y.astype(dtype)


@functools.lru_cache(maxsize=None)
def reference(S, dtype_name, seed=0):
    """The inputs at the largest row count of ``S`` and the host statement of them, computed once: a run on the leading
    ``n`` rows is compared with the leading ``n`` entries (rows are independent). Treat the arrays as read-only."""
    means, var, y = ensemble(S, max(rows_for(S)), seed, np.dtype(dtype_name))
    ref = mixture_calibration_host(means, var, y)
    return means, var, y, ref


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


def summary(pit, crps, levels=LEVELS, n_bins=N_BINS):
    return summary_of(pit, crps, levels, n_bins)


# ---- independent statements

def dense_crps(means, var, y):
    """The mixture CRPS with the whole ``S x S`` matrix of pairs, every sum in ``np.longdouble``: ``(crps, T / S)``."""
    import math
    mu, var, y = (np.asarray(a, dtype=np.float64) for a in (means, var, y))
    S, n_rows = mu.shape
    erf = np.vectorize(math.erf)

    def A(d, c):
        e = c * SQRT2
        u = d / e
        return (e * (u * erf(u) + np.exp(-(u * u)) * INV_SQRTPI)).astype(np.longdouble)

    crps, first = np.empty(n_rows), np.empty(n_rows)
    c = np.sqrt(var[:, None] + var[None, :])
    for r in range(n_rows):
        m = mu[:, r]
        T = np.sum(A(y[r] - m, np.sqrt(var))) / S
        pairs = np.sum(A(m[:, None] - m[None, :], c))
        crps[r], first[r] = float(T - pairs / (2 * np.longdouble(S) * S)), float(T)
    return crps, first


def gaussian_crps(mu, sd, y):
    """The closed-form CRPS of one Gaussian (Gneiting and Raftery 2007): ``sd (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi))``."""
    from scipy.stats import norm
    z = (y - mu) / sd
    return sd * (z * (2.0 * norm.cdf(z) - 1.0) + 2.0 * norm.pdf(z) - 1.0 / np.sqrt(np.pi))
