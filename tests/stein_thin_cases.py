"""Sizes, matrices and samples shared by ``test_stein_thin.py`` (no GPU) and ``test_stein_thin_gpu.py``: the cases of the Stein
thinning kernel K17 (include/sgmcmc_hip_thin.h, csrc/sgmcmc_stein_thin.hip) and of its host statement
``diagnostics.stein.stein_thinning_indices``."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64

# every block size (64, 256, 1024 threads) and every columns-per-thread count (1 .. 4) of sgmcmc_stein_thin_plan, on each side
# of the wave edge (63 | 64 | 65), the block edges (255 | 256 | 257, 1023 | 1024 | 1025) and the column-count edges
SIZES = (2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3073, 4096)
M_SHORT = 24                     # picks of the table's cases: m = min(n, 24)
REPEAT_N = (65, 1025)            # also m = 3 n: rows repeat
DISTINCT_N = (64, 257, 4096)     # also DISTINCT with m = n, in f32

# the two biased-Gaussian cases: (n, d, m)
GAUSS = ((300, 7, 40), (1000, 20, 100))

# tied columns of the n = 4096 tie matrices: a pair inside a wave, across a wave edge, across the waves of a block, across
# the block edge (two slots of one thread's neighbour), two slots of ONE thread, and one column in each of the four slots
TIES = ((0, 63), (63, 64), (64, 1023), (1023, 1024), (1024, 2048), (5, 1029, 2053, 3077))
TIE_N = 4096


def seed_of(n, dtype):
    return 1000 * n + np.dtype(dtype).itemsize


@functools.lru_cache(maxsize=None)
def matrix(n, dtype):
    """Random symmetric: K = G G^T + a positive diagonal with G (n, 8) standard normal, cast to ``dtype`` and mirrored from
    the upper triangle, so the f32 matrix is itself exactly symmetric. Read-only: shared by the tests."""
    rng = np.random.default_rng(seed_of(n, dtype))
    G = rng.standard_normal((n, 8))
    K = G @ G.T + np.diag(rng.uniform(0.5, 2.0, size=n))
    K = K.astype(dtype)
    K = np.triu(K) + np.triu(K, 1).T
    K.setflags(write=False)
    return K


def biased(rng, n, d):
    """A biased Gaussian sample: X = 1.3 z + 0.3 against a standard normal target, scores -X."""
    X = 1.3 * rng.standard_normal((n, d)) + 0.3
    return X, -X


@functools.lru_cache(maxsize=None)
def _gauss_samples():
    rng = np.random.default_rng(0)                   # ONE generator, the cases drawn in the order of GAUSS
    return {(n, d): biased(rng, n, d) for n, d, _ in GAUSS}


def gauss(n, d):
    """The samples and scores of a case of GAUSS (copies)."""
    X, S = _gauss_samples()[(n, d)]
    return X.copy(), S.copy()


def tie_matrix(cols, dtype, n=TIE_N):
    """Integer-valued symmetric matrix whose columns ``cols`` are identical (rows too) and win every step: their objective is
    1 + 2 t after t picks among them, every other column's at least 500, so the tied columns tie exactly at every step."""
    rng = np.random.default_rng(len(cols) * 100003 + cols[-1])
    K = rng.integers(3, 7, size=(n, n)).astype(dtype)
    K = np.triu(K) + np.triu(K, 1).T
    K[np.arange(n), np.arange(n)] = 1000 + 2 * rng.integers(0, 50, size=n)
    cols = list(cols)
    K[:, cols] = 3
    K[cols, :] = 3
    K[np.ix_(cols, cols)] = 2
    return K


# The refusals of sgmcmc_stein_thin_*, in the order of the header's list: (what is wrong, the text). Each entry overrides
# valid arguments with n = 8, m = 4, batch = 2 and ld_m = 8.
REFUSALS = [
    (dict(matrix=None), b"stein_thin: null pointer"),
    (dict(n=1), b"stein_thin: n = 1 outside [2, 4096]"),
    (dict(m=0), b"stein_thin: m = 0 outside [1, 65536]"),
    (dict(batch=0), b"stein_thin: batch = 0 outside [1, 65535]"),
    (dict(ld_m=7), b"stein_thin: ld_m < n"),
    (dict(batch_stride=0), b"stein_thin: batch > 1 needs batch_stride > 0"),
    (dict(flags=3), b"stein_thin: unknown flag bits 0x2"),
    (dict(flags=1, m=9), b"stein_thin: DISTINCT needs m <= n, got m = 9, n = 8"),
]
