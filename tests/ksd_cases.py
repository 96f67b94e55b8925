"""Cases, inputs and bars of the kernel Stein discrepancy kernel K16 (include/sgmcmc_hip_ksd.h, csrc/sgmcmc_ksd.hip), shared by
``test_ksd.py`` (no GPU) and ``test_ksd_gpu.py``.

``python tests/ksd_cases.py`` prints, for every case of the table, how far the host statement
``diagnostics.stein.stein_kernel_matrix`` with its three sums in the case's own precision is from the statement in the next
wider one (f64 for f32, 80-bit long double for f64), in units of the entrywise bar at C = 1: the figures behind ``C`` below."""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pysgmcmc_amd.diagnostics.stein import stein_kernel_matrix, stein_sums            # noqa: E402

F32, F64 = np.float32, np.float64
LONG_DOUBLE_IS_WIDER = np.finfo(np.longdouble).eps < 2.0 ** -60
MEAN, GRAM, REDUCE, PAIR, FINISH = 1, 2, 3, 4, 5        # launch ids of the header
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}                  # unit roundoff of T

# (n, d): why
TABLE = [
    (2, 1),         # smallest
    (63, 5),        # one short of a block edge
    (64, 64),       # exact block and tile edges
    (65, 67),       # one past both, ragged
    (129, 40),      # three blocks: diagonal and off-diagonal pairs
    (257, 3),       # one past a block edge (and past one round of the 256 lanes of a row sum)
]
# the base kernels: the default IMQ (1 / sqrt), an IMQ with another exponent (pow) and the RBF kernel with h2 = 1 (the
# samples are N(0, 1 / d) per coordinate, so r2 is about 2)
KERNELS = collections.OrderedDict([
    ("imq", dict(kernel="imq", c=1.0, beta=-0.5)),
    ("imq_pow", dict(kernel="imq", c=0.7, beta=-0.25)),
    ("rbf", dict(kernel="rbf", bandwidth=1.0)),
])
# GRAM is the only launch whose capped grid walks over dim. The walk cases sit at  cap * tile + tile + 3  columns with cap
# and tile read from ksd_plan: at 2 samples (one block pair, cap 512) and at 257 (15 pairs, cap 34)
WALK_N = (2, 257)
# MEAN and GRAM run once per phase of 65 536 columns, GRAM from the second phase on starting from its own partial blocks: one
# case with a second, ragged phase of one tile and three columns
PHASE_COLS = 65536
PHASE_N = 129
# above 31 blocks there are more block pairs than the 512 workgroups the splits are capped for: the cap clamps at 1 and one
# workgroup per pair walks every tile (33 blocks, 561 pairs)
CLAMP_CASES = [(2049, 35)]


def walk_dim(plan):
    """Smallest ragged dim at which the capped GRAM grid of ``plan`` walks: cap * tile + tile + 3."""
    gram = [l for l in plan if l.id == GRAM]
    assert len(gram) == 1 and gram[0].cap > 0 and gram[0].tile > 0
    return gram[0].cap * gram[0].tile + gram[0].tile + 3


def _like(dtype):
    import torch
    return torch.float32 if dtype == F32 else torch.float64


def walk_cases(dtype):
    """[(n, d)] of the walk cases in ``dtype`` (numpy type); needs the built library, not a GPU."""
    from pysgmcmc_amd import _lib, kernels
    _lib.build()                                  # the table is read at collection time: compile the library if it is stale
    return [(n, walk_dim(kernels.ksd_plan(n, 1, _like(dtype)))) for n in WALK_N]


def phase_cases(dtype):
    """[(n, d)]: two phases, the second a full GRAM tile plus three columns"""
    from pysgmcmc_amd import _lib, kernels
    _lib.build()
    tile = [l for l in kernels.ksd_plan(PHASE_N, 1, _like(dtype)) if l.id == GRAM][0].tile
    return [(PHASE_N, PHASE_COLS + tile + 3)]


def inputs(n, d, dtype):
    """X = 0.3 + N(0, 1) / sqrt(d), S ~ N(0, 1), from default_rng([n, d, itemsize])"""
    rng = np.random.default_rng([n, d, np.dtype(dtype).itemsize])
    X = (0.3 + rng.normal(size=(n, d)) / np.sqrt(d)).astype(dtype)
    S = rng.normal(size=(n, d)).astype(dtype)
    return X, S


Reference = collections.namedtuple("Reference", "X S K M rows total trace v u")
_refs = {}


def magnitude(parts, d):
    """The first-order magnitude M_ij of k_p's error per unit of relative error in the sums, from the fp64 pieces:
    phi |s_i| |s_j| + 2 |phi'| (|s_i| + |s_j|) (|x~_i| + |x~_j|) + |dk_p / dr2| (|x~_i| + |x~_j|)^2."""
    sn, xn = np.sqrt(np.diag(parts["B"])), np.sqrt(np.diag(parts["A"]))
    ss, xx = sn[:, None] + sn[None, :], xn[:, None] + xn[None, :]
    dk = parts["d1"] * parts["B"] + 2 * parts["d2"] * parts["t"] - (2 * d + 4) * parts["d2"] - 4 * parts["d3"] * parts["r2"]
    return parts["phi"] * sn[:, None] * sn[None, :] + 2 * np.abs(parts["d1"]) * ss * xx + np.abs(dk) * xx * xx


def reference(n, d, dtype, kern):
    """The fp64 host statement on the f32 / f64 inputs and the magnitudes of the bar; computed once, never modified."""
    key = (n, d, np.dtype(dtype).name, kern)
    if key not in _refs:
        X, S = inputs(n, d, dtype)
        K, parts = stein_kernel_matrix(X, S, dtype=F64, details=True, **KERNELS[kern])
        M = magnitude(parts, d)
        rows, total, trace = stein_sums(K)
        for a in (X, S, K, M, rows):
            a.setflags(write=False)
        _refs[key] = Reference(X, S, K, M, rows, total, trace, total / (float(n) * n), (total - trace) / (float(n) * (n - 1)))
    return _refs[key]


def units(K, ref, dtype):
    """max |K - ref| / (u_T M): the entrywise distance in units of the bar at C = 1"""
    diff = np.abs(np.asarray(K).astype(np.longdouble) - ref.K.astype(np.longdouble))
    return float(np.max(diff / (U[dtype] * ref.M)))


def sum_bars(ref, dtype):
    """(row sums, V, U) bars at C = 1: the entrywise bar summed over the entries of each sum"""
    n = ref.M.shape[0]
    rows = U[dtype] * ref.M.sum(axis=1)
    off = ref.M.sum() - np.trace(ref.M)
    return rows, U[dtype] * ref.M.sum() / (float(n) * n), U[dtype] * off / (float(n) * (n - 1))


def narrow_against_wide(n, d, dtype, kern):
    """Units of the bar at C = 1 of the host statement with its sums in ``dtype`` against the next wider precision, both
    column by column (``order="k"``): the figures do not depend on the BLAS kernel a CPU picks."""
    wide = F64 if dtype == F32 else np.longdouble
    ref = reference(n, d, dtype, kern)
    narrow = stein_kernel_matrix(ref.X, ref.S, dtype=dtype, order="k", **KERNELS[kern])
    wider = stein_kernel_matrix(ref.X, ref.S, dtype=wide, order="k", **KERNELS[kern])
    diff = np.abs(narrow.astype(np.longdouble) - wider.astype(np.longdouble))
    return float(np.max(diff / (U[dtype] * ref.M)))


# |k_p - ref_ij| <= C u_T M_ij, C = 8 x the largest figure, in these units, that the HOST STATEMENT ITSELF makes over TABLE
# and KERNELS with its three sums in the case's own precision, column by column (the margin svgd_many_cases.py gives a
# matrix-core order over the oracle's). Measured on the CPU (imq, imq_pow, rbf):
ORACLE_UNITS = {
    (2, 1, 'float32'): (0.068, 0.077, 0.077),
    (63, 5, 'float32'): (1.356, 1.589, 0.881),
    (64, 64, 'float32'): (1.509, 1.866, 1.463),
    (65, 67, 'float32'): (1.134, 1.361, 1.463),
    (129, 40, 'float32'): (1.430, 1.633, 1.377),
    (257, 3, 'float32'): (1.238, 1.361, 1.193),
    (2, 1, 'float64'): (1.712, 1.277, 0.760),
    (63, 5, 'float64'): (1.573, 2.365, 1.806),
    (64, 64, 'float64'): (1.649, 1.976, 1.981),
    (65, 67, 'float64'): (1.578, 1.500, 2.010),
    (129, 40, 'float64'): (1.543, 1.867, 1.659),
    (257, 3, 'float64'): (2.450, 5.536, 3.168),
}
# the worst row of each dtype (n, d, kernel) and its figure; test_ksd.py recomputes it
WORST = {F32: ((64, 64, "imq_pow"), 1.866), F64: ((257, 3, "imq_pow"), 5.536)}
C = {F32: 8 * WORST[F32][1], F64: 8 * WORST[F64][1]}

if __name__ == "__main__":
    assert LONG_DOUBLE_IS_WIDER, "long double is no wider than double here: the f64 rows cannot be measured"
    for dtype in (F32, F64):
        worst = (None, 0.0)
        for n, d in TABLE:
            row = [narrow_against_wide(n, d, dtype, kern) for kern in KERNELS]
            for kern, r in zip(KERNELS, row):
                if r > worst[1]:
                    worst = ((n, d, kern), r)
            print("    (%d, %d, %r): (%.3f, %.3f, %.3f)," % ((n, d, np.dtype(dtype).name) + tuple(row)), flush=True)
        print("worst %s: %r %.3f" % (np.dtype(dtype).name, worst[0], worst[1]))
