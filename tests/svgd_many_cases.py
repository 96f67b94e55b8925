"""Cases, inputs and bars of the many-particle SVGD path (include/sgmcmc_hip_svgd_many.h, csrc/sgmcmc_svgd_many.hip), shared
by ``test_svgd_many.py`` (no GPU) and ``test_svgd_many_gpu.py``.

``python tests/svgd_many_cases.py`` prints, for every step case, how far the oracle in the case's own precision is from the
oracle in the next wider one (f64 for f32, 80-bit long double for f64) in units of the displacement bar at c = 1: the figures
behind ``C`` below (about a minute)."""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import sgmcmc_oracle as O                                                  # noqa: E402
import test_svgd_tile_walk_gpu as W                                                    # noqa: E402  (step_reference, step_bars, bar_units)

F32, F64 = np.float32, np.float64
EPS, ALPHA, FUDGE = W.EPS, W.ALPHA, W.FUDGE
TOL = W.TOL                                   # K and the bandwidth words: the bars of test_svgd_gpu.py
SWEEP_RTOL = W.SWEEP_RTOL
LONG_DOUBLE_IS_WIDER = np.finfo(np.longdouble).eps < 2.0 ** -60
GRAM, UPDATE, MEAN = 1, 8, 11                 # launch ids of the header

# (n, d): why
TABLE = [
    (129, 1),       # first n above the register-resident path; n * n odd; one column
    (129, 40),
    (130, 64),      # n * n even; exact tile edge
    (161, 257),     # ragged in both directions
    (257, 3),       # one past a block edge
    (512, 70),
    (1024, 3),      # the limit
    (1024, 65),     # the limit; one column past a tile edge
]
# GRAM is the only launch whose capped grid walks over dim (UPDATE, KGRAD: one workgroup per 16 columns, no cap; SELECT and
# NEXT stride over the n * n keys, eight per lane from 46 particles on, so every case above walks them). The walk cases sit
# at  cap * tile + tile + 3  columns with cap and tile read from svgd_many_plan: at 129 particles (cap 85: 5507 columns in
# f32, 2755 in f64) and at 1024 (cap 3: 259 and 131). The dispatch picks no other instantiation at a larger n; the second row
# is there because the cap itself depends on n. All are far below 64 MB of particles.
WALK_N = (129, 1024)
# MEAN and GRAM run once per phase of 65 536 columns, GRAM from the second phase on starting from its own partial blocks:
# one case with a second, ragged phase of one tile and three columns (34 MB of particles in f32, 68 MB in f64)
PHASE_COLS = 65536

Case = collections.namedtuple("Case", "n dim dtype sign")


def walk_dim(plan):
    """Smallest ragged dim at which the capped GRAM grid of ``plan`` walks: cap * tile + tile + 3."""
    gram = [l for l in plan if l.id == GRAM]
    assert len(gram) == 1 and gram[0].cap > 0 and gram[0].tile > 0
    return gram[0].cap * gram[0].tile + gram[0].tile + 3


def walk_cases(dtype):
    """[(n, d)] of the walk cases in ``dtype`` (numpy type); needs the built library, not a GPU."""
    import torch
    from pysgmcmc_amd import _lib, kernels
    _lib.build()                                  # the table is read at collection time: compile the library if it is stale
    like = torch.float32 if dtype == F32 else torch.float64
    return [(n, walk_dim(kernels.svgd_many_plan(n, 1, like))) for n in WALK_N]


def phase_cases(dtype):
    """[(n, d)]: two phases, the second a full GRAM tile plus three columns"""
    return [(129, PHASE_COLS + (64 if dtype == F32 else 32) + 3)]


def cloud(n, d, dtype, seed=0, offset=0.0, scale=1.0):
    """``_cloud`` of test_svgd_gpu.py"""
    rng = np.random.default_rng(seed)
    return (offset + scale * rng.normal(size=(n, d))).astype(dtype)


def kernel_inputs(n, d, dtype):
    return cloud(n, d, dtype, seed=n * 1000 + d, scale=1.0 / np.sqrt(d))


_kernel_refs = {}


def kernel_reference(n, d, dtype):
    """(X, K, kernel gradients, h, median) of the f64 oracle on the f32 / f64 inputs; computed once, never modified."""
    key = (n, d, np.dtype(dtype).name)
    if key not in _kernel_refs:
        X = kernel_inputs(n, d, dtype)
        K, kg, h, D = O.svgd_kernel(X.astype(np.float64))
        for a in (X, K, kg):
            a.setflags(write=False)
        _kernel_refs[key] = (X, K, kg, float(h), float(O.svgd_median(D)))
    return _kernel_refs[key]


_step_refs = {}


def step_reference(case, wide=np.float64):
    """``W.step_reference`` (inputs: X = 0.3 + N(0,1)/sqrt(d), G ~ N(0,1), H ~ U(0.05,1) from default_rng([n, d, itemsize]))
    once per case."""
    key = (case, np.dtype(wide).name)
    if key not in _step_refs:
        ref = W.step_reference(case, wide)
        for a in ref:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _step_refs[key] = ref
    return _step_refs[key]


def narrow_against_wide(case):
    """Units of the bar at c = 1 (X, H) of the oracle in the case's dtype against the oracle in the next wider one."""
    wide = np.float64 if case.dtype == F32 else np.longdouble
    ref = W.step_reference(case, wide)
    Xn, Hn = ref.X.copy(), ref.H.copy()
    O.svgd_step(Xn, ref.G, Hn, EPS, ALPHA, FUDGE, float(case.sign))
    return W.bar_units(ref, case.dtype, Xn, Hn)


# The displacement bar of test_svgd_tile_walk_gpu.py:  bar_X = eps J (c u S) + 2 ulp(x_new),  bar_H = 2 (1 - alpha) |gt|
# (c u S) + 2 ulp(h_new),  c = 8 x the largest error, in units of the bar at c = 1, that the ORACLE ITSELF makes over TABLE
# with both signs. Measured on the CPU (X, H), sign +1 | sign -1:
ORACLE_UNITS = {
    (129, 1, "float32"): (0.590, 0.552, 0.614, 0.560),
    (129, 40, "float32"): (1.093, 0.648, 1.005, 0.647),
    (130, 64, "float32"): (1.028, 0.647, 1.013, 0.649),
    (161, 257, "float32"): (0.319, 0.649, 0.291, 0.650),
    (257, 3, "float32"): (0.919, 0.634, 1.068, 0.644),
    (512, 70, "float32"): (3.503, 0.650, 3.912, 0.650),
    (1024, 3, "float32"): (1.157, 0.660, 1.892, 0.674),
    (1024, 65, "float32"): (2.331, 0.650, 2.551, 0.650),
    (129, 1, "float64"): (0.416, 0.809, 0.380, 0.573),
    (129, 40, "float64"): (1.741, 0.500, 2.463, 0.500),
    (130, 64, "float64"): (3.624, 0.500, 2.715, 0.500),
    (161, 257, "float64"): (0.311, 0.500, 0.323, 0.500),
    (257, 3, "float64"): (0.539, 0.500, 0.703, 0.500),
    (512, 70, "float64"): (0.670, 0.500, 1.137, 0.500),
    (1024, 3, "float64"): (0.905, 0.500, 1.873, 0.500),
    (1024, 65, "float64"): (4.484, 0.500, 2.765, 0.500),
}
# the worst row of each dtype (n, d, sign) and its figure; test_svgd_many.py recomputes it
WORST = {F32: ((512, 70, -1), 3.912), F64: ((1024, 65, 1), 4.484)}
C = {F32: 8 * 3.912, F64: 8 * 4.484}

if __name__ == "__main__":
    assert LONG_DOUBLE_IS_WIDER, "long double is no wider than double here: the f64 rows cannot be measured"
    for dtype in (F32, F64):
        worst = (None, 0.0)
        for n, d in TABLE:
            row = []
            for sign in (1, -1):
                rx, rh = narrow_against_wide(Case(n, d, dtype, sign))
                row += [rx, rh]
                if max(rx, rh) > worst[1]:
                    worst = ((n, d, sign), max(rx, rh))
            print("    (%4d, %3d, %r): (%.3f, %.3f, %.3f, %.3f)," % ((n, d, np.dtype(dtype).name) + tuple(row)), flush=True)
        print("worst %s: %r %.3f" % (np.dtype(dtype).name, worst[0], worst[1]))
