"""What ``test_svgd_tile_walk_gpu.py`` rests on, checked without a GPU: every row of its two tables really makes a
workgroup of the named kernel run its tile loop more than once with a ragged last tile, the dispatch line each cap was
read from still holds that cap, and the displacement bar is one the reference itself meets with room to spare (the
narrower oracle against the wider one, at the three cheapest rows).

``python tests/test_svgd_tile_walk.py`` prints, for every update row, how far the narrower oracle is from the wider one in
units of the bar at c = 1: the figures behind ``C`` in the GPU file (two minutes and a few GB: the f64 rows run the oracle
in long double)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import sgmcmc_oracle as O                                                  # noqa: E402
import test_svgd_tile_walk_gpu as W                                                    # noqa: E402

SOURCE = os.path.join(ROOT, "pysgmcmc_amd", "csrc", "sgmcmc_svgd.hip")
LONG_DOUBLE_IS_WIDER = np.finfo(np.longdouble).eps < 2.0 ** -60


def _cost(case):
    """Multiply-adds of the oracle's products; those of an f64 row run in long double, without BLAS (about 3 x)."""
    return case.n * case.n * case.dim * (1 if case.dtype == W.F32 else 3)


CHEAPEST = sorted(W.UPDATE_CASES, key=_cost)[:3]


@pytest.mark.parametrize("case", W.DIST_CASES + W.UPDATE_CASES, ids=W.case_id)
def test_row_walks_with_a_ragged_last_tile(case):
    span = case.cap * case.tile                                     # columns of one round of the capped grid
    assert case.rounds in (1, 3)
    assert case.dim == case.rounds * span + case.tile + 3
    # dim exceeds cap x tile by less than one extra round, or by exactly the two rounds stated plus that
    assert 0 < case.dim - case.rounds * span < span
    n_tiles = -(-case.dim // case.tile)
    assert n_tiles > case.rounds * case.cap and case.dim % case.tile == 3          # some workgroup walks; ragged last tile
    assert case.dim % 2 == 1                                        # pitch = dim takes the element-wise branches
    assert (case.n * (case.dim + 1) + 257) * np.dtype(case.dtype).itemsize < 150e6  # each device buffer: under 150 MB
    if case.kernel.startswith("svgd_sqdist_kernel"):
        assert case.tile == W.sqdist_tile(case.n, np.dtype(case.dtype).itemsize)
    if case.kernel.startswith("svgd_sqdist_small_kernel"):
        cpl = (16 if case.n <= 8 else 8) // np.dtype(case.dtype).itemsize
        assert case.tile == 256 * cpl and case.n <= 12


def test_cited_dispatch_lines_hold_the_caps():
    """The table's caps are literals read from the launch helpers; if the source moves or a cap changes, re-read them."""
    with open(SOURCE) as f:
        lines = f.read().split("\n")
    assert "SVGD_MAX_PARTS = 1024" in lines[49 - 1] and "SVGD_THREADS = 256" in lines[48 - 1]
    assert "SVGD_MT = 128" in lines[764 - 1] and "SVGD_GT64 = 64" in lines[1298 - 1]
    for case in W.DIST_CASES + W.UPDATE_CASES:
        assert case.token in lines[case.line - 1], (
            "csrc/sgmcmc_svgd.hip:%d no longer reads %r (%s): re-read the cap and the tile of %s and bring the row, its dim "
            "and the table in DESIGN.md 3.4 up to date" % (case.line, case.token, lines[case.line - 1].strip(), case.kernel))
    # the dispatch on particle count and dtype that sends each row to its kernel
    by_kernel = {(c.kernel.split("<")[0], c.n, c.dtype) for c in W.DIST_CASES + W.UPDATE_CASES}
    for n, dtype in ((8, W.F32), (3, W.F64), (9, W.F32), (12, W.F64)):
        assert ("svgd_sqdist_small_kernel", n, dtype) in by_kernel
    assert "if (n >= 13)" in lines[1504 - 1] and "if (n <= 8)" in lines[1577 - 1]
    assert "n <= 16" in lines[1482 - 1] and "n <= 32" in lines[1483 - 1] and "n <= 64" in lines[1484 - 1]
    assert "n <= 16" in lines[1491 - 1] and "n <= 32" in lines[1492 - 1] and "n <= 64" in lines[1493 - 1]
    assert "if (n <= 64)" in lines[1590 - 1] and "if (n > 64)" in lines[1619 - 1]


def narrow_against_wide(case):
    """Runs the oracle in the case's dtype and in the next wider one; returns (reference, x_new, h_new of the narrow run)."""
    wide = np.float64 if case.dtype == W.F32 else np.longdouble
    ref = W.step_reference(case, wide)
    Xn, Hn = ref.X.copy(), ref.H.copy()
    O.svgd_step(Xn, ref.G, Hn, W.EPS, W.ALPHA, W.FUDGE, float(case.sign))
    return ref, Xn, Hn


@pytest.mark.parametrize("case", CHEAPEST, ids=W.case_id)
def test_the_oracle_itself_meets_the_bar(case):
    """min K > 1e-4 (no entry of the kernel matrix is compared through atol alone, nothing underflows), and the oracle in
    the row's own precision sits within c / 8 of the displacement bar built from the wider oracle."""
    if case.dtype == W.F64 and not LONG_DOUBLE_IS_WIDER:
        ref = W.step_reference(case)
        assert ref.K.min() > 1e-4
        return
    ref, Xn, Hn = narrow_against_wide(case)
    assert ref.K.min() > 1e-4
    rx, rh = W.bar_units(ref, case.dtype, Xn, Hn)
    print("%s: the %s oracle is %.3f (X), %.3f (H) units of the bar at c = 1 from the wider one" % (
        W.case_id(case), np.dtype(case.dtype).name, rx, rh))
    assert max(rx, rh) <= W.C[case.dtype] / 8
    bar_x, bar_h = W.step_bars(ref, case.dtype, W.C[case.dtype] / 8)
    assert np.all(np.abs((Xn.astype(np.float64) - ref.X.astype(np.float64)) - ref.disp) <= bar_x)
    assert np.all(np.abs(Hn.astype(np.float64) - ref.Hn) <= bar_h)


def test_f32_rows_are_present_among_the_cheapest():
    assert any(c.dtype == W.F32 for c in CHEAPEST)


if __name__ == "__main__":
    assert LONG_DOUBLE_IS_WIDER, "long double is no wider than double here: the f64 rows cannot be measured"
    for case in W.UPDATE_CASES:
        ref, Xn, Hn = narrow_against_wide(case)
        rx, rh = W.bar_units(ref, case.dtype, Xn, Hn)
        bar_1, _ = W.step_bars(ref, case.dtype, 1.0)
        bar_0, _ = W.step_bars(ref, case.dtype, 0.0)
        bar_x, _ = W.step_bars(ref, case.dtype, 8 * max(rx, rh))
        print("%-40s %s  units at c = 1: X %.3f  H %.3f | min K %.2e | median (c u S term at c = 1) / (2 ulp) %.3f | "
              "median bar / |displacement| at c = 8 x that: %.2e" % (
                  W.case_id(case), np.dtype(case.dtype).name, rx, rh, ref.K.min(), np.median((bar_1 - bar_0) / bar_0),
                  np.median(bar_x / np.abs(ref.disp))), flush=True)
