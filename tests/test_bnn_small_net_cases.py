"""The case table of tests/small_net_cases.py without a GPU: the library's row tiles equal the table at every net and element
size, refusals included; the table (with ``predict_grad_cases.NETS``) reaches every tile, the LDS ceiling, every footprint class
and both loop forms, as CONDITIONS; the restated LDS regions are aligned, disjoint and end at the stated byte count; the grid
rule; and the two restatements the GPU tests bound the kernels with stay within the bars on their own. What the kernels compute
at these nets is checked on the GPU (tests/test_bnn_small_net_tiles_gpu.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import predict_grad_cases as C
import small_net_cases as N
from pysgmcmc_amd import _lib, kernels

EINVAL = -1
DT = {4: torch.float32, 8: torch.float64}
CELLS = [(kernel, esize) for kernel in N.KERNELS for esize in N.ESIZES]


def _row_tile(kernel, sizes, esize):
    lib = _lib.lib()
    rc = getattr(lib, N.ENTRY[kernel])((ctypes.c_int * len(sizes))(*sizes), len(sizes) - 1, esize)
    return rc, lib.sgmcmc_last_error()


def test_the_table_names_fifteen_nets_beyond_the_pinned_five():
    assert len(N.NETS) == len(set(map(tuple, N.NETS))) == 15
    assert not set(map(tuple, N.NETS)) & set(map(tuple, C.NETS))
    for sizes in N.NETS:
        assert 2 <= len(sizes) <= 9 and sizes[-1] == 1 and min(sizes) >= 1


@pytest.mark.parametrize("sizes", N.NETS, ids=N.NET_IDS)
def test_the_library_s_row_tiles_equal_the_table(sizes):
    for kernel, esize in CELLS:
        cell = N.table_cell(sizes, kernel, esize)
        rc, msg = _row_tile(kernel, sizes, esize)
        plan = N.plan(sizes, kernel, esize)
        if cell is None:
            assert plan is None, (kernel, esize, plan)
            assert rc == EINVAL and msg.startswith(N.WHAT[kernel]), (kernel, esize, rc, msg)
            assert N.refusal(sizes, esize, kernel) in msg, (kernel, esize, msg)
            binding = kernels.bnn_predict_row_tile if kernel == N.K11 else kernels.bnn_predict_grad_row_tile
            with pytest.raises(_lib.SgmcmcLibraryError, match="160 KiB"):
                binding(sizes, DT[esize])
        else:
            assert rc == cell[0], (kernel, esize, rc, cell, msg)
            assert plan is not None and (plan["tile"], plan["bytes"]) == cell, (kernel, esize, plan, cell)
            assert N.refusal(sizes, esize, kernel) is None
    # K14's restatement rests on predict_grad_cases' rule
    for esize in N.ESIZES:
        cell = N.table_cell(sizes, N.K14, esize)
        assert C.row_tile_rule(sizes, esize) == (cell[0] if cell else None)
        if cell:
            assert C.footprint_bytes(sizes, esize, cell[0]) == cell[1]


def _reached():
    """(kernel, esize) -> [(sizes, tile, bytes)] over the table and the five pinned nets."""
    out = {cell: [] for cell in CELLS}
    for sizes in N.NETS + C.NETS:
        for kernel, esize in CELLS:
            plan = N.plan(sizes, kernel, esize)
            if plan is not None:
                assert _row_tile(kernel, sizes, esize)[0] == plan["tile"], (sizes, kernel, esize)
                out[(kernel, esize)].append((sizes, plan["tile"], plan["bytes"]))
    return out


def test_the_nets_reach_every_tile_the_ceiling_and_both_loop_forms():
    reached = _reached()
    for cell, hits in reached.items():
        # every tile, for each (kernel, dtype)
        assert {tile for _, tile, _ in hits} == {1, 2, 4, 8, 16, 32}, (cell, sorted({tile for _, tile, _ in hits}))
        # the ceiling: within 100 B of 160 KiB
        assert max(b for _, _, b in hits) >= 163740, (cell, max(b for _, _, b in hits))
        assert max(b for _, _, b in hits) <= N.LDS_MAX
    everything = [hit for hits in reached.values() for hit in hits]
    # the opt-in above 64 KiB in each third of what lies above it
    for lo, hi in ((64, 96), (96, 128), (128, 160)):
        assert any(lo * 1024 < b <= hi * 1024 for _, _, b in everything), (lo, hi)
    assert any(b == N.LDS_MAX for _, _, b in everything)
    # both loop forms at a tile below 32
    forms = set()
    for sizes, tile, _ in everything:
        if tile < 32:
            forms |= set(N.forward_pairs(sizes))
    assert forms == {True, False}
    back = set()
    for sizes, tile, _ in reached[(N.K14, 4)] + reached[(N.K14, 8)]:
        if tile < 32:
            back |= set(N.backward_pairs(sizes))
    assert back == {True, False}
    # a layer of even width that takes the scalar loop because of its offset alone
    odd = [sizes for sizes in N.NETS if N.even_width_on_an_odd_offset(sizes)]
    assert [2, 60, 1, 60, 1] in odd
    off_w, off_b = N.param_offsets([2, 60, 1, 60, 1])
    assert off_w[3] == 241 and off_b[3] == 301 and N.forward_pairs([2, 60, 1, 60, 1]) == [True, False, False]
    assert N.backward_pairs([2, 60, 1, 60, 1]) == [True, False, False]
    assert 1 in [2, 60, 1, 60, 1][1:-1]                   # and a hidden layer of width 1
    # a layer wider than the workgroup at a small tile: tile * nout / 2 > 256 at tile <= 8
    for cell, hits in reached.items():
        assert any(tile <= 8 and tile * max(sizes[1:-1]) // 2 > N.THREADS and N.widest_loop(sizes, tile) > N.THREADS
                   for sizes, tile, _ in hits if len(sizes) > 2), cell
    assert N.widest_loop([2, 1279, 1], 1) == 1279         # scalar loop, five trips of 256 lanes
    assert N.widest_loop([2, 284, 1], 8) == 8 * 142
    # an X tile larger than one pass of the copy loop
    assert any(tile * sizes[0] > N.THREADS for sizes, tile, _ in everything if sizes[0] in (33, 100))
    assert {33, 100} <= {sizes[0] for sizes in N.NETS}


@pytest.mark.parametrize("sizes", N.NETS + C.NETS, ids=N.NET_IDS + C.NET_IDS)
def test_the_restated_regions_are_aligned_disjoint_and_end_at_the_footprint(sizes):
    for kernel, esize in CELLS:
        plan = N.plan(sizes, kernel, esize)
        if plan is None:
            continue
        at = 0
        for name, start, length in plan["regions"]:
            assert start % 4 == 0, (kernel, esize, name, start)
            assert start >= at, (kernel, esize, name, start, at)          # begins behind the one before it
            at = start + length
        assert N.round4(at) * esize == plan["bytes"] <= N.LDS_MAX, (kernel, esize, at, plan["bytes"])
        names = [name for name, _, _ in plan["regions"]]
        L = len(sizes) - 1
        assert names == (["params", "x", "a0", "a1"] if kernel == N.K11 else
                         ["params", "x"] + ["h%d" % l for l in range(1, L)] + ["d0", "d1"])
    # where round4 actually rounds: a region's length is no multiple of 4 somewhere in the table
    if sizes == [2, 1279, 1]:
        plan = N.k11_plan(sizes, 4)
        assert [length % 4 for _, _, length in plan["regions"]] == [2, 2, 3, 3]


def test_the_grid_rule():
    """grid.y = min(n_tiles, ceil(4096 / S), 65535). The header's third term can never bind: S >= 1, so ceil(4096 / S) <= 4096
    < 65535. It stays in the code; this test only says that no launch can reach it."""
    assert N.grid_y(65, 10 ** 6) == 64
    assert N.grid_y(4095, 10 ** 6) == 2
    assert N.grid_y(4096, 10 ** 6) == 1 and N.grid_y(4100, 10 ** 6) == 1
    assert N.grid_y(65, 3) == 3 and N.grid_y(4095, 1) == 1 and N.grid_y(1, 7) == 7
    assert N.grid_y(1, 10 ** 6) == 4096
    assert max(-(-N.GRID_TARGET // S) for S in range(1, 5000)) == 4096 < 65535


# ---- the references alone stay within the bars -----------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", N.NETS, ids=N.NET_IDS)
def test_the_fp64_statements_in_k_order_stay_within_a_quarter_of_the_f64_bar(sizes):
    """The f64 kernels are held to 1e-12 * max(1, |truth|) against numpy's float64 statements. That bar is fair at these widths
    only if the k-ordered float64 chain itself is far inside it: against ``np.longdouble`` it stays within a quarter."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    theta, X = N.make_data(sizes, np.float64, 5, 2)
    truth_mean, truth_grad = N.truth64(theta, X, sizes)
    for s, row in enumerate(theta):
        mean, grad = N.kernel_order(C.split(row, sizes), X)
        wide_mean, wide_grad = N.kernel_order(C.split(row.astype(np.longdouble), sizes), X.astype(np.longdouble))
        assert mean.dtype == grad.dtype == np.float64 and wide_mean.dtype == wide_grad.dtype == np.longdouble
        for got, wide, truth in ((mean, wide_mean, truth_mean[s]), (grad, wide_grad, truth_grad[s])):
            bar = 0.25 * 1e-12 * np.maximum(1.0, np.abs(truth))
            assert np.all(np.abs(got - wide) <= bar), (s, float(np.abs(got - wide).max()))
            assert np.all(np.abs(truth - wide) <= bar), (s, float(np.abs(truth - wide).max()))


def _dyadic_case(sizes, rows):
    """Parameters and rows that are small multiples of 2^-3 in [-1, 1]: with no tanh in the way (one weight layer) every
    product and every partial sum is exact in float32, so the fused and the unfused forms agree bit for bit."""
    rng = np.random.RandomState(11)
    P = C.n_params(sizes)
    theta = (rng.randint(-8, 9, size=P) / 8.0).astype(np.float32)
    X = (rng.randint(-8, 9, size=(rows, sizes[0])) / 8.0).astype(np.float32)
    return theta, X


def test_the_fp32_emulation_is_the_scalar_loop_bit_for_bit():
    """The vectorised float32 restatement (float32 -> float64 product and sum -> float32) against one scalar operation at a
    time. With ``math.fma`` the scalar loop has the same two roundings at any data, so general data are compared; without it the
    loop is ``np.float32`` product and sum, equal to a fused chain only where products are exact: dyadic data, and the layers
    behind the first tanh compared on the first layer's pre-activations alone."""
    def bits(a):
        return np.ascontiguousarray(a).view(np.uint32)

    if hasattr(math, "fma"):
        for sizes in ([3, 7, 13, 1], [2, 60, 1, 60, 1], [5, 1]):
            theta, X = N.make_data(sizes, np.float32, 3, 1)
            got, want = N.kernel_order(C.split(theta[0], sizes), X), N.scalar_loop_f32(C.split(theta[0], sizes), X)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), sizes
        return
    # exact products: a single weight layer of dyadic values, 40 inputs (every partial sum is a multiple of 2^-6 below 2^6)
    sizes = [40, 1]
    theta, X = _dyadic_case(sizes, 7)
    got, want = N.kernel_order(C.split(theta, sizes), X), N.scalar_loop_f32(C.split(theta, sizes), X)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    exact = X.astype(np.float64) @ theta[:40].astype(np.float64) + float(theta[40])
    assert np.array_equal(got[0].astype(np.float64), exact)
    # the indexing of a deep net (rows, units, both sweeps): dyadic W_1 and rows, so the first layer is exact; behind the tanh
    # the two forms differ by roundings only, a few ulp of the sums
    sizes = [3, 6, 5, 1]
    theta, X = _dyadic_case(sizes, 4)
    got, want = N.kernel_order(C.split(theta, sizes), X), N.scalar_loop_f32(C.split(theta, sizes), X)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32
        assert np.all(np.abs(a.astype(np.float64) - b) <= 32 * 2.0 ** -24 * max(1.0, float(np.abs(b).max())))
    # and the emulated fma itself rounds ONCE where float32 product-and-sum rounds twice
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-1.0)
    fused = N.fma(np.array([a]), np.array([b]), np.array([c]))[0]
    assert fused == np.float32(2.0 ** -11 + 2.0 ** -24) and fused.dtype == np.float32
    assert np.float32(a * b) + c == np.float32(2.0 ** -11)
