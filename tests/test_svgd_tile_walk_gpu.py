"""fp64 parity of the SVGD kernels (csrc/sgmcmc_svgd.hip) where a workgroup WALKS: every kernel with a capped grid visits
its column tiles with ``for (tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)``, and ``test_svgd_gpu.py`` compares
with the oracle only at sizes where n_tiles <= cap, i.e. where every workgroup runs that loop body once. What can be
wrong from the second iteration on -- LDS state kept from the previous tile, a barrier missing between two rounds,
partial sums overwritten instead of accumulated, the ragged last tile handled in a late round -- shows at none of them.

Each row of the two tables below is the smallest ``dim`` at which some workgroup of the named kernel runs the body twice
with a ragged last tile: ``dim = rounds * cap * tile + tile + 3`` (rounds = 1, or 3 where the cap is small enough to pay
for it: a stride that is right only once passes a single extra round). ``cap`` and ``tile`` were read from the dispatch
line cited in the row; ``test_svgd_tile_walk.py`` (no GPU) checks the arithmetic and that the cited line still holds that
cap. The kernels are driven as in ``test_svgd_gpu.py`` (``kernels.svgd_workspace / svgd_kernel / svgd_step``) and
compared with ``oracle.sgmcmc_oracle.svgd_kernel / svgd_step`` in float64 on the same inputs, with the input recipe of
that file's random sweep.

Two launch paths have no row:
  * ``svgd_update_small_kernel`` and ``svgd_update_reg_kernel`` launch one workgroup per tile with no cap: no walk;
  * ``svgd_update_kernel`` caps its grid at 2**20 tiles of 64 columns: a walk needs more than 64 M columns per particle,
    out of reach for a test of seconds.

Every row runs in two layouts: "vector" (row pitch = next multiple of 4 above dim, 16-byte aligned base: the kernels'
``vec`` / ``fullq`` branches) and "scalar" (pitch = dim, which is odd, base shifted by one element: the element-wise
branches). All buffers are filled with a canary that must survive in the row padding and in 256 elements behind the
last row. Every case runs twice from the same inputs and must give the same bits (fixed-order partial sums, no atomics).
"""
import collections

import numpy as np
import pytest
import torch

from oracle import sgmcmc_oracle as O
from pysgmcmc_amd import kernels

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
EPS, ALPHA, FUDGE = 0.05, 0.9, 1e-6
CANARY, TAIL = 7.0, 256
# bars of test_svgd_gpu.py on the kernel matrix and the bandwidth words (twice the rtol on h^2)
TOL = {F32: dict(rtol=3e-5, atol=3e-6), F64: dict(rtol=1e-10, atol=1e-12)}
# bars of that file's random sweep on X (rtol = atol) and H (10 rtol, atol = 1e-2 rtol): the second, looser assert
SWEEP_RTOL = {F32: 3e-5, F64: 1e-10}
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}

# The displacement bar (see ``step_bars``) is  c * u * S  carried through the element-wise tail, plus 2 ulp of the stored
# value. c is 8 x the largest error, in units of the bar at c = 1, that the ORACLE ITSELF makes: the f32 oracle against the
# f64 oracle at every f32 row of UPDATE_CASES, the f64 oracle against the same oracle in 80-bit long double at every f64
# row (``python tests/test_svgd_tile_walk.py`` prints the table). One power of two would not be enough room, since the
# kernels add in another order than numpy. Measured on the CPU, (X, H) per row:
#   f32  13 x 524 355: 0.445, 0.773   17 x 524 355: 0.419, 0.741   33 x 524 355: 0.385, 0.683
#        65 x 49 219:  0.345, 0.655   128 x 16 451: 0.329, 0.651                                   -> c = 8 x 0.773
#   f64  16 x 524 355: 0.497, 0.500   32 x 524 355: 0.402, 0.500   33 x 49 219: 0.359, 0.500   64 x 49 219: 0.320, 0.500
#        65 x 24 611:  0.349, 0.500   128 x 8 227:  0.299, 0.500                                   -> c = 8 x 0.500
# With this recipe (x ~ 0.3, one step ~ 0.015) u S carried through the tail is 0.4 .. 2.5 % of the 2 ulp term, so the bar
# is 2.03 .. 2.2 ulp of x: 1.7e-5 .. 1.5e-4 of the displacement in f32 (3.6e-14 .. 2.8e-13 in f64), against 2.6e-3 for the
# sweep's bar on X. The repulsion term is a few 1e-3 of the update at 524 355 columns (particles ~ 2e-3 apart per column)
# and more at the shorter rows, so a wrong K X product in one tile cannot hide below this bar.
C = {F32: 8 * 0.773, F64: 8 * 0.500}

# kernel: the kernel the row aims at; line / token: the dispatch line of csrc/sgmcmc_svgd.hip the cap was read from and the
# text that must still stand on it; cap x tile: grid cap and columns per tile; rounds: full rounds of the capped grid
# below dim (dim = rounds * cap * tile + tile + 3); sign: repulsion_sign of the step rows
Case = collections.namedtuple("Case", "kernel line token n dtype cap tile rounds dim sign")


def _dist(kernel, line, token, n, dtype, cap, tile, dim):
    return Case(kernel, line, token, n, dtype, cap, tile, 1, dim, 0)


# Distance and bandwidth stage (svgd_kernel(..., kernel_gradients=False)).
# svgd_sqdist_small_kernel: a "tile" is the 256 lanes x CPL columns one workgroup covers per iteration of the loop at line
#   548; CPL = 16 / sizeof(T) for n <= 8, 8 / sizeof(T) for 9..12 (SmallCfg, line 1413).
# svgd_sqdist_kernel: tile = tc(n) as computed at line 1515 ff. (``sqdist_tile`` below): 32 f64 columns at 65 particles, 16
#   at 128.
DIST_CASES = [
    _dist("svgd_sqdist_small_kernel<f32,8,4>", 1422, "SVGD_MAX_PARTS", 8, F32, 1024, 256 * 4, 1_049_603),
    _dist("svgd_sqdist_small_kernel<f64,8,2>", 1422, "SVGD_MAX_PARTS", 3, F64, 1024, 256 * 2, 524_803),
    _dist("svgd_sqdist_small_kernel<f32,16,2>", 1422, "SVGD_MAX_PARTS", 9, F32, 1024, 256 * 2, 524_803),
    _dist("svgd_sqdist_small_kernel<f64,16,1>", 1422, "SVGD_MAX_PARTS", 12, F64, 1024, 256 * 1, 262_403),
    _dist("svgd_gram_mfma16_kernel<f32,1>", 1467, "IB <= 2 ? 2048 : 1024", 13, F32, 2048, 64, 131_139),
    _dist("svgd_gram_mfma16_kernel<f64,1>", 1467, "IB <= 2 ? 2048 : 1024", 16, F64, 2048, 64, 131_139),
    _dist("svgd_gram_mfma16_kernel<f32,2>", 1467, "IB <= 2 ? 2048 : 1024", 32, F32, 2048, 64, 131_139),
    _dist("svgd_gram_mfma16_kernel<f64,2>", 1467, "IB <= 2 ? 2048 : 1024", 17, F64, 2048, 64, 131_139),
    _dist("svgd_gram_mfma16_kernel<f64,4>", 1467, "IB <= 2 ? 2048 : 1024", 33, F64, 1024, 64, 65_603),
    _dist("svgd_gram_mfma16_kernel<f64,4>", 1467, "IB <= 2 ? 2048 : 1024", 64, F64, 1024, 64, 65_603),
    _dist("svgd_gram_mfma_kernel<2>", 1442, "IB == 2 ? 1024 : 512", 33, F32, 1024, 128, 131_203),
    _dist("svgd_gram_mfma_kernel<2>", 1442, "IB == 2 ? 1024 : 512", 64, F32, 1024, 128, 131_203),
    _dist("svgd_gram_mfma_kernel<4>", 1442, "IB == 2 ? 1024 : 512", 65, F32, 512, 128, 65_667),
    _dist("svgd_gram_mfma_kernel<4>", 1442, "IB == 2 ? 1024 : 512", 128, F32, 512, 128, 65_667),
    _dist("svgd_sqdist_kernel<f64,2>", 1522, "SVGD_MAX_PARTS", 65, F64, 1024, 32, 32_803),
    _dist("svgd_sqdist_kernel<f64,3>", 1522, "SVGD_MAX_PARTS", 128, F64, 1024, 16, 16_403),
]

# Update stage (svgd_step). The 524 355-column rows also walk their distance kernels (4 rounds of svgd_gram_mfma16_kernel,
# 5 of svgd_gram_mfma_kernel<2>); the rows above exist so that a failure names one stage.
UPDATE_CASES = [
    Case("svgd_update_mfma16_kernel<f32,1>", 1598, "n_tiles < 8192", 13, F32, 8192, 64, 1, 524_355, -1),
    Case("svgd_update_mfma16_kernel<f32,2>", 1598, "n_tiles < 8192", 17, F32, 8192, 64, 1, 524_355, 1),
    Case("svgd_update_mfma16_kernel<f32,4>", 1598, "n_tiles < 8192", 33, F32, 8192, 64, 1, 524_355, -1),
    Case("svgd_update_mfma16_kernel<f64,1>", 1639, "ib <= 2 ? 8192 : 256", 16, F64, 8192, 64, 1, 524_355, 1),
    Case("svgd_update_mfma16_kernel<f64,2>", 1639, "ib <= 2 ? 8192 : 256", 32, F64, 8192, 64, 1, 524_355, -1),
    Case("svgd_update_mfma16_kernel<f64,4>", 1639, "ib <= 2 ? 8192 : 256", 33, F64, 256, 64, 3, 49_219, 1),
    Case("svgd_update_mfma16_kernel<f64,4>", 1639, "ib <= 2 ? 8192 : 256", 64, F64, 256, 64, 3, 49_219, -1),
    Case("svgd_update_mfma_kernel<4,64>", 1610, "n_tiles < 256", 65, F32, 256, 64, 3, 49_219, -1),
    Case("svgd_update_mfma_kernel<4,64>", 1610, "n_tiles < 256", 128, F32, 256, 64, 1, 16_451, 1),
    Case("svgd_update_mfma_f64_big_kernel", 1623, "n_tiles < 256", 65, F64, 256, 32, 3, 24_611, 1),
    Case("svgd_update_mfma_f64_big_kernel", 1623, "n_tiles < 256", 128, F64, 256, 32, 1, 8_227, -1),
]


def case_id(case):
    return "%s-n%d-d%d" % (case.kernel.replace("svgd_", "").replace("_kernel", ""), case.n, case.dim)


def sqdist_tile(n, itemsize):
    """Columns per tile of svgd_sqdist_kernel, as svgd_kernel_matrix_impl computes them (line 1515 ff.): the largest power
    of two in [16, 1024] whose transposed tile of pitch np + 4 fits the 32 KiB LDS tile."""
    pitch = ((n + 3) & ~3) + 4
    log2 = 4
    while log2 < 10 and (2 << log2) * pitch * itemsize <= 32 * 1024:
        log2 += 1
    return 1 << log2


def inputs(case):
    """The sweep's recipe: X = 0.3 + N(0, 1) / sqrt(d), G ~ N(0, 1), H ~ U(0.05, 1), in the case's dtype."""
    n, d = case.n, case.dim
    rng = np.random.default_rng([n, d, np.dtype(case.dtype).itemsize])
    X = (0.3 + rng.normal(size=(n, d)) / np.sqrt(d)).astype(case.dtype)
    G = rng.normal(size=(n, d)).astype(case.dtype)
    H = rng.uniform(0.05, 1.0, size=(n, d)).astype(case.dtype)
    return X, G, H


StepRef = collections.namedtuple("StepRef", "X G H K h disp Hn Xn S J gt")


def step_reference(case, wide=np.float64):
    """One oracle step in ``wide`` precision on the case's inputs, and what the bars are made of:
    S_ic = (sum_j K_ij |G_jc| + (sum_j K_ij |X_jc| + |X_ic| ksum_i) / h^2) / n bounds the terms that are added up into
    grad_theta (svgd.py:124-127, 176-181), so u * S is the scale of its rounding error whatever the order of summation;
    J = 1 / (fudge + sqrt(h_new)) bounds |d adj / d grad_theta| (the second term of that derivative has the opposite sign
    and is smaller, since (1 - alpha) gt^2 <= h_new)."""
    return step_reference_on(inputs(case), case.sign, wide)


def step_reference_on(xgh, sign, wide=np.float64):
    """``step_reference`` on given inputs (X, G, H) of one dtype"""
    X, G, H = xgh
    n = X.shape[0]
    Xw, Gw, Hw = X.astype(wide), G.astype(wide), H.astype(wide)
    Xn, Hn = Xw.copy(), Hw.copy()
    K, h = O.svgd_step(Xn, Gw, Hn, EPS, ALPHA, FUDGE, float(sign))
    f = lambda a: np.asarray(a, dtype=np.float64)
    disp = f(Xn - Xw)
    K, Xn, Hn, h = f(K), f(Xn), f(Hn), float(h)                     # the bars themselves need no more than f64
    absX, absG = np.abs(X.astype(np.float64)), np.abs(G.astype(np.float64))
    S = (K @ absG + (K @ absX + absX * K.sum(axis=1)[:, None]) / (h * h)) / n
    J = 1.0 / (FUDGE + np.sqrt(Hn))
    gt = np.abs(disp) / EPS / J
    return StepRef(X, G, H, K, h, disp, Hn, Xn, S, J, gt)


def step_bars(ref, dtype, c):
    """Per-element bars on the displacement x_new - x_old and on H for arithmetic in ``dtype``:
        bar_X = eps J (c u S) + 2 ulp(x_new)                 the ulp term: rounding of the final store (both sides)
        bar_H = 2 (1 - alpha) |gt| (c u S) + 2 ulp(h_new)    d h_new / d gt = 2 (1 - alpha) gt; alpha H, gt^2, its
                                                             product and the sum round once each, all below h_new
    The element-wise tail's own roundings of adj (a division, a square root, a sum: a few u |adj|) are inside the first
    term, since S >= |gt| and c >= 8."""
    u = U[dtype]
    ulp = lambda a: np.spacing(np.abs(a).astype(dtype)).astype(np.float64)
    bar_x = EPS * ref.J * (c * u * ref.S) + 2 * ulp(ref.Xn)
    bar_h = 2 * (1 - ALPHA) * ref.gt * (c * u * ref.S) + 2 * ulp(ref.Hn)
    return bar_x, bar_h


def bar_units(ref, dtype, x_new, h_new):
    """Largest error of (x_new - x_old, h_new) in units of the bar at c = 1: (for X, for H). An error of r units is
    inside the bar at any c >= r (the bar grows with c and, below 1, shrinks no faster than c)."""
    bar_x, bar_h = step_bars(ref, dtype, 1.0)
    ex = np.abs((x_new.astype(np.float64) - ref.X.astype(np.float64)) - ref.disp)
    eh = np.abs(h_new.astype(np.float64) - ref.Hn)
    return float(np.max(ex / bar_x)), float(np.max(eh / bar_h))


_cache = {}


def _cached(kind, case, make):
    """One reference per row, shared by its layouts; only the last row's is kept (the largest holds five 134 MB arrays)."""
    key = (kind, case)
    if key not in _cache:
        _cache.clear()
        _cache[key] = make(case)
    return _cache[key]


def _layout(dim, layout):
    """(row pitch, base offset in elements)"""
    if layout == "vector":
        return (dim // 4 + 1) * 4, 0
    return dim, 1


def _device(a, ld, offset):
    """Canary-filled device buffer holding the rows of ``a`` at pitch ld from element ``offset``, and the view the kernels get."""
    n, d = a.shape
    buf = torch.full((offset + n * ld + TAIL,), CANARY, dtype=torch.from_numpy(a[:1, :1]).dtype, device=DEV)
    view = buf[offset:]
    view[:n * ld].view(n, ld)[:, :d] = torch.from_numpy(a).to(DEV)
    return buf, view


def _rows(host, n, d, ld, offset):
    return host[offset:offset + n * ld].reshape(n, ld)[:, :d]


def _canary_intact(host, n, d, ld, offset):
    keep = np.ones(host.shape[0], bool)
    for i in range(n):
        keep[offset + i * ld:offset + i * ld + d] = False
    return bool(np.all(host[keep] == CANARY))


def _where(case, idx):
    """Names the element: particle, column, the update tile that holds it and the round of the walk that visits the tile."""
    i, col = int(idx[0]), int(idx[1])
    tile = col // case.tile
    return "particle %d, column %d of %d: tile %d of %d, round %d of the walk (cap %d, csrc/sgmcmc_svgd.hip:%d)" % (
        i, col, case.dim, tile, -(-case.dim // case.tile), tile // case.cap, case.cap, case.line)


def _assert_within(case, layout, what, got, want, bar):
    excess = np.abs(got - want) / bar
    idx = np.unravel_index(np.argmax(excess), excess.shape)
    print("%s [%s] %s: worst |error| / bar = %.3f at %s" % (case_id(case), layout, what, excess[idx], _where(case, idx)))
    assert excess[idx] <= 1.0, "%s of %s [%s]: |error| %.3e is %.2f x its bar %.3e (got %r, want %r) at %s" % (
        what, case.kernel, layout, abs(got[idx] - want[idx]), excess[idx], bar[idx], got[idx], want[idx], _where(case, idx))


@pytest.mark.parametrize("layout", ["vector", "scalar"])
@pytest.mark.parametrize("case", DIST_CASES, ids=case_id)
def test_kernel_matrix_where_the_distance_kernel_walks(case, layout):
    """K and the three bandwidth words against the f64 oracle at the bars of test_svgd_gpu.py, exact symmetry and unit
    diagonal, same bits on a second run."""
    n, d = case.n, case.dim

    def reference(case):
        X = inputs(case)[0]
        K, _, h, D = O.svgd_kernel(X.astype(np.float64))
        return X, K, float(h), float(O.svgd_median(D))
    X, K_ref, h_ref, med_ref = _cached("dist", case, reference)
    ld, offset = _layout(d, layout)
    buf, x = _device(X, ld, offset)
    ws = kernels.svgd_workspace(n, x)
    runs = []
    for _ in range(2):
        ws.fill_(float("nan"))                                        # a partial that is read but never written shows
        K, _, bw = kernels.svgd_kernel(x, n, d, ws, ld=ld, kernel_gradients=False)
        torch.cuda.synchronize()
        runs.append((K.cpu().numpy(), bw.cpu().numpy()))
    K, bw = runs[0]
    n_tiles = -(-d // case.tile)
    what = "%s [%s], %d tiles of %d columns on %d workgroups (csrc/sgmcmc_svgd.hip:%d): %d rounds" % (
        case.kernel, layout, n_tiles, case.tile, case.cap, case.line, -(-n_tiles // case.cap))
    tol = TOL[case.dtype]
    rel = np.abs(K - K_ref) / np.abs(K_ref)
    print("%s: max relative error of K %.3e, of h %.3e" % (what, rel.max(), abs(bw[1] - h_ref) / h_ref))
    host = buf.cpu().numpy()
    assert _canary_intact(host, n, d, ld, offset) and np.array_equal(_rows(host, n, d, ld, offset), X), \
        "the distance stage wrote to X: " + what
    np.testing.assert_allclose(bw[0], med_ref, rtol=tol["rtol"], err_msg=what)
    np.testing.assert_allclose(bw[1], h_ref, rtol=tol["rtol"], err_msg=what)
    np.testing.assert_allclose(bw[2], h_ref * h_ref, rtol=2 * tol["rtol"], err_msg=what)
    np.testing.assert_allclose(K, K_ref, err_msg=what, **tol)
    assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1), what               # exact structure
    assert np.array_equal(runs[1][0], K) and np.array_equal(runs[1][1], bw), "second run differs in bits: " + what


@pytest.mark.parametrize("layout", ["vector", "scalar"])
@pytest.mark.parametrize("case", UPDATE_CASES, ids=case_id)
def test_step_where_the_update_kernel_walks(case, layout):
    """The DISPLACEMENT x_new - x_old and H against the f64 oracle at the per-element bars of ``step_bars``, then X and H
    at the sweep's bars, the canary around every row, and the same bits on a second run.

    The sweep's rtol = atol = 3e-5 on X is a bar on x ~ 0.3, while one step moves x by ~0.015 (eps / sqrt(1 - alpha) at
    most): 2.6e-3 of the update itself, which a wrong product K G or K X in one tile of a late round can stay below. The
    displacement bar is the rounding of the sums and of the final store, 2e-5 .. 1.5e-4 of the update in f32."""
    n, d = case.n, case.dim
    ref = _cached("step", case, step_reference)
    ld, offset = _layout(d, layout)
    runs = []
    for _ in range(2):
        (bx, x), (_, g), (bh, h) = (_device(a, ld, offset) for a in (ref.X, ref.G, ref.H))
        ws = kernels.svgd_workspace(n, x)
        ws.fill_(float("nan"))                                        # a partial that is read but never written shows
        kernels.svgd_step(x, g, h, n, d, EPS, ALPHA, FUDGE, ws, ld=ld, repulsion_sign=case.sign)
        torch.cuda.synchronize()
        runs.append((bx.cpu().numpy(), bh.cpu().numpy()))
        del bx, x, g, bh, h, ws
    hx, hh = runs[0]
    assert np.array_equal(runs[1][0], hx) and np.array_equal(runs[1][1], hh), \
        "second run of %s [%s] differs in bits" % (case.kernel, layout)
    assert _canary_intact(hx, n, d, ld, offset), "%s [%s] wrote X outside its rows (pitch %d)" % (case.kernel, layout, ld)
    assert _canary_intact(hh, n, d, ld, offset), "%s [%s] wrote H outside its rows (pitch %d)" % (case.kernel, layout, ld)
    x_new = _rows(hx, n, d, ld, offset).astype(np.float64)
    h_new = _rows(hh, n, d, ld, offset).astype(np.float64)
    bar_x, bar_h = step_bars(ref, case.dtype, C[case.dtype])
    print("%s [%s]: %.3f (X), %.3f (H) units of the bar at c = 1; c = %g" % (
        (case_id(case), layout) + bar_units(ref, case.dtype, x_new, h_new) + (C[case.dtype],)))
    _assert_within(case, layout, "displacement", x_new - ref.X.astype(np.float64), ref.disp, bar_x)
    _assert_within(case, layout, "H", h_new, ref.Hn, bar_h)
    rtol = SWEEP_RTOL[case.dtype]
    _assert_within(case, layout, "X (sweep's bar)", x_new, ref.Xn, rtol + rtol * np.abs(ref.Xn))
    _assert_within(case, layout, "H (sweep's bar)", h_new, ref.Hn, rtol * 1e-2 + 10 * rtol * np.abs(ref.Hn))
