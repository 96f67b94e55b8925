"""Cases and exact operands for the BNN's three matrix-core launches (``csrc/sgmcmc_bnn_gemm.hip``, ``csrc/sgmcmc_bnn_gw.hip``),
shared by tests/test_bnn_matrix_core_cases.py (no device: the preconditions below are proved there) and
tests/test_bnn_matrix_core_gpu.py (the kernels against them).

THE METHOD. Operands are drawn from small dyadic grids such that every product a kernel forms, and every partial sum of
such products in ANY order, is a multiple of a granularity g with magnitude at most B, B / g <= 2^24: every one of them is an
fp32 number, no addition rounds, and the result does not depend on summation order, K split, ring depth or tiling. It is
compared with ``torch.equal`` against the fp64 product (exact for the same reason), and the first wrong
(row tile, column tile, K) or (z, tile row, tile column) is named.

Restated here in Python, from the kernels' host code: ``plan_columns()`` (which columns run as 32 x 64 tiles and which as
32 x 32 half tiles), the workgroup -> tile map of the weight-gradient launch, and the three-way bf16 split.
"""
import numpy as np
import torch

BM, BK = 32, 64
# K = 64, 80, ..., 768: every tail K % 64 in {0, 16, 32, 48} at every chunk count nk = ceil(K / 64) = 1 .. 12. The ring (NS = 4,
# D = 3) enters its unrolled steady loop while kc + 7 < nk, i.e. first at nk = 8, and the drain loop behind it starts with
# nk - kc = nk (nk <= 7) or nk - 4 (nk = 8 .. 11) or nk - 8 (nk = 12) chunks left: 1 .. 7, then 4, 5, 6, 7, 4.
K_SWEEP = tuple(range(64, 769, 16))
K_MAX = K_SWEEP[-1]
TWO24 = float(2 ** 24)


# ---------------------------------------------------------------------------------------------------------------------------
# dense layers: column plan and tile layouts

def plan_columns(M, N, cus):
    """``plan_columns()`` of sgmcmc_bnn_gemm.hip: (n_full, parts). Columns [0, n_full) run as 32 x 64 tiles, the rest as 32 x 32
    half tiles; parts = n_full / 64 + (N - n_full) / 32 rows of ``dot_parts``."""
    tiles_m, col_tiles = M // BM, N // 64
    tiles = tiles_m * col_tiles
    if tiles <= cus or tiles % cus == 0:
        return N, col_tiles
    full_cols = (tiles // cus) * cus // tiles_m
    left = col_tiles - full_cols
    if full_cols >= 1 and 2 * left * tiles_m <= cus:
        return full_cols * 64, full_cols + 2 * left
    return N, col_tiles


def launches(M, N, cus):
    """The one or two launches of a layer as dicts: tile width bn, first column, columns, workgroups, XCD map on?"""
    n_full, _ = plan_columns(M, N, cus)
    out = []
    for bn, base, cols in ((64, 0, n_full), (32, n_full, N - n_full)):
        if cols:
            wgs = (M // BM) * (cols // bn)
            out.append(dict(bn=bn, n_base=base, n_cols=cols, workgroups=wgs, xcd_map=wgs % 8 == 0))
    return out


def column_tile(n, n_full):
    """Row of ``dot_parts`` (= column tile number) that column n belongs to."""
    return n // 64 if n < n_full else n_full // 64 + (n - n_full) // 32


def column_tile_edges(N, n_full):
    """First column of every column tile, and N behind them."""
    return list(range(0, n_full, 64)) + list(range(n_full, N, 32)) + [N]


# name -> (M, N): full tiles only wherever the device has at least 9 compute units
FULL_LAYOUTS = {
    "1 full tile": (32, 64),
    "9 full tiles, map off": (96, 192),
    "8 full tiles, map on": (64, 256),
}
# name -> (M, half tiles wanted): N is the smallest one whose plan has that many half-tile workgroups on the device at hand
HALF_LAYOUTS = {
    "2 half tiles, map off": (32, 2),
    "8 half tiles, map on": (32, 8),
    "2 row tiles in 4 half tiles, map off": (64, 4),
}
LAYOUTS = tuple(FULL_LAYOUTS) + tuple(HALF_LAYOUTS)


def find_half_layout(cus, M, halves):
    """Smallest N (a multiple of 64) at which an M x N layer on ``cus`` compute units launches ``halves`` half-tile workgroups, or
    None. On 256 compute units: 64 (cus + 1), 64 (cus + 4) and, for M = 64, 64 (cus / 2 + 1)."""
    for col_tiles in range(1, cus + 66):
        N = 64 * col_tiles
        n_full, _ = plan_columns(M, N, cus)
        if (M // BM) * ((N - n_full) // 32) == halves:
            return N
    return None


def layout_shape(name, cus):
    """(M, N) of a named layout on a device with ``cus`` compute units; None where that device has no such layout."""
    if name in FULL_LAYOUTS:
        M, N = FULL_LAYOUTS[name]
        ls = launches(M, N, cus)
        want_map = "map on" in name
        if len(ls) != 1 or ls[0]["bn"] != 64 or (ls[0]["workgroups"] > 1 and ls[0]["xcd_map"] != want_map):
            return None
        return M, N
    M, halves = HALF_LAYOUTS[name]
    N = find_half_layout(cus, M, halves)
    return None if N is None else (M, N)


# ---------------------------------------------------------------------------------------------------------------------------
# dense layers: exact operands (host tensors; deterministic) and their bounds

def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def backward_operands(M, N, seed=0):
    """delta [M][K_MAX + 4] and W [N][K_MAX + 12]: integers in [-4, 4] (the columns behind K of a slice ``[:, :K]`` are its pitch,
    filled like the rest); act [M][N] in {0, +-1/4, +-1/2, +-3/4}: 1 - act^2 in {1, 15/16, 3/4, 7/16} is exact."""
    g = torch.Generator().manual_seed(1000 + seed)
    return dict(delta=_ints(g, -4, 4, (M, K_MAX + 4)), W=_ints(g, -4, 4, (N, K_MAX + 12)), act=_ints(g, -3, 3, (M, N)) / 4)


def forward_operands(M, N, seed=0):
    """h [M][K_MAX + 8]: integers in [-4, 4]; W [K_MAX][N + 4]: integers in [-4, 4] times 2^-7; bias [N]: multiples of 2^-7 in
    [-1/2, 1/2]; w_next [N]: standard normal (the dot products are not exact: tanh is not)."""
    g = torch.Generator().manual_seed(2000 + seed)
    return dict(h=_ints(g, -4, 4, (M, K_MAX + 8)), W=_ints(g, -4, 4, (K_MAX, N + 4)) / 128, bias=_ints(g, -64, 64, (N,)) / 128,
                w_next=torch.randn(N, generator=g))


def dense_bounds(direction, M, K):
    """Quantity -> (granularity g, a-priori magnitude bound B) of everything the launch adds up, for operands as above."""
    if direction == "forward":
        # sum_k h W: |h W| <= 16 * 2^-7 per term; + bias
        return {"h W": (2.0 ** -7, 16.0 * K / 128), "h W + bias": (2.0 ** -7, 16.0 * K / 128 + 0.5)}
    return {"delta W^T": (1.0, 16.0 * K),                               # integers
            "out": (2.0 ** -4, 16.0 * K),                               # x (16, 15, 12 or 7) / 16, never larger than the product
            "colsum_parts": (2.0 ** -4, 32 * 16.0 * K),                 # 32 rows of out
            "colsum": (2.0 ** -4, M * 16.0 * K)}                        # all M rows


def colsum_abs_bound(ops, M, N, K):
    """max over columns of sum_m sum_k |delta W| (1 - act^2): bounds every partial sum of the column sums in any order, for THESE
    operands (tighter than M * 16 K, which 96 x 768 misses by a factor 1.125)."""
    d, W, act = ops["delta"][:, :K].double().abs(), ops["W"][:N, :K].double().abs(), ops["act"].double()
    return float(((d @ W.t()) * (1.0 - act ** 2)).sum(0).max())


# ---------------------------------------------------------------------------------------------------------------------------
# weight gradients on bf16 planes

GW_TILE = 128
# (nA, nB, count): features of the two operands, products in the launch
GW_SHAPES = ((1100, 300, 1), (1100, 300, 2), (2100, 140, 1), (200, 1100, 3), (128, 128, 1), (136, 128, 9))
# what each row is there for: workgroups T, T % 8 (r8), T // 8 (q8), tile rows % 8 (rows of the last, short panel)
GW_CLASSES = {
    (1100, 300, 1): dict(T=27, r8=3, q8=3, panel_rest=1),              # 9 x 3 tiles, both edges cut
    (1100, 300, 2): dict(T=54, r8=6, q8=6, panel_rest=1),              # the boundary between z = 0 and 1 inside an XCD's range
    (2100, 140, 1): dict(T=34, r8=2, q8=4, panel_rest=1),              # 17 x 2: two full panels and a row
    (200, 1100, 3): dict(T=54, r8=6, q8=6, panel_rest=2),              # 2 x 9: one short panel, three products
    (128, 128, 1): dict(T=1, r8=1, q8=0, panel_rest=1),
    (136, 128, 9): dict(T=18, r8=2, q8=2, panel_rest=2),
}
GW_PAIRS = ("i", "ii", "iii")


def gw_tiles(nA, nB):
    return (nA + GW_TILE - 1) // GW_TILE, (nB + GW_TILE - 1) // GW_TILE


def gw_xcd_ranges(T):
    """[(first tile number, count)] of XCD x = workgroup id % 8."""
    q8, r8 = T >> 3, T & 7
    return [(x * q8 + min(x, r8), q8 + (1 if x < r8 else 0)) for x in range(8)]


def gw_tile_of_workgroup(b, T, tiles_i, tiles_j):
    """(z, tile row, tile column) of workgroup b of T = count * tiles_i * tiles_j: the map at the top of ``gw_bf16x3_kernel``."""
    per = tiles_i * tiles_j
    q8, r8, x = T >> 3, T & 7, b & 7
    t = x * q8 + min(x, r8) + (b >> 3)
    z = t // per
    r = t - z * per
    panel = 8 * tiles_j
    gidx = r // panel
    rows = min(tiles_i - 8 * gidx, 8)
    w = r - gidx * panel
    return z, 8 * gidx + w % rows, w // rows


def gw_pair_M(pair):
    return 16 if pair == "iii" else 32


def gw_operands(pair, nA, nB, count, seed=0):
    """(A [count][M][nA], B [count][M][nB], g, bound) for one of the three exact operand pairs; the bf16 planes x = x0 + x1 + x2 hold
    8 significant bits each, and the launch forms a0 b0 | a0 b1, a1 b0 | a0 b2, a1 b1, a2 b0 and drops a1 b2, a2 b1, a2 b2:
      i    A multiples of 2^-16, |a| < 2 (18 bits: all three planes), B integers |b| <= 2 (plane 0 only), M = 32: a0 b0, a1 b0, a2 b0
      ii   the roles swapped: a0 b0, a0 b1, a0 b2
      iii  both multiples of 2^-9, |.| < 2 (11 bits: planes 0 and 1), M = 16: a0 b0, a0 b1, a1 b0, a1 b1
    Every product of planes is a multiple of g = 2^-16 (2^-18 for iii) and every partial sum is at most M * 4 in magnitude."""
    M = gw_pair_M(pair)
    g = torch.Generator().manual_seed(3000 + 7 * seed + GW_PAIRS.index(pair))
    fine = lambda n: _ints(g, -(2 ** 17 - 1), 2 ** 17 - 1, (count, M, n)) / 2 ** 16
    small = lambda n: _ints(g, -2, 2, (count, M, n))
    mid = lambda n: _ints(g, -(2 ** 10 - 1), 2 ** 10 - 1, (count, M, n)) / 2 ** 9
    if pair == "i":
        return fine(nA), small(nB), 2.0 ** -16, 4.0 * M
    if pair == "ii":
        return small(nA), fine(nB), 2.0 ** -16, 4.0 * M
    return mid(nA), mid(nB), 2.0 ** -18, 4.0 * M


def split3(x):
    """The split of ``split_pair()`` on a float32 array, in integers: plane 0 = the top 16 bits of x, plane 1 = the top 16 bits of
    the residual x - x0 (an exact fp32 subtraction), plane 2 = the top 16 bits of the residual of that. Returns the three planes
    as float32 values."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    top = lambda v: (v.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    p0 = top(x)
    r = x - p0
    p1 = top(r)
    low = r - p1
    return p0, p1, top(low)


def plane_bits(p):
    """bf16 bit patterns (as int16) of a plane whose values have zero low 16 bits."""
    return (np.ascontiguousarray(p, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16).view(np.int16)


def planes_image(x):
    """What ``sgmcmc_bnn_split_planes_f32`` writes for X [M][N]: int16 [3][M / 8][N][8], P[p][m / 8][n][m % 8]."""
    M, N = x.shape
    return np.stack([plane_bits(p).reshape(M // 8, 8, N).transpose(0, 2, 1) for p in split3(x)])


def gw_emulate(A, B):
    """The launch's accumulation in numpy float32 for one product: per 16 batch rows one step of a0 b0 into one accumulator and
    of the five small products (order of the kernel) into another; the two are added at the end."""
    M = A.shape[0]
    a, b = split3(A), split3(B)
    accm = np.zeros((A.shape[1], B.shape[1]), np.float32)
    accs = np.zeros_like(accm)
    for c in range(0, M, 16):
        dot = lambda pa, pb: (a[pa][c:c + 16].T.astype(np.float32) @ b[pb][c:c + 16]).astype(np.float32)
        accm = accm + dot(0, 0)
        for pa, pb in ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0)):
            accs = accs + dot(pa, pb)
    return accm + accs


def split_domain_values(g, shape):
    """float32 values with magnitudes uniform in exponent over [2^-100, 2^100], random signs, and +-0 sprinkled in."""
    e = torch.rand(shape, generator=g, dtype=torch.float64) * 200.0 - 100.0
    x = (torch.exp2(e) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)).float()
    u = torch.rand(shape, generator=g)
    x = torch.where(u < 0.02, torch.zeros_like(x), x)
    return torch.where(u < 0.01, -torch.zeros_like(x), x)


# below the exact domain: all 24 significant bits set at exponent -115. Planes 0 and 1 take 16 of them, the residual
# (2^8 - 1) 2^-138 is an fp32 denormal, and bf16 keeps its multiples of 2^-133 only: plane 2 = 7 * 2^-133, the sum is short by
# 2^-133 - 2^-138
SUBDOMAIN_X = float(np.float32(2.0 ** -115) * np.float32(2.0 - 2.0 ** -23))
SUBDOMAIN_BOUND = 2.0 ** -133


# ---------------------------------------------------------------------------------------------------------------------------
# reporting

def first_wrong_dense(got, want, n_full, K):
    """None, or where ``got`` first differs from ``want`` ([M][N] tensors) as (row tile, column tile, K)."""
    bad = (got != want).nonzero()
    if bad.shape[0] == 0:
        return None
    m, n = (int(v) for v in bad[0])
    return ("K = %d (tail %d, nk %d): element (%d, %d) = row tile %d, column tile %d (%s): got %r, want %r; %d of %d wrong"
            % (K, K % 64, (K + 63) // 64, m, n, m // BM, column_tile(n, n_full), "full" if n < n_full else "half",
               float(got[m, n]), float(want[m, n]), bad.shape[0], got.numel()))


def first_wrong_gw(got, want):
    """None, or where ``got`` first differs from ``want`` ([count][nA][nB]) as (z, tile row, tile column)."""
    bad = (got != want).nonzero()
    if bad.shape[0] == 0:
        return None
    z, i, j = (int(v) for v in bad[0])
    return ("product z = %d, element (%d, %d) = tile (%d, %d): got %r, want %r; %d of %d wrong"
            % (z, i, j, i // GW_TILE, j // GW_TILE, float(got[z, i, j]), float(want[z, i, j]), bad.shape[0], got.numel()))
