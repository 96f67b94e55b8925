"""The cases of tests/test_bnn_matrix_core_gpu.py, checked without a device (tests/bnn_matrix_core_cases.py): the exact operands
are exact -- by bound and by example --, the Python restatements of the column plan and of the weight-gradient tile map say what
the library's host code says, and every layout and tile-map class the GPU file claims is the one its shapes produce on the 256
compute units of an MI355X."""
import numpy as np
import pytest
import torch

import bnn_matrix_core_cases as C

CUS = 256


def _host_cus():
    """Compute units the library's host arithmetic uses here: those of the current device, or MI355X's 256 without one."""
    if torch.cuda.is_available():
        return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return CUS


def test_k_sweep_has_every_tail_at_every_ring_phase():
    """45 values: the four tails at nk = 1 .. 12; the steady loop is not entered (nk <= 7), entered once (8 .. 11) and twice (12),
    and the drain loop behind it starts with 4, 5, 6 and 7 chunks left."""
    assert len(C.K_SWEEP) == 45 and C.K_MAX == 768
    seen = {(K % 64, (K + 63) // 64) for K in C.K_SWEEP}
    assert seen == {(t, nk) for t in (0, 16, 32, 48) for nk in range(2, 13)} | {(0, 1)}      # (K >= 64: nk = 1 has no tail)
    NS, D = 4, 3
    left_after_steady = {}
    for nk in range(1, 13):
        kc = 0
        while kc + D + NS < nk:
            kc += NS
        left_after_steady[nk] = (kc // NS, nk - kc)
    assert [left_after_steady[nk] for nk in range(1, 8)] == [(0, nk) for nk in range(1, 8)]
    assert [left_after_steady[nk] for nk in range(8, 13)] == [(1, 4), (1, 5), (1, 6), (1, 7), (2, 4)]


def test_column_plan_restatement_equals_the_library():
    """``plan_columns`` in Python against ``sgmcmc_bnn_dense_tanh_dot_parts`` (host arithmetic) over a grid of (M, N)."""
    from pysgmcmc_amd import _lib
    parts = _lib.lib().sgmcmc_bnn_dense_tanh_dot_parts
    cus = _host_cus()
    col_tiles = sorted(set(range(1, 40)) | {cus // 8 + d for d in range(-2, 14)} | {cus // 4 + d for d in range(-2, 6)}
                       | {cus // 2 + d for d in range(-2, 6)} | {cus + d for d in range(-2, 10)} | {76, 136, 3 * cus // 2, 2 * cus + 1})
    n = 0
    for M in (32, 64, 96, 128, 160, 256, 512):
        for ct in col_tiles:
            if ct >= 1:
                assert parts(M, 64 * ct) == C.plan_columns(M, 64 * ct, cus)[1], (M, 64 * ct)
                n += 1
    assert n > 500
    if cus == CUS:
        assert C.plan_columns(256, 4864, cus) == (4096, 88) and C.plan_columns(64, 8704, cus) == (8192, 144)
        assert C.plan_columns(32, 8320, cus) == (8320, 130)       # 130 tiles on 256 compute units: no half tile


def test_every_dense_layout_exists_on_256_compute_units():
    want = {  # name: (M, N, [(tile width, workgroups, XCD map on)])
        "1 full tile": (32, 64, [(64, 1, False)]),
        "9 full tiles, map off": (96, 192, [(64, 9, False)]),
        "8 full tiles, map on": (64, 256, [(64, 8, True)]),
        "2 half tiles, map off": (32, 64 * (CUS + 1), [(64, CUS, True), (32, 2, False)]),
        "8 half tiles, map on": (32, 64 * (CUS + 4), [(64, CUS, True), (32, 8, True)]),
        "2 row tiles in 4 half tiles, map off": (64, 64 * (CUS // 2 + 1), [(64, CUS, True), (32, 4, False)]),
    }
    assert set(want) == set(C.LAYOUTS)
    for name, (M, N, ls) in want.items():
        assert C.layout_shape(name, CUS) == (M, N), name
        got = [(l["bn"], l["workgroups"], l["xcd_map"]) for l in C.launches(M, N, CUS)]
        assert got == ls, (name, got)
        n_full, parts = C.plan_columns(M, N, CUS)
        edges = C.column_tile_edges(N, n_full)
        assert len(edges) == parts + 1 and all(C.column_tile(edges[t], n_full) == t for t in range(parts))
        assert all(b - a == (64 if a < n_full else 32) for a, b in zip(edges, edges[1:]))
    # another device: a layout is found with the half-tile count asked for, or reported missing
    for cus in (8, 64, 80, 104, 304):
        for name, (M, halves) in C.HALF_LAYOUTS.items():
            shape = C.layout_shape(name, cus)
            if shape is not None:
                assert sum(l["workgroups"] for l in C.launches(shape[0], shape[1], cus) if l["bn"] == 32) == halves


@pytest.mark.parametrize("name", C.LAYOUTS)
def test_dense_operands_are_exact(name):
    """By bound: granularity g and magnitude B of everything a launch adds up, B / g <= 2^24, at every K of the sweep (the one
    a-priori bound that misses, the 96-row column sums beyond K = 682, is replaced by the sum of magnitudes of the operands
    themselves). By example: the fp64 results at K_MAX lie on the grid and survive the round trip through fp32."""
    M, N = C.layout_shape(name, CUS)
    bw, fw = C.backward_operands(M, N), C.forward_operands(M, N)
    assert float(bw["delta"].abs().max()) == 4 and float(bw["W"].abs().max()) == 4
    assert set(np.unique(bw["act"].numpy())) == {-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75}
    assert torch.equal(bw["delta"], bw["delta"].round()) and torch.equal(bw["W"], bw["W"].round())
    assert float(fw["h"].abs().max()) == 4 and torch.equal(fw["h"], fw["h"].round())
    assert float((fw["W"] * 128).abs().max()) == 4 and torch.equal(fw["W"] * 128, (fw["W"] * 128).round())
    assert float(fw["bias"].abs().max()) <= 0.5 and torch.equal(fw["bias"] * 128, (fw["bias"] * 128).round())
    for K in C.K_SWEEP:
        for direction in ("forward", "backward"):
            for what, (g, B) in C.dense_bounds(direction, M, K).items():
                if what == "colsum" and B / g > C.TWO24:
                    assert (M, K > 682) == (96, True)
                    B = C.colsum_abs_bound(bw, M, N, K)
                assert B / g <= C.TWO24, (name, K, what)
    K = C.K_MAX
    d, W, act = bw["delta"][:, :K].double(), bw["W"][:, :K].double(), bw["act"].double()
    out = (d @ W.t()) * (1.0 - act ** 2)
    for v, g in ((d @ W.t(), 1.0), (out, 2.0 ** -4), (out.view(M // 32, 32, N).sum(1), 2.0 ** -4), (out.sum(0), 2.0 ** -4)):
        assert torch.equal(v.float().double(), v) and torch.equal((v / g).round(), v / g)
    assert float(out.abs().max()) > 0
    z = fw["h"][:, :K].double() @ fw["W"][:K, :N].double()
    for v in (z, z + fw["bias"].double()):
        assert torch.equal(v.float().double(), v) and torch.equal((v * 128).round(), v * 128)
    assert 0.5 < float(z.std()) < 3.0                             # of order 1: tanh is not saturated


@pytest.mark.parametrize("nA,nB,count", C.GW_SHAPES)
def test_gw_tile_map_classes_and_bijection(nA, nB, count):
    ti, tj = C.gw_tiles(nA, nB)
    T = count * ti * tj
    cls = C.GW_CLASSES[(nA, nB, count)]
    assert dict(T=T, r8=T % 8, q8=T // 8, panel_rest=ti % 8) == cls
    ranges = C.gw_xcd_ranges(T)
    assert sum(n for _, n in ranges) == T and all(a + n == b for (a, n), (b, _) in zip(ranges, ranges[1:]))
    seen = [C.gw_tile_of_workgroup(b, T, ti, tj) for b in range(T)]
    assert sorted(seen) == [(z, i, j) for z in range(count) for i in range(ti) for j in range(tj)]
    if (nA, nB, count) == (1100, 300, 2):                         # the first tile of z = 1 lies strictly inside an XCD's range
        assert any(a < ti * tj < a + n for a, n in ranges) and T % 8 != 0


def test_gw_classes_cover_what_the_map_can_do():
    cls = list(C.GW_CLASSES.values())
    assert any(c["T"] > 8 and c["r8"] != 0 for c in cls) and any(c["T"] < 8 for c in cls)
    assert any(c["panel_rest"] == 1 and c["T"] > 8 for c in cls)
    assert any(C.gw_tiles(nA, nB)[0] > 16 for nA, nB, _ in C.GW_SHAPES)      # more than two panels


@pytest.mark.parametrize("pair", C.GW_PAIRS)
def test_gw_operand_pairs_are_exact_and_use_the_planes_they_should(pair):
    """Bound: B / g <= 2^24. Planes: which of the three are non-zero, so that the dropped products a1 b2, a2 b1, a2 b2 vanish and
    the three pairs together use all six products the launch forms. Example: the fp64 product round-trips through fp32, and
    the launch's accumulation, emulated in float32, gives it bit for bit."""
    nA, nB, count = 200, 136, 2
    A, B, g, bound = C.gw_operands(pair, nA, nB, count)
    M = C.gw_pair_M(pair)
    assert A.shape == (count, M, nA) and B.shape == (count, M, nB) and bound / g <= C.TWO24
    assert float(A.abs().max()) * float(B.abs().max()) * M <= bound
    used = []
    for X in (A, B):
        planes = C.split3(X.numpy())
        assert np.array_equal((planes[0] + planes[1]) + planes[2], X.numpy())
        assert all(np.array_equal(p.view(np.uint32) & 0xffff, np.zeros_like(p, dtype=np.uint32)) for p in planes)
        used.append(tuple(bool(np.any(p != 0)) for p in planes))
    assert used == {"i": [(True, True, True), (True, False, False)], "ii": [(True, False, False), (True, True, True)],
                    "iii": [(True, True, False), (True, True, False)]}[pair]
    formed = {(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)}
    nonzero = {(pa, pb) for pa in range(3) for pb in range(3) if used[0][pa] and used[1][pb]}
    assert nonzero <= formed                                      # nothing the launch drops is non-zero
    for z in range(count):
        a, b = A[z].numpy(), B[z].numpy()
        ref = a.astype(np.float64).T @ b.astype(np.float64)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and np.array_equal(np.round(ref / g), ref / g)
        assert np.array_equal(C.gw_emulate(a, b).astype(np.float64), ref)


def test_gw_operand_pairs_together_use_all_six_products():
    used = set()
    for pair in C.GW_PAIRS:
        A, B, _, _ = C.gw_operands(pair, 64, 64, 1)
        pa = [bool(np.any(p != 0)) for p in C.split3(A.numpy())]
        pb = [bool(np.any(p != 0)) for p in C.split3(B.numpy())]
        used |= {(i, j) for i in range(3) for j in range(3) if pa[i] and pb[j]}
    assert used == {(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)}


def test_split_restatement_and_its_exact_domain():
    """On [2^-100, 2^100] and at +-0 the three planes add up to x by value; -0 comes back as +0 (plane 0 keeps the sign bit, the
    residual of -0 is +0); below 2^-110 plane 2 loses what bf16 denormals cannot hold, less than 2^-133."""
    x = C.split_domain_values(torch.Generator().manual_seed(5), (64, 300)).numpy()
    assert (x == 0).sum() > 100 and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    assert 2.0 ** -101 < np.abs(x[x != 0]).min() < 2.0 ** -90 and 2.0 ** 90 < np.abs(x).max() < 2.0 ** 101
    p = C.split3(x)
    assert np.array_equal((p[0] + p[1]) + p[2], x)
    assert C.planes_image(x).shape == (3, 8, 300, 8) and C.planes_image(x)[1, 2, 5, 3] == C.plane_bits(p[1])[19, 5]
    # the smallest magnitudes of the exact domain, every mantissa bit set
    edge = np.array([2.0 ** -110 * (2.0 - 2.0 ** -23), -(2.0 ** -110) * (2.0 - 2.0 ** -23)], np.float32)
    pe = C.split3(edge)
    assert np.array_equal((pe[0] + pe[1]) + pe[2], edge) and np.all(pe[2] != 0)
    # -0
    pz = C.split3(np.array([-0.0], np.float32))
    assert C.plane_bits(pz[0])[0] == np.int16(-0x8000) and C.plane_bits(pz[1])[0] == 0 and C.plane_bits(pz[2])[0] == 0
    assert not np.signbit((pz[0] + pz[1]) + pz[2])[0]
    # below the domain
    xs = np.array([C.SUBDOMAIN_X], np.float32)
    ps = C.split3(xs)
    err = float(xs[0]) - (float(ps[0][0]) + float(ps[1][0]) + float(ps[2][0]))
    assert float(ps[2][0]) == 7 * 2.0 ** -133 and err == 2.0 ** -133 - 2.0 ** -138 and 0 < err < C.SUBDOMAIN_BOUND
