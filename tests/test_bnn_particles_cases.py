"""The case table of tests/particles_cases.py without a GPU: the restated LDS plan of K15 is sound and equals the library's
footprint at every row, refusals included; every row reaches the loop forms, the trip counts and the footprint it is in the
table for, and the rows together reach every form with more than one trip, every remainder of the unrolled loops, both depths
and the full 160 KiB in both dtypes, as CONDITIONS on the restated plan; and the two references the GPU tests bound the kernel
with agree with the oracle and with a scalar loop on their own. What the kernel computes at these rows is checked on the GPU
(tests/test_bnn_particles_forms_gpu.py)."""
import numpy as np
import pytest
import torch

import particles_cases as K
import predict_grad_cases as C
import small_net_cases as N
from pysgmcmc_amd import kernels

TORCH = {K.F32: torch.float32, K.F64: torch.float64}
PAIR, SCALAR, LAST = K.PAIR, K.SCALAR, K.LAST
CASES = [pytest.param(sizes, B, dt, id=name) for (sizes, B, dt), name in zip(K.CASES, K.CASE_IDS)]
SHAPES = sorted({(tuple(sizes), B) for sizes, B, _ in K.CASES})
TABLE_BATCHES = {}
for _sizes, _batches, _, _ in K.TABLE:
    TABLE_BATCHES.setdefault(tuple(_sizes), set()).update(_batches)


def _layer(sizes, B, l):
    return K.forms(sizes, B)[l - 1]


# ---- the plan ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes, B, dt", CASES)
def test_the_restated_plan_is_sound_and_its_footprint_is_the_library_s(sizes, B, dt):
    total = K.check_plan(sizes, B, K.ESIZE[dt])
    assert total == K.lds_bytes(sizes, B, K.ESIZE[dt]) == kernels.bnn_particles_lds_bytes(sizes, B, TORCH[dt])
    assert 0 < total <= K.LDS_MAX
    assert K.k8_takes(sizes, B, dt) and 0 < K.k8_lds_bytes(sizes, B, K.ESIZE[dt]) <= total


def test_the_region_order_even_regions_first():
    # odd batch, mixed widths: h_0 (10), h_1 (20), h_2 (30), d_1, d_2 are even; h_3 (15), h_4 (5), d_3, d_4, y are odd
    regions = K.plan([2, 4, 6, 3, 1], 5)
    assert list(regions) == ["params", "h0", "h1", "h2", "d1", "d2", "h3", "h4", "d3", "d4", "y"]
    assert regions["h0"] == (68, 10) and regions["h3"] == (68 + 10 + 20 + 30 + 20 + 30, 15) and regions["y"][1] == 5
    # even batch: everything is even and lies in the header's order
    assert list(K.plan([2, 4, 6, 3, 1], 8)) == ["params", "h0", "h1", "h2", "h3", "h4", "d1", "d2", "d3", "d4", "y"]
    # every region odd: the header's order again, behind round4(n_params)
    regions = K.plan([3] * 8 + [1], 3)
    assert all(length % 2 == 1 for name, (_, length) in regions.items() if name != "params")
    assert list(regions)[1:] == ["h%d" % l for l in range(9)] + ["d%d" % l for l in range(1, 9)] + ["y"]
    assert regions["h0"][0] == N.round4(C.n_params([3] * 8 + [1]))
    # one input, one output, an odd batch: h_0, h_L, delta_L and y are odd and lie behind the even ones, on alternating parity
    regions = K.plan(K.DEFAULT, 49)
    assert list(regions)[-4:] == ["h0", "h4", "d4", "y"] and [regions[name][1] for name in list(regions)[-4:]] == [49] * 4
    assert [regions[name][0] % 2 for name in list(regions)[-4:]] == [0, 1, 0, 1]


@pytest.mark.parametrize("sizes, top, dt", K.CEILINGS, ids=["%s-%s" % ("x".join(map(str, c[0])), K.NAME[c[2]]) for c in K.CEILINGS])
def test_one_batch_past_a_ceiling_is_refused(sizes, top, dt):
    esize = K.ESIZE[dt]
    assert K.lds_bytes(sizes, top, esize) == kernels.bnn_particles_lds_bytes(sizes, top, TORCH[dt]) > 0
    assert K.lds_bytes(sizes, top + 1, esize) == kernels.bnn_particles_lds_bytes(sizes, top + 1, TORCH[dt]) == 0
    assert (sizes, top, dt) in K.CASES
    rows = 2 * sum(sizes) + 1
    assert K.LDS_MAX - K.lds_bytes(sizes, top, esize) < rows * esize          # no larger batch fits


def test_the_refusal_batches_are_the_issue_s():
    assert sorted(top + 1 for _, top, _ in K.CEILINGS) == [50, 91, 117, 300, 715]


# ---- every row reaches what it is in the table for -------------------------------------------------------------------------------

def test_pairs_and_scalars_in_one_net_and_every_remainder_of_the_unrolled_loops():
    sizes = [2, 4, 6, 3, 1]
    batches = TABLE_BATCHES[tuple(sizes)]
    assert batches == {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17}
    for B in batches:
        layers = K.forms(sizes, B)
        assert [f.gw for f in layers] == [PAIR, PAIR, SCALAR, SCALAR]
        assert [f.delta for f in layers] == [None, PAIR, SCALAR, SCALAR]
        assert [f.forward for f in layers] == [PAIR, PAIR, SCALAR, LAST]
    assert {B % 4 for B in batches} == set(range(4)) and {B % 8 for B in batches} == set(range(8))
    assert {B // 8 for B in batches} == {0, 1, 2}                          # no full round of the unroll, one, two
    # the j-pair loop of the pair delta (unrolled 4) runs nout / 2 = 3 times here, 33 at [2, 64, 66, 1], 24 at [2, 48, 48, 1] and
    # 6 at [3, 12, 12, 1]: every remainder
    assert [sizes[2] // 2 % 4, 66 // 2 % 4, 48 // 2 % 4, 12 // 2 % 4] == [3, 1, 0, 2]
    # odd regions behind even ones at an odd batch
    for B in (1, 3, 5, 7, 9, 17):
        lengths = [length % 2 for name, (_, length) in K.plan(sizes, B).items() if name != "params"]
        assert lengths == sorted(lengths) and 0 in lengths and 1 in lengths


def test_even_widths_on_odd_offsets_take_the_scalar_loops():
    sizes = [2, 3, 4, 6, 1]
    off_w, off_b = N.param_offsets(sizes)
    assert (off_w[2], off_w[3]) == (9, 25)
    layers = K.forms(sizes, 5)
    assert [f.gw for f in layers] == [SCALAR] * 4 and [f.delta for f in layers] == [None] + [SCALAR] * 3
    assert [f.forward for f in layers] == [SCALAR, SCALAR, SCALAR, LAST]
    # layer 3 has both widths even: the offset alone decides
    assert sizes[2] % 2 == 0 and sizes[3] % 2 == 0 and off_w[3] % 2 == 1
    assert N.even_width_on_an_odd_offset(sizes) == [2, 3]


def test_both_depths_in_both_forms():
    deep_pair, deep_scalar = [2] * 8 + [1], [3] * 8 + [1]
    assert len(deep_pair) - 1 == len(deep_scalar) - 1 == K.MAX_LAYERS
    layers = K.forms(deep_pair, 3)
    assert [f.gw for f in layers] == [PAIR] * 7 + [SCALAR] and [f.delta for f in layers] == [None] + [PAIR] * 6 + [SCALAR]
    assert [f.forward for f in layers] == [PAIR] * 7 + [LAST]
    layers = K.forms(deep_scalar, 3)
    assert [f.gw for f in layers] == [SCALAR] * 8 and [f.delta for f in layers] == [None] + [SCALAR] * 7
    assert [f.forward for f in layers] == [SCALAR] * 7 + [LAST]
    assert {len(sizes) - 1 for sizes, _, _ in K.CASES} >= {1, 8}


def test_the_trip_counts_the_table_names():
    f = _layer([2, 27, 21, 1], 4, 2)
    assert (f.gw, f.items["gw"], K.trips(f.items["gw"])) == (SCALAR, 567, 2) and 567 % K.THREADS != 0
    f = _layer([2, 64, 66, 1], 17, 2)
    assert (f.gw, f.items["gw"], K.trips(f.items["gw"])) == (PAIR, 1056, 3) and 1056 % K.THREADS != 0
    assert (f.delta, f.items["delta"], K.trips(f.items["delta"])) == (PAIR, 544, 2) and 544 % K.THREADS != 0
    assert K.trips(1056) != -(-1056 // K.K8_THREADS) and K.trips(544) != -(-544 // K.K8_THREADS)      # K8's differ
    first, last = K.forms([2, 600, 1], 3)
    assert first.nout > K.THREADS and (first.gw, first.items["gw"], first.items["gb"]) == (PAIR, 300, None)
    assert (last.gw, last.items["gw"], last.items["gb"]) == (SCALAR, 600, 1)
    assert (last.delta, last.items["delta"], K.trips(last.items["delta"])) == (SCALAR, 1800, 4)
    first = _layer([3, 600, 1], 2, 1)
    assert (first.gw, first.items["gw"], first.items["gb"], K.trips(first.items["gb"])) == (SCALAR, 1800, 600, 2)
    g = K.global_items([4, 1], 513)
    assert K.trips(g["copy_y"]) == K.trips(g["head"]) == K.trips(_layer([4, 1], 513, 1).items["forward"]) == 2
    assert K.trips(g["copy_x"]) == 5
    f = _layer([3, 12, 12, 1], 714, 2)
    assert (f.delta, f.items["delta"], K.trips(f.items["delta"])) == (PAIR, 4284, 9)
    assert K.trips(K.global_items([3, 12, 12, 1], 714)["head"]) == 2
    assert {f.gw for f in K.forms([3, 31, 31, 1], 299)} == {SCALAR}
    f = _layer([2, 48, 48, 1], 90, 2)
    assert (f.delta, f.items["delta"]) == (PAIR, 2160)
    assert _layer(K.DEFAULT, 49, 2).items["delta"] == 1225 and _layer(K.DEFAULT, 116, 3).items["delta"] == 2900
    assert _layer(K.DEFAULT, 49, 2).items["gw"] == 625


def test_the_footprints_the_table_names():
    want = {(K.F32, 36): 65104, (K.F32, 37): 66324, (K.F64, 9): 64168, (K.F64, 10): 66608}
    for (dt, B), total in want.items():
        assert K.lds_bytes(K.DEFAULT, B, K.ESIZE[dt]) == total and (K.DEFAULT, B, dt) in K.CASES
    assert 65104 <= K.OPT_IN < 66324 and 64168 <= K.OPT_IN < 66608
    assert K.lds_bytes([2, 64, 66, 1], 17, 8) == 72904 > K.OPT_IN
    for sizes, B, dt in K.FULL_LDS:
        assert K.lds_bytes(sizes, B, K.ESIZE[dt]) == K.LDS_MAX == 163840 and (sizes, B, dt) in K.CASES
    assert {dt for _, _, dt in K.FULL_LDS} == {K.F32, K.F64}
    assert K.lds_bytes(K.DEFAULT, 20, 8) > K.OPT_IN                        # the f64 opt-in of tests/test_bnn_particles_gpu.py
    for sizes, B, dt in K.LAUNCH_CASES:
        assert (sizes, B, dt) in K.CASES


def test_the_rows_together_cover_every_form_with_more_than_one_trip():
    """All three loops (forward, gW, delta) in both forms, each with more than one trip in at least one dtype; the pair delta
    and, with it, every loop the f64 rows run, in both dtypes; the scalar form's gb loop; the head."""
    reached = {}
    for sizes, B, dt in K.CASES:
        for f in K.forms(sizes, B):
            for loop, form in (("forward", f.forward), ("gw", f.gw), ("delta", f.delta)):
                if form in (PAIR, SCALAR):
                    key = (loop, form, dt)
                    reached[key] = max(reached.get(key, 0), K.trips(f.items[loop]))
            if f.items["gb"] is not None:
                reached[("gb", SCALAR, dt)] = max(reached.get(("gb", SCALAR, dt), 0), K.trips(f.items["gb"]))
            if f.forward == LAST:
                reached[("last", LAST, dt)] = max(reached.get(("last", LAST, dt), 0), K.trips(f.items["forward"]))
    for loop in ("forward", "gw", "delta"):
        for form in (PAIR, SCALAR):
            assert max(reached[(loop, form, K.F32)], reached[(loop, form, K.F64)]) > 1, (loop, form)
            assert min(reached[(loop, form, K.F32)], reached[(loop, form, K.F64)]) >= 1, (loop, form)
    for dt in K.BOTH:
        assert reached[("delta", PAIR, dt)] > 1 and reached[("gw", PAIR, dt)] > 1 and reached[("gw", SCALAR, dt)] > 1
        assert reached[("gb", SCALAR, dt)] > 1 and reached[("last", LAST, dt)] > 1
    assert {B % 8 for _, B, dt in K.CASES if dt == K.F32} == {B % 8 for _, B, dt in K.CASES if dt == K.F64} == set(range(8))
    assert len(K.CASES) == len(set((tuple(s), B, dt) for s, B, dt in K.CASES))


# ---- the references --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes, B", SHAPES, ids=["%s-B%d" % ("x".join(map(str, s)), B) for s, B in SHAPES])
def test_kernel_order_in_f64_agrees_with_the_oracle(oracle, sizes, B):
    """Per layer block within 1e-12 * max|g| of ``oracle.bnn_cost_and_grad``: the restatement and the oracle were written apart,
    so they are not wrong alike. The truth of the GPU tests is held to the oracle the same way."""
    sizes = list(sizes)
    theta, X, y = K.make_data(sizes, B, K.F64, n=2)
    c = K.consts(B)
    for row in theta:
        params = C.split(row, sizes)
        want_cost, want = oracle.bnn_cost_and_grad(params, X, y.reshape(-1, 1), c["batch_size"], c["n_examples"], c["wdecay"],
                                                   c["prior_mean"], c["prior_var"])
        want = K.flatten(want)
        for name, (cost, grads) in (("kernel_order", K.kernel_order(params, X, y, c, K.F64)),
                                    ("statement", K.statement(params, X, y, c, K.F64))):
            got = K.flatten(grads)
            assert got.dtype == np.float64 and got.shape == want.shape
            assert abs(float(cost) - want_cost) <= 1e-12 * abs(want_cost), (name, cost, want_cost)
            for block, _, where in K.blocks(sizes):
                top = float(np.abs(want[where]).max())
                assert top > 0.0
                dev = float(np.abs(got[where] - want[where]).max())
                assert dev <= 1e-12 * top, (name, block, dev, top)


def test_the_prior_term_of_kernel_order_is_one_multiply_and_one_add():
    sizes, B = [2, 4, 6, 3, 1], 5
    for dt in K.BOTH:
        theta, X, y = K.make_data(sizes, B, dt, n=1)
        c = K.consts(B)
        params = C.split(theta[0], sizes)
        cost_raw, raw = K.kernel_order(params, X, y, c, dt, add_prior=False)
        cost_full, full = K.kernel_order(params, X, y, c, dt)
        coef = dt(c["wdecay"] / ((float(C.n_params(sizes)) + (2.0 * 1e-16 + 1e-16)) * c["n_examples"]))
        want = K.flatten(raw) + coef * theta[0]
        assert want.dtype == np.dtype(dt) and np.array_equal(K.flatten(full), want) and cost_raw == cost_full
        assert not np.array_equal(K.flatten(full), K.flatten(raw))


def test_the_f32_kernel_order_is_the_scalar_loop_bit_for_bit():
    def bits(a):
        return np.ascontiguousarray(a).view(np.uint32)

    sizes = [2, 4, 6, 3, 1]
    for B in (5, 8):
        theta, X, y = K.make_data(sizes, B, K.F32, n=2)
        for row in theta:
            for add_prior in (True, False):
                cost, grads = K.kernel_order(C.split(row, sizes), X, y, K.consts(B), K.F32, add_prior=add_prior)
                want_cost, want = K.scalar_loop_f32(C.split(row, sizes), X, y, K.consts(B), add_prior=add_prior)
                assert cost.dtype == want_cost.dtype == np.float32 and bits(cost) == bits(want_cost)
                for k, (g, w) in enumerate(zip(grads, want)):
                    assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, k
                    assert np.array_equal(bits(g), bits(w)), (B, add_prior, k)


def test_the_emulated_block_sum_has_the_kernel_s_order():
    rng = np.random.RandomState(3)
    v = rng.randn(1300)
    # 1300 = 2 full rounds of 512 lanes and 276: lane t holds v[t] + v[t + 512] + v[t + 1024] added in that order
    parts = np.zeros(K.THREADS)
    for t in range(K.THREADS):
        for i in range(t, v.size, K.THREADS):
            parts[t] = parts[t] + v[i]
    waves = []
    for w in range(8):
        lanes = list(parts[64 * w:64 * w + 64])
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[t] + lanes[t ^ o] for t in range(64)]
        assert len(set(lanes)) == 1                                    # the butterfly leaves one value in every lane
        waves.append(lanes[0])
    total = 0.0
    for w in waves:
        total = total + w
    assert K.block_sum(v) == total and abs(total - v.sum()) <= 1e-12


def test_the_reference_s_own_error_is_measured_per_layer_and_never_a_lucky_zero():
    """E of a layer is taken over gW_l and gb_l of all particles together, so a block of one element (gb of the last layer,
    d / d log_var) is not bounded by its own, possibly zero, error alone."""
    for dt in K.BOTH:
        if dt == K.F64 and not K.LONG_DOUBLE_IS_WIDER:
            continue
        case = K.case([2, 4, 6, 3, 1], 5, dt)
        assert set(case.E) == {1, 2, 3, 4, "dlog_var", "cost"}
        for layer in (1, 2, 3, 4):
            assert 0.0 < case.E[layer] <= 64 * K.U[dt] * float(np.abs(case.truth_grad).max()), (dt, layer, case.E[layer])
        names = [name for name, _, _, _ in K.bounds(case, 0)]
        assert names == ["gW1", "gb1", "gW2", "gb2", "gW3", "gb3", "gW4", "gb4", "dlog_var", "cost"]
        for name, where, E, bound in K.bounds(case, 0):
            assert bound > 0.0 and bound >= 4.0 * E
        by_name = {name: E for name, _, E, _ in K.bounds(case, 0)}
        assert by_name["gW4"] == by_name["gb4"] == case.E[4]


# ---- what no test of the values can see ------------------------------------------------------------------------------------------

def test_the_parity_conditions_and_the_strides_the_restatement_rests_on_are_the_source_s():
    """Two edits leave every VALUE as it is, so the GPU tests cannot see them (tried by hand, profiles/bnn_particles_forms.txt):
    a pair loop on an odd weight offset (the LDS replays the misaligned access: cycles, not bits) and a strided loop that
    strides by less than the workgroup (items computed twice, equal values written again). The conditions ``forms`` restates and
    the stride of every strided loop are therefore read from the source; if the kernel is rewritten, re-read them."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pysgmcmc_amd", "csrc")
    with open(os.path.join(csrc, "sgmcmc_bnn_particles.hip")) as f:
        kernel = " ".join(f.read().split())
    with open(os.path.join(csrc, "sgmcmc_bnn_small_net.hpp")) as f:
        core = " ".join(f.read().split())
    assert "const bool pj = (nout % 2 == 0) && ((ow | a.net.lds_d[l]) % 2 == 0);" in kernel
    assert "const bool pk = (nin % 2 == 0) && (a.net.lds_h[l - 1] % 2 == 0);" in kernel
    assert "if (pj && pk && a.net.lds_d[l - 1] % 2 == 0) {" in kernel
    assert "const bool pairs = (nout % 2 == 0) && ((net.off_w[l] | net.off_b[l]) % 2 == 0);" in core
    assert "constexpr int PARTICLES_THREADS = %d;" % K.THREADS in kernel and "const int tid = threadIdx.x, nt = blockDim.x;" in kernel
    body = kernel[kernel.index("__global__ void __launch_bounds__(PARTICLES_THREADS) bnn_particles_kernel"):
                  kernel.index("// the checks every entry shares")]
    strided = re.findall(r"for \(int (\w+) = tid; \w+ < [^;]+; (\w+) \+= ([^)]+)\)", body)
    assert len(strided) == 9, strided                     # X, y, the sum of squares, the head, gW x 2, gb, delta x 2
    assert all(var == again and step == "nt" for var, again, step in strided), strided
    forward = core[core.index("forward_tile(const SmallNet &net"):core.index("// ens_mean[r]")]
    strided = re.findall(r"for \(int (\w+) = tid; \w+ < [^;]+; (\w+) \+= ([^)]+)\)", forward)
    assert len(strided) == 3 and all(var == again and step == "nt" for var, again, step in strided), strided
