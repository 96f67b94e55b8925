"""The premise of ``svgd_many_exact_cases.py`` without a GPU: for every lattice cloud, in both dtypes, the squared distances
are exact integers that the dtype holds, no partial sum of a column sum or of a centred Gram entry can leave the dtype in any
order of summation, ``fl(fl(sqrt(k))^2)`` is the oracle's D bit for bit, and an emulation of the kernels' own order (eight
interleaved row chains times fl(1 / n) for the mean, the centred Gram columns added in shuffled orders, DIST's expression)
gives that same D. Then the structural fact each family is there for, and the oracle's own error at the small-n and
translated step cases against the table behind ``svgd_many_cases.C``, which stays as it is."""
import numpy as np
import pytest

import svgd_many_cases as M
import svgd_many_exact_cases as E

F32, F64 = M.F32, M.F64
DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]
LATTICE = [pytest.param(*case, id="%s-%dx%d" % case) for case in E.LATTICE]


def test_the_cases_are_the_issue_s():
    assert [c[1:] for c in E.LATTICE if c[0] == "balanced"] == [(3, 2), (46, 5), (129, 3), (130, 40), (161, 7), (1024, 6)]
    assert [c[1:] for c in E.LATTICE if c[0] == "clusters"] == [(130, 3), (256, 3)] and E.CLUSTER_POINT == (3, -1, 2)
    assert [c[1:] for c in E.LATTICE if c[0] == "offset"] == [(256, 33), (512, 5)]
    assert E.OFFSET_C == {(256, 33): 4096, (512, 5): 1000}
    assert [c[1:] for c in E.LATTICE if c[0] in ("sphere", "boundary")] == [(256, 258), (256, 258)]
    # the issue's r = 8 in f32 puts the keys on both sides of 2^23, where they cannot agree in their upper bytes: that cloud
    # is the family ``boundary``, and ``sphere`` uses r = 7 in f32
    assert E.SPHERE_R == {"sphere": {F32: 7, F64: 185363}, "boundary": {F32: 8, F64: 131072}}
    assert 2 * (256 * 8) ** 2 == 2 ** 23 and 2 * (256 * 131072) ** 2 == 2 ** 51
    assert 2 ** 22 < 2 * (256 * 7) ** 2 < 2 ** 23 - 2 ** 16 and 2 ** 52 - 2 ** 45 < 2 * (256 * 185363) ** 2 < 2 ** 52
    assert E.SMALL == [(2, 1), (3, 2), (16, 5), (17, 33), (45, 7), (46, 7), (65, 20), (127, 3)]
    assert E.TRANSLATED == [(129, 40), (257, 3)] and E.TRANSLATION == 100.0
    assert max(n for _, n, _ in E.LATTICE) == 1024 and max(n * d for _, n, d in E.LATTICE) == 256 * 258


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,n,d", LATTICE)
def test_every_sum_of_a_lattice_cloud_is_exact(family, n, d, dtype):
    ref = E.exact_reference(family, n, d, dtype)
    X, bits = ref.X, E.MANTISSA[dtype]
    k = E.exact_sqdist(X)
    assert k.min() == 0 and np.all(np.diag(k) == 0) and np.array_equal(k, k.T)
    assert k.max() < 2 ** bits, "a squared distance needs more than %d bits" % bits
    col, gram, s, Y = E.partial_sum_bounds(X, dtype)
    print("%s %d x %d %s: largest k %d, column sum %d, Gram partial sum %d / %d (limit 2^%d)" % (
        family, n, d, np.dtype(dtype).name, k.max(), col, gram, s * s, bits))
    assert col <= 2 ** bits and gram <= 2 ** bits
    # the mean is a number of the dtype, and so are the three terms of DIST:  g_ii + g_jj,  2 g_ij,  their difference
    g = Y @ Y.T                                                       # s^2 x the centred Gram matrix, exact in int64
    diag = np.diag(g)
    assert E.fits(diag[:, None] + diag[None, :], dtype) and E.fits(2 * g, dtype)
    assert np.array_equal((diag[:, None] + diag[None, :]) - 2 * g, s * s * k)
    mean = E.emulated_mean(X)
    assert np.array_equal(mean.astype(np.float64) * n, X.astype(np.float64).sum(axis=0)), "the mean is not exact"
    # fl(fl(sqrt(k))^2) is the oracle's D in the case's dtype, and so is the kernels' order of summation
    D = E.roundtrip(k, dtype)
    assert D.dtype == ref.D.dtype == dtype and np.array_equal(E.keys(D), E.keys(ref.D))
    rng = np.random.default_rng([n, d, 7])
    for order in [np.arange(d), np.arange(d)[::-1]] + [rng.permutation(d) for _ in range(3)]:
        assert np.array_equal(E.keys(E.emulated_sqdist(X, order)), E.keys(ref.D)), "the Gram form of D is not the oracle's"
    assert ref.med == M.O.svgd_median(ref.D) and np.asarray(ref.med).dtype == dtype


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,n,d", LATTICE)
def test_each_family_puts_the_median_where_it_is_meant_to_be(family, n, d, dtype):
    ref = E.exact_reference(family, n, d, dtype)
    f = E.select_facts(ref.D)
    print("%s %d x %d %s: %d distinct keys, count_le - mid = %d" % (family, n, d, np.dtype(dtype).name, f.distinct,
                                                                   f.count_le - f.mid))
    assert f.N == n * n and f.mid == n * n // 2
    assert (n * n) % 2 == (1 if n in (3, 129, 161) else 0)
    k = np.sort(E.keys(ref.D))
    if family == "clusters":
        # half the keys 0, half 56': the upper middle value is NEXT's next_key, and one off in `> mid` gives 0 or 56'
        fifty_six = E.roundtrip(np.array([56]), dtype)[0]
        assert f.lo == 0 and f.count_le == f.mid and f.distinct == 2
        assert f.next_key == int(E.keys(np.array([fifty_six]))[0])
        assert ref.med == fifty_six / dtype(2) and ref.med not in (0, fifty_six)
    else:
        assert f.count_le > f.mid                                    # the rank falls inside a tie
    if family == "balanced":
        below = int(np.searchsorted(k, f.lo, side="left"))
        assert below <= f.rank < f.count_le and 3 <= f.distinct <= 64
        if n >= 46:
            assert f.count_le - below > 2 * n                        # a tie that no continuous cloud has
    nonzero = k[k != 0]
    if family == "sphere" or (family == "boundary" and dtype == F64):
        assert int(nonzero[0]) ^ int(nonzero[-1]) < 2 ** 16          # the early passes see one bin; the last ones decide
        assert 60 <= f.distinct <= 80
    if family == "boundary":
        edge = 2.0 ** 23 if dtype == F32 else 2.0 ** 51
        positive = ref.D[ref.D > 0]
        if dtype == F32:
            assert positive.min() == edge - 0.5 and positive.max() > edge     # both sides of the exponent boundary
            assert int(nonzero[0]) ^ int(nonzero[-1]) >= 2 ** 24      # pass 0 splits them, every later byte differs
            assert f.lo > int(E.keys(np.array([edge], dtype))[0])     # the median is above, the lower keys are skipped
        else:
            assert positive.min() == edge + 0.5
    if family == "offset":
        assert np.array_equal(E.emulated_mean(ref.X), np.full(d, E.OFFSET_C[(n, d)], dtype))
        assert float(np.abs(ref.X).max()) ** 2 * d > 100 * float(ref.D.max())     # uncentred Gram entries dwarf D


def test_the_select_grid_sizes_the_small_cases_are_there_for():
    import torch
    from pysgmcmc_amd import kernels
    grid = lambda n: [l.grid for l in kernels.svgd_many_plan(n, 3, torch.float32) if l.id == 4][0]
    assert (grid(45), grid(46), grid(129), grid(1024)) == (1, 2, 9, 256)
    for n, np16, blocks in ((2, 16, 1), (16, 16, 1), (17, 32, 1), (65, 80, 2), (127, 128, 2)):
        plan = {l.id: l for l in kernels.svgd_many_plan(n, 3, torch.float32)}
        assert plan[7].grid == np16 and plan[M.GRAM].grid == blocks * (blocks + 1) // 2


# ---- the oracle's own error at the new step cases: C stays -----------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_the_oracle_s_own_error_at_the_new_step_cases_is_inside_the_table_s_worst(dtype):
    if dtype == F64 and not M.LONG_DOUBLE_IS_WIDER:
        return                                                   # nothing wider than f64 to measure against here
    worst = M.WORST[dtype][1]
    assert M.C[dtype] == 8 * worst and M.WORST == {F32: ((512, 70, -1), 3.912), F64: ((1024, 65, 1), 4.484)}
    for n, d in E.SMALL:
        for sign in (1, -1):
            rx, rh = M.narrow_against_wide(M.Case(n, d, dtype, sign))
            print("%s small %d x %d sign %+d: %.3f (X), %.3f (H) units" % (np.dtype(dtype).name, n, d, sign, rx, rh))
            assert max(rx, rh) <= worst, (n, d, sign)
    for n, d in E.TRANSLATED:
        for sign in (1, -1):
            rx, rh = E.translated_narrow_against_wide(n, d, dtype, sign)
            print("%s translated %d x %d sign %+d: %.3f (X), %.3f (H) units" % (np.dtype(dtype).name, n, d, sign, rx, rh))
            assert max(rx, rh) <= worst, (n, d, sign)
