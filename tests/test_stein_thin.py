"""Greedy Stein thinning without a GPU: the host statement ``diagnostics.stein.stein_thinning_indices`` of K17's arithmetic
contract (include/sgmcmc_hip_thin.h) against the brute-force definition, its path against the direct sum, thinned against
strided subsets, ties, DISTINCT, the numpy route of ``diagnostics.stein_thinning``, the launch plan and the refusals of the C
entry points (checked on the host before anything is launched)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pysgmcmc_amd import _lib, diagnostics, kernels
from pysgmcmc_amd.diagnostics import stein

import stein_thin_cases as M

WIDE = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64


def test_the_new_names_are_exported():
    for name in ("stein_thin", "stein_thin_plan", "stein_thin_max_samples"):
        assert name in kernels.__all__ and callable(getattr(kernels, name))
    for name in ("SteinThinning", "stein_thinning", "stein_thinning_indices"):
        assert name in diagnostics.__all__ and hasattr(diagnostics, name) and name in stein.__all__
    assert diagnostics.SteinThinning._fields == ("indices", "ksd_path", "v_path", "discrepancy")
    assert diagnostics.SteinDiscrepancy._fields[-1] == "thinning"            # still the stride of a thinned trace
    assert kernels.stein_thin_max_samples() == stein.MAX_SAMPLES == 4096
    assert _lib.lib().sgmcmc_stein_thin_abi_version() == _lib.THIN_ABI_VERSION == 1


def test_both_new_files_are_build_dependencies():
    deps = [os.path.basename(p) for p in _lib.build_dependencies()]
    assert "sgmcmc_stein_thin.hip" in deps and "sgmcmc_hip_thin.h" in deps


def test_the_size_table_reaches_every_launch_form():
    forms = lambda sizes: {kernels.stein_thin_plan(n, 1)[:2] + kernels.stein_thin_plan(n, 1)[3:] for n in sizes}
    every = forms(range(2, 4097))
    assert forms(M.SIZES) == every
    assert every == {(64, 1, 1), (256, 1, 4), (1024, 1, 16), (1024, 2, 16), (1024, 3, 16), (1024, 4, 16)}
    for n in range(2, 4097):
        p = kernels.stein_thin_plan(n, 7, 5)
        assert p.block * p.columns_per_thread >= n and p.waves * 64 == p.block and p.grid == 5
        assert p.block == 64 or n > p.block // 4                             # the smallest block that holds n
    # m and batch do not move the form
    assert kernels.stein_thin_plan(300, 65536, 65535)[:2] == kernels.stein_thin_plan(300, 1, 1)[:2]
    for bad in ((1, 1, 1), (4097, 1, 1), (8, 0, 1), (8, 65537, 1), (8, 1, 0), (8, 1, 65536)):
        with pytest.raises(_lib.SgmcmcLibraryError, match="stein_thin_plan: "):
            kernels.stein_thin_plan(*bad)


# ---- the host statement -----------------------------------------------------------------------------------------------------

def _gauss_matrix(n, d):
    X, S = M.gauss(n, d)
    return stein.stein_kernel_matrix(X, S)


_GAUSS = {}


def _gauss_case(n, d, m):
    if (n, d) not in _GAUSS:
        K = _gauss_matrix(n, d)
        K.setflags(write=False)
        _GAUSS[(n, d)] = (K,) + stein.stein_thinning_indices(K, m)
    return _GAUSS[(n, d)]


def _brute_force(K, m):
    """pi(t) = argmin_j K_jj / 2 + sum_{t' < t} K[pi(t'), j], the objective recomputed from scratch at every step."""
    Kw = K.astype(WIDE)
    picks, gaps = [], []
    for _ in range(m):
        obj = np.diag(Kw) / 2 + (Kw[picks].sum(axis=0) if picks else 0)
        order = np.argsort(obj, kind="stable")
        picks.append(int(order[0]))
        gaps.append(float((obj[order[1]] - obj[order[0]]) / abs(obj[order[0]])))
    return picks, min(gaps)


@pytest.mark.parametrize("n,d,m", M.GAUSS)
def test_picks_equal_the_brute_force_definition(n, d, m):
    K, idx, path = _gauss_case(n, d, m)
    want, gap = _brute_force(K, m)
    print("n = %d, d = %d, m = %d: smallest relative gap between the best and the second objective %.2e" % (n, d, m, gap))
    assert gap > 1e-6                                                        # far above rounding: no tie risk
    assert idx.dtype == np.int32 and path.dtype == np.float64 and idx.tolist() == want


@pytest.mark.parametrize("n,d,m", M.GAUSS)
def test_the_path_is_the_v_statistic_of_the_picks(n, d, m):
    K, idx, path = _gauss_case(n, d, m)
    sub = K[np.ix_(idx, idx)]
    direct = float(np.sum(sub)) / (m * m)
    bound = (m * m) * 2.0 ** -53 * float(np.abs(sub).sum()) / (m * m)
    print("path[-1] = %.17g, direct = %.17g, difference %.2e, bound %.2e" % (path[-1], direct, abs(path[-1] - direct), bound))
    assert abs(path[-1] - direct) <= bound
    for t in (1, 2, m // 2):                                                 # and of every prefix
        s = K[np.ix_(idx[:t], idx[:t])]
        assert abs(path[t - 1] - float(np.sum(s)) / (t * t)) <= 2.0 ** -53 * float(np.abs(s).sum())


@pytest.mark.parametrize("n,d,m", M.GAUSS)
def test_thinned_is_below_strided(n, d, m):
    K, idx, path = _gauss_case(n, d, m)
    strided = np.arange(0, n, n // m)[:m]
    v_strided = float(np.sum(K[np.ix_(strided, strided)])) / (m * m)
    v_full = float(np.sum(K)) / (n * n)
    print("n = %d, m = %d: V thinned %.3f, strided %.3f, full sample %.3f" % (n, m, path[-1], v_strided, v_full))
    assert path[-1] < v_strided


def test_ties_go_to_the_smallest_index():
    K = np.full((9, 9), 2.5)
    idx, path = stein.stein_thinning_indices(K, 7)
    assert idx.tolist() == [0] * 7 and np.array_equal(path, np.full(7, 2.5))
    idx, _ = stein.stein_thinning_indices(K, 9, distinct=True)
    assert idx.tolist() == list(range(9))
    for cols in ((0, 63), (5, 1029, 2053, 3077)):
        T = M.tie_matrix(cols, M.F32, n=3100)
        idx, _ = stein.stein_thinning_indices(T, 6)
        assert idx.tolist() == [cols[0]] * 6
        idx, _ = stein.stein_thinning_indices(T, len(cols) + 2, distinct=True)
        assert idx.tolist()[:len(cols)] == list(cols)


def test_a_duplicated_sample_is_picked_at_its_first_row():
    n, d, m = 40, 5, 30
    X, S = M.biased(np.random.default_rng(1), n, d)
    X[5] = X[17] = 0.05                                                      # one sample near the target's mode, twice
    S[5] = S[17] = -0.05
    K = stein.stein_kernel_matrix(X, S, order="k")
    assert np.array_equal(K[5], K[17]) and np.array_equal(K[:, 5], K[:, 17])
    idx, _ = stein.stein_thinning_indices(K, m)
    assert 5 in idx.tolist() and 17 not in idx.tolist()                      # equal objectives at every step: 5 wins
    idx, _ = stein.stein_thinning_indices(K, m, distinct=True)
    idx = idx.tolist()
    assert 5 in idx and (17 not in idx or idx.index(5) < idx.index(17))


@pytest.mark.parametrize("n", [2, 37])
def test_distinct_with_m_equal_n_is_a_permutation(n):
    K = M.matrix(64, M.F64)[:n, :n]
    idx, path = stein.stein_thinning_indices(K, n, distinct=True)
    assert sorted(idx.tolist()) == list(range(n))
    assert abs(path[-1] - float(np.sum(K)) / (n * n)) <= 2.0 ** -53 * float(np.abs(K).sum())    # all of them: the full V


def test_argument_errors():
    K = M.matrix(64, M.F64)
    with pytest.raises(ValueError, match=r"must be \(n, n\)"):
        stein.stein_thinning_indices(K[:, :5], 3)
    with pytest.raises(ValueError, match=r"must be \(n, n\)"):
        stein.stein_thinning_indices(K[:1, :1], 1)
    with pytest.raises(ValueError, match="m must be at least 1"):
        stein.stein_thinning_indices(K, 0)
    with pytest.raises(ValueError, match="distinct picks need m <= n"):
        stein.stein_thinning_indices(K, 65, distinct=True)
    X, S = M.biased(np.random.default_rng(2), 30, 4)
    with pytest.raises(ValueError, match="m must be at least 1"):
        diagnostics.stein_thinning(X, S, 0)
    with pytest.raises(ValueError, match="distinct picks need m <= 30"):
        diagnostics.stein_thinning(X, S, 31, distinct=True)
    with pytest.raises(ValueError, match="distinct picks need m <= 10"):
        diagnostics.stein_thinning(X.reshape(3, 10, 4), S.reshape(3, 10, 4), 11, distinct=True, per_chain=True)
    with pytest.raises(ValueError, match=r"per_chain=True needs samples as \(chains, n, d\)"):
        diagnostics.stein_thinning(X, S, 3, per_chain=True)
    with pytest.raises(ValueError, match="differ in shape"):
        diagnostics.stein_thinning(X.reshape(3, 10, 4), S.reshape(2, 15, 4), 3, per_chain=True)
    with pytest.raises(ValueError, match="at least 2 rows"):
        diagnostics.stein_thinning(X.reshape(30, 1, 4), S.reshape(30, 1, 4), 1, per_chain=True)
    with pytest.raises(ValueError, match="kernel must be"):
        diagnostics.stein_thinning(X, S, 3, kernel="laplace")
    with pytest.raises(ValueError, match="4096.*thin"):
        diagnostics.stein_thinning(np.zeros((4097, 2)), np.zeros((4097, 2)), 3)


def test_the_numpy_route_is_the_two_host_statements():
    n, d, m = 90, 6, 12
    X, S = M.biased(np.random.default_rng(3), n, d)
    for kw in (dict(), dict(kernel="rbf", bandwidth=3.0), dict(distinct=True)):
        kern = {k: v for k, v in kw.items() if k != "distinct"}
        K = stein.stein_kernel_matrix(X, S, **kern)
        idx, path = stein.stein_thinning_indices(K, m, **{k: v for k, v in kw.items() if k == "distinct"})
        got = diagnostics.stein_thinning(X.reshape(3, 30, d), S.reshape(3, 30, d), m, **kw)       # pooled
        assert isinstance(got, diagnostics.SteinThinning)
        assert np.array_equal(got.indices, idx) and np.array_equal(got.v_path, path)
        assert np.array_equal(got.ksd_path, np.sqrt(np.maximum(path, 0.0)))
        want = diagnostics.kernel_stein_discrepancy(X, S, return_matrix=True, **kern)
        assert got.discrepancy.v_statistic == want.v_statistic and np.array_equal(got.discrepancy.matrix, K)
        assert got.discrepancy.thinning == 1
        chains = diagnostics.stein_thinning(X.reshape(3, 30, d), S.reshape(3, 30, d), m, per_chain=True, **kw)
        assert chains.indices.shape == chains.v_path.shape == chains.ksd_path.shape == (3, m)
        for p in range(3):
            blk = K[30 * p:30 * p + 30, 30 * p:30 * p + 30]
            i, v = stein.stein_thinning_indices(blk, m, kw.get("distinct", False))
            assert np.array_equal(chains.indices[p], i) and np.array_equal(chains.v_path[p], v)
    t = diagnostics.stein_thinning(torch.from_numpy(X), torch.from_numpy(S), m)                   # CPU tensors: the same route
    assert t.indices.dtype == torch.int32 and t.v_path.dtype == torch.float64
    K = stein.stein_kernel_matrix(X, S)
    idx, path = stein.stein_thinning_indices(K, m)
    assert np.array_equal(t.indices.numpy(), idx) and np.array_equal(t.v_path.numpy(), path)


# ---- the C entry points refuse on the host ----------------------------------------------------------------------------------

# never dereferenced: every call below fails before anything is launched
_BASE = dict(matrix=4096, ld_m=8, n=8, m=4, batch=2, batch_stride=72, flags=0, indices=8192, path=12288)
REFUSALS = M.REFUSALS


def thin_call(sfx, **over):
    a = dict(_BASE, **over)
    f = getattr(_lib.lib(), "sgmcmc_stein_thin_" + sfx)
    return f(a["matrix"], a["ld_m"], a["n"], a["m"], a["batch"], a["batch_stride"], a["flags"], a["indices"], a["path"], None)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_refusals_come_in_the_header_s_order(sfx):
    lib = _lib.lib()
    for i, (wrong, text) in enumerate(REFUSALS):
        assert thin_call(sfx, **wrong) == -1 and lib.sgmcmc_last_error() == text
        for later, _ in REFUSALS[i + 1:]:                                    # an earlier check wins over a later one
            assert thin_call(sfx, **dict(later, **wrong)) == -1
            assert lib.sgmcmc_last_error() == text, (wrong, later)
    for wrong, text in ((dict(indices=None), b"stein_thin: null pointer"), (dict(n=4097), b"stein_thin: n = 4097 outside [2, 4096]"),
                        (dict(m=65537), b"stein_thin: m = 65537 outside [1, 65536]"),
                        (dict(batch=65536), b"stein_thin: batch = 65536 outside [1, 65535]")):
        assert thin_call(sfx, **wrong) == -1 and lib.sgmcmc_last_error() == text
    out = (ctypes.c_int * 4)()
    assert lib.sgmcmc_stein_thin_plan(1, 1, 1, out, 4) == -1 and lib.sgmcmc_last_error().startswith(b"stein_thin_plan: n = 1")
    assert lib.sgmcmc_stein_thin_plan(300, 5, 7, out, 4) == 1 and list(out) == [1024, 1, 7, 16]
    assert lib.sgmcmc_stein_thin_plan(300, 5, 7, None, 0) == 1


def test_the_front_end_checks_the_matrix_and_the_outputs():
    K = torch.zeros(8, 8)
    with pytest.raises(TypeError, match="float32/float64"):
        kernels.stein_thin(K.to(torch.float16), 3)
    with pytest.raises(ValueError, match="two-dimensional"):
        kernels.stein_thin(K.reshape(-1), 3)
    with pytest.raises(ValueError, match="dense rows"):
        kernels.stein_thin(K.t()[:, ::2], 3)
    with pytest.raises(ValueError, match="does not lie inside"):
        kernels.stein_thin(K, 3, n=4, batch=3, batch_stride=4 * 8 + 4)
    with pytest.raises(ValueError, match="does not lie inside"):
        kernels.stein_thin(K, 3, n=9)
    with pytest.raises(ValueError, match="indices must be 3 contiguous"):
        kernels.stein_thin(K, 3, indices=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(_lib.SgmcmcLibraryError):                             # no CPU path
        kernels.stein_thin(K, 3)
