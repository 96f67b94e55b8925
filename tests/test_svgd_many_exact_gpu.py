"""The many-particle SVGD path (csrc/sgmcmc_svgd_many.hip) on the GPU where ``test_svgd_many_gpu.py`` cannot see it:

  * lattice clouds (``svgd_many_exact_cases.py``): every sum of MEAN, GRAM, REDUCE and DIST is exact, so the median that SELECT,
    NEXT and BANDWIDTH leave in the header is compared with the oracle's IN THE CASE'S DTYPE with ``==``, with the rank inside
    ties of up to 1e5 keys, at ``count_le == mid`` exactly, at odd counts, and with keys that differ in their last bytes only;
  * the raw entries at 2 .. 127 particles, next to the register-resident path, which runs all of them;
  * a cloud 100 away from the origin (the centring);
  * every subset of the kernel entry's three outputs;
  * a workspace that has just held a larger problem.

Bars: ``TOL`` and ``C`` of svgd_many_cases.py, unchanged, through the helpers of test_svgd_many_gpu.py. Measured on an MI355X,
units of the displacement bar at c = 1 (X, H): see profiles/svgd_many.txt, section 4."""
import math

import numpy as np
import pytest
import torch

from pysgmcmc_amd import kernels

import svgd_many_cases as M
import svgd_many_exact_cases as E
import test_svgd_many_gpu as G

pytestmark = pytest.mark.gpu

DEV = G.DEV
F32, F64 = M.F32, M.F64
CANARY, TAIL = G.CANARY, G.TAIL
DTYPES = G.DTYPES
LATTICE = [pytest.param(*case, id="%s-%dx%d" % case) for case in E.LATTICE]
SMALL = [pytest.param(n, d, id="%dx%d" % (n, d)) for n, d in E.SMALL]
TRANSLATED = [pytest.param(n, d, id="%dx%d" % (n, d)) for n, d in E.TRANSLATED]


def _name(dtype):
    return np.dtype(dtype).name


def _fresh(n, like):
    ws = kernels.svgd_many_workspace(n, like)
    ws.fill_(float("nan"))                                            # a word that is read but never written shows
    return ws


def _check_words(what, words, med, n, dtype):
    """{median, h, h^2} of the header: the median and h^2 = h * h bit for bit, h to the rounding of log and sqrt"""
    assert words.dtype == dtype and words.shape == (3,)
    med = np.asarray(med, dtype)
    assert words[0] == med and E.keys(words[:1])[0] == E.keys(med.reshape(1))[0], \
        "%s: median %r, the oracle's %r (%d keys apart)" % (what, words[0], med[()], int(E.keys(words[:1])[0]) - int(E.keys(med.reshape(1))[0]))
    assert E.keys(words[2:3])[0] == E.keys(np.asarray(words[1] * words[1], dtype).reshape(1))[0], what + ": h2 is not h * h"
    np.testing.assert_allclose(float(words[1]), math.sqrt(0.5 * float(med) / math.log(n + 1.0)), rtol=M.TOL[dtype]["rtol"],
                               err_msg=what)


# ---- B: median and bandwidth words on lattice clouds, exact ------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,n,d", LATTICE)
def test_the_median_of_a_lattice_cloud_is_the_oracle_s_bit_for_bit(family, n, d, dtype):
    ref = E.exact_reference(family, n, d, dtype)
    what = "%s %d x %d %s" % (family, n, d, _name(dtype))
    x = G._dev(ref.X)
    ws = _fresh(n, x)
    K, kg, bw = kernels.svgd_many_kernel(x.reshape(-1), n, d, ws)
    torch.cuda.synchronize()
    assert torch.equal(x, G._dev(ref.X)), what + ": the kernel entry wrote to X"
    K, kg, bw = K.cpu().numpy(), kg.cpu().numpy(), bw.cpu().numpy()
    _check_words(what + " [kernel entry]", bw, ref.med, n, dtype)
    assert np.array_equal(E.keys(ws[:3].cpu().numpy()), E.keys(bw))
    G._check_kernel(what, ref.X, K, kg, bw, ref.K, ref.kg, ref.h, ref.med64, dtype)   # K symmetric bit for bit, unit diagonal
    if family == "clusters":
        same = np.all(ref.X[:, None, :] == ref.X[None, :, :], axis=2)
        assert same.sum() == n * n // 2 and np.all(K[same] == 1.0), what + ": K is not exactly 1 inside a cluster"
    # the same words after the step entry's own kernel-matrix pass
    X, Gr, H = E.lattice_step_inputs(family, n, d, dtype)
    xs, g, h = (G._dev(a).reshape(-1) for a in (X, Gr, H))
    ws = _fresh(n, xs)
    kernels.svgd_many_step(xs, g, h, n, d, M.EPS, M.ALPHA, M.FUDGE, ws, repulsion_sign=-1)
    torch.cuda.synchronize()
    words = ws[:3].cpu().numpy()
    _check_words(what + " [step entry]", words, ref.med, n, dtype)
    assert np.array_equal(E.keys(words), E.keys(bw)), what + ": the two entries leave different header words"
    assert torch.isfinite(xs).all() and torch.isfinite(h).all() and not torch.equal(xs, G._dev(X).reshape(-1))
    assert torch.equal(g, G._dev(Gr).reshape(-1))


# ---- C: the raw entries below 64 particles and up to 127 ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", SMALL)
def test_kernel_matrix_below_128_particles(n, d, dtype):
    G.test_kernel_matrix_matches_the_oracle(n, d, dtype)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", SMALL)
def test_single_step_below_128_particles(n, d, dtype, sign):
    G.test_single_step_matches_the_oracle(n, d, dtype, sign)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", SMALL)
def test_both_paths_agree_below_128_particles(n, d, dtype):
    G.test_both_paths_agree_where_both_run(n, d, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", [(3, 2), (46, 5)])
def test_both_paths_on_a_lattice_cloud(n, d, dtype):
    """The tiled path's median is exact; the register-resident path's, which forms D another way, at its ``rtol``."""
    ref = E.exact_reference("balanced", n, d, dtype)
    x = G._dev(ref.X).reshape(-1)
    tol = M.TOL[dtype]
    new = [t.cpu().numpy() for t in kernels.svgd_many_kernel(x, n, d, _fresh(n, x))]
    old = [t.cpu().numpy() for t in kernels.svgd_kernel(x, n, d, kernels.svgd_workspace(n, x))]
    _check_words("tiled balanced %d x %d %s" % (n, d, _name(dtype)), new[2], ref.med, n, dtype)
    for (K, kg, bw), name in ((old, "register-resident"), (new, "tiled")):
        G._check_kernel("%s balanced %d x %d" % (name, n, d), ref.X, K, kg, bw, ref.K, ref.kg, ref.h, ref.med64, dtype)
    np.testing.assert_allclose(old[2][0], float(ref.med), rtol=tol["rtol"])
    np.testing.assert_allclose(new[0], old[0], **tol)
    np.testing.assert_allclose(new[2][:2], old[2][:2], rtol=tol["rtol"])


# ---- D: translation, requested outputs, a used workspace -------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", TRANSLATED)
def test_a_cloud_100_away_from_the_origin(n, d, dtype):
    """MEAN's centring: K, h and the kernel gradients against the f64 oracle on the rounded inputs at ``TOL`` (the gradient
    scale is |X|.max() of the shifted cloud), one step per sign at ``C``."""
    X, K_ref, kg_ref, h_ref, med_ref = E.translated_kernel_reference(n, d, dtype)
    assert 90 < np.abs(X).min() and X.dtype == dtype
    x = G._dev(X)
    K, kg, bw = kernels.svgd_many_kernel(x.reshape(-1), n, d, _fresh(n, x))
    torch.cuda.synchronize()
    assert torch.equal(x, G._dev(X))
    G._check_kernel("translated K %d x %d %s" % (n, d, _name(dtype)), X, K.cpu().numpy(), kg.cpu().numpy(), bw.cpu().numpy(),
                    K_ref, kg_ref, h_ref, med_ref, dtype)
    for sign in (1, -1):
        ref = E.translated_step_reference(n, d, dtype, sign)
        xs, g, h = (G._dev(a).reshape(-1) for a in (ref.X, ref.G, ref.H))
        kernels.svgd_many_step(xs, g, h, n, d, M.EPS, M.ALPHA, M.FUDGE, _fresh(n, xs), repulsion_sign=sign)
        torch.cuda.synchronize()
        G._check_step("translated step %d x %d %s sign %+d" % (n, d, _name(dtype), sign), ref, dtype,
                      xs.cpu().numpy().reshape(n, d), h.cpu().numpy().reshape(n, d))


def _subset_inputs(kind, n, d, dtype):
    return E.exact_reference("balanced", n, d, dtype).X if kind == "lattice" else M.kernel_reference(n, d, dtype)[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,n,d", [("lattice", 130, 40), ("gaussian", 161, 257)])
def test_any_subset_of_the_outputs_has_the_bits_of_all_three(kind, n, d, dtype):
    X = _subset_inputs(kind, n, d, dtype)
    x = G._dev(X)
    f = getattr(kernels.lib(), "sgmcmc_svgd_many_kernel_" + ("f32" if dtype == F32 else "f64"))
    sizes = {"kernel_out": n * n, "kernel_grad_out": n * d, "bandwidth_out": 3}
    runs = {}
    for mask in range(7, -1, -1):                                     # all three first
        wanted = [name for bit, name in enumerate(sizes) if mask >> bit & 1]
        bufs = {name: torch.full((size + TAIL,), CANARY, dtype=x.dtype, device=DEV) for name, size in sizes.items()}
        ptr = {name: (bufs[name].data_ptr() if name in wanted else None) for name in sizes}
        ws = _fresh(n, x)
        rc = f(x.data_ptr(), n, d, d, ws.data_ptr(), ptr["kernel_out"], ptr["kernel_grad_out"], d, ptr["bandwidth_out"],
               torch.cuda.current_stream().cuda_stream)
        assert rc == 0, kernels.lib().sgmcmc_last_error()
        torch.cuda.synchronize()
        host = {name: b.cpu().numpy() for name, b in bufs.items()}
        runs[mask] = dict(host, header=ws[:3].cpu().numpy())
        what = "%s %d x %d %s, outputs %r" % (kind, n, d, _name(dtype), wanted)
        assert torch.equal(x, G._dev(X)), what + ": X written"
        for name, size in sizes.items():
            if name in wanted:
                assert np.all(host[name][size:] == CANARY), "%s: %s written past its end" % (what, name)
                assert np.array_equal(E.keys(host[name][:size]), E.keys(runs[7][name][:size])), "%s: %s differs in bits" % (what, name)
            else:
                assert np.all(host[name] == CANARY), "%s: %s was not requested and was written" % (what, name)
        assert np.array_equal(E.keys(runs[mask]["header"]), E.keys(runs[7]["header"])), what + ": header words differ"
    full = runs[7]
    assert np.all(np.isfinite(full["kernel_out"][:n * n])) and np.all(np.isfinite(full["kernel_grad_out"][:n * d]))
    assert np.array_equal(E.keys(full["bandwidth_out"][:3]), E.keys(full["header"]))
    if kind == "lattice":
        _check_words("subset lattice", full["header"], E.exact_reference("balanced", n, d, dtype).med, n, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_workspace_that_held_a_larger_problem_gives_the_bits_of_a_fresh_one(dtype):
    """1024 x 3, then 129 x 40, then 17 x 33 in ONE buffer that is never refilled: every word that is read is written first in
    the same call (DIST zeroes the select counters, KMATRIX rewrites all of np x np, GRAM every partial block it reduces)."""
    esize = np.dtype(dtype).itemsize
    like = G._dev(np.zeros(1, dtype))
    nbytes = int(kernels.lib().sgmcmc_svgd_many_workspace_bytes(1024, esize))
    assert nbytes > 0 and nbytes % esize == 0
    used = torch.full((nbytes // esize,), float("nan"), dtype=like.dtype, device=DEV)
    assert used.data_ptr() % 32 == 0

    def both_entries(n, d, ws):
        X = M.kernel_reference(n, d, dtype)[0]
        ref = M.step_reference(M.Case(n, d, dtype, -1))
        out = list(kernels.svgd_many_kernel(G._dev(X).reshape(-1), n, d, ws))
        x, g, h = (G._dev(a).reshape(-1) for a in (ref.X, ref.G, ref.H))
        kernels.svgd_many_step(x, g, h, n, d, M.EPS, M.ALPHA, M.FUDGE, ws, repulsion_sign=-1)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out + [x, h, ws[:3]]]

    for n, d in ((1024, 3), (129, 40), (17, 33)):
        assert kernels.lib().sgmcmc_svgd_many_workspace_bytes(n, esize) <= nbytes
        got = both_entries(n, d, used)
        want = both_entries(n, d, _fresh(n, like))
        for name, a, b in zip(("K", "kernel gradients", "bandwidth words", "X", "H", "header"), got, want):
            assert np.all(np.isfinite(b)), name
            assert np.array_equal(E.keys(a), E.keys(b)), "%d x %d %s: %s differs from a fresh workspace's" % (n, d, _name(dtype), name)
