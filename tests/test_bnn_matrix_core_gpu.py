"""The BNN's matrix-core launches -- ``sgmcmc_bnn_dense_tanh_f32``, ``sgmcmc_bnn_dense_tanh_backward_f32``
(csrc/sgmcmc_bnn_gemm.hip), ``sgmcmc_bnn_split_planes_f32``, ``sgmcmc_bnn_gw_planes_f32`` (csrc/sgmcmc_bnn_gw.hip) -- pinned with
EXACT operands (tests/bnn_matrix_core_cases.py, proved exact in tests/test_bnn_matrix_core_cases.py): every product and every
partial sum is an fp32 number, so the result cannot depend on summation order or tiling and is compared bit for bit.

Dense layers: K = 64, 80, ..., 768 -- every K tail {0, 16, 32, 48} at every chunk count 1 .. 12 (steady loop of the ring not
entered, entered, drained with 4, 5, 6, 7 chunks left) -- on six tile layouts: full tiles with the XCD map off (1 and 9 tiles) and
on (8), half tiles with the map off (2; 4 in two row tiles) and on (8). tests/test_bnn_dense_gpu.py keeps the large shapes and
Gaussian operands.
Weight gradients: tile counts with T % 8 != 0 above and below 8, short last panels, a product boundary inside an XCD's range;
three operand pairs that together use all six plane products. The planes themselves bit for bit against an integer restatement.

bias_tanh and the forward epilogue: the forward launch's tanh is asserted bit-equal to ``kernels.bias_tanh`` on the same
(exact) pre-activation."""
import numpy as np
import pytest
import torch

import bnn_matrix_core_cases as C

pytestmark = pytest.mark.gpu


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _layout(gpu, name):
    """(M, N, n_full, parts) of a named layout on this device; the restated plan must be the library's."""
    from pysgmcmc_amd import kernels
    cus = _cus(gpu)
    shape = C.layout_shape(name, cus)
    if shape is None:
        assert cus != 256, "every layout exists on 256 compute units"
        pytest.skip("no layout '%s' on %d compute units" % (name, cus))
    M, N = shape
    n_full, parts = C.plan_columns(M, N, cus)
    assert kernels.bnn_dense_tanh_dot_parts(M, N, gpu) == parts, (M, N, cus)
    return M, N, n_full, parts


def _verdict(checks, explain):
    """One device read per K: ``checks`` is [(name, 0-d bool tensor)]; returns the names that failed, explained."""
    flags = torch.stack([ok for _, ok in checks]).cpu().tolist()
    return [explain(name) for (name, _), ok in zip(checks, flags) if not ok]


@pytest.mark.parametrize("name", C.LAYOUTS)
def test_dense_backward_is_exact_at_every_k_tail_and_ring_phase(gpu, name):
    """out = (delta W^T)(1 - act^2), the 32-row column sums, and their totals (by ``colsum_finish`` and as the side job of a
    following launch, which also repeats the launch: same bits) equal the exact values bit for bit; the row behind ``out``, its
    pitch columns, and the rows / elements behind the sums stay untouched."""
    from pysgmcmc_amd import kernels
    M, N, n_full, _ = _layout(gpu, name)
    ops = {k: v.to(gpu) for k, v in C.backward_operands(M, N).items()}
    d64, W64 = ops["delta"].double(), ops["W"].double()
    tanh1 = 1.0 - ops["act"].double() ** 2
    mt = M // 32
    obuf = torch.empty(M + 1, N + 8, device=gpu)
    parts = torch.empty(mt + 1, N, device=gpu)
    colsum = torch.empty(N + 4, device=gpu)
    o2, p2, c2 = torch.empty(M, N, device=gpu), torch.empty(mt, N, device=gpu), torch.empty(N, device=gpu)
    failures = []
    for K in C.K_SWEEP:
        delta, W = ops["delta"][:, :K], ops["W"][:, :K]          # pitches K_MAX + 4 and K_MAX + 12
        for t, v in ((obuf, -7.0), (parts, -3.0), (colsum, -5.0), (o2, -1.0), (p2, -1.0), (c2, -1.0)):
            t.fill_(v)
        out = obuf[:M, :N]
        assert kernels.bnn_dense_tanh_backward_fits(delta, W, ops["act"], out)
        kernels.bnn_dense_tanh_backward(delta, W, ops["act"], out, colsum_parts=parts[:mt])
        kernels.colsum_finish(parts[:mt], colsum[:N])
        kernels.bnn_dense_tanh_backward(delta, W, ops["act"], o2, colsum_parts=p2, finish=(parts[:mt], c2, None, 0.0))
        ref64 = (d64[:, :K] @ W64[:, :K].t()) * tanh1
        ref, ref_parts64 = ref64.float(), ref64.view(mt, 32, N).sum(1)
        ref_parts, ref_colsum = ref_parts64.float(), ref64.sum(0).float()
        checks = [("reference round trip", (ref.double() == ref64).all() & (ref_parts.double() == ref_parts64).all()
                   & (ref_colsum.double() == ref64.sum(0)).all()),
                  ("out", (out == ref).all()),
                  ("guards of out", (obuf[M] == -7.0).all() & (obuf[:, N:] == -7.0).all()),
                  ("colsum_parts", (parts[:mt] == ref_parts).all()),
                  ("guard row of colsum_parts", (parts[mt] == -3.0).all()),
                  ("colsum_finish", (colsum[:N] == ref_colsum).all()),
                  ("guard of colsum", (colsum[N:] == -5.0).all()),
                  ("second launch: out", (o2 == out).all()),
                  ("second launch: colsum_parts", (p2 == parts[:mt]).all()),
                  ("side-job finish", (c2 == ref_colsum).all())]

        def explain(what):
            where = {"out": lambda: C.first_wrong_dense(out, ref, n_full, K),
                     "second launch: out": lambda: C.first_wrong_dense(o2, out, n_full, K),
                     "colsum_parts": lambda: C.first_wrong_dense(parts[:mt].repeat_interleave(32, 0), ref_parts.repeat_interleave(32, 0), n_full, K),
                     "colsum_finish": lambda: C.first_wrong_dense(colsum[None, :N], ref_colsum[None], n_full, K),
                     "side-job finish": lambda: C.first_wrong_dense(c2[None], ref_colsum[None], n_full, K)}.get(what, lambda: "K = %d" % K)()
            return "%s: %s" % (what, where)
        failures += _verdict(checks, explain)
    assert not failures, "%s (%d x K x %d): %d failures, first:\n%s" % (name, M, N, len(failures), "\n".join(failures[:6]))


# |tanhf - tanh| of the device, as this file's bar for the forward launch has been since the kernel was written
FORWARD_BAR = 4e-6


@pytest.mark.parametrize("name", C.LAYOUTS)
def test_dense_forward_at_every_k_tail_and_ring_phase(gpu, name):
    """The pre-activation z = h W + b is exact, so: out = tanhf(z) bit-equal to ``bias_tanh`` of the exact z, and within 4e-6 of
    fp64; the half-tile columns bit-equal to the same columns as a narrow launch of full tiles; ``dot_parts`` row t against
    the fp64 dot product of the launch's own ``out`` over exactly the columns of tile t (64, or 32 behind n_full) within the
    bound of a 64-term fp32 sum, 64 * 2^-24 * sum |out w_next|, and their sum as in tests/test_bnn_dense_gpu.py; the row and
    the pitch columns behind ``out`` untouched; a second launch gives the same bits."""
    from pysgmcmc_amd import kernels
    M, N, n_full, n_parts = _layout(gpu, name)
    ops = {k: v.to(gpu) for k, v in C.forward_operands(M, N).items()}
    h64, W64, b64, w64 = ops["h"].double(), ops["W"][:, :N].double(), ops["bias"].double(), ops["w_next"].double()
    bias, w_next = ops["bias"], ops["w_next"]
    obuf = torch.empty(M + 1, N + 8, device=gpu)
    parts, parts2 = torch.empty(n_parts + 1, M, device=gpu), torch.empty(n_parts, M, device=gpu)
    out2 = torch.empty(M, N, device=gpu)
    edges = C.column_tile_edges(N, n_full)
    assert len(edges) == n_parts + 1
    nh = N - n_full
    if nh:                                                       # the half-tile columns once more, as a layer of their own
        assert C.plan_columns(M, nh, _cus(gpu)) == (nh, nh // 64)
        Wn, bn, outn = ops["W"][:, n_full:N].contiguous(), bias[n_full:].contiguous(), torch.empty(M, nh, device=gpu)

    def tile_sums(v):                                            # [M][N] -> [parts][M]: sums over the columns of each tile
        full = v[:, :n_full].reshape(M, n_full // 64, 64).sum(2)
        return torch.cat([full, v[:, n_full:].reshape(M, nh // 32, 32).sum(2)], 1).t() if nh else full.t()
    failures, worst = [], dict(fp64=0.0, parts=0.0, parts_sum=0.0)
    for K in C.K_SWEEP:
        h, W = ops["h"][:, :K], ops["W"][:K, :N]                 # pitches K_MAX + 8 and N + 4
        for t, v in ((obuf, -7.0), (parts, -3.0), (parts2, -1.0), (out2, -1.0)):
            t.fill_(v)
        out = obuf[:M, :N]
        assert kernels.bnn_dense_tanh_fits(h, W, out)
        kernels.bnn_dense_tanh(h, W, bias, out, w_next=w_next, dot_parts=parts[:n_parts])
        kernels.bnn_dense_tanh(h, W, bias, out2, w_next=w_next, dot_parts=parts2)
        z64 = h64[:, :K] @ W64[:K]
        act = z64.float()                                        # exact
        kernels.bias_tanh(act, bias)                             # tanhf(z + b) of the activation launch
        zb64 = z64 + b64
        err = (out.double() - torch.tanh(zb64)).abs().max()
        prod = out.double() * w64
        want_parts, bound = tile_sums(prod), 64 * 2.0 ** -24 * tile_sums(prod.abs())
        perr = (parts[:n_parts].double() - want_parts).abs()
        serr = (parts[:n_parts].double().sum(0) - out.double() @ w64).abs().max()
        checks = [("reference round trip", (z64.float().double() == z64).all() & (zb64.float().double() == zb64).all()),
                  ("out against fp64", err < FORWARD_BAR),
                  ("out against bias_tanh", (out == act).all()),
                  ("guards of out", (obuf[M] == -7.0).all() & (obuf[:, N:] == -7.0).all()),
                  ("dot_parts per tile", (perr <= bound).all()),
                  ("dot_parts sum", serr <= 1e-4),
                  ("guard row of dot_parts", (parts[n_parts] == -3.0).all()),
                  ("second launch: out", (out2 == out).all()),
                  ("second launch: dot_parts", (parts2 == parts[:n_parts]).all())]
        if nh:
            kernels.bnn_dense_tanh(h, Wn[:K], bn, outn)
            checks.append(("half tiles against full tiles", (out[:, n_full:] == outn).all()))

        def explain(what):
            where = "K = %d" % K
            if what == "out against bias_tanh":
                where = "%s; largest difference %.3g" % (C.first_wrong_dense(out, act, n_full, K), float((out - act).abs().max()))
            elif what == "out against fp64":
                where = "K = %d: %.3g" % (K, float(err))
            elif what == "second launch: out":
                where = C.first_wrong_dense(out2, out, n_full, K)
            elif what == "half tiles against full tiles":
                full = out.clone()
                full[:, n_full:] = outn
                where = C.first_wrong_dense(out, full, n_full, K)
            elif what == "dot_parts per tile":
                t, m = (int(v) for v in (perr > bound).nonzero()[0])
                where = "K = %d: tile %d (columns %d..%d) row %d: got %r, want %r +- %.3g" % (
                    K, t, edges[t], edges[t + 1] - 1, m, float(parts[t, m]), float(want_parts[t, m]), float(bound[t, m]))
            elif what == "dot_parts sum":
                where = "K = %d: %.3g" % (K, float(serr))
            return "%s: %s" % (what, where)
        failures += _verdict(checks, explain)
        for k, v in (("fp64", err), ("parts", (perr / bound).max()), ("parts_sum", serr)):
            worst[k] = max(worst[k], float(v))
    print("%s (%d x K x %d): max |out - tanh(z)| %.3g (bar %.1g); dot_parts worst error / bound %.3g; sum of parts %.3g (bar 1e-4)"
          % (name, M, N, worst["fp64"], FORWARD_BAR, worst["parts"], worst["parts_sum"]))
    assert not failures, "%s (%d x K x %d): %d failures, first:\n%s" % (name, M, N, len(failures), "\n".join(failures[:6]))


# ---------------------------------------------------------------------------------------------------------------------------
# weight gradients on bf16 planes

@pytest.mark.parametrize("pair", C.GW_PAIRS)
@pytest.mark.parametrize("nA,nB,count", C.GW_SHAPES)
def test_gw_planes_is_exact_on_every_tile_of_the_map(gpu, nA, nB, count, pair):
    """The three operand pairs whose dropped plane products vanish: C_z = A_z^T B_z bit-equal to the fp64 product on every tile,
    for workgroup counts with and without a remainder modulo 8 and short last panels; pitched gradient slices, the row and the
    columns behind each untouched; a second launch gives the same bits."""
    from pysgmcmc_amd import kernels
    A, B, g, bound = C.gw_operands(pair, nA, nB, count)
    M = C.gw_pair_M(pair)
    A, B = A.to(gpu), B.to(gpu)
    pa = torch.empty(count * kernels.bnn_planes_bytes(M, nA), dtype=torch.uint8, device=gpu)
    pb = torch.empty(count * kernels.bnn_planes_bytes(M, nB), dtype=torch.uint8, device=gpu)
    kernels.bnn_split_planes([A[z] for z in range(count)], pa)
    kernels.bnn_split_planes([B[z] for z in range(count)], pb)
    cbuf = torch.full((count, nA + 1, nB + 8), -7.0, device=gpu)
    kernels.bnn_gw_planes(pa, pb, [cbuf[z, :nA, :nB] for z in range(count)], M)
    ref64 = torch.bmm(A.double().transpose(1, 2), B.double())
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64) and float(ref64.abs().max()) <= bound
    got = cbuf[:, :nA, :nB]
    assert torch.equal(got, ref), "(%d, %d, %d) pair %s: %s" % (nA, nB, count, pair, C.first_wrong_gw(got, ref))
    assert torch.all(cbuf[:, nA] == -7.0) and torch.all(cbuf[:, :, nB:] == -7.0)
    again = torch.full_like(cbuf, -7.0)
    kernels.bnn_gw_planes(pa, pb, [again[z, :nA, :nB] for z in range(count)], M)
    assert torch.equal(again, cbuf)


def _device_planes(gpu, X):
    """Planes of the matrices X [count][M][ldx][:N] as the device writes them: int16 [count][3][M / 8][N][8]."""
    from pysgmcmc_amd import kernels
    count, M, N = X.shape
    one = kernels.bnn_planes_bytes(M, N)
    buf = torch.full((count * one + 64,), 0x5A, dtype=torch.uint8, device=gpu)
    kernels.bnn_split_planes([X[z] for z in range(count)], buf[:count * one])
    assert bool((buf[count * one:] == 0x5A).all())               # nothing behind the last set
    return buf[:count * one].view(torch.int16).view(count, 3, M // 8, N, 8).cpu().numpy()


@pytest.mark.parametrize("M,N,ldx,count", [(32, 300, 308, 3), (16, 1100, 1101, 4)])
def test_split_planes_bit_for_bit_on_the_exact_domain(gpu, M, N, ldx, count):
    """Every plane of every set z, from a pitched source (ldx > N), of magnitudes spread over [2^-100, 2^100] and +-0: equal to the
    integer restatement (top 16 bits, residual, residual again) bit for bit; (p0 + p1) + p2 gives x back by value."""
    xbuf = C.split_domain_values(torch.Generator().manual_seed(M + N), (count, M, ldx))
    X = xbuf.to(gpu)[:, :, :N]
    got = _device_planes(gpu, X)
    for z in range(count):
        x = xbuf[z, :, :N].numpy()
        want = C.planes_image(x)
        bad = np.argwhere(got[z] != want)
        assert bad.shape[0] == 0, "set z = %d: plane %d, m8 %d, feature %d, row %d: got %#x, want %#x (%d wrong)" % (
            (z,) + tuple(bad[0]) + (int(got[z][tuple(bad[0])]) & 0xffff, int(want[tuple(bad[0])]) & 0xffff, bad.shape[0]))
        p = torch.from_numpy(got[z].copy()).view(torch.bfloat16).float()         # [3][M / 8][N][8]
        back = ((p[0] + p[1]) + p[2]).permute(0, 2, 1).reshape(M, N).numpy()
        assert np.array_equal(back, x)


def test_split_planes_at_the_edge_of_its_exact_domain(gpu):
    """Exact down to |x| = 2^-110 (every mantissa bit set); -0 keeps its sign in plane 0 and comes back as +0; one value below the
    domain, 2^-115 (2 - 2^-23), loses 2^-133 - 2^-138 < 2^-133 (include/sgmcmc_hip.h)."""
    edge = np.float32(2.0 ** -110) * np.float32(2.0 - 2.0 ** -23)
    x = np.zeros((16, 4), np.float32)
    x[0, 0], x[1, 0], x[2, 0], x[3, 0], x[4, 0] = edge, -edge, -0.0, 0.0, C.SUBDOMAIN_X
    got = _device_planes(gpu, torch.from_numpy(x).to(gpu)[None])[0]
    assert np.array_equal(got, C.planes_image(x))
    p = torch.from_numpy(got.copy()).view(torch.bfloat16).double()[:, 0, 0, :]    # [3][8 rows of feature 0]
    back = (p[0] + p[1]) + p[2]
    assert float(back[0]) == float(edge) and float(back[1]) == -float(edge) and float(p[2][0]) != 0.0
    assert got[0, 0, 0, 2] == np.int16(-0x8000) and got[1, 0, 0, 2] == 0 and got[2, 0, 0, 2] == 0
    assert float(back[2]) == 0.0 and not np.signbit(float(back[2])) and float(back[3]) == 0.0
    err = C.SUBDOMAIN_X - float(back[4])
    assert float(p[2][4]) == 7 * 2.0 ** -133 and err == 2.0 ** -133 - 2.0 ** -138 and 0.0 < err < C.SUBDOMAIN_BOUND
