"""What tests/test_bnn_small_net_cases.py and tests/test_bnn_small_net_tiles_gpu.py share: the nets at which the small-net core
(csrc/sgmcmc_bnn_small_net.hpp) is pinned beyond ``predict_grad_cases.NETS``, independent Python restatements of the LDS plans of
K11 (``predict_plan``) and K14 (``pgrad_plan``), of the loop form every layer takes and of the grid rule, the suite's data
recipe, and the kernel's own statements in the kernel's order (k-ordered fma chains) as the float32 reference for wide layers.
No test lives here.

Why a reference in the kernel's order: the project's f32 bound elsewhere is 4 x the error of float32 ``mlp_forward`` on the CPU
+ 4 * 2^-23 * max|truth|. torch sums a wide layer in blocks, which is more accurate than the sequential chain the kernels
promise (equal bits whatever the tile needs ONE order): at [2, 1279, 1] the chain's error is about 4 x torch's, so a correct
kernel would pass that bound by a hair or not at all. The restatement below has the kernel's order, so 4 x ITS error is a fair
bound at any width."""
import math

import numpy as np
import torch

import predict_grad_cases as C
from pysgmcmc_amd.models.bayesian_neural_network import init_mlp_params, mlp_forward

LDS_MAX = 160 * 1024
LDS_SHARE = 40 * 1024
MAX_TILE = 32
THREADS = 256
GRID_TARGET = 4096
K11, K14 = "K11", "K14"
KERNELS = (K11, K14)
ESIZES = (4, 8)
ENTRY = {K11: "sgmcmc_bnn_predict_row_tile", K14: "sgmcmc_bnn_predict_grad_row_tile"}
WHAT = {K11: b"bnn_predict_row_tile: ", K14: b"bnn_predict_grad_row_tile: "}

# net -> ((K11 f32), (K11 f64), (K14 f32), (K14 f64)), each (tile, LDS bytes); None = the plan refuses (the parameters alone, or
# ONE test row, need more than 160 KiB). Worked out from the header's rules, not from the library.
_R = None
TABLE = [
    ([6, 150, 1], ((16, 24400), (8, 29216), (16, 34000), (8, 38816)), "small footprint, shrunk tile"),
    ([2, 284, 1], ((8, 22800), (4, 27360), (8, 31888), (4, 36448)), "layer wider than 256 lanes"),
    ([2, 512, 1], ((4, 24624), (2, 32832), (4, 32816), (1, 28736)), "layer wider than 256 lanes at tiles 4, 2, 1"),
    ([2, 1279, 1], ((1, 30736), (1, 61472), (1, 35856), (1, 71712)), "tile 1, odd width, 5 strided trips"),
    ([2, 60, 1, 60, 1], ((32, 17312), (32, 34624), (32, 32800), (16, 34496)), "hidden width 1; even width on an odd offset"),
    ([3, 120, 120, 1], ((32, 91600), (16, 152096), (16, 91408), (8, 151904)), "all pair loops, large LDS"),
    ([2, 135, 135, 1], ((32, 110432), (4, 159936), (32, 144992), (2, 159968)), "odd widths, large LDS"),
    ([2, 139, 138, 1], ((32, 115360), (2, 163552), (32, 150816), (1, 163552)), "mixed loops, large LDS"),
    ([10, 123, 121, 1], ((32, 98688), (8, 148224), (32, 129920), (8, 163840)), "the full 160 KiB"),
    ([100, 194, 1], ((32, 141632), (1, 162272), (16, 122816), (1, 163840)), "D0 = 100, the full 160 KiB"),
    ([33, 603, 1], ((16, 163728), _R, (8, 143376), _R), "D0 = 33"),
    ([10, 193, 191, 1], ((4, 163824), _R, (2, 163760), _R), "tile 4 / 2 at the ceiling"),
    ([2, 197, 197, 1], ((2, 162368), _R, (1, 162400), _R), "tile 2 / 1 at the ceiling"),
    ([100, 389, 1], ((1, 162256), _R, (1, 163824), _R), "D0 = 100 at tile 1"),
    # without this one K11 f64 stops 288 B short of the ceiling (163 552 B at [2, 139, 138, 1])
    ([2, 93, 196, 1], ((32, 126048), (4, 163840), (16, 119328), (2, 162176)), "the full 160 KiB in K11 f64"),
]
NETS = [row[0] for row in TABLE]
NET_IDS = ["x".join(str(v) for v in sizes) for sizes in NETS]
FULL_LDS_NETS = ([10, 123, 121, 1], [100, 194, 1], [2, 93, 196, 1])      # 163 840 B: K14 f64, K14 f64, K11 f64


def table_cell(sizes, kernel, esize):
    """(tile, LDS bytes) of the table, or None where the plan refuses."""
    row = TABLE[NETS.index(list(sizes))][1]
    return row[2 * KERNELS.index(kernel) + ESIZES.index(esize)]


# ---- the plan restated ------------------------------------------------------------------------------------------------------

def round4(v):
    return (v + 3) & ~3


def param_offsets(sizes):
    """(off_w, off_b), 1-based like the header's: the parameter order is W1, b1, ..., WL, bL, log_var."""
    off_w, off_b, off = [None], [None], 0
    for l in range(1, len(sizes)):
        off_w.append(off)
        off += sizes[l - 1] * sizes[l]
        off_b.append(off)
        off += sizes[l]
    assert off + 1 == C.n_params(sizes)
    return off_w, off_b


def _budget(sizes, esize):
    return min(max(2 * round4(C.n_params(sizes)) * esize, LDS_SHARE), LDS_MAX)


def refusal(sizes, esize, kernel):
    """None, or the words the plan refuses the net in."""
    if C.n_params(sizes) > LDS_MAX // esize:
        return b"the parameters alone need more than 160 KiB of LDS"
    plan = k11_plan(sizes, esize) if kernel == K11 else k14_plan(sizes, esize)
    return None if plan is not None else b"ONE test row need"


def _k11_elems(sizes, tile):
    hidden = sizes[1:-1]
    widest = max(hidden) if hidden else 0
    return round4(C.n_params(sizes)) + round4(tile * sizes[0]) + 2 * round4(tile * widest)


def k11_plan(sizes, esize):
    """``predict_plan`` restated: dict(tile, bytes, regions) with regions = [(name, start, length)] in elements, the parameter
    copy first; None where one test row does not fit the 160 KiB. K11 keeps two activation buffers of the widest hidden layer:
    layer l's activations are in ``a[l & 1]``."""
    if C.n_params(sizes) > LDS_MAX // esize:
        return None
    budget, tile = _budget(sizes, esize), MAX_TILE
    while tile > 1 and _k11_elems(sizes, tile) * esize > budget:
        tile //= 2
    if _k11_elems(sizes, tile) * esize > LDS_MAX:
        return None
    hidden = sizes[1:-1]
    widest = max(hidden) if hidden else 0
    w = round4(C.n_params(sizes))
    regions = [("params", 0, C.n_params(sizes)), ("x", w, tile * sizes[0])]
    at = w + round4(tile * sizes[0])
    for k in (0, 1):
        regions.append(("a%d" % k, at, tile * widest))
        at += round4(tile * widest)
    return dict(tile=tile, bytes=at * esize, regions=regions)


def k14_plan(sizes, esize):
    """``pgrad_plan`` restated on ``predict_grad_cases.row_tile_rule`` / ``footprint_bytes``: K14 keeps EVERY hidden layer's
    activations (``h1`` .. ``h{L-1}``) and two delta buffers of the widest hidden layer (``d0``, ``d1``)."""
    if C.n_params(sizes) > LDS_MAX // esize:
        return None
    tile = C.row_tile_rule(sizes, esize)
    if tile is None:
        return None
    hidden = sizes[1:-1]
    widest = max(hidden) if hidden else 0
    w = round4(C.n_params(sizes))
    regions = [("params", 0, C.n_params(sizes)), ("x", w, tile * sizes[0])]
    at = w + round4(tile * sizes[0])
    for l, h in enumerate(hidden, start=1):
        regions.append(("h%d" % l, at, tile * h))
        at += round4(tile * h)
    for k in (0, 1):
        regions.append(("d%d" % k, at, tile * widest))
        at += round4(tile * widest)
    assert at * esize == C.footprint_bytes(sizes, esize, tile)
    return dict(tile=tile, bytes=at * esize, regions=regions)


def plan(sizes, kernel, esize):
    return k11_plan(sizes, esize) if kernel == K11 else k14_plan(sizes, esize)


def forward_pairs(sizes):
    """Per hidden layer l = 1 .. L-1: True where ``forward_tile`` takes the pair loop (even width AND W_l, b_l on even
    elements), False where it takes the scalar loop. The last layer has one unit and a loop of its own."""
    off_w, off_b = param_offsets(sizes)
    return [sizes[l] % 2 == 0 and (off_w[l] | off_b[l]) % 2 == 0 for l in range(1, len(sizes) - 1)]


def backward_pairs(sizes):
    """Per layer l = 1 .. L-1 whose transposed weights K14's sweep walks with ``row_dot``: True where the rows of W_l are read
    two elements at a time (n_l even AND W_l on an even element)."""
    off_w, _ = param_offsets(sizes)
    return [sizes[l] % 2 == 0 and off_w[l] % 2 == 0 for l in range(1, len(sizes) - 1)]


def even_width_on_an_odd_offset(sizes):
    """The hidden layers whose width is even and whose loop is scalar all the same: only the offset says so."""
    return [l for l, pairs in enumerate(forward_pairs(sizes), start=1) if sizes[l] % 2 == 0 and not pairs]


def widest_loop(sizes, tile):
    """The largest trip space of a strided ``idx`` loop of ``forward_tile`` at a full tile: B * n_l / 2 in the pair loop,
    B * n_l in the scalar one. Above 256 a lane takes more than one trip."""
    return max([tile * sizes[l] // (2 if pairs else 1) for l, pairs in enumerate(forward_pairs(sizes), start=1)] or [0])


def grid_y(S, n_tiles):
    """The header's rule, grid.y = min(n_tiles, ceil(4096 / S), 65535). The third term never binds."""
    return min(n_tiles, -(-GRID_TARGET // S), 65535)


# ---- the data: the suite's recipe -------------------------------------------------------------------------------------------

def make_data(sizes, npdt, rows, n_samples):
    """(theta (S, P), X (rows, D0)) in ``npdt``: sample s = init_mlp_params flattened + 0.1 * randn with a distinct log_var,
    X uniform in [-1, 1]."""
    P = C.n_params(sizes)
    rng = np.random.RandomState(len(sizes) * 131 + sizes[0])
    base = torch.cat([p.reshape(-1) for p in init_mlp_params(sizes[0], hidden=sizes[1:-1], seed=5)]).numpy()
    theta = base[None, :] + 0.1 * rng.randn(n_samples, P)
    # the suite's log_var up to 66 samples; beyond, the ramp starts again (exp(0.07 * 4100) is no float32)
    theta[:, -1] = np.log(1e-3) + 0.07 * (np.arange(n_samples) % 66) - 0.011 * rng.rand(n_samples)
    X = rng.uniform(-1.0, 1.0, size=(rows, sizes[0]))
    return theta.astype(npdt), X.astype(npdt)


def forward64(flat, sizes, X):
    """The oracle's forward statements layer by layer in float64 (numpy products), for a net of any depth."""
    params = C.split(flat, sizes)
    L = len(sizes) - 1
    h = X
    for l in range(L - 1):
        h = np.tanh(h @ params[2 * l] + params[2 * l + 1])
    return (h @ params[2 * L - 2] + params[2 * L - 1])[:, 0]


def truth64(theta, X, sizes):
    """(means (S, N), grads (S, N, D0)): the float64 statements on the float64-widened samples and rows."""
    X64 = X.astype(np.float64)
    pairs = []
    for row in theta:
        flat = row.astype(np.float64)
        mean, grad = C.backward_statement(C.split(flat, sizes), X64)
        assert np.array_equal(mean, forward64(flat, sizes, X64))
        pairs.append((mean, grad))
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def torch_cpu(theta, X, sizes):
    """(means, grads) of ``mlp_forward`` + ``torch.autograd.grad`` on the CPU in the arrays' dtype: for the record only."""
    means, grads = [], []
    for row in theta:
        x = torch.from_numpy(X.copy()).requires_grad_()
        mean = mlp_forward([torch.from_numpy(p.copy()) for p in C.split(row, sizes)], x)[:, 0]
        grads.append(torch.autograd.grad(mean.sum(), x)[0].numpy())
        means.append(mean.detach().numpy())
    return np.stack(means), np.stack(grads)


# ---- the kernel's statements in the kernel's order -------------------------------------------------------------------------

def fma(a, b, c):
    """``fma(a, b, c)`` elementwise in the arrays' common dtype. float32: the product of two float32 values is exact in
    float64, the sum is rounded to float64 and then to float32 (the second rounding differs from a fused one only where the
    float64 sum lies within 2^-29 ulp of a float32 tie). float64 and longdouble: product and sum, two roundings -- the f64
    kernels' fma has one, which is the smaller error."""
    dt = np.result_type(a, b, c)
    if dt == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def kernel_order(params, X):
    """``(mean (N,), grad (N, D0))`` of one network in the arrays' dtype by the kernels' statements in the kernels' order.

    Forward (``forward_tile``): acc = bias; for k ascending: acc = fma(h[k], W[k], acc); tanh in the dtype.
    Backward (K14): delta_{L-1} = W_L * (1 - h * h) with h * h rounded first; for l = L-1 .. 2: acc = 0, for j ascending:
    acc = fma(W_l[k][j], delta_l[j], acc), delta_{l-1} = acc * (1 - h * h); grad[d] = the same chain through W_1.
    Vectorised over rows and output units; the loops run over k (or j) only."""
    dt = X.dtype.type
    L = (len(params) - 1) // 2
    hs = [X]
    for l in range(L):
        W, bias, h = params[2 * l], params[2 * l + 1], hs[-1]
        acc = np.repeat(bias[None, :], X.shape[0], axis=0).astype(dt)
        for k in range(W.shape[0]):
            acc = fma(h[:, k][:, None], W[k][None, :], acc)
        hs.append(np.tanh(acc) if l < L - 1 else acc)
        assert hs[-1].dtype == dt
    mean = hs[L][:, 0]
    if L == 1:
        return mean, np.repeat(params[0][:, 0][None, :], X.shape[0], axis=0)
    one = dt(1)

    def one_minus_square(h):
        hh = h * h
        return one - hh

    delta = params[2 * L - 2][:, 0][None, :] * one_minus_square(hs[L - 1])
    for l in range(L - 1, 0, -1):                         # W_l is params[2 * (l - 1)], (n_{l-1}, n_l)
        W = params[2 * (l - 1)]
        acc = np.zeros((X.shape[0], W.shape[0]), dtype=dt)
        for j in range(W.shape[1]):
            acc = fma(W[:, j][None, :], delta[:, j][:, None], acc)
        delta = acc * one_minus_square(hs[l - 1]) if l > 1 else acc
        assert delta.dtype == dt
    return mean, delta


def kernel_order_all(theta, X, sizes):
    """``kernel_order`` over the samples of ``theta``: (means (S, N), grads (S, N, D0)) in the arrays' dtype."""
    pairs = [kernel_order(C.split(row, sizes), X) for row in theta]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def scalar_loop_f32(params, X):
    """``kernel_order`` in float32 as plain Python loops over (row, unit, k), one scalar operation at a time: ``math.fma`` on
    the float32 values widened to float (one rounding to float64, then one to float32) where the interpreter has it, else
    ``np.float32`` product and sum (two float32 roundings: equal to the fused form only where every product is exact)."""
    f32 = np.float32
    if hasattr(math, "fma"):
        step = lambda a, b, c: f32(math.fma(float(a), float(b), float(c)))
    else:
        step = lambda a, b, c: f32(f32(a) * f32(b)) + f32(c)
    L = (len(params) - 1) // 2
    N = X.shape[0]
    hs = [X]
    for l in range(L):
        W, bias, h = params[2 * l], params[2 * l + 1], hs[-1]
        out = np.empty((N, W.shape[1]), dtype=f32)
        for b in range(N):
            for j in range(W.shape[1]):
                acc = f32(bias[j])
                for k in range(W.shape[0]):
                    acc = step(h[b, k], W[k, j], acc)
                out[b, j] = np.tanh(acc) if l < L - 1 else acc
        hs.append(out)
    mean = hs[L][:, 0]
    if L == 1:
        return mean, np.repeat(params[0][:, 0][None, :], N, axis=0)
    delta = np.empty((N, hs[L - 1].shape[1]), dtype=f32)
    for b in range(N):
        for k in range(delta.shape[1]):
            hh = f32(hs[L - 1][b, k] * hs[L - 1][b, k])
            delta[b, k] = params[2 * L - 2][k, 0] * f32(f32(1) - hh)
    for l in range(L - 1, 0, -1):
        W = params[2 * (l - 1)]
        out = np.empty((N, W.shape[0]), dtype=f32)
        for b in range(N):
            for k in range(W.shape[0]):
                acc = f32(0)
                for j in range(W.shape[1]):
                    acc = step(W[k, j], delta[b, j], acc)
                if l > 1:
                    hh = f32(hs[l - 1][b, k] * hs[l - 1][b, k])
                    acc = f32(acc * f32(f32(1) - hh))
                out[b, k] = acc
        delta = out
    return mean, delta
