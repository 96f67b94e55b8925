"""What tests/test_bnn_predict_grad.py and tests/test_bnn_predict_grad_gpu.py share: independent Python restatements of
include/sgmcmc_hip_predict_grad.h -- the backward sweep of the input gradient, the reduction of the ensemble, the footprint
rule behind the row tile -- and the nets K14 is pinned at (the ones K11 is pinned at). No test lives here."""
import numpy as np

NETS = [[1, 50, 50, 50, 1], [3, 7, 13, 1], [4, 50, 49, 50, 1], [5, 1], [3, 8, 8, 8, 8, 8, 8, 8, 1]]
NET_IDS = ["default_3x50", "odd_widths_odd_offsets", "paired_and_scalar_mixed", "single_weight_layer", "eight_weight_layers"]


def n_params(sizes):
    return sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)) + 1


def split(flat, sizes):
    """Flat parameter row -> [W1 (in, out), b1, ..., WL, bL, log_var (1, 1)] (the kernel's order and layout)."""
    out, off = [], 0
    for l in range(len(sizes) - 1):
        nin, nout = sizes[l], sizes[l + 1]
        out.append(flat[off:off + nin * nout].reshape(nin, nout))
        off += nin * nout
        out.append(flat[off:off + nout])
        off += nout
    out.append(flat[off:off + 1].reshape(1, 1))
    assert off + 1 == flat.size
    return out


def backward_statement(params, X):
    """``(mean (N,), grad (N, D0))`` of one network at the rows of ``X``, in the arrays' dtype: the header's statements --
    delta_{L-1} = W_L[:, 0] * (1 - h * h), delta_{l-1} = (W_l delta_l) * (1 - h * h), grad = W_1 delta_1 -- with numpy
    products for the header's fma chains (so the summation order, not the statement, differs from the kernel's)."""
    L = (len(params) - 1) // 2
    hs = [X]
    for l in range(L - 1):
        hs.append(np.tanh(hs[-1] @ params[2 * l] + params[2 * l + 1]))
    mean = (hs[-1] @ params[2 * L - 2] + params[2 * L - 1])[:, 0]
    if L == 1:
        return mean, np.repeat(params[0][:, 0][None, :], X.shape[0], axis=0)
    delta = params[2 * L - 2][:, 0][None, :] * (1.0 - hs[L - 1] * hs[L - 1])
    for l in range(L - 1, 1, -1):                           # W_l is params[2 * (l - 1)]
        delta = (delta @ params[2 * (l - 1)].T) * (1.0 - hs[l - 1] * hs[l - 1])
    return mean, delta @ params[0].T


def ensemble_statement(means, grads, ens_mean):
    """``(dmean, dvar)``, float64 ``(N, D0)``: the header's reduction, a loop over s ascending, elementwise over (r, d), on
    the given ``means (S, N)``, ``grads (S, N, D0)`` and ``ens_mean (N,)``. Every operation is one float64 rounding, as in the
    kernel, so equal inputs give equal bits."""
    S = means.shape[0]
    G = np.zeros(grads.shape[1:], dtype=np.float64)
    C = np.zeros(grads.shape[1:], dtype=np.float64)
    for s in range(S):
        g = grads[s].astype(np.float64)
        dev = means[s].astype(np.float64) - ens_mean
        G = G + g
        C = C + dev[:, None] * g
    return G / float(S), (2.0 * C) / float(S)


def _round4(v):
    return (v + 3) & ~3


def footprint_bytes(sizes, esize, tile):
    """The header's footprint: parameter copy + X tile + every hidden layer's activations for the tile + two delta buffers
    of the widest hidden layer, every region rounded up to 4 elements."""
    hidden = sizes[1:-1]
    widest = max(hidden) if hidden else 0
    elems = _round4(n_params(sizes)) + _round4(tile * sizes[0]) + 2 * _round4(tile * widest)
    return (elems + sum(_round4(tile * h) for h in hidden)) * esize


def row_tile_rule(sizes, esize):
    """The tile the header promises: the largest power of two <= 32 within max(40 KiB, twice the parameter copy) (at most
    the 160 KiB of a CU); 1 if only that fits the 160 KiB; None for a net whose single row does not."""
    budget = min(max(2 * _round4(n_params(sizes)) * esize, 40 * 1024), 160 * 1024)
    tile = 32
    while tile > 1 and footprint_bytes(sizes, esize, tile) > budget:
        tile //= 2
    return tile if footprint_bytes(sizes, esize, tile) <= 160 * 1024 else None
