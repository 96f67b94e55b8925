"""What tests/test_bnn_particles_cases.py and tests/test_bnn_particles_forms_gpu.py share: the (net, batch, dtype) rows at which
the particle gradient kernel K15 (csrc/sgmcmc_bnn_particles.hip, include/sgmcmc_hip_particles.h) is pinned beyond
tests/test_bnn_particles_gpu.py, an independent Python restatement of its LDS plan (``particles_plan``), of the form every loop
of every layer takes and of the trip space of every strided loop, the suite's data recipe, the kernel's own statements in the
kernel's order (``kernel_order``) and the same statements with numpy products in any precision (``statement``). No test lives
here.

The plan is restated from the header and the kernel's comments, not from the library: 160 bytes for the block sums, the
parameter copy rounded up to 4 elements, then h_0 (the minibatch's X), h_1 .. h_L, delta_1 .. delta_L and y packed without
padding, the regions of an even number of elements first. ``round4(n_params)`` is even and every region in front of an even one
is even, so every even region starts on an even element: a pair access (8 bytes in f32, 16 in f64) only ever touches regions of
``batch * width`` elements with an even width, which are even whatever the batch. The form of a loop therefore depends on the
net alone (widths and parameter offsets); ``forms`` asserts it.

Why a bound from ``kernel_order``: the kernel promises ONE order for every chain (b ascending for gW and gb, j ascending for a
delta), so 4 x the error the same order makes in the same precision on the CPU, + 4 roundings of the result, is a fair bar at
any width and batch, per layer block. The factor 4 is the project's allowance for the vendor's tanh and exp against numpy's."""
import collections

import numpy as np
import torch

import predict_grad_cases as C
import small_net_cases as N
from pysgmcmc_amd.models import bnn_particles

F32, F64 = np.float32, np.float64
LONG_DOUBLE_IS_WIDER = np.finfo(np.longdouble).eps < 2.0 ** -60
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}                    # unit roundoff of T
ESIZE = {F32: 4, F64: 8}
NAME = {F32: "f32", F64: "f64"}
BOTH = (F32, F64)

THREADS = 512                                             # lanes of K15's one workgroup per particle (K8 runs 1024)
LDS_MAX = 160 * 1024
OPT_IN = 64 * 1024                                        # above it the entry opts the kernel in
RED_BYTES = 160                                           # the block sums in front of the parameter copy
MAX_LAYERS = 8
DEFAULT = [1, 50, 50, 50, 1]
N_PARTICLES = 4                                           # per case: what E is pooled over
N_EXAMPLES = 160


def wide(dtype):
    """The next wider precision: the truth of an f32 row is f64, of an f64 row the 80-bit long double (f64 where long double
    is no wider: the truth then differs from ``kernel_order`` by the order of the sums alone)."""
    return F64 if dtype == F32 else (np.longdouble if LONG_DOUBLE_IS_WIDER else F64)


# ---- the plan restated ------------------------------------------------------------------------------------------------------

def lds_bytes(sizes, batch, esize):
    """The header's rule: 160 + ((2 * sum(sizes) + 1) * batch + n_params + 4) * esize, 0 above 160 KiB."""
    rows = 2 * sum(sizes) + 1
    total = RED_BYTES + (rows * batch + C.n_params(sizes) + 4) * esize
    return total if total <= LDS_MAX else 0


def k8_lds_bytes(sizes, batch, esize):
    """The whole-step kernel's own footprint (include/sgmcmc_hip.h [whole-step]): the same regions rounded up to 4 elements
    as a whole, then the parameter copy. Never more than ``lds_bytes``, so K8 takes every row K15 takes."""
    rows = 2 * sum(sizes) + 1
    total = RED_BYTES + (N.round4(rows * batch) + C.n_params(sizes)) * esize
    return total if total <= LDS_MAX else 0


def plan(sizes, batch):
    """``particles_plan`` restated: OrderedDict name -> (start, length) in elements from the parameter copy, in the order the
    regions lie in the LDS: ``params``, then the regions of an even length in the order h_0 .. h_L, d_1 .. d_L, y, then the odd
    ones in the same order."""
    L = len(sizes) - 1
    wanted = [("h%d" % l, batch * sizes[l]) for l in range(L + 1)] + [("d%d" % l, batch * sizes[l]) for l in range(1, L + 1)]
    wanted.append(("y", batch))
    regions = collections.OrderedDict(params=(0, C.n_params(sizes)))
    at = N.round4(C.n_params(sizes))
    for odd in (0, 1):
        for name, length in wanted:
            if length % 2 == odd:
                regions[name] = (at, length)
                at += length
    return regions


def plan_end(sizes, batch):
    """One past the last element of the packed regions."""
    start, length = list(plan(sizes, batch).values())[-1]
    return start + length


Layer = collections.namedtuple("Layer", "l nin nout forward gw delta items")
PAIR, SCALAR, LAST = "pair", "scalar", "last"


def forms(sizes, batch):
    """Per weight layer l = 1 .. L: the form of ``forward_tile``'s loop (``LAST``: the one output unit's own loop), of the gW
    loop and of the loop that makes delta_{l-1} (None at l = 1), and ``items``: the trip space of each strided loop --
    ``forward``, ``gw``, ``gb`` (the scalar form's own loop; None where gb rides the pair loop) and ``delta``.

    The forms are taken from the kernel's conditions on the restated plan AND from the net alone; the two must agree, and every
    region a pair access touches must start on an even element."""
    L = len(sizes) - 1
    off_w, off_b = N.param_offsets(sizes)
    regions = plan(sizes, batch)
    at = {name: start for name, (start, _) in regions.items()}
    assert at["params"] == 0 and N.round4(C.n_params(sizes)) % 2 == 0
    out = []
    for l in range(1, L + 1):
        nin, nout = sizes[l - 1], sizes[l]
        # the kernel's conditions, on the plan
        pj = nout % 2 == 0 and (off_w[l] | at["d%d" % l]) % 2 == 0
        pk = nin % 2 == 0 and at["h%d" % (l - 1)] % 2 == 0
        gw_pair = pj and pk
        delta_pair = l > 1 and gw_pair and at["d%d" % (l - 1)] % 2 == 0
        fwd_pair = l < L and nout % 2 == 0 and (off_w[l] | off_b[l]) % 2 == 0
        # the net alone
        net_pair = nin % 2 == 0 and nout % 2 == 0 and off_w[l] % 2 == 0
        assert gw_pair == net_pair and delta_pair == (l > 1 and net_pair), (sizes, batch, l)
        if gw_pair:
            assert at["h%d" % (l - 1)] % 2 == 0 and at["d%d" % l] % 2 == 0, (sizes, batch, l)
        if delta_pair:
            assert at["d%d" % (l - 1)] % 2 == 0, (sizes, batch, l)
        if fwd_pair:
            assert at["h%d" % l] % 2 == 0 and off_b[l] % 2 == 0, (sizes, batch, l)
        items = dict(
            forward=batch if l == L else batch * nout // (2 if fwd_pair else 1),
            gw=(nin // 2) * (nout // 2) if gw_pair else nin * nout,
            gb=None if gw_pair else nout,
            delta=None if l == 1 else batch * nin // (2 if delta_pair else 1))
        out.append(Layer(l, nin, nout, LAST if l == L else (PAIR if fwd_pair else SCALAR), PAIR if gw_pair else SCALAR,
                         None if l == 1 else (PAIR if delta_pair else SCALAR), items))
    return out


def global_items(sizes, batch):
    """The strided loops outside the layers: the copies of X and y, the sum of squares, the head."""
    return dict(copy_x=batch * sizes[0], copy_y=batch, tsq=C.n_params(sizes), head=batch)


def trips(items):
    """Trips the busiest lane of 512 takes through a strided loop of ``items``."""
    return -(-items // THREADS)


def check_plan(sizes, batch, esize):
    """The restated regions are disjoint, in order, even ones first, every even one on an even element, and they fit the
    footprint the launch asks for. Returns the footprint."""
    total = lds_bytes(sizes, batch, esize)
    assert total, (sizes, batch, esize)
    regions = list(plan(sizes, batch).items())
    L = len(sizes) - 1
    assert sorted(name for name, _ in regions) == sorted(
        ["params", "y"] + ["h%d" % l for l in range(L + 1)] + ["d%d" % l for l in range(1, L + 1)])
    at, seen_odd = N.round4(C.n_params(sizes)), False
    for name, (start, length) in regions[1:]:
        assert start == at and length > 0, (name, start, at)
        at += length
        if length % 2:
            seen_odd = True
        else:
            assert not seen_odd and start % 2 == 0, (name, start)
    assert at == plan_end(sizes, batch) and RED_BYTES + at * esize <= total, (sizes, batch, esize, at, total)
    forms(sizes, batch)
    return total


# ---- the case table ----------------------------------------------------------------------------------------------------------

# (net, batches, dtypes, what the row is there for). K8 (1024 lanes) takes every row: its footprint is never above K15's rule
# (``k8_lds_bytes``), so the column "K8 takes it" of profiles/bnn_particles_forms.txt is yes throughout; the GPU test asserts it.
TABLE = [
    ([2, 4, 6, 3, 1], (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17), BOTH,
     "pair gW at l = 1, 2, pair delta at l = 2, scalar gW and delta at l = 3, 4; every remainder of the unroll-4 and unroll-8 "
     "b loops; odd regions behind even ones at odd batch"),
    ([2, 3, 4, 6, 1], (5,), BOTH, "even widths on odd offsets: every loop scalar, forward included"),
    ([2, 2, 2, 2, 2, 2, 2, 2, 1], (3,), BOTH, "L = 8, all pair"),
    ([3, 3, 3, 3, 3, 3, 3, 3, 1], (3,), BOTH, "L = 8, all scalar, every region odd"),
    ([2, 27, 21, 1], (4,), BOTH, "scalar gW of 567 items: a second, ragged trip"),
    ([2, 64, 66, 1], (17,), BOTH, "pair gW of 1056 items (three trips), pair delta of 544 items (two trips); 72 904 B in f64"),
    ([2, 600, 1], (3,), BOTH, "a layer wider than the workgroup: scalar gW of 600 items, scalar delta of 1800 items"),
    ([3, 600, 1], (2,), BOTH, "scalar gW of 1800 items; the scalar form's own gb loop of 600 items: a second, ragged trip"),
    ([4, 1], (513,), BOTH, "B > 512: the copy of y, the head and the last layer's loop take two trips; L = 1"),
    ([3, 12, 12, 1], (714,), (F32,), "exactly 163 840 B; B > 512; pair delta of 4284 items, nine trips"),
    ([3, 31, 31, 1], (299,), (F32,), "exactly 163 840 B; odd widths, all scalar"),
    ([2, 48, 48, 1], (90,), (F64,), "exactly 163 840 B; pair delta of 2160 items in f64"),
    (DEFAULT, (49,), (F64,), "the f64 ceiling of the default net; pair delta of 1225 items"),
    (DEFAULT, (116,), (F32,), "the f32 ceiling of the default net; pair delta of 2900 items"),
    (DEFAULT, (36, 37), (F32,), "either side of the opt-in: 65 104 B and 66 324 B"),
    (DEFAULT, (9, 10), (F64,), "either side of the opt-in: 64 168 B and 66 608 B"),
]
CASES = [(sizes, B, dt) for sizes, batches, dts, _ in TABLE for B in batches for dt in dts]
CASE_IDS = ["%s-B%d-%s" % ("x".join(map(str, sizes)), B, NAME[dt]) for sizes, B, dt in CASES]
# (net, the largest batch the rule accepts, dtype): the batch one larger is refused
CEILINGS = [(DEFAULT, 116, F32), (DEFAULT, 49, F64), ([3, 12, 12, 1], 714, F32), ([3, 31, 31, 1], 299, F32),
            ([2, 48, 48, 1], 90, F64)]
FULL_LDS = [([3, 12, 12, 1], 714, F32), ([3, 31, 31, 1], 299, F32), ([2, 48, 48, 1], 90, F64)]       # exactly 163 840 B
# the rows of the launch-invariance test; n = 300 at the two full-LDS ones: more workgroups than compute units, one per CU
LAUNCH_CASES = [([2, 4, 6, 3, 1], 5, F32), ([2, 4, 6, 3, 1], 5, F64), ([2, 4, 6, 3, 1], 8, F32), ([2, 4, 6, 3, 1], 8, F64),
                ([2, 64, 66, 1], 17, F32), ([2, 64, 66, 1], 17, F64), ([3, 12, 12, 1], 714, F32), ([2, 48, 48, 1], 90, F64)]
K8_THREADS = 1024


def k8_takes(sizes, batch, dtype):
    """Does ``bnn_fused_sghmc_steps`` accept the row (1 .. 8 layers, its own footprint within 160 KiB)?"""
    return 1 <= len(sizes) - 1 <= MAX_LAYERS and k8_lds_bytes(sizes, batch, ESIZE[dtype]) != 0


# ---- the data: the recipe of tests/test_bnn_particles_gpu.py -------------------------------------------------------------------

def consts(batch):
    """The constants of the cost. ``batch_size`` is NOT the number of rows: ``models.bnn_posterior_scores`` runs K15 on chunks
    of rows with the batch size of the whole data set, so the two enter the head separately."""
    return dict(batch_size=float(batch + 3), n_examples=float(N_EXAMPLES), wdecay=1.0, prior_mean=1e-6, prior_var=0.01)


def make_data(sizes, batch, dtype, n=N_PARTICLES, seed=0):
    """(theta (n, P), X (batch, D0), y (batch,)) in ``dtype``: ``bnn_particles`` rows + 0.1 * randn (no bias is zero, no
    gradient element trivially so) with a distinct log_var per particle; X uniform in [-1, 1], y = sum sinc(2 x) + noise."""
    rng = np.random.RandomState(sizes[0] * 7 + len(sizes) + 1000 * batch + 13 * seed)
    X = rng.uniform(-1.0, 1.0, size=(batch, sizes[0]))
    y = np.sinc(X * 2.0).sum(axis=1) + 0.05 * rng.randn(batch)
    rows = torch.stack(bnn_particles(n, sizes[0], hidden=sizes[1:-1], seed=seed + 1, dtype=torch.float64)).numpy()
    rows = rows + 0.1 * rng.randn(*rows.shape)
    rows[:, -1] = -1.0 + 0.3 * rng.randn(n)
    return rows.astype(dtype), X.astype(dtype), y.astype(dtype)


def blocks(sizes):
    """[(name, layer or None, slice of the flat gradient)]: gW_l and gb_l of every layer, then d / d log_var."""
    off_w, off_b = N.param_offsets(sizes)
    out = []
    for l in range(1, len(sizes)):
        out.append(("gW%d" % l, l, slice(off_w[l], off_b[l])))
        out.append(("gb%d" % l, l, slice(off_b[l], off_b[l] + sizes[l])))
    P = C.n_params(sizes)
    out.append(("dlog_var", None, slice(P - 1, P)))
    return out


def flatten(grads):
    return np.concatenate([np.asarray(g).reshape(-1) for g in grads])


# ---- the kernel's statements in the kernel's order -----------------------------------------------------------------------------

def block_sum(v):
    """``particles_block_sum`` of the per-lane partial sums of a strided loop over ``v``: lane t adds v[t], v[t + 512], ... in
    that order, a wave adds its 64 lanes as an xor butterfly (32, 16, ..., 1), lane 0 adds the 8 waves in order."""
    kind = v.dtype.type
    parts = np.zeros(THREADS, dtype=kind)
    for at in range(0, v.size, THREADS):
        chunk = v[at:at + THREADS]
        parts[:chunk.size] = parts[:chunk.size] + chunk
    w = parts.reshape(THREADS // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    total = kind(0)
    for k in range(w.shape[0]):
        total = total + w[k, 0]
    return total


def _head(kind, s, tot, tsq, B, P, c):
    """The head's scalars behind the two sums, in ``kind`` (double in the kernel): (cost, d / d log_var, coef), uncast."""
    es = np.exp(s)
    inv = 1.0 / (es + kind(1e-16))
    wp_den = kind(P) + kind(2.0 * 1e-16 + 1e-16)
    lvp_den = kind(2.0 * c["prior_var"]) + kind(2.0 * 1e-16 + 1e-16)
    ln_pm, ln_pv = kind(np.log(c["prior_mean"])), kind(np.log(c["prior_var"]))
    bs, n_ex, Bd = kind(c["batch_size"]), kind(c["n_examples"]), kind(B)
    log_like = (-(tot * (0.5 * inv)) - 0.5 * s * Bd) / bs
    d = s - ln_pm
    lvp = -(d * d) / lvp_den - 0.5 * ln_pv
    wp = (-0.5 * kind(c["wdecay"])) * tsq / wp_den
    cost = -(log_like + lvp / n_ex + wp / n_ex)
    dlv = -((tot * (0.5 * es * inv * inv) - 0.5 * Bd) / bs + (-2.0 * d / lvp_den) / n_ex)
    coef = kind(c["wdecay"]) / (wp_den * n_ex)
    return cost, dlv, coef, inv, bs


def kernel_order(params, Xb, yb, consts, dtype, add_prior=True):
    """``(cost, [gW1, gb1, ..., gWL, gbL, d / d log_var (1, 1)])`` of one particle in ``dtype`` (float32, float64 or
    numpy.longdouble) by K15's statements in K15's order.

    Forward as ``small_net_cases.kernel_order``: acc = bias, k ascending fma chain, tanh in the dtype, every layer kept. The head
    in double (in long double for a long double run): inv = 1 / (exp(s) + 1e-16), delta_L = (T)(r * -(inv / batch_size)), the
    two sums in the order of the kernel's block sum, one cast of the cost and of d / d log_var at the end. gW one b-ascending fma
    chain from 0, gb a b-ascending plain sum, delta_{l-1} one j-ascending fma chain from 0 times (1 - h * h) with h * h rounded
    first; the prior term one multiply and one add, skipped when coef == 0. Vectorised over the output elements: the Python
    loops run over the reduction index only."""
    dt = np.dtype(dtype).type
    kind = np.longdouble if dt == np.longdouble else F64
    params = [np.asarray(p).astype(dt) for p in params]
    X, y = np.asarray(Xb).astype(dt), np.asarray(yb).astype(dt).reshape(-1)
    L, B = (len(params) - 1) // 2, X.shape[0]
    hs = [X]
    for l in range(L):
        W, bias, h = params[2 * l], params[2 * l + 1], hs[-1]
        acc = np.repeat(bias[None, :], B, axis=0)
        for k in range(W.shape[0]):
            acc = N.fma(h[:, k][:, None], W[k][None, :], acc)
        hs.append(np.tanh(acc) if l < L - 1 else acc)
        assert hs[-1].dtype == dt
    flat = flatten(params)
    wide_flat = flat.astype(kind)
    tsq = block_sum(wide_flat * wide_flat)
    r = y.astype(kind) - hs[L][:, 0].astype(kind)
    tot = block_sum(r * r)
    cost, dlv, coef, inv, bs = _head(kind, kind(flat[-1]), tot, tsq, B, flat.size, consts)
    delta = (r * -(inv / bs)).astype(dt)[:, None]
    grads = [None] * (2 * L) + [np.full((1, 1), dt(dlv), dtype=dt)]
    one = dt(1)
    for l in range(L, 0, -1):
        W, hin = params[2 * (l - 1)], hs[l - 1]
        gW, gb = np.zeros(W.shape, dtype=dt), np.zeros(W.shape[1], dtype=dt)
        for b in range(B):
            gW = N.fma(hin[b][:, None], delta[b][None, :], gW)
            gb = gb + delta[b]
        grads[2 * (l - 1)], grads[2 * (l - 1) + 1] = gW, gb
        if l > 1:
            acc = np.zeros((B, W.shape[0]), dtype=dt)
            for j in range(W.shape[1]):
                acc = N.fma(delta[:, j][:, None], W[:, j][None, :], acc)
            hh = hin * hin
            delta = acc * (one - hh)
        assert gW.dtype == gb.dtype == delta.dtype == dt
    coef = dt(coef)
    if add_prior and coef != 0:
        grads = [g + coef * p for g, p in zip(grads, params)]
    assert all(g.dtype == dt for g in grads)
    return dt(cost), grads


def statement(params, Xb, yb, consts, dtype, add_prior=True):
    """The same statements in ``dtype`` with numpy products and sums instead of the kernel's chains, nothing rounded to a
    narrower type on the way: the truth of a row when ``dtype`` is the next wider precision."""
    kind = np.dtype(dtype).type
    params = [np.asarray(p).astype(kind) for p in params]
    X, y = np.asarray(Xb).astype(kind), np.asarray(yb).astype(kind).reshape(-1)
    L, B = (len(params) - 1) // 2, X.shape[0]
    hs = [X]
    for l in range(L):
        a = hs[-1] @ params[2 * l] + params[2 * l + 1]
        hs.append(np.tanh(a) if l < L - 1 else a)
    flat = flatten(params)
    r = y - hs[L][:, 0]
    cost, dlv, coef, inv, bs = _head(kind, flat[-1], (r * r).sum(), (flat * flat).sum(), B, flat.size, consts)
    delta = (r * -(inv / bs))[:, None]
    grads = [None] * (2 * L) + [np.full((1, 1), dlv, dtype=kind)]
    for l in range(L, 0, -1):
        W, hin = params[2 * (l - 1)], hs[l - 1]
        grads[2 * (l - 1)], grads[2 * (l - 1) + 1] = hin.T @ delta, delta.sum(axis=0)
        if l > 1:
            delta = (delta @ W.T) * (1 - hin * hin)
    if add_prior:
        grads = [g + coef * p for g, p in zip(grads, params)]
    assert all(g.dtype == kind for g in grads)
    return cost, grads


def scalar_loop_f32(params, Xb, yb, consts, add_prior=True):
    """``kernel_order`` in float32 as plain Python loops, one scalar operation at a time. An fma is the product and the sum of
    the float32 values as Python floats (the product exact, the sum rounded to float64) rounded to float32: the arithmetic of
    ``small_net_cases.fma``, so the two agree bit for bit where the indexing does."""
    f32 = np.float32
    step = lambda a, b, c: f32(float(a) * float(b) + float(c))              # noqa: E731
    params = [np.asarray(p, dtype=f32) for p in params]
    X, y = np.asarray(Xb, dtype=f32), np.asarray(yb, dtype=f32).reshape(-1)
    L, B = (len(params) - 1) // 2, X.shape[0]
    hs = [X]
    for l in range(L):
        W, bias, h = params[2 * l], params[2 * l + 1], hs[-1]
        out = np.empty((B, W.shape[1]), dtype=f32)
        for b in range(B):
            for j in range(W.shape[1]):
                acc = f32(bias[j])
                for k in range(W.shape[0]):
                    acc = step(h[b, k], W[k, j], acc)
                out[b, j] = np.tanh(acc) if l < L - 1 else acc
        hs.append(out)

    def lanes_sum(values):
        parts = [0.0] * THREADS
        for i, v in enumerate(values):
            parts[i % THREADS] = parts[i % THREADS] + v
        total = 0.0
        for w in range(THREADS // 64):
            wave = parts[64 * w:64 * w + 64]
            for o in (32, 16, 8, 4, 2, 1):
                wave = [wave[t] + wave[t ^ o] for t in range(64)]
            total = total + wave[0]
        return F64(total)

    flat = flatten(params)
    tsq = lanes_sum([float(v) * float(v) for v in flat])
    r = [float(y[b]) - float(hs[L][b, 0]) for b in range(B)]
    tot = lanes_sum([v * v for v in r])
    cost, dlv, coef, inv, bs = _head(F64, F64(flat[-1]), tot, tsq, B, flat.size, consts)
    dscale = -(inv / bs)
    delta = np.array([[f32(F64(r[b]) * dscale)] for b in range(B)], dtype=f32)
    grads = [None] * (2 * L) + [np.full((1, 1), f32(dlv), dtype=f32)]
    for l in range(L, 0, -1):
        W, hin = params[2 * (l - 1)], hs[l - 1]
        gW, gb = np.empty(W.shape, dtype=f32), np.empty(W.shape[1], dtype=f32)
        for k in range(W.shape[0]):
            for j in range(W.shape[1]):
                acc = f32(0)
                for b in range(B):
                    acc = step(hin[b, k], delta[b, j], acc)
                gW[k, j] = acc
        for j in range(W.shape[1]):
            acc = f32(0)
            for b in range(B):
                acc = f32(acc + delta[b, j])
            gb[j] = acc
        grads[2 * (l - 1)], grads[2 * (l - 1) + 1] = gW, gb
        if l > 1:
            prev = np.empty((B, W.shape[0]), dtype=f32)
            for b in range(B):
                for k in range(W.shape[0]):
                    acc = f32(0)
                    for j in range(W.shape[1]):
                        acc = step(delta[b, j], W[k, j], acc)
                    hh = f32(hin[b, k] * hin[b, k])
                    prev[b, k] = f32(acc * f32(f32(1) - hh))
            delta = prev
    coef = f32(coef)
    if add_prior and coef != 0:
        grads = [(g + f32(coef) * p).astype(f32) for g, p in zip(grads, params)]
    return f32(cost), grads


# ---- a case: data, truth and the reference's own error, computed once and never modified ---------------------------------------

Case = collections.namedtuple("Case", "sizes B dtype P consts theta X y truth_cost truth_grad ko_cost ko_grad E")
_cases = {}


def case(sizes, B, dtype, n=N_PARTICLES, seed=0, log_var=None):
    """The row's data, the truth (``statement`` in the next wider precision on the widened inputs, full gradient), ``kernel_order``
    in the row's own dtype, and ``E``: per layer (gW_l and gb_l together), for ``dlog_var`` and for ``cost`` the largest error
    of ``kernel_order`` against the truth over all ``n`` particles. ``log_var``: values that replace the first particles'."""
    key = (tuple(sizes), B, np.dtype(dtype).name, n, seed, None if log_var is None else tuple(log_var))
    if key not in _cases:
        theta, X, y = make_data(sizes, B, dtype, n, seed)
        if log_var is not None:
            theta[:len(log_var), -1] = np.asarray(log_var, dtype=dtype)
        c, w = consts(B), wide(dtype)
        truth = [statement(C.split(row, sizes), X, y, c, w) for row in theta]
        ko = [kernel_order(C.split(row, sizes), X, y, c, dtype) for row in theta]
        truth_cost, truth_grad = np.array([t[0] for t in truth]), np.stack([flatten(t[1]) for t in truth])
        ko_cost, ko_grad = np.array([k[0] for k in ko]), np.stack([flatten(k[1]) for k in ko])
        assert ko_cost.dtype == ko_grad.dtype == np.dtype(dtype) and truth_grad.dtype == np.dtype(w)
        err = np.abs(ko_grad.astype(w) - truth_grad)
        E = {"cost": float(np.abs(ko_cost.astype(w) - truth_cost).max())}
        for name, layer, where in blocks(sizes):
            block = layer if layer is not None else name
            E[block] = max(E.get(block, 0.0), float(err[:, where].max()))
        for a in (theta, X, y, truth_cost, truth_grad, ko_cost, ko_grad):
            a.setflags(write=False)
        _cases[key] = Case(list(sizes), B, dtype, C.n_params(sizes), c, theta, X, y, truth_cost, truth_grad, ko_cost, ko_grad, E)
    return _cases[key]


def bounds(case_, p):
    """[(name, slice or None, E of the block, bound)] for particle ``p``: 4 * E + 4 * u_T * max|truth over the block|, the block
    of the last entry (slice None) being the cost."""
    u = U[case_.dtype]
    out = []
    for name, layer, where in blocks(case_.sizes):
        E = case_.E[layer if layer is not None else name]
        out.append((name, where, E, 4.0 * E + 4.0 * u * float(np.abs(case_.truth_grad[p, where]).max())))
    out.append(("cost", None, case_.E["cost"], 4.0 * case_.E["cost"] + 4.0 * u * float(abs(case_.truth_cost[p]))))
    return out
