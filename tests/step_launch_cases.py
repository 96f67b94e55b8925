"""Cases and reference side for the launch variants of the fused update (``sgmcmc_{sghmc,sgld,rsghmc}_step_{f32,f64}``), shared by
tests/test_step_launch_cases.py (no device: the table's own claims are proved there) and tests/test_step_launch_variants_gpu.py
(the kernels against it).

Three things live here:

* ``plan()``: a Python restatement of ``resolve_launch``, ``launch``, ``launch_vec`` and ``launch_scalar`` of
  ``csrc/sgmcmc_stream.hpp`` -- which kernel instantiation one call becomes, its grid and its number of grid-stride passes;
* the case list (``cases(kind, dtype)``): the smallest shapes at which each path can still go wrong. With G = block_threads x grid
  (the lanes of a launch) and P = G x quads (the quads of one pass): single pass at n = 1, 2, 3, 4 bt .. 4 bt + 3 and
  4 (2 bt + 5) + 2; grid-capped at max_blocks 1 and 3, every block size and quads per lane, n / 4 in {P + 1, 2 P - 1, 2 P + G + 7}
  with tails 0 and 3; element-wise at every misalignment, uncapped and grid-strided. The largest case is 27 679 elements
  (256 lanes x 3 blocks x 4 quads, the last of the three lengths);
* the reference side, which needs only numpy and the CPU oracle: states, gradients, the expected arrays after each of two
  consecutive steps and the expected statistics as float64 sums (``math.fsum``) of the oracle's arrays.
"""
import math
from collections import OrderedDict

import numpy as np

KINDS = ("sghmc", "sgld", "rsghmc")
DTYPES = ("f32", "f64")
NP = {"f32": np.float32, "f64": np.float64}
BLOCKS = (64, 128, 192, 256)
NT_AUTO_BYTES = 640 << 20
PATHS = ("single", "loop1", "loop2", "loop4", "elementwise")

# the state arrays of an entry in its argument order; `mom` = theta's partner (V, or p of the relativistic step)
ROWS = {"sghmc": ("theta", "V", "grad", "tau", "g", "v_hat", "minv", "r"),
        "sgld": ("theta", "grad", "tau", "g", "v_hat", "minv", "r"),
        "rsghmc": ("theta", "p", "grad")}
# by-value scalars of the entries (eps first). rsghmc: (eps, mass, c, D, b_hat) with flag = m^2 c^2 is a power of two
SCALARS = {"sghmc": (0.01, 50.0, 0.05), "sgld": (0.01, 1.0, 50.0)}
RSGHMC_MC = {True: (1.0, 1.0), False: (1.3, 0.7)}
STATS_MASK = {"sghmc": 0xF, "sgld": 0xD, "rsghmc": 0x3}
GRAD_DECAY = 3.7e-4
SEED = 2024


def scalars(kind, flag):
    if kind == "rsghmc":
        m, c = RSGHMC_MC[bool(flag)]
        return (0.01, m, c, 1.0, 0.0)
    return SCALARS[kind]


def elems_per_param(kind, flag, injected):
    """``elems()`` of the per-sampler translation units: elements streamed per parameter (sizes the nontemporal switch)."""
    if kind == "sghmc":
        return (12 if flag else 6) + (1 if injected else 0)
    if kind == "sgld":
        return (10 if flag else 4) + (1 if injected else 0)
    return 6 if injected else 5


def written(kind, flag, r_given):
    """Arrays a step writes; every other array of ROWS[kind] must come back unchanged."""
    if kind == "rsghmc":
        return ("theta", "p")
    out = ["theta"] + (["V"] if kind == "sghmc" else [])
    if flag:
        out += ["tau", "g", "v_hat", "minv"] + (["r"] if r_given else [])
    return tuple(out)


# -----------------------------------------------------------------------------------------------------------------------------
# the restatement

def resolve_launch(block_threads=0, quads_per_thread=0, max_blocks=0, nontemporal=-1):
    """``resolve_launch``: 0 (nontemporal: -1) keeps the default {auto block, 1 quad, 2^20 blocks, auto nontemporal}."""
    if block_threads not in (0, -1, 64, 128, 192, 256) or quads_per_thread not in (0, 1, 2, 4) or max_blocks < 0 \
            or nontemporal not in (-1, 0, 1, 2):
        raise ValueError("the library refuses this geometry")
    return dict(block_threads=block_threads or -1, qpt=quads_per_thread or 1, max_blocks=max_blocks or 1 << 20,
                nt=2 if nontemporal == -1 else nontemporal)


def want_blocks(n, bt, qpt):
    return max(1, -(-(n // 4) // (bt * qpt)))


def plan(n, dtype, aligned, cfg, kind="sghmc", flag=False, injected=False, stats=0, moments=False, gather=False, big_hint=False):
    """What ``launch()`` does with one call of n > 0 elements: cfg = the four LaunchConfig fields as a dict (missing = default),
    stats = 0 none / 1 all / 2 sum theta'^2 only. ``grid`` = the workgroups of the update = the statistics records written."""
    c = resolve_launch(**cfg)
    size = 4 if dtype == "f32" else 8
    big = big_hint or n * size * elems_per_param(kind, flag, injected) > NT_AUTO_BYTES
    bt = c["block_threads"] if c["block_threads"] > 0 else (128 if big else 256)
    out = dict(block_threads=bt, stats=stats, moments_fused=False, copy_fused=False, last_pass_partial=False)
    if not aligned:
        nq = (n + 3) // 4
        grid = min(max(1, -(-nq // bt)), c["max_blocks"])
        out.update(path="elementwise", quads=1, nontemporal=False, grid=grid, passes=-(-nq // (grid * bt)))
        return out
    nt = (big and size == 4) if c["nt"] == 2 else c["nt"] != 0
    q = 1 if size == 8 else (4 if c["qpt"] >= 4 else c["qpt"])
    fast = q == 1 and not injected
    want = want_blocks(n, bt, q)
    grid = min(want, c["max_blocks"])
    if q == 1 and want <= c["max_blocks"]:
        out.update(path="single", quads=1, nontemporal=nt, grid=grid, passes=1, moments_fused=fast and moments, copy_fused=gather)
        return out
    per_pass = grid * bt * q
    passes = max(1, -(-(n // 4) // per_pass))
    rem = n // 4 - (passes - 1) * per_pass
    out.update(path="loop%d" % q, quads=q, nontemporal=nt, grid=grid, passes=passes, last_pass_partial=0 < rem < per_pass)
    return out


def stats_records(n, dtype, cfg):
    """``sgmcmc_step_stats_records_sized``: the record count of a vector-path launch."""
    c = resolve_launch(**cfg)
    return min(want_blocks(n, c["block_threads"], 1 if dtype == "f64" else c["qpt"]), c["max_blocks"])


# -----------------------------------------------------------------------------------------------------------------------------
# the case list

def _geometries(dtype):
    """[(label, n, cfg, offsets)]: offsets = {array name or "all": elements off a 16-byte boundary}; {} = every array aligned."""
    out = []
    for bt in BLOCKS:
        for n in (1, 2, 3, 4 * bt, 4 * bt + 1, 4 * bt + 2, 4 * bt + 3, 4 * (2 * bt + 5) + 2):
            for nt in (0, 1):
                out.append(("single bt=%d n=%d nt=%d" % (bt, n, nt), n, dict(block_threads=bt, nontemporal=nt), {}))
    for mb in (1, 3):
        for bt in BLOCKS:
            for q in (1, 2, 4):
                used = 1 if dtype == "f64" else q                 # an f64 launch is asked for q quads and streams one
                G = bt * mb
                P = G * used
                for nq in (P + 1, 2 * P - 1, 2 * P + G + 7):
                    for tail in (0, 3):
                        for nt in (0, 1):
                            out.append(("capped mb=%d bt=%d q=%d nq=%d tail=%d nt=%d" % (mb, bt, q, nq, tail, nt), 4 * nq + tail,
                                        dict(block_threads=bt, quads_per_thread=q, max_blocks=mb, nontemporal=nt), {}))
    offs = [{"all": k} for k in ((1, 2, 3) if dtype == "f32" else (1,))] + [{"grad": 1}, {"xi": 1}, {"r": 1}, {"moments": 1}]
    for off in offs:
        for mb in (0, 2):
            for n in (3, 4 * 256 + 1, 4 * (5 * 256) + 3):
                out.append(("element-wise %s mb=%d n=%d" % (sorted(off.items()), mb, n), n, dict(max_blocks=mb), off))
    return out


def cases(kind, dtype):
    """The cases of one operator and dtype. Within each (path, nontemporal) group the operator instantiation
    (burn-in / frozen or POW2 / general division, injected / in-register noise) and the statistics mode rotate with the case's
    position, so that every reachable cell is met; ``r`` is given in every second dozen of burn-in cases and ``grad_decay`` is
    non-zero on every second case. A lone misaligned ``xi`` needs injected noise, a lone misaligned ``r`` a burn-in step that is given one
    (the relativistic step has no ``r``: that variant does not exist there), misaligned moments a call that asks for them."""
    out, seen = [], {}
    for label, n, cfg, off in _geometries(dtype):
        if "r" in off and kind == "rsghmc":
            continue
        p0 = plan(n, dtype, not off, cfg)
        key = (p0["path"], p0["nontemporal"])
        i = seen.get(key, 0)
        seen[key] = i + 1
        flag, injected, stats = bool(i & 1), bool(i & 2), (i // 4) % 3
        if "xi" in off:
            injected = True
        if "r" in off:
            flag = True
        case = dict(kind=kind, dtype=dtype, label=label, n=n, cfg=cfg, offsets=off, flag=flag, injected=injected, stats=stats,
                    r_given=("r" in off) or (kind != "rsghmc" and flag and (i // 12) % 2 == 0), moments="moments" in off,
                    grad_decay=GRAD_DECAY if (i + i // 12) % 2 else 0.0, index=len(out))
        case["plan"] = plan(n, dtype, not off, cfg, kind, flag, injected, stats, moments=case["moments"])
        out.append(case)
    return out


def offset_of(case, name):
    """Elements by which array ``name`` of the case starts off a 16-byte boundary."""
    off = case["offsets"]
    if name in ("mean", "m2"):
        return off.get("moments", off.get("all", 0))
    return off.get(name, off.get("all", 0))


def reachable_cells(kind, dtype):
    """Every (path, nontemporal, statistics mode, flag, injected) the library can reach for this operator and dtype: an f64 launch
    streams one quad per lane, and the element-wise kernel has no nontemporal form."""
    cells = set()
    for path in PATHS:
        if dtype == "f64" and path in ("loop2", "loop4"):
            continue
        for nt in ((False,) if path == "elementwise" else (False, True)):
            for stats in (0, 1, 2):
                for flag in (False, True):
                    for injected in (False, True):
                        cells.add((path, nt, stats, flag, injected))
    return cells


def cell(case):
    p = case["plan"]
    return (p["path"], p["nontemporal"], p["stats"], case["flag"], case["injected"])


# the high counter word of philox_quad (global quad >> 32): (first_element, n). The first straddles global quad 2^32
HIGH_WORD_CASES = ((2 ** 34 - 4 * 130, 1031), (2 ** 40 + 4, 1031))
HIGH_WORD_SEED, HIGH_WORD_STEP = 77, 5


# -----------------------------------------------------------------------------------------------------------------------------
# the reference side

def initial_state(case):
    dt = NP[case["dtype"]]
    n = case["n"]
    rng = np.random.default_rng([KINDS.index(case["kind"]), DTYPES.index(case["dtype"]), case["index"]])
    st = OrderedDict()
    st["theta"] = (rng.normal(size=n) * 0.5).astype(dt)
    st["V" if case["kind"] != "rsghmc" else "p"] = (rng.normal(size=n) * 0.1).astype(dt)
    if case["kind"] != "rsghmc":
        st["tau"] = (1.0 + rng.random(n)).astype(dt)
        st["g"] = (rng.normal(size=n) * 0.2).astype(dt)
        st["v_hat"] = (0.1 + rng.random(n)).astype(dt)
        st["minv"] = (0.5 + rng.random(n)).astype(dt)
        st["r"] = np.full(n, 0.5, dt)
    if case["kind"] == "sgld":
        del st["V"]
    st["mean"] = (rng.normal(size=n) * 0.3).astype(dt)
    st["m2"] = rng.random(n).astype(dt)
    grads = [(rng.normal(size=n) * 0.3).astype(dt) for _ in range(2)]
    xis = [rng.normal(size=n).astype(dt) for _ in range(2)]
    return st, grads, xis


def oracle_step(oracle, case, st, grad, xi, seed=0, step=0):
    """One step of the C oracle on the dict of arrays ``st`` (in place; ``r`` only where the call is given one). xi = None draws
    the oracle's own Philox stream for (seed, step)."""
    dt = NP[case["dtype"]]
    c = oracle.CState(st["theta"], dt)
    for name in ("V", "p", "tau", "g", "v_hat", "minv", "r"):
        if name in st:
            getattr(c, name)[:] = st[name]
    kind, flag, wd = case["kind"], case["flag"], case["grad_decay"]
    s = scalars(kind, flag)
    if kind == "sghmc":
        oracle.c_sghmc_step(c, grad, s[0], s[1], s[2], flag, xi, seed=seed, step=step, grad_decay=wd)
    elif kind == "sgld":
        oracle.c_sgld_step(c, grad, s[0], s[1], s[2], flag, xi, seed=seed, step=step, grad_decay=wd)
    else:
        oracle.c_rsghmc_step(c, grad, s[0], s[1], s[2], s[3], s[4], xi, seed=seed, step=step, grad_decay=wd)
    for name in written(kind, flag, case["r_given"]):
        st[name] = getattr(c, name).copy()
    return st


def true_sums(case, st):
    """{sum theta^2, sum V^2 (p^2), sum minv, sum minv^2} of the arrays in float64: squares of f32 values are exact in float64
    (of f64 values: rounded once, relative error <= 2^-53) and math.fsum adds them with one rounding. Slots the operator does not
    reduce are 0.0."""
    def sq(a):
        a = a.astype(np.float64)
        return math.fsum(a * a)
    mom = st.get("V", st.get("p"))
    out = [sq(st["theta"]), sq(mom) if mom is not None else 0.0, 0.0, 0.0]
    if case["kind"] != "rsghmc":
        out[2] = math.fsum(st["minv"].astype(np.float64))
        out[3] = sq(st["minv"])
    return out


def stats_bound(case, records=None):
    """Relative bound on a statistic against its true sum, from the kernel's code. Every term is non-negative, so each rounding
    a term passes through costs at most one unit roundoff of the format it happens in. In the kernel's dtype T: the product
    (1), the quad's adds in ``accumulate`` (3: the first adds to 0), the lane's running total where that is kept in T (the
    single pass: 1, the second quad a tail lane adds; f64 looping kernels: one per further quad of the lane), the ``(T)acc`` cast
    where the total was kept in double and T is float (1), the six DPP adds of ``wave_sum_dpp_lane63`` (6). In double: the
    lane's running total of an f32 looping or element-wise kernel (one per quad of the lane), the adds over waves and records
    (waves + records: an add with an exact 0 does not round), and the reference's own rounding (1).
    Returns (count in T, count in double, bound): f32 single pass 10 -> 5.96e-7, with a tail 11 -> 6.6e-7; f64 11..15 -> 1.2e-15..1.7e-15."""
    p = case["plan"]
    f32 = case["dtype"] == "f32"
    tail = 1 if case["n"] % 4 else 0
    lane_quads = p["passes"] * p["quads"] + (tail if p["path"] != "elementwise" else 0)
    in_t, in_d = 1 + 3 + 6, 1 + (p["block_threads"] // 64) + (p["grid"] if records is None else records)
    if p["path"] == "single":
        in_t += tail
    elif f32:
        in_t += 1
        in_d += lane_quads
    else:
        in_t += lane_quads - 1
    u = 2.0 ** -24 if f32 else 2.0 ** -53
    k = in_t * u
    return in_t, in_d, k / (1.0 - k) + in_d * 2.0 ** -53


def noise_bar(z, near_one, dtype):
    """The noise bar of tests/test_hip_parity.py: f32 |gpu - oracle| <= 4e-6 max(1, |z|), 1e-4 where u is within 2^-20 of 1;
    f64 1e-12."""
    if dtype == "f64":
        return np.full(z.shape, 1e-12)
    return np.where(near_one, 1e-4, 4e-6 * np.maximum(1.0, np.abs(z.astype(np.float64))))


def near_one_mask(oracle, seed, step, first_element, n):
    """Per element: the Philox word that feeds log() of its pair is above 0xFFFFF000 (u within 2^-20 of 1)."""
    q0 = first_element // 4
    out = np.zeros(4 * ((n + 3) // 4), bool)
    for k in range((n + 3) // 4):
        q = q0 + k
        x = oracle.py_philox4x32_10((step & 0xFFFFFFFF, step >> 32, q & 0xFFFFFFFF, q >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        out[4 * k:4 * k + 2] = x[0] > 0xFFFFF000
        out[4 * k + 2:4 * k + 4] = x[2] > 0xFFFFF000
    return out[:n]
