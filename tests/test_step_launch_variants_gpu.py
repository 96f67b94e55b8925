"""The fused update at every launch variant (``csrc/sgmcmc_stream.hpp``: single pass, grid-capped with 1, 2 and 4 quads per
lane, element-wise; nontemporal or plain; no statistics, all, theta^2 only; every operator instantiation; f32 and f64) against
the CPU oracle. The cases, the restated launch logic and the reference side are tests/step_launch_cases.py; what the table
claims about itself is proved without a device in tests/test_step_launch_cases.py.

Every test walks its geometries inside one function and reports every miss it met, not only the first.
"""
import numpy as np
import pytest
import torch

import step_launch_cases as C

pytestmark = pytest.mark.gpu

TH = {"f32": torch.float32, "f64": torch.float64}
ALL = [(k, d) for k in C.KINDS for d in C.DTYPES]
GUARD = 4            # elements in front of and behind every array (16 / 32 bytes: the slice behind them is 16-byte aligned)
SENTINEL = -7.0


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(_bits(np.ascontiguousarray(got)), _bits(np.ascontiguousarray(want)))


class Placed(object):
    """Host arrays as slices of guarded device buffers, each ``offsets[name]`` elements off a 16-byte boundary."""

    def __init__(self, gpu, dtype):
        self.gpu, self.dtype, self.buf, self.view, self.span = gpu, TH[dtype], {}, {}, {}

    def put(self, name, host, off=0):
        n = host.size
        buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=self.dtype, device=self.gpu)
        view = buf[GUARD + off:GUARD + off + n]
        view.copy_(torch.from_numpy(np.ascontiguousarray(host)))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (off * buf.element_size()) % 16
        self.buf[name], self.view[name], self.span[name] = buf, view, (GUARD + off, GUARD + off + n)
        return view

    def get(self, name):
        return self.view[name].cpu().numpy()

    def guards_intact(self, name):
        lo, hi = self.span[name]
        b = self.buf[name]
        return bool((b[:lo] == SENTINEL).all()) and bool((b[hi:] == SENTINEL).all())


def _place_case(gpu, case, st):
    d = Placed(gpu, case["dtype"])
    for name, a in st.items():
        d.put(name, a, C.offset_of(case, name))
    return d


def _step(K, case, d, grad, xi, step, seed=C.SEED, stats=None, opts=None, launch="case", step_dev=None, views=None):
    kind, flag = case["kind"], case["flag"]
    s = C.scalars(kind, flag)
    v = d.view if views is None else views
    cfg = K.LaunchConfig(**case["cfg"]) if isinstance(launch, str) else launch
    kw = dict(xi=xi, seed=seed, step=step, step_dev=step_dev, stats=stats, grad_decay=case["grad_decay"], launch=cfg, opts=opts)
    if kind == "sghmc":
        K.sghmc_step(v["theta"], v["V"], grad, v["tau"], v["g"], v["v_hat"], v["minv"], v["r"] if case["r_given"] else None,
                     s[0], s[1], s[2], flag, **kw)
    elif kind == "sgld":
        K.sgld_step(v["theta"], grad, v["tau"], v["g"], v["v_hat"], v["minv"], v["r"] if case["r_given"] else None,
                    s[0], s[1], s[2], flag, **kw)
    else:
        K.rsghmc_step(v["theta"], v["p"], grad, s[0], s[1], s[2], s[3], s[4], **kw)


def _noise(K, gpu, case, t):
    """(xi for the kernel, xi for the oracle). In-register cases: the oracle is fed ``kernels.philox_normal`` at the default
    geometry, copied to the host -- the stream tests/test_hip_parity.py::test_philox_normal_f32_tolerance and
    ::test_philox_normal_f64_tolerance pin to the oracle's own."""
    z = torch.empty(case["n"], dtype=TH[case["dtype"]], device=gpu)
    K.philox_normal(z, C.SEED, t)
    return None, z.cpu().numpy()


def _records(stats):
    return int(stats.workspace.view(torch.int64)[0])


def _check_stats(case, got, want, mode, bound, what, miss):
    """``bound`` = step_launch_cases.stats_bound(case)[2]: roundings in the kernel's dtype {product 1, quad adds 3, running total or
    cast 0 .. 5, DPP tree 6} x its unit roundoff + (lane quads + waves + records + 1) x 2^-53. f32: 10 roundings -> 5.96e-7
    (single pass), 11 -> 6.56e-7 (a tail lane, every looping and element-wise kernel); f64: 10 .. 15 -> 1.1e-15 .. 1.7e-15, with
    the double part 1.2e-15 .. 3e-15 in all."""
    mask = C.STATS_MASK[case["kind"]] & (1 if mode == 2 else 0xF)
    for k in range(4):
        if (mask >> k) & 1:
            if not abs(got[k] - want[k]) <= bound * want[k]:
                miss.append("%s: statistic %d = %r, true sum %r, relative error %.3g > %.3g" % (
                    what, k, got[k], want[k], abs(got[k] - want[k]) / want[k], bound))
        elif got[k] != 0.0:
            miss.append("%s: statistic %d = %r outside the mask, must be exactly 0" % (what, k, got[k]))


def _report(miss):
    assert not miss, "%d misses, first 12:\n%s" % (len(miss), "\n".join(miss[:12]))


@pytest.mark.parametrize("kind,dtype", ALL)
def test_arrays_and_statistics_on_every_case(gpu, oracle, kind, dtype):
    """Every case of the table, two consecutive steps. Injected noise: every array the operator writes is bit-equal to the oracle,
    every other array and every guard element unchanged. In-register noise: the same against the oracle step fed with
    ``kernels.philox_normal(out, seed, step)`` at the default geometry (see ``_noise``). With a workspace: the header's record
    count is the restated grid; the statistics equal the float64 sums of the oracle's arrays within the derived bound
    (``step_launch_cases.stats_bound``: 10 or 11 roundings in f32 -> 5.96e-7 / 6.6e-7 relative, 10 .. 15 in f64 -> 1.2e-15 ..
    1.7e-15, plus (lane quads + waves + records + 1) x 2^-53); slots outside the mask are exactly 0 (theta^2 only: slots 1-3).
    A call that asks for moments on misaligned arrays gets the separate Welford pass, bit-equal to the oracle's."""
    from pysgmcmc_amd import kernels as K
    cases = C.cases(kind, dtype)
    stats = K.StepStats(max(c["n"] for c in cases), gpu)
    miss = []
    for case in cases:
        ref, grads, xis = C.initial_state(case)
        d = _place_case(gpu, case, ref)
        before = {k: v.copy() for k, v in ref.items()}
        wr = C.written(kind, case["flag"], case["r_given"]) + (("mean", "m2") if case["moments"] else ())
        in_t, in_d, bound = C.stats_bound(case)
        for t in range(2):
            what = "%s step %d" % (case["label"], t)
            grad = d.put("grad", grads[t], C.offset_of(case, "grad"))
            if case["injected"]:
                xi, xi_host = d.put("xi", xis[t], C.offset_of(case, "xi")), xis[t]
            else:
                xi, xi_host = _noise(K, gpu, case, t)
            opts = {}
            if case["stats"] == 2:
                opts["theta_sq_only"] = True
            if case["moments"]:
                opts["moments"] = (d.view["mean"], d.view["m2"], 5 + t)
            stats.workspace.zero_()
            _step(K, case, d, grad, xi, t, stats=stats if case["stats"] else None, opts=opts or None)
            C.oracle_step(oracle, case, ref, grads[t], xi_host)
            if case["moments"]:
                oracle.c_moments_update(ref["theta"], ref["mean"], ref["m2"], 5 + t)
            for name in ref:
                want = ref[name] if name in wr else before[name]
                got = d.get(name)
                if not _same(got, want):
                    bad = np.flatnonzero(_bits(got) != _bits(want))
                    miss.append("%s: %s %s in %d of %d elements, first at %d: gpu %r oracle %r" % (
                        what, name, "differs" if name in wr else "was written", bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))
                if not d.guards_intact(name):
                    miss.append("%s: a guard element of %s was written" % (what, name))
            if not _same(d.get("grad"), grads[t]) or not d.guards_intact("grad"):
                miss.append("%s: grad or its guards were written" % what)
            if case["stats"]:
                if _records(stats) != case["plan"]["grid"]:
                    miss.append("%s: %d records in the header, restated grid %d" % (what, _records(stats), case["plan"]["grid"]))
                got = K.step_stats_finish(stats).cpu().numpy()
                _check_stats(case, got, C.true_sums(case, ref), case["stats"], bound, what, miss)
    _report(miss)


@pytest.mark.parametrize("kind,dtype", ALL)
def test_theta_sq_only_on_every_path(gpu, oracle, kind, dtype):
    """``stats_select = SGMCMC_STATS_THETA_SQ`` on every theta^2-only case of the table (every path, nontemporal mode and
    operator instantiation): slot 0 is bit-equal to slot 0 of the full reduction of the same launch, slots 1-3 are exactly 0.0
    as include/sgmcmc_hip.h says, the chain is the chain of the full reduction."""
    from pysgmcmc_amd import kernels as K
    cases = [c for c in C.cases(kind, dtype) if c["stats"] == 2]
    assert {(c["plan"]["path"], c["plan"]["nontemporal"], c["flag"], c["injected"]) for c in cases} == {
        cell[:2] + cell[3:] for cell in C.reachable_cells(kind, dtype)}
    full, only = K.StepStats(max(c["n"] for c in cases), gpu), K.StepStats(max(c["n"] for c in cases), gpu)
    miss = []
    for case in cases:
        st, grads, xis = C.initial_state(case)
        a, b = _place_case(gpu, case, st), _place_case(gpu, case, st)
        grad = a.put("grad", grads[0], C.offset_of(case, "grad"))
        xi = a.put("xi", xis[0], C.offset_of(case, "xi")) if case["injected"] else None
        # (a lone misaligned moments pair is what sends its cases down the element-wise path: both launches ask for moments)
        mom = (lambda d: dict(moments=(d.view["mean"], d.view["m2"], 5))) if case["moments"] else (lambda d: {})
        _step(K, case, a, grad, xi, 1, stats=full, opts=mom(a) or None)
        _step(K, case, b, grad, xi, 1, stats=only, opts=dict(theta_sq_only=True, **mom(b)))
        fa, fb = K.step_stats_finish(full).cpu().numpy().copy(), K.step_stats_finish(only).cpu().numpy().copy()
        if fa[0] != fb[0] or not fb[0] > 0:
            miss.append("%s: sum theta^2 %r, full reduction %r" % (case["label"], fb[0], fa[0]))
        if np.any(fb[1:] != 0.0):
            miss.append("%s: statistics 1-3 = %r, the header says 0" % (case["label"], fb[1:]))
        if _records(only) != case["plan"]["grid"] or _records(full) != case["plan"]["grid"]:
            miss.append("%s: record counts %d / %d, restated grid %d" % (case["label"], _records(full), _records(only), case["plan"]["grid"]))
        for name in st:
            if not torch.equal(a.view[name], b.view[name]):
                miss.append("%s: %s differs between the two reductions" % (case["label"], name))
    _report(miss)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_philox_normal_is_the_same_on_every_geometry(gpu, dtype):
    """``NormalFillOp`` goes through the same streaming kernels: ``philox_normal(..., launch=cfg)`` on every geometry of the table,
    and on outputs 1, 2 and 3 elements (f64: 1) off a 16-byte boundary, returns the bits of the default geometry."""
    from pysgmcmc_amd import kernels as K
    seen, miss = set(), []
    for case in C.cases("sghmc", dtype):
        off = case["offsets"].get("all", 0)
        if case["offsets"] and not off:
            continue
        key = (case["n"], off, tuple(sorted(case["cfg"].items())))
        if key in seen:
            continue
        seen.add(key)
        want = torch.empty(case["n"], dtype=TH[dtype], device=gpu)
        K.philox_normal(want, C.SEED, 3)
        d = Placed(gpu, dtype)
        out = d.put("out", np.zeros(case["n"], C.NP[dtype]), off)
        K.philox_normal(out, C.SEED, 3, launch=K.LaunchConfig(**case["cfg"]))
        if not torch.equal(out, want) or not d.guards_intact("out"):
            miss.append("%s: %d of %d draws differ from the default geometry (guards intact: %s)" % (
                case["label"], int((out != want).sum()), case["n"], d.guards_intact("out")))
    assert len(seen) > 300
    _report(miss)


def _pick(kind, dtype, path_prefix, **want):
    for c in C.cases(kind, dtype):
        if c["plan"]["path"].startswith(path_prefix) and all(c[k] == v for k, v in want.items()) and c["plan"]["passes"] > 1 \
                and set(c["offsets"]) <= {"all"}:
            return c
    raise AssertionError("no such case in the table")


@pytest.mark.parametrize("kind,dtype", ALL)
def test_device_step_counter_on_looping_and_element_wise_launches(gpu, kind, dtype):
    """``step_dev``: a grid-capped and an element-wise in-register launch that take the step from a device counter (3) plus a
    by-value step (4) draw the stream of the by-value step 7, on both instantiations of the operator."""
    from pysgmcmc_amd import kernels as K
    counter = torch.tensor([3], dtype=torch.int64, device=gpu)
    for prefix in ("loop", "elementwise"):
        for flag in (False, True):
            case = dict(_pick(kind, dtype, prefix), injected=False, flag=flag, r_given=False)
            st, grads, _ = C.initial_state(case)
            a, b = _place_case(gpu, case, st), _place_case(gpu, case, st)
            grad = a.put("grad", grads[0], C.offset_of(case, "grad"))
            _step(K, case, a, grad, None, 4, step_dev=counter)
            _step(K, case, b, grad, None, 7)
            for name in st:
                assert torch.equal(a.view[name], b.view[name]), (case["label"], name)
            assert not torch.equal(a.view["theta"], torch.from_numpy(st["theta"]).to(gpu))
            _step(K, case, b, grad, None, 4)            # another step: another stream
            assert not torch.equal(a.view["theta"], b.view["theta"])


@pytest.mark.parametrize("quads", [1, 2, 4])
@pytest.mark.parametrize("kind,dtype", ALL)
def test_slices_of_looping_and_element_wise_launches(gpu, kind, dtype, quads):
    """``first_element`` slices issued as grid-capped, uncapped-with-several-quads and element-wise launches reproduce the single
    launch bit for bit, in any order; with each slice's record count from ``kernels.step_stats_records(n, launch, dtype)`` the
    shared workspace holds exactly the records the slices wrote (the header's count) and finishes to the single launch's
    statistics, to the tolerance of tests/test_step_opts_gpu.py::test_slice_launches_equal_the_single_launch. An f64 launch
    streams one quad per lane whatever ``quads_per_thread`` says; its count must say so too."""
    from pysgmcmc_amd import kernels as K
    n = 20_003
    cuts = [0, 4 * 1000, 4 * 2301, 4 * 2302, n]
    spans = list(zip(cuts[:-1], cuts[1:]))
    miss = []
    for flag in (False, True):
        case = dict(kind=kind, dtype=dtype, n=n, flag=flag, r_given=False, grad_decay=0.0, index=1000 + int(flag), offsets={}, cfg={})
        st, grads, _ = C.initial_state(case)
        one = _place_case(gpu, case, st)
        grad = one.put("grad", grads[0])
        s_one = K.StepStats(n, gpu)
        _step(K, case, one, grad, None, 7, seed=11, stats=s_one, launch=None)
        want = K.step_stats_finish(s_one).cpu().numpy().copy()
        for variant, max_blocks in (("grid-capped", 3), ("uncapped", 0), ("element-wise", 2)):
            off = 1 if variant == "element-wise" else 0
            sl_case = dict(case, offsets={"all": off} if off else {})
            got = _place_case(gpu, sl_case, st)
            g = got.put("grad", grads[0], off)
            cfg = dict(block_threads=128, quads_per_thread=quads, max_blocks=max_blocks)
            launch = K.LaunchConfig(**cfg)
            plans = [C.plan(hi - lo, dtype, not off, cfg, kind, flag) for lo, hi in spans]
            blocks = [K.step_stats_records(hi - lo, launch, TH[dtype]) for lo, hi in spans]
            if blocks != [p["grid"] for p in plans]:
                miss.append("%s flag=%s: step_stats_records says %r, the launches use %r" % (variant, flag, blocks, [p["grid"] for p in plans]))
            bases = np.concatenate([[0], np.cumsum(blocks)[:-1]])
            s_got = K.StepStats(n, gpu)
            s_got.workspace.zero_()
            for i in (2, 0, 3, 1):
                lo, hi = spans[i]
                views = {k: v[lo:hi] for k, v in got.view.items()}
                _step(K, sl_case, got, g[lo:hi], None, 7, seed=11, stats=s_got, launch=launch, views=views,
                      opts=dict(first_element=lo, stats_base=int(bases[i]), stats_total=int(sum(blocks))))
            for name in st:
                if not torch.equal(one.view[name], got.view[name]) or not got.guards_intact(name):
                    miss.append("%s flag=%s: %s differs from the single launch" % (variant, flag, name))
            if _records(s_got) != sum(p["grid"] for p in plans):
                miss.append("%s flag=%s: header holds %d records, the slices wrote %d" % (variant, flag, _records(s_got), sum(p["grid"] for p in plans)))
            have = K.step_stats_finish(s_got).cpu().numpy()
            if not np.allclose(want, have, rtol=2e-6 if dtype == "f32" else 1e-13) or not want[0] > 0:
                miss.append("%s flag=%s: statistics %r, single launch %r" % (variant, flag, have, want))
    _report(miss)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_high_counter_word_on_every_path(gpu, oracle, dtype):
    """``philox_quad`` feeds (gq, gq >> 32) into the counter. In-register noise at first_element = 2^34 - 520 (the 1031 elements
    straddle global quad 2^32) and at 2^40 + 4, on the single-pass, grid-capped and element-wise paths: a frozen SGHMC step with
    theta = V = grad = 0, minv = 1, grad_decay = 0 gives V' = sigma z in one rounding, so
    |V'_gpu - V'_oracle| <= sigma bar(z) + 1 ulp with the oracle fed ``c_philox_normal_range(seed, step, first_element, n)`` and
    bar the noise bar of tests/test_hip_parity.py. No element is excluded; tests/test_step_launch_cases.py shows that a dropped
    high word misses this by orders of magnitude."""
    from pysgmcmc_amd import kernels as K
    dt = C.NP[dtype]
    eps, sg, md = C.SCALARS["sghmc"]
    miss = []
    for first, n in C.HIGH_WORD_CASES:
        z = oracle.c_philox_normal_range(C.HIGH_WORD_SEED, C.HIGH_WORD_STEP, first, n, dt)
        zero = np.zeros(n, dt)

        def oracle_v(xi):
            c = oracle.CState(zero, dt)
            oracle.c_sghmc_step(c, zero, eps, sg, md, False, xi)
            return c.V.astype(np.float64)
        sigma = oracle_v(np.ones(n, dt))
        want = oracle_v(z)
        assert np.all(sigma == sigma[0]) and sigma[0] > 0
        bound = sigma * C.noise_bar(z, C.near_one_mask(oracle, C.HIGH_WORD_SEED, C.HIGH_WORD_STEP, first, n), dtype) + np.spacing(np.abs(want.astype(dt))).astype(np.float64)
        for path, cfg, off in (("single", {}, 0), ("loop2" if dtype == "f32" else "loop1", dict(block_threads=64, quads_per_thread=2, max_blocks=1), 0),
                               ("elementwise", dict(max_blocks=2, block_threads=64), 1)):
            plan = C.plan(n, dtype, not off, cfg)
            assert plan["path"] == path and (path == "single" or plan["passes"] >= 2)
            d = Placed(gpu, dtype)
            for name in ("theta", "V", "grad"):
                d.put(name, zero, off)
            d.put("minv", np.ones(n, dt), off)
            v = d.view
            K.sghmc_step(v["theta"], v["V"], v["grad"], None, None, None, v["minv"], None, eps, sg, md, False, seed=C.HIGH_WORD_SEED,
                         step=C.HIGH_WORD_STEP, launch=K.LaunchConfig(**cfg), opts=dict(first_element=first))
            got = d.get("V").astype(np.float64)
            err = np.abs(got - want)
            if not np.all(err <= bound):
                k = int(np.argmax(err / bound))
                miss.append("first_element %d, %s: %d of %d elements miss the bar, worst at %d: gpu %r oracle %r bound %.3g" % (
                    first, path, int((err > bound).sum()), n, k, got[k], want[k], bound[k]))
            if not _same(d.get("theta"), d.get("V")) or not all(d.guards_intact(k) for k in v):
                miss.append("first_element %d, %s: theta' != V' or a guard was written" % (first, path))
    _report(miss)


@pytest.mark.parametrize("kind,dtype", ALL)
def test_gather_and_moments_fall_back_on_looping_and_element_wise_launches(gpu, oracle, kind, dtype):
    """Launches without a fused form for them (grid-capped, element-wise) still deliver ``opts.gather_*`` (``finish_side_copy``)
    and the Welford moments (the separate K4 launch): the window lands as
    tests/test_step_opts_gpu.py::test_window_gather_rides_in_the_step_launch asserts, mean / m2 are the bits
    ::test_fused_moments_equal_the_separate_welford_pass asserts -- and here the chain, the moments and the statistics are also
    held against the oracle."""
    from pysgmcmc_amd import kernels as K
    B, D, N = 32, 12, 500
    g = torch.Generator(device=gpu).manual_seed(3)
    X = torch.randn(N, D, dtype=TH[dtype], device=gpu, generator=g)
    y = torch.randn(N, dtype=TH[dtype], device=gpu, generator=g)
    start = 100 if dtype == "f64" else 96
    miss = []
    for prefix in ("loop", "elementwise"):
        case = _pick(kind, dtype, prefix, stats=1)
        assert not case["plan"]["moments_fused"] and not case["plan"]["copy_fused"]
        ref, grads, xis = C.initial_state(case)
        d = _place_case(gpu, case, ref)
        before = {k: v.copy() for k, v in ref.items()}
        stats = K.StepStats(case["n"], gpu)
        wr = C.written(kind, case["flag"], case["r_given"]) + ("mean", "m2")
        for t in range(2):
            what = "%s step %d" % (case["label"], t)
            xbuf = torch.full((B, D + 4), SENTINEL, dtype=TH[dtype], device=gpu)
            ybuf = torch.full((B,), SENTINEL, dtype=TH[dtype], device=gpu)
            grad = d.put("grad", grads[t], C.offset_of(case, "grad"))
            if case["injected"]:
                xi, xi_host = d.put("xi", xis[t], C.offset_of(case, "xi")), xis[t]
            else:
                xi, xi_host = _noise(K, gpu, case, t)
            _step(K, case, d, grad, xi, t, stats=stats,
                  opts=dict(moments=(d.view["mean"], d.view["m2"], 5 + t), gather=(X, y, start + t, xbuf[:, :D], ybuf)))
            C.oracle_step(oracle, case, ref, grads[t], xi_host)
            oracle.c_moments_update(ref["theta"], ref["mean"], ref["m2"], 5 + t)
            for name in ref:
                if not _same(d.get(name), ref[name] if name in wr else before[name]) or not d.guards_intact(name):
                    miss.append("%s: %s differs from the oracle" % (what, name))
            if not (torch.equal(xbuf[:, :D], X[start + t:start + t + B]) and bool(torch.all(xbuf[:, D:] == SENTINEL))
                    and torch.equal(ybuf, y[start + t:start + t + B])):
                miss.append("%s: the gathered window is not X / y[%d:%d]" % (what, start + t, start + t + B))
            _check_stats(case, K.step_stats_finish(stats).cpu().numpy(), C.true_sums(case, ref), 1, C.stats_bound(case)[2], what, miss)
    _report(miss)
