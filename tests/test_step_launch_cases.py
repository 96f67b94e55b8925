"""The cases of tests/test_step_launch_variants_gpu.py, checked without a device (tests/step_launch_cases.py): the table reaches
every launch variant the library can reach, its grid-capped cases really loop, the Python restatement of the launch logic counts
the blocks the library's host arithmetic counts, the reference side is finite, and the large-offset cases can tell a kept high
counter word from a dropped one."""
import ctypes

import numpy as np
import pytest

import step_launch_cases as C

ALL = [(k, d) for k in C.KINDS for d in C.DTYPES]


@pytest.mark.parametrize("kind,dtype", ALL)
def test_every_reachable_cell_is_reached(kind, dtype):
    """{single pass, grid-capped with 1, 2 and 4 quads, element-wise} x {nontemporal on, off} x {no statistics, all, theta^2 only}
    x {each operator instantiation}: read from the restatement, case by case. f32: 9 x 3 x 4 = 108 cells per operator,
    f64 (one quad per lane): 5 x 3 x 4 = 60."""
    want = C.reachable_cells(kind, dtype)
    assert len(want) == (108 if dtype == "f32" else 60)
    got = {C.cell(c) for c in C.cases(kind, dtype)}
    assert got == want, sorted(want - got) + sorted(got - want)
    cases = C.cases(kind, dtype)
    assert max(c["n"] for c in cases) == 4 * (2 * 3072 + 768 + 7) + 3 if dtype == "f32" else True
    assert all(c["n"] <= 27_679 for c in cases)
    # the options that ride on the cells
    adapt = [c for c in cases if c["flag"] and kind != "rsghmc"]
    assert kind == "rsghmc" or ({c["r_given"] for c in adapt} == {True, False})
    decay = [c["grad_decay"] != 0.0 for c in cases]
    assert 0.4 < sum(decay) / len(decay) < 0.6
    for path in C.PATHS:
        here = [c for c in cases if c["plan"]["path"] == path]
        if here:
            assert {c["grad_decay"] != 0.0 for c in here} == {True, False}, path
    ew = [c for c in cases if c["plan"]["path"] == "elementwise"]
    lone = {tuple(sorted(c["offsets"])) for c in ew}
    assert lone == {("all",), ("grad",), ("xi",), ("moments",)} | ({("r",)} if kind != "rsghmc" else set())
    assert {c["offsets"]["all"] for c in ew if "all" in c["offsets"]} == ({1, 2, 3} if dtype == "f32" else {1})
    assert {c["plan"]["passes"] for c in ew} >= {1, 3} and {c["n"] for c in ew} == {3, 1025, 5123}
    assert all(c["injected"] for c in ew if "xi" in c["offsets"]) and all(c["flag"] and c["r_given"] for c in ew if "r" in c["offsets"])
    assert not [c for c in cases if c["offsets"] and c["plan"]["path"] != "elementwise"]


@pytest.mark.parametrize("kind,dtype", ALL)
def test_grid_capped_cases_loop_and_end_in_a_partly_valid_pass(kind, dtype):
    capped = [c for c in C.cases(kind, dtype) if c["plan"]["path"].startswith("loop")]
    assert len(capped) == 2 * 4 * 3 * 3 * 2 * 2
    for c in capped:
        p = c["plan"]
        assert p["passes"] >= 2 and p["grid"] == c["cfg"]["max_blocks"], c["label"]
        if p["quads"] > 1:
            assert p["last_pass_partial"], c["label"]
    assert {(c["plan"]["block_threads"], c["plan"]["grid"], c["plan"]["quads"]) for c in capped} == {
        (bt, mb, q) for bt in C.BLOCKS for mb in (1, 3) for q in ((1, 2, 4) if dtype == "f32" else (1,))}
    # one quad per lane: 2 P + G + 7 = 3 P + 7 quads take four passes; with 2 or 4 quads per lane they take three
    assert {c["plan"]["passes"] for c in capped} == ({2, 4} if dtype == "f64" else {2, 3, 4})
    assert {c["n"] % 4 for c in capped} == {0, 3}
    single = [c for c in C.cases(kind, dtype) if c["plan"]["path"] == "single"]
    assert all(c["plan"]["passes"] == 1 for c in single)
    assert {c["n"] for c in single} == {1, 2, 3} | {4 * bt + k for bt in C.BLOCKS for k in range(4)} | {4 * (2 * bt + 5) + 2 for bt in C.BLOCKS}


def test_restated_grid_equals_the_library_s_record_count():
    """``sgmcmc_step_stats_records`` and ``sgmcmc_step_stats_records_sized`` are host arithmetic: over the f32 vector cases of the
    table, over a grid of other (n, block_threads, quads, max_blocks), and for f64 (one quad per lane whatever is asked)."""
    from pysgmcmc_amd import _lib
    lib = _lib.lib()

    def records(n, cfg, elem=None):
        s = _lib.LaunchStruct(cfg.get("block_threads", 0), cfg.get("quads_per_thread", 0), cfg.get("max_blocks", 0),
                              cfg.get("nontemporal", -1), None, None)
        if elem is None:
            return lib.sgmcmc_step_stats_records(n, ctypes.byref(s))
        return lib.sgmcmc_step_stats_records_sized(n, elem, ctypes.byref(s))
    seen = 0
    for kind in C.KINDS:
        for dtype, elem in (("f32", 4), ("f64", 8)):
            for c in C.cases(kind, dtype):
                if c["plan"]["path"] != "elementwise":
                    assert records(c["n"], c["cfg"], elem) == c["plan"]["grid"], c["label"]
                    if dtype == "f32":
                        assert records(c["n"], c["cfg"]) == c["plan"]["grid"], c["label"]
                    seen += 1
    assert seen > 1000
    for n in (1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4099, 70_003, 3_000_001, (1 << 28) + 3, 5 * 10 ** 9):
        for bt in C.BLOCKS:
            for q in (0, 1, 2, 4):
                for mb in (0, 1, 2, 7, 40, 1 << 20):
                    cfg = dict(block_threads=bt, quads_per_thread=q, max_blocks=mb)
                    assert records(n, cfg) == C.stats_records(n, "f32", cfg) == C.plan(n, "f32", True, cfg)["grid"]
                    assert records(n, cfg, 4) == records(n, cfg)
                    assert records(n, cfg, 8) == C.stats_records(n, "f64", cfg) == C.plan(n, "f64", True, cfg)["grid"]
                    assert records(n, cfg, 8) == records(n, dict(cfg, quads_per_thread=1))
    # the count of an f64 launch differs from the f32 one as soon as more than one quad per lane is asked for
    cfg = dict(block_threads=128, quads_per_thread=4)
    assert records(70_003, cfg) == 35 and records(70_003, cfg, 8) == 137
    # refusals: no explicit block size, an element size that is no dtype's
    assert records(100, dict(block_threads=-1)) == 0 and b"block_threads must be explicit" in lib.sgmcmc_last_error()
    assert records(100, dict(block_threads=64), 2) == 0 and b"elem_bytes" in lib.sgmcmc_last_error()
    # the element-wise grid counts the ragged tail as a quad of its own: one block more exactly where n / 4 fills the blocks
    assert C.plan(4 * 256 + 1, "f32", False, {})["grid"] == 2 and C.plan(4 * 256 + 1, "f32", True, {})["grid"] == 1


@pytest.mark.parametrize("kind,dtype", ALL)
def test_expected_arrays_are_finite(oracle, kind, dtype):
    """Two consecutive oracle steps of every case (in-register cases: the oracle's own stream) leave finite arrays and positive
    sums; the derived statistics bound of every case is near 5e-7 in f32 and of order 1e-15 in f64."""
    for c in C.cases(kind, dtype):
        st, grads, xis = C.initial_state(c)
        for t in range(2):
            C.oracle_step(oracle, c, st, grads[t], xis[t] if c["injected"] else None, seed=C.SEED, step=t)
            for name, a in st.items():
                assert np.isfinite(a).all(), (c["label"], t, name)
            if kind != "rsghmc":
                assert (st["minv"] > 0).all()
            sums = C.true_sums(c, st)
            assert all(np.isfinite(sums)) and sums[0] > 0
        in_t, in_d, bound = C.stats_bound(c)
        if dtype == "f32":
            assert 10 <= in_t <= 11 and 5.9e-7 < bound < 6.7e-7, (c["label"], in_t, bound)
        else:
            assert 10 <= in_t <= 15 and 1.2e-15 < bound < 3e-15, (c["label"], in_t, in_d, bound)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_large_offset_streams_depend_on_the_high_counter_word(oracle, dtype):
    """The oracle's stream at ``first_element`` differs from its stream at ``first_element mod 2^34`` (what a kernel that drops
    ``gq >> 32`` would draw) wherever the global quad is 2^32 or more -- by far more than the bar the GPU test holds."""
    dt = C.NP[dtype]
    for first, n in C.HIGH_WORD_CASES:
        kept = oracle.c_philox_normal_range(C.HIGH_WORD_SEED, C.HIGH_WORD_STEP, first, n, dt).astype(np.float64)
        past = (first + np.arange(n)) // 4 >= 2 ** 32
        assert past.any() and (first == C.HIGH_WORD_CASES[0][0]) == (not past.all())
        lo = oracle.c_philox_normal_range(C.HIGH_WORD_SEED, C.HIGH_WORD_STEP, first % 2 ** 34, n, dt).astype(np.float64)
        # first mod 2^34 + i wraps past 2^34 in the straddling case: a dropped high word restarts at quad 0 there
        wrap = (first % 2 ** 34 + np.arange(n)) >= 2 ** 34
        if wrap.any():
            k = int(np.argmax(wrap))
            lo[k:] = oracle.c_philox_normal_range(C.HIGH_WORD_SEED, C.HIGH_WORD_STEP, 0, n - k, dt)
        assert np.array_equal(kept[~past], lo[~past])
        diff = np.abs(kept - lo)[past]
        assert np.median(diff) > 0.1 and (diff > 1e-3).mean() > 0.99
        near = C.near_one_mask(oracle, C.HIGH_WORD_SEED, C.HIGH_WORD_STEP, first, n)
        assert near.shape == (n,) and near.sum() <= 2
