"""``sgmcmc_toy_chains_f32/_f64`` (pysgmcmc_amd/csrc/sgmcmc_toy.hip, the kernel behind ``BuiltinTargetChains``) against
tests/toy_reference.py, through ``kernels.toy_chains``, in both dtypes. tests/test_toy_reference.py validates that
reference on the CPU (bit-equal to the oracle's C toy chain, within its bound of long double arithmetic).

(a) GRADIENT PROBE. One relativistic step with scalars (eps, mass, c, D, b_hat) = (1, 1, 1, 0, 0) from p = 0 leaves
    p' = -grad_cost(theta) exactly: the noise scale is sqrt(1 (0 - 0)) = 0, the friction term 0 pg = 0 and 0 + g adds no
    rounding. One launch of 4099 chains (65 blocks, the last ragged) reads the kernel's gradient at 4099 points.

    * banana: no transcendental, contraction off -> BIT-EQUAL to ``cost_grad``.
    * mixtures, against ``cost_grad`` (same program, same inputs; only the device's double ``exp`` may differ from libm's,
      by <= 1 ulp of double, which after the rounding to T moves an ``e_i = (T)exp(t_i - max)`` by at most one ulp of T,
      relative eps_T). To first order, with r_i = e_i / s the responsibilities and q_i the component's own gradient
      ((x - mu_i) / var_i, or x - c_i), the gradient g = sum_i r_i q_i moves by
          sum_i |r_i q_i| x ( eps_T        the change of e_i itself
                            + eps_T        the change of s = sum_j e_j, a weighted mean of the changes of the e_j
                            + eps_T        the division e_i / s rounding differently on the changed operands
                            + eps_T        the product r_i q_i likewise
                            + k eps_T )    the k - 1 additions of s and the k - 1 of g, half an ulp (eps_T / 2) each
      = (k + 4) eps_T sum_i |r_i q_i|. (Were every rounding of both evaluations to flip adversarially the additions
      would count a full ulp each, (2 k + 2) eps_T; the bar is the tighter (k + 4).) Where an e_i is subnormal in T its
      error is absolute, one subnormal spacing; that adds 2 tiny_T sum_i (1 + |q_i|) (``toy_reference._floor``).
    * mixtures, against ``cost_grad_exact`` (long double): the bound also carries the rounding of t_i BEFORE the exp,
      which the exp turns into a relative error of e_i. With u = eps_T / 2 per operation:
        1-D: t_i = (a_i - b_i) - (0.5 d^2) / var_i, d = x - mu_i. Rounded constants a_i, b_i (log in double, then to T):
        2u (|a_i| + |b_i|); a_i - b_i: u |a_i - b_i|; Q_i = 0.5 d^2 / var_i carries 4 roundings (d, d d, the product
        with 0.5 is exact, / var): 4u Q_i; the outer subtraction u |t_i|. With K = max_i (|a_i| + |b_i|), |a_i - b_i| <= K
        and Q_i <= |t_i| + K: |dt_i| <= u (5 |t_i| + 7 K). Then t_i - max rounds (u 2 max|t|) and the exp and its
        rounding to T add eps_T: e_i is off by eta <= eps_T (6 max|t| + 7 K + 1), which moves g by 2 eta sum|r_i q_i|
        (directly and through s). The remaining roundings (q_i: 2, s: k - 1, division, product, g: k - 1) add
        (k + 1) eps_T. Total <= eps_T sum|r_i q_i| (k + 3 + 14 K + 12 max|t|) <= c eps_T (1 + max|t|) sum|r_i q_i| with
        c = k + 15 + 14 K.
        2-D: t_i = -0.5 (dx^2 + dy^2): 4 roundings, |dt_i| <= 4u |t_i|; eta <= eps_T (5 max|t| + 1); the remaining
        roundings (k + 1) eps_T; total <= eps_T sum|r_i q_i| (k + 3 + 10 max|t|), c = k + 13.
    * k = 1: e = s = r = 1 exactly, so g is the twice-rounded (x - mu) / var itself: bit-equal to it, within eps_T of exact.
    Measured on an MI355X (reported by the test, not asserted): the kernel's gradient is bit-equal to ``cost_grad`` at
    100 % of the probed mixture values in f32 (36 891 of 36 891: a 1-ulp difference of the double exp never survived the
    rounding to f32) and at 99.57 % in f64 (36 733 of 36 891; per sweep 98.63 % ... 100 %); where it differs, by at most
    0.17 of the (k + 4) bound. Against long double the kernel sits where ``cost_grad`` does (<= 0.02 of that bound).

(b) ONE STEP FROM ARBITRARY STATE, bit-equal: the oracle's step fed the gradient the probe read at the same theta and the K5
    noise (``kernels.philox_normal``; tests/test_hip_parity.py shows the in-register draw equals it). Pins the operator
    wiring and ``A.s[0..4]``, the second copy of the scalar blocks of sgmcmc_sghmc/sgld/rsghmc.hip, at scalars that are
    neither defaults nor representable.

(c) SHORT FREE-RUNNING CHAINS against ``toy_reference.chain`` with K5 noise. Tolerance from the reference alone: 4 x the
    largest spread of 8 twins whose every gradient is moved one ulp, plus 2 ulp of max(1, |x|) (``toy_reference.allowance``).

(d) EXACT INVARIANTS, no tolerance: partitions of a run, independence of chains, the kept layout, 64-bit step indices;
    perpetual adaptation and ``BuiltinTargetChains`` interleaved with ``next`` under (c)'s tolerance.

(e) REFUSALS of the C ABI and of the Python wrapper.
"""
import ctypes

import numpy as np
import pytest
import torch

import toy_reference as R

pytestmark = pytest.mark.gpu

NPDT = [np.float32, np.float64]
TH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
ROW_ARG = ("theta", "mom", "tau", "g", "v_hat", "minv")


def _dev(a, gpu):
    return torch.from_numpy(np.array(a, order="C")).to(gpu)         # a copy: the launch never writes into the caller's array


def _seed_tensor(seeds, gpu):
    """Philox keys are unsigned 64-bit; the device array is int64 (same bits)."""
    return torch.tensor([int(s) - (1 << 64) if int(s) >= (1 << 63) else int(s) for s in seeds], dtype=torch.int64, device=gpu)


def _launch(gpu, kind, target, params, state, scalars, seeds, first_step, n_steps, burn_in_steps, keep_every=1, keep=True):
    """One launch from the numpy ``state``; rows the sampler does not own are passed as None. Returns numpy
    ``(kept or None, final state)``."""
    from pysgmcmc_amd import kernels
    dev = {name: _dev(state[name], gpu) for name in R.STATE_ROWS[kind]}
    n, dim = state["theta"].shape
    kept = None
    if keep:
        kept = torch.full(((n_steps + keep_every - 1) // keep_every, n, dim), float("nan"), dtype=dev["theta"].dtype, device=gpu)
    kernels.toy_chains(kind, target, params, *[dev.get(name) for name in ROW_ARG], scalars, _seed_tensor(seeds, gpu),
                       first_step, n_steps, burn_in_steps, keep_every, kept)
    return (None if kept is None else kept.cpu().numpy()), {name: t.cpu().numpy() for name, t in dev.items()}


def _probe(gpu, target, params, theta):
    """The kernel's own d cost / d theta at every row of ``theta`` (see (a))."""
    theta = np.ascontiguousarray(theta)
    state = {"theta": theta, "mom": np.zeros_like(theta)}
    _, final = _launch(gpu, R.RSGHMC, target, params, state, (1.0, 1.0, 1.0, 0.0, 0.0), [0] * theta.shape[0], 0, 1, 0, keep=False)
    return -final["mom"]


def _k5_table(gpu, seeds, first_step, n_steps, dtype):
    """NoiseTable of the device's K5 stream: xi(seed_c, step, 0..1) for every chain and step."""
    from pysgmcmc_amd import kernels
    out = torch.empty(len(seeds), n_steps, 2, dtype=TH[np.dtype(dtype)], device=gpu)
    for c, seed in enumerate(seeds):
        for s in range(n_steps):
            kernels.philox_normal(out[c, s], int(seed), first_step + s)
    return R.NoiseTable(out.cpu().numpy(), first_step)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want, equal_nan=True):
        bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError("%s: %d of %d elements differ, first at %s: kernel %r reference %r" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- (a) ---------------------------------------------------------------------------------------------------------------

PROBE_NAMES = [name for name, _, _, _ in R.probe_sets(np.float64)]


@pytest.mark.parametrize("dtype", NPDT)
@pytest.mark.parametrize("sweep", PROBE_NAMES)
def test_gradient_probe(gpu, sweep, dtype):
    name, target, params, theta = [s for s in R.probe_sets(dtype) if s[0] == sweep][0]
    assert theta.shape == (R.N_PROBE, R.DIM[target])
    got = _probe(gpu, target, params, theta)
    want = R.cost_grad(target, params, theta, dtype)
    assert np.isfinite(got).all() and np.isfinite(want).all()        # no point is skipped: every theta has a finite t_i
    if target == R.BANANA:
        _same(got, want, "banana gradient")
        return
    exact, terms = R.cost_grad_exact(target, params, theta, dtype, terms=True)
    equal = got == want
    d_ref = np.abs(got.astype(np.float64) - want.astype(np.float64))
    d_exact = np.abs(got.astype(np.float64) - exact.astype(np.float64))
    b_ref, b_exact = R.bound_vs_cost_grad(terms, dtype), R.bound_vs_exact(target, terms, dtype)
    tiny = np.finfo(np.float64).tiny
    print("%s %s: bit-equal to cost_grad at %d of %d values (%.4f %%); worst |d| / bound: %.3g vs cost_grad, %.3g vs exact" % (
        name, np.dtype(dtype).name, equal.sum(), equal.size, 100.0 * equal.mean(),
        np.max(d_ref / np.maximum(b_ref, tiny)), np.max(d_exact / np.maximum(b_exact, tiny))))
    assert (d_ref <= b_ref).all(), (name, np.max(d_ref / np.maximum(b_ref, tiny)))
    assert (d_exact <= b_exact).all(), (name, np.max(d_exact / np.maximum(b_exact, tiny)))
    if name == "k1":
        mu, var = np.asarray(params[:2], np.float64).astype(dtype)
        _same(got[:, 0], (theta[:, 0] - mu) / var, "k = 1 gradient")
        assert (d_exact <= float(np.finfo(dtype).eps) * np.abs(exact.astype(np.float64))).all()


# ---- (b) ---------------------------------------------------------------------------------------------------------------

ONE_STEP = [
    ("sghmc-adapt", R.SGHMC, True, (0.013, 7.0, 0.03)), ("sghmc-frozen", R.SGHMC, False, (0.013, 7.0, 0.03)),
    ("sgld-adapt", R.SGLD, True, (0.013, 0.7, 7.0)), ("sgld-frozen", R.SGLD, False, (0.013, 0.7, 7.0)),
    ("sgld-adapt-negative-scale", R.SGLD, True, (0.013, 0.7, -7.0)),
    ("sgld-frozen-negative-scale", R.SGLD, False, (0.013, 0.7, -7.0)),
    ("relativistic", R.RSGHMC, True, (0.013, 1.3, 0.7, 0.9, 0.1)), ("relativistic-m-c-1", R.RSGHMC, True, (0.013, 1.0, 1.0, 0.9, 0.1)),
]


def _arbitrary_state(kind, target, dtype, n, rng):
    dim = R.DIM[target]
    st = {"theta": (3.0 * rng.normal(size=(n, dim))).astype(dtype), "mom": rng.normal(size=(n, dim)).astype(dtype),
          "tau": rng.uniform(0.5, 3.0, size=(n, dim)).astype(dtype), "g": rng.normal(size=(n, dim)).astype(dtype),
          "v_hat": rng.uniform(0.1, 2.0, size=(n, dim)).astype(dtype), "minv": rng.uniform(0.5, 2.0, size=(n, dim)).astype(dtype)}
    st["v_hat"][0:8], st["v_hat"][8:12], st["v_hat"][12:16] = 0.0, -1e-16, 1e-30      # as test_edge_cases_bit_exact
    st["g"][4:10] = 0.0
    return {name: st[name] for name in R.STATE_ROWS[kind]}


@pytest.mark.parametrize("dtype", NPDT)
@pytest.mark.parametrize("label,kind,adapt,scalars", ONE_STEP, ids=[c[0] for c in ONE_STEP])
def test_one_step_from_arbitrary_state_is_bit_equal(gpu, label, kind, adapt, scalars, dtype):
    n, step = 130, 12345
    rng = np.random.default_rng(77)
    seeds = [(1 << 63) + 5 + c for c in range(4)] + [(1 << 64) - 1] + [int(v) for v in rng.integers(0, 1 << 62, size=n - 5)]
    noise = _k5_table(gpu, seeds, step, 1, dtype)
    for name in ("gmm2", "banana", "gmm2d"):
        target, params = R.BUILTIN[name]
        state = _arbitrary_state(kind, target, dtype, n, rng)
        grad = _probe(gpu, target, params, state["theta"])
        burn_in = step + 1 if adapt else step          # step < burn_in_steps adapts; both are > 0 (not perpetual)
        _, want = R.chain(kind, target, params, state, scalars, seeds, step, 1, burn_in, 1, noise=noise, grad_fn=lambda th: grad)
        kept, got = _launch(gpu, kind, target, params, state, scalars, seeds, step, 1, burn_in)
        for row in R.STATE_ROWS[kind]:
            _same(got[row], want[row], "%s %s %s" % (label, name, row))
        _same(kept[0], want["theta"], "%s %s kept" % (label, name))
        assert np.isfinite(got["theta"]).all()
        if kind != R.RSGHMC and not adapt:
            for row in ("tau", "g", "v_hat", "minv"):
                _same(got[row], state[row], "frozen step left %s alone" % row)


# ---- (c) ---------------------------------------------------------------------------------------------------------------

class _FreeCases(object):
    """The reference runs of the free-running cases, each computed once (K5 noise of the candidate pool per dtype)."""

    def __init__(self, gpu):
        self.gpu, self.noise, self.cases = gpu, {}, {}

    def pool_noise(self, dtype, first_step=R.FREE["first_step"]):
        key = (np.dtype(dtype), first_step)
        if key not in self.noise:
            self.noise[key] = _k5_table(self.gpu, R.free_seeds(), first_step, R.FREE["n_steps"], dtype)
        return self.noise[key]

    def get(self, kind, name, dtype, **overrides):
        key = (kind, name, np.dtype(dtype), tuple(sorted(overrides.items())))
        if key not in self.cases:
            noise = self.pool_noise(dtype, overrides.get("first_step", R.FREE["first_step"]))
            self.cases[key] = R.free_case(kind, name, dtype, noise, **overrides)
            assert self.cases[key]["spread"].max() <= R.SPREAD_CAP
        return self.cases[key]


@pytest.fixture(scope="module")
def free_cases(gpu):
    return _FreeCases(gpu)


def _first(case, n):
    return {k: v[:n] for k, v in case["state"].items()}


def _assert_within(got_kept, got_final, case, n, what):
    spread = case["spread"][:n].max()
    worst = R.within(got_kept, case["kept"][:, :n], spread)
    for row, v in got_final.items():
        worst = max(worst, R.within(v, case["final"][row][:n], spread))
    print("%s: twin spread %.3g eps, worst |kernel - reference| / allowance %.3g" % (what, spread, worst))
    assert worst <= 1.0, (what, spread, worst)


@pytest.mark.parametrize("dtype", NPDT)
@pytest.mark.parametrize("n_chains", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name", ["gmm1", "gmm2", "gmm3", "banana", "gmm2d"])
@pytest.mark.parametrize("kind", [R.SGHMC, R.SGLD, R.RSGHMC])
def test_short_free_running_chains(gpu, free_cases, kind, name, n_chains, dtype):
    case = free_cases.get(kind, name, dtype)
    kept, final = _launch(gpu, kind, case["target"], case["params"], _first(case, n_chains), case["scalars"],
                          case["seeds"][:n_chains], **R.FREE)
    assert kept.shape == (16, n_chains, R.DIM[case["target"]])
    _assert_within(kept, final, case, n_chains, "kind %d %s x%d %s" % (kind, name, n_chains, np.dtype(dtype).name))
    if case["target"] == R.BANANA:      # no transcendental anywhere: the whole run is bit-equal
        _same(kept, case["kept"][:, :n_chains], "banana kept")
        for row in final:
            _same(final[row], case["final"][row][:n_chains], "banana " + row)


# ---- (d) ---------------------------------------------------------------------------------------------------------------

def _run_parts(gpu, kind, case, parts, burn_in_steps, first_step=0):
    state, rows = case["state"], []
    for n in parts:
        kept, state = _launch(gpu, kind, case["target"], case["params"], state, case["scalars"], case["seeds"], first_step,
                              n, burn_in_steps)
        rows.append(kept)
        first_step += n
    return np.concatenate(rows), state


@pytest.mark.parametrize("dtype", NPDT)
@pytest.mark.parametrize("kind", [R.SGHMC, R.SGLD, R.RSGHMC])
def test_partitions_of_a_run_are_bit_equal(gpu, free_cases, kind, dtype):
    """48 steps in one launch == (1, 6, 13, 1, 27) (the burn-in boundary, step 20, on a launch edge) == (5, 43) (inside)."""
    for name in ("gmm3", "gmm2d"):
        case = free_cases.get(kind, name, dtype)
        whole_kept, whole = _run_parts(gpu, kind, case, (48,), 20)
        assert whole_kept.shape[0] == 48 and np.isfinite(whole_kept).all()
        for parts in ((1, 6, 13, 1, 27), (5, 43)):
            kept, final = _run_parts(gpu, kind, case, parts, 20)
            _same(kept, whole_kept, "%s %r kept" % (name, parts))
            for row in final:
                _same(final[row], whole[row], "%s %r %s" % (name, parts, row))


@pytest.mark.parametrize("dtype", NPDT)
@pytest.mark.parametrize("kind", [R.SGHMC, R.SGLD, R.RSGHMC])
def test_chains_are_independent_of_their_neighbours_and_index(gpu, free_cases, kind, dtype):
    for name in ("gmm2", "banana"):
        case = free_cases.get(kind, name, dtype)
        kept, final = _launch(gpu, kind, case["target"], case["params"], case["state"], case["scalars"], case["seeds"], **R.FREE)
        for c in (0, 63, 64, 129):
            k1, f1 = _launch(gpu, kind, case["target"], case["params"], {k: v[c:c + 1] for k, v in case["state"].items()},
                             case["scalars"], case["seeds"][c:c + 1], **R.FREE)
            _same(k1[:, 0], kept[:, c], "%s chain %d alone" % (name, c))
            for row in final:
                _same(f1[row][0], final[row][c], "%s chain %d alone %s" % (name, c, row))
        perm = np.random.default_rng(3).permutation(R.FREE_CHAINS)
        assert (perm != np.arange(R.FREE_CHAINS)).sum() > 100
        k2, f2 = _launch(gpu, kind, case["target"], case["params"], {k: v[perm] for k, v in case["state"].items()},
                         case["scalars"], [case["seeds"][i] for i in perm], **R.FREE)
        _same(k2, kept[:, perm], name + " permuted kept")
        for row in final:
            _same(f2[row], final[row][perm], "%s permuted %s" % (name, row))


@pytest.mark.parametrize("dtype", NPDT)
@pytest.mark.parametrize("kind", [R.SGHMC, R.SGLD, R.RSGHMC])
def test_kept_layout_and_untouched_neighbours(gpu, free_cases, kind, dtype):
    """kept[j] = theta after step j * keep_every of the launch, ceil(n / k) rows, [kept][chain][dim]; the element after
    every array and the row after ``kept`` keep their sentinel; ``kept=None`` changes nothing else."""
    from pysgmcmc_amd import kernels
    case = free_cases.get(kind, "gmm2d", dtype)
    n, dim, thdt = R.FREE_CHAINS, 2, TH[np.dtype(dtype)]
    trace, _ = _run_parts(gpu, kind, case, (50,), 20)                  # the state after every step
    seeds = _seed_tensor(case["seeds"], gpu)
    sentinel = -12345.0
    for n_steps, every in ((50, 7), (3, 7), (48, 1), (49, 48)):
        rows = (n_steps + every - 1) // every
        finals = []
        for keep in (True, False):
            bufs = {name: torch.full((n * dim + 8,), sentinel, dtype=thdt, device=gpu) for name in R.STATE_ROWS[kind]}
            dev = {name: b[:n * dim].view(n, dim) for name, b in bufs.items()}
            for name in dev:
                dev[name].copy_(_dev(case["state"][name], gpu))
            kbuf = torch.full(((rows + 1) * n * dim,), sentinel, dtype=thdt, device=gpu)
            kept = kbuf[:rows * n * dim].view(rows, n, dim) if keep else None
            kernels.toy_chains(kind, case["target"], case["params"], *[dev.get(name) for name in ROW_ARG], case["scalars"],
                               seeds, 0, n_steps, 20, every, kept)
            for name, b in bufs.items():
                assert (b[n * dim:] == sentinel).all(), (name, n_steps, every)
            assert (kbuf[rows * n * dim:] == sentinel).all(), (n_steps, every)
            if keep:
                _same(kept.cpu().numpy(), trace[0:n_steps:every], "kept rows of (%d, %d)" % (n_steps, every))
                assert kept.shape[0] == len(range(0, n_steps, every)) == rows
                if (n_steps - 1) % every == 0:
                    assert torch.equal(kept[-1], dev["theta"])
            else:
                assert (kbuf == sentinel).all()
            _same(dev["theta"].cpu().numpy(), trace[n_steps - 1], "final theta of (%d, %d)" % (n_steps, every))
            finals.append({name: t.cpu().numpy() for name, t in dev.items()})
        for name in finals[0]:
            _same(finals[1][name], finals[0][name], "kept=None %s" % name)


@pytest.mark.parametrize("dtype", NPDT)
@pytest.mark.parametrize("kind", [R.SGHMC, R.SGLD, R.RSGHMC])
def test_step_indices_beyond_32_bits(gpu, kind, dtype):
    """first_step = 2^32 - 3, 8 steps, burn-in 2^32 + 1, on the banana (bit-equal: no transcendental): the noise is the K5
    stream at those 64-bit steps and adaptation stops exactly at step 2^32 + 1 (4 adapting steps, 4 frozen)."""
    first, burn_in, n = (1 << 32) - 3, (1 << 32) + 1, 65
    target, params = R.BUILTIN["banana"]
    state = {k: v[:n] for k, v in R.free_state(kind, "banana", dtype).items()}
    seeds = [(1 << 63) + 17 * c for c in range(n)]
    noise = _k5_table(gpu, seeds, first, 8, dtype)
    scalars = R.FREE_SCALARS[kind]
    want_kept, want = R.chain(kind, target, params, state, scalars, seeds, first, 8, burn_in, 1, noise=noise)
    kept, got = _launch(gpu, kind, target, params, state, scalars, seeds, first, 8, burn_in)
    _same(kept, want_kept, "kept")
    for row in got:
        _same(got[row], want[row], row)
    if kind != R.RSGHMC:
        # the comparison can tell: one adapting step more or less, or the noise of the low word alone, is another chain
        for other in (burn_in - 1, burn_in + 1):
            _, off = R.chain(kind, target, params, state, scalars, seeds, first, 8, other, 1, noise=noise)
            assert not np.array_equal(off["tau"], want["tau"]) and not np.array_equal(off["theta"], want["theta"])
    low = _k5_table(gpu, seeds[:2], 0, 1, dtype)                  # step 2^32 with its high word dropped
    assert not np.array_equal(low.xi[:, 0], noise.xi[:2, 3])


@pytest.mark.parametrize("dtype", NPDT)
@pytest.mark.parametrize("burn_in_steps", [0, -5])
@pytest.mark.parametrize("kind", [R.SGHMC, R.SGLD])
def test_perpetual_adaptation(gpu, free_cases, kind, burn_in_steps, dtype):
    """burn_in_steps <= 0: every step adapts (reference quirk Q4). The mixtures under (c)'s tolerance; the banana, which
    has no transcendental, bit for bit."""
    run = dict(R.FREE, burn_in_steps=burn_in_steps)
    for name in ("gmm1", "gmm2"):
        case = free_cases.get(kind, name, dtype, burn_in_steps=burn_in_steps)
        kept, final = _launch(gpu, kind, case["target"], case["params"], case["state"], case["scalars"], case["seeds"], **run)
        _assert_within(kept, final, case, R.FREE_CHAINS, "perpetual kind %d %s %d" % (kind, name, burn_in_steps))
        assert (case["final"]["tau"] != 1).all()         # the reference adapted
    target, params = R.BUILTIN["banana"]
    n = R.FREE_CHAINS
    state = {k: v[:n] for k, v in R.free_state(kind, "banana", dtype).items()}
    seeds, scalars = R.free_seeds()[:n], R.FREE_SCALARS[kind]
    want_kept, want = R.chain(kind, target, params, state, scalars, seeds, noise=free_cases.pool_noise(dtype), **run)
    kept, final = _launch(gpu, kind, target, params, state, scalars, seeds, **run)
    _same(kept, want_kept, "banana kept")
    for row in final:
        _same(final[row], want[row], "banana " + row)


@pytest.mark.parametrize("sampler", ["sghmc", "sgld"])
def test_builtin_target_chains_interleaved_with_next(gpu, sampler):
    """f32: 7 x next, run(9), 3 x next, run(30), 2 x next across a burn-in of 20, with the sampler's default
    store_minv_every_step: every state after every step, and every row of the arena at the end, against the reference
    with K5 noise under (c)'s tolerance (``next`` differentiates the cost by autograd, the launch analytically)."""
    from pysgmcmc_amd.diagnostics.objective_functions import gmm2_log_likelihood, to_negative_log_likelihood
    from pysgmcmc_amd.samplers import SGHMCSampler, SGLDSampler
    from pysgmcmc_amd.samplers.builtin_target_chains import BuiltinTargetChains
    from pysgmcmc_amd.stepsize_schedules import ConstantStepsizeSchedule
    ctor, kind = (SGHMCSampler, R.SGHMC) if sampler == "sghmc" else (SGLDSampler, R.SGLD)
    target, params = R.BUILTIN["gmm2"]
    pool, n = 24, 8

    def make(c):
        s = ctor(params=[torch.tensor(0.4 + c / 128.0, dtype=torch.float32, device=gpu)],
                 cost_fun=to_negative_log_likelihood(gmm2_log_likelihood), stepsize_schedule=ConstantStepsizeSchedule(0.05),
                 burn_in_steps=20, session=gpu, dtype=torch.float32, seed=100 + c)
        s.sample_format = "view"
        return s

    cands = [make(c) for c in range(pool)]
    assert cands[0].store_minv_every_step
    names = {"theta": "theta", "mom": "V", "tau": "tau", "g": "g", "v_hat": "v_hat", "minv": "minv"}
    state = {row: np.stack([s.arena.row(names[row]).cpu().numpy() for s in cands]) for row in R.STATE_ROWS[kind]}
    seeds = [s._philox_seed for s in cands]
    scalars = tuple(float(v) for v in cands[0]._step_scalars(0.05))
    noise = _k5_table(gpu, seeds, 0, 51, np.float32)
    want_kept, want, spread = R.twin_spread(kind, target, params, state, scalars, seeds, 0, 51, 20, 1, noise=noise)
    sel = [int(i) for i in np.flatnonzero(spread <= R.FREE_PICK)[:n]]
    assert len(sel) == n
    chosen = [cands[i] for i in sel]
    chains = BuiltinTargetChains(chosen)
    rows = []

    def step_all(k):
        for _ in range(k):
            for s in chosen:
                next(s)
            rows.append(torch.stack([s.arena.row("theta").clone() for s in chosen]))

    step_all(7)
    rows.extend(chains.run(9))
    step_all(3)
    rows.extend(chains.run(30))
    step_all(2)
    assert all(s.n_iterations == 51 for s in chosen) and not chosen[0]._adapting
    got_kept = torch.stack(rows).cpu().numpy()
    assert got_kept.shape == (51, n, 1)
    got = {row: np.stack([s.arena.row(names[row]).cpu().numpy() for s in chosen]) for row in R.STATE_ROWS[kind]}
    case = {"kept": want_kept[:, sel], "final": {k: v[sel] for k, v in want.items()}, "spread": spread[sel]}
    _assert_within(got_kept, got, case, n, "BuiltinTargetChains interleaved " + sampler)


# ---- (e) ---------------------------------------------------------------------------------------------------------------

def _abi_args(gpu, thdt, kind=R.SGHMC, target=R.GMM1D, n=5):
    dim = R.DIM[target]
    tens = {name: torch.full((n, dim), 0.25 * (i + 1), dtype=thdt, device=gpu) for i, name in enumerate(ROW_ARG)}
    tens["seeds"] = torch.arange(n, dtype=torch.int64, device=gpu)
    tens["kept"] = torch.full((4, n, dim), 7.0, dtype=thdt, device=gpu)
    tp = {R.GMM1D: R.BUILTIN["gmm2"][1], R.BANANA: [0.0], R.GMM2D: R.BUILTIN["gmm2d"][1]}[target]
    args = dict(sampler=kind, target=target, tp=(ctypes.c_double * len(tp))(*tp), k=0 if target == R.BANANA else 3,
                theta=tens["theta"].data_ptr(), mom=tens["mom"].data_ptr(), tau=tens["tau"].data_ptr(), g=tens["g"].data_ptr(),
                v_hat=tens["v_hat"].data_ptr(), minv=tens["minv"].data_ptr(), n_chains=n, dim=dim,
                scalars=(ctypes.c_double * 5)(0.05, 1.0, 0.05, 1.0, 0.0), seeds=tens["seeds"].data_ptr(), first_step=0, n_steps=4,
                burn_in_steps=2, keep_every=1, kept=tens["kept"].data_ptr(), stream=None)
    return args, tens


ABI_ORDER = ("sampler", "target", "tp", "k", "theta", "mom", "tau", "g", "v_hat", "minv", "n_chains", "dim", "scalars", "seeds",
             "first_step", "n_steps", "burn_in_steps", "keep_every", "kept", "stream")

REFUSALS = [
    ("sampler -1", {}, dict(sampler=-1), "sampler"), ("sampler 3", {}, dict(sampler=3), "sampler"),
    ("target -1", {}, dict(target=-1), "target"), ("target 3", {}, dict(target=3, dim=2), "target"),
    ("dim 2 for the 1-D mixture", {}, dict(dim=2), "dim"),
    ("dim 1 for the banana", dict(target=R.BANANA), dict(dim=1), "dim"),
    ("dim 1 for the 2-D mixture", dict(target=R.GMM2D), dict(dim=1), "dim"),
    ("k 0", {}, dict(k=0), "components"), ("k 17", {}, dict(k=17), "components"),
    ("k 0, 2-D", dict(target=R.GMM2D), dict(k=0), "components"), ("k 17, 2-D", dict(target=R.GMM2D), dict(k=17), "components"),
    ("NULL target_params", {}, dict(tp=None), "target_params"),
    ("NULL target_params, 2-D", dict(target=R.GMM2D), dict(tp=None), "target_params"),
    ("keep_every 0", {}, dict(keep_every=0), "keep_every"),
    ("NULL theta", {}, dict(theta=None), "theta"), ("NULL seeds", {}, dict(seeds=None), "seeds"),
    ("NULL scalars", {}, dict(scalars=None), "scalars"),
    ("NULL mom, SGHMC", {}, dict(mom=None), "mom"), ("NULL mom, relativistic", dict(kind=R.RSGHMC), dict(mom=None), "mom"),
] + [("NULL %s, %s" % (row, "SGLD" if kind == R.SGLD else "SGHMC"), dict(kind=kind), {row: None}, row)
     for kind in (R.SGHMC, R.SGLD) for row in ("tau", "g", "v_hat", "minv")]


@pytest.mark.parametrize("dtype", NPDT)
def test_c_abi_refusals_name_the_cause_and_touch_nothing(gpu, dtype):
    from pysgmcmc_amd._lib import lib
    thdt = TH[np.dtype(dtype)]
    f = getattr(lib(), "sgmcmc_toy_chains_" + ("f32" if dtype is np.float32 else "f64"))
    for label, setup, change, word in REFUSALS:
        args, tens = _abi_args(gpu, thdt, **setup)
        before = {k: v.clone() for k, v in tens.items()}
        args.update(change)
        rc = f(*[args[k] for k in ABI_ORDER])
        torch.cuda.synchronize()
        message = (lib().sgmcmc_last_error() or b"").decode()
        assert rc != 0, label
        assert "toy_chains" in message and word in message, (label, message)
        for k in tens:
            assert torch.equal(tens[k], before[k]), (label, k)
    for change in (dict(n_chains=0), dict(n_steps=0), dict(n_steps=0, sampler=7, theta=None)):      # nothing to do: 0
        args, tens = _abi_args(gpu, thdt)
        before = {k: v.clone() for k, v in tens.items()}
        args.update(change)
        assert f(*[args[k] for k in ABI_ORDER]) == 0, change
        torch.cuda.synchronize()
        for k in tens:
            assert torch.equal(tens[k], before[k]), (change, k)
    # lone rows the sampler does not own may be NULL: the launch still runs
    args, tens = _abi_args(gpu, thdt, kind=R.SGLD)
    args.update(mom=None)
    assert f(*[args[k] for k in ABI_ORDER]) == 0
    args, tens = _abi_args(gpu, thdt, kind=R.RSGHMC)
    args.update(tau=None, g=None, v_hat=None, minv=None, scalars=(ctypes.c_double * 5)(0.05, 1.0, 1.0, 1.0, 0.0))
    assert f(*[args[k] for k in ABI_ORDER]) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(tens["theta"]).all() and not (tens["kept"] == 7.0).any()


@pytest.mark.parametrize("dtype", NPDT)
def test_python_wrapper_refusals(gpu, dtype):
    from pysgmcmc_amd import kernels
    from pysgmcmc_amd._lib import SgmcmcLibraryError
    thdt = TH[np.dtype(dtype)]
    other = torch.float64 if thdt is torch.float32 else torch.float32
    n = 5
    params = R.BUILTIN["gmm2"][1]

    def call(seeds=None, kept=None, target=R.GMM1D, kind=R.SGHMC, keep_every=2, dim=1, params=params, n_steps=4, drop=()):
        rows = {name: torch.full((n, dim), 0.5, dtype=thdt, device=gpu) for name in ROW_ARG}
        before = {k: v.clone() for k, v in rows.items()}
        seeds = torch.arange(n, dtype=torch.int64, device=gpu) if seeds is None else seeds
        try:
            kernels.toy_chains(kind, target, params, *[None if name in drop else rows[name] for name in ROW_ARG],
                               (0.05, 1.0, 0.05), seeds, 0, n_steps, 2, keep_every, kept)
        finally:
            torch.cuda.synchronize()
            for k in rows:
                assert torch.equal(rows[k], before[k]), k

    with pytest.raises(TypeError, match="int64"):
        call(seeds=torch.arange(n, dtype=torch.int32, device=gpu))
    with pytest.raises(TypeError, match="one entry per chain"):
        call(seeds=torch.arange(n + 1, dtype=torch.int64, device=gpu))
    with pytest.raises(ValueError, match="kept"):
        call(kept=torch.zeros(3, n, 1, dtype=thdt, device=gpu))               # 2 rows wanted
    with pytest.raises(ValueError, match="kept"):
        call(kept=torch.zeros(2, n, 1, dtype=other, device=gpu))
    with pytest.raises(ValueError, match="keep_every"):
        call(keep_every=0)
    with pytest.raises(ValueError, match="unsigned"):
        call(n_steps=-1)
    for kwargs, word in ((dict(kind=3), "sampler"), (dict(kind=-1), "sampler"), (dict(target=3, dim=2), "target"),
                         (dict(target=-1), "target"), (dict(dim=2), "dim"), (dict(target=R.BANANA, params=[]), "dim"),
                         (dict(target=R.GMM2D, params=R.BUILTIN["gmm2d"][1]), "dim"), (dict(params=[]), "components"),
                         (dict(params=[0.0, 1.0, 1.0] * 17), "components"),
                         (dict(target=R.GMM2D, dim=2, params=[0.0] * 34), "components"),
                         (dict(drop=("mom",)), "mom"), (dict(drop=("tau",)), "tau"), (dict(kind=R.SGLD, drop=("minv",)), "minv")):
        with pytest.raises(SgmcmcLibraryError, match=word):
            call(**kwargs)
    # nothing to do
    rows = [torch.full((n, 1), 0.5, dtype=thdt, device=gpu) for _ in ROW_ARG]
    assert kernels.toy_chains(R.SGHMC, R.GMM1D, params, *rows, (0.05, 1.0, 0.05), torch.arange(n, dtype=torch.int64, device=gpu),
                              0, 0, 2) is None
    torch.cuda.synchronize()
    assert all((r == 0.5).all() for r in rows)
