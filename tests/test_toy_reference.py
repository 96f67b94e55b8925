"""The host reference of the toy-chains kernel (tests/toy_reference.py) checked against the C oracle and against long
double arithmetic, on the CPU: what tests/test_toy_chains_kernel_gpu.py compares the kernel with must itself be right.
Noise here is the oracle's Philox stream (the GPU tests use the device's K5 stream)."""
import numpy as np
import pytest

import toy_reference as R

DTYPES = [np.float32, np.float64]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["gmm2", "banana"])
def test_relativistic_chain_is_bit_equal_to_the_c_toy_chain(oracle, name, dtype):
    """`chain` (numpy gradient + oracle_rsghmc_step per step) against oracle_rsghmc_toy_chain (gradient and update in
    C): the gradients' op order, the libm exp/log and the kept layout agree bit for bit."""
    target, params = R.BUILTIN[name]
    n, eps, seeds = 3, 0.3, [7, 2 ** 63 + 11, 12345678901]
    state = R.free_state(R.RSGHMC, name, dtype, n)
    kept, final = R.chain(R.RSGHMC, target, params, state, (eps, 1.0, 1.0, 1.0, 0.0), seeds, 11, 200, 0, 7)
    assert kept.shape == (29, n, R.DIM[target])
    for c in range(n):
        th, p = state["theta"][c].copy(), state["mom"][c].copy()
        want = oracle.c_rsghmc_toy_chain(name, th, p, eps, 200, 7, first_step=11, seed=seeds[c])
        assert np.array_equal(kept[:, c, :], want), (name, dtype, c)
        assert np.array_equal(final["theta"][c], th) and np.array_equal(final["mom"][c], p)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cost_grad_stays_within_the_conditioned_bound_of_the_exact_gradient(dtype):
    """Every sweep of the GPU gradient probe: the rounded reference against long double, within
    c eps_T (1 + max|t_i|) sum_i |r_i q_i| (derivation: tests/test_toy_chains_kernel_gpu.py); the banana within its
    own forward bound; k = 1 equals (x - mu) / var to 1 ulp."""
    eps = float(np.finfo(dtype).eps)
    for name, target, params, theta in R.probe_sets(dtype):
        got = R.cost_grad(target, params, theta, dtype).astype(np.float64)
        assert np.isfinite(got).all(), name
        exact, terms = R.cost_grad_exact(target, params, theta, dtype, terms=True)
        err = np.abs(got - exact.astype(np.float64))
        if target == R.BANANA:
            # u: 4 roundings of terms bounded by |y| + 0.1 x^2 + 10; g_x: 2 constants + 4 more roundings
            x, y = theta[:, 0].astype(np.float64), theta[:, 1].astype(np.float64)
            mag = np.abs(y) + 0.1 * x * x + 10.0
            assert (err[:, 1] <= 3 * eps * mag).all(), name
            assert (err[:, 0] <= 6 * eps * (0.01 * np.abs(x) + 0.2 * np.abs(x) * mag)).all(), name
            continue
        bound = R.bound_vs_exact(target, terms, dtype)
        worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
        print("%s %s: worst |cost_grad - exact| / bound = %.3g" % (name, np.dtype(dtype).name, worst))
        assert (err <= bound).all(), (name, worst)
        if name == "k1":
            mu, var = np.asarray(params[:2], np.float64).astype(dtype)
            assert np.array_equal(got[:, 0], ((theta[:, 0] - mu) / var).astype(np.float64))
            assert (err <= eps * np.abs(exact.astype(np.float64))).all()


def test_tie_points_are_ties():
    """the probe's special points: at every tie point two components' terms agree (to the root's rounding)"""
    for name in ("gmm2", "gmm3"):
        params = R.BUILTIN[name][1]
        pts = R.tie_points(params, -40.0, 40.0)
        assert pts.size >= 2
        _, terms = R.cost_grad_exact(R.GMM1D, params, pts.reshape(-1, 1), np.float64, terms=True)
        mu, var, a, b = R.gmm1d_constants(params, np.float64)
        t = (a - b)[None, :] - 0.5 * (pts[:, None] - mu[None, :]) ** 2 / var[None, :]
        gaps = np.abs(t[:, :, None] - t[:, None, :]) + 1e9 * np.eye(3)[None]
        assert (gaps.min(axis=(1, 2)) < 1e-9).all()


@pytest.fixture(scope="module")
def oracle_noise_tables(oracle):
    out = {}
    for dtype in DTYPES:
        steps = range(R.FREE["first_step"], R.FREE["first_step"] + R.FREE["n_steps"])
        xi = np.stack([np.stack([oracle.c_philox_normal(seed, step, 2, dtype) for step in steps]) for seed in R.free_seeds()])
        out[np.dtype(dtype)] = R.NoiseTable(xi, R.FREE["first_step"])
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["gmm1", "gmm2", "gmm3", "banana", "gmm2d"])
@pytest.mark.parametrize("kind", [R.SGHMC, R.SGLD, R.RSGHMC])
def test_twin_spread_of_every_free_running_case_stays_under_its_cap(oracle_noise_tables, kind, name, dtype):
    """The cases of the GPU free-running comparison are not chaotic over their 48 steps: moving every gradient by one
    ulp moves no kept row and no final state array of a chosen chain by more than SPREAD_CAP eps_T max(1, |x|); the
    pool of candidates holds enough tame chains, with room (the GPU test draws the device's noise, not the oracle's)."""
    case = R.free_case(kind, name, dtype, oracle_noise_tables[np.dtype(dtype)])
    print("kind %d %s %s: twin spread %.3g eps; %d of %d candidates above %g eps (worst %.3g)" % (
        kind, name, np.dtype(dtype).name, case["spread"].max(), (case["pool_spread"] > R.FREE_PICK).sum(), R.FREE_POOL,
        R.FREE_PICK, case["pool_spread"].max()))
    assert case["kept"].shape == (16, R.FREE_CHAINS, R.DIM[case["target"]]) and np.isfinite(case["kept"]).all()
    assert all(np.isfinite(v).all() for v in case["final"].values())
    assert case["spread"].max() <= R.SPREAD_CAP
    assert (case["pool_spread"] <= R.FREE_PICK).sum() >= R.FREE_CHAINS + 20
    # a twin is a perturbation: the spread is not identically zero
    assert case["spread"].max() > 0
