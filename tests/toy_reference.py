"""Host reference of the many-chains toy-target kernel (``sgmcmc_toy_chains_*``, pysgmcmc_amd/csrc/sgmcmc_toy.hip):
plain numpy for the analytic gradients, the C oracle for the update operators. TEST INFRASTRUCTURE ONLY.

* :func:`cost_grad` restates the kernel's three gradients one IEEE rounding at a time in the kernel's dtype and op order
  (the order of ``gmm_cost_grad`` in oracle/sgmcmc_oracle_body.inc); ``exp`` and ``log`` go through libm in double and
  are then rounded, as the kernel and the oracle do (``math.exp``, not ``numpy.exp``: numpy's vectorised ``exp`` is a
  different implementation and need not round like libm's).
* :func:`cost_grad_exact` is the same derivative in ``np.longdouble`` with a stable logsumexp: the high-precision truth.
* :func:`chain` steps ``oracle.c_sghmc_step`` / ``c_sgld_step`` / ``c_rsghmc_step`` on a flat ``CState`` that holds all
  chains, fed :func:`cost_grad`.
* :func:`twin_spread` measures how far a chain moves when every gradient is moved by one ulp: the tolerance of the
  free-running comparisons comes from it, never from the kernel's output.

Targets and their parameters are the kernel's: 0 = 1-D Gaussian mixture ``[mu[k], var[k], w[k]]``, 1 = banana ``[]``,
2 = 2-D unit-variance equal-weight mixture ``[x_0, y_0, x_1, y_1, ...]``.
"""
import math

import numpy as np

from oracle import sgmcmc_oracle as O

GMM1D, BANANA, GMM2D = 0, 1, 2
SGHMC, SGLD, RSGHMC = 0, 1, 2
DIM = {GMM1D: 1, BANANA: 2, GMM2D: 2}
_THIRD = 1.0 / 3.0
# the built-in targets as pysgmcmc_amd/samplers/builtin_target_chains.py hands them to the kernel
BUILTIN = {
    "gmm1": (GMM1D, [-5, 0, 5, 1.0, 1.0, 1.0, _THIRD, _THIRD, _THIRD]),
    "gmm2": (GMM1D, [-5, 0, 5, 1.0 / 0.5, 0.5, 1.0 / 0.5, _THIRD, _THIRD, _THIRD]),
    "gmm3": (GMM1D, [-5, 0, 5, 1.0 / 0.3, 0.3, 1.0 / 0.3, _THIRD, _THIRD, _THIRD]),
    "banana": (BANANA, []),
    "gmm2d": (GMM2D, [-5.0, 0.0, 0.0, 0.0, 5.0, 0.0]),
}
STATE_ROWS = {SGHMC: ("theta", "mom", "tau", "g", "v_hat", "minv"), SGLD: ("theta", "tau", "g", "v_hat", "minv"),
              RSGHMC: ("theta", "mom")}

_libm_exp = np.frompyfunc(math.exp, 1, 1)
_TWO_PI = 2.0 * 3.14159265358979323846


def _exp_via_double(t, T):
    """``(T)exp((double)t)`` element-wise through libm."""
    return _libm_exp(np.asarray(t, np.float64)).astype(np.float64).astype(T)


def gmm1d_constants(params, dtype):
    """``(mu, var, a, b)`` as ``toy_chains()`` rounds them: ``a_i = (T)log((double)(T)w_i)``,
    ``b_i = T(0.5) * (T)log(2 pi (double)(T)var_i)``."""
    T = np.dtype(dtype).type
    k = len(params) // 3
    p = np.asarray(params, np.float64)
    mu, var, w = p[:k].astype(T), p[k:2 * k].astype(T), p[2 * k:].astype(T)
    a = np.array([math.log(float(v)) for v in w], np.float64).astype(T)
    b = T(0.5) * np.array([math.log(_TWO_PI * float(v)) for v in var], np.float64).astype(T)
    return mu, var, a, b


def cost_grad(target, params, theta, dtype):
    """d cost / d theta of ``theta[n, dim]`` in ``dtype``, every operation rounded once, in the kernel's order."""
    T = np.dtype(dtype).type
    theta = np.asarray(theta, T).reshape(-1, DIM[target])
    n = theta.shape[0]
    out = np.zeros((n, DIM[target]), T)
    if target == BANANA:
        x, y = theta[:, 0], theta[:, 1]
        u = (y + T(0.1) * (x * x)) - T(10)
        out[:, 0] = T(0.01) * x + u * (T(0.2) * x)
        out[:, 1] = u
        return out
    if target == GMM1D:
        mu, var, a, b = gmm1d_constants(params, T)
        k = mu.size
        x = theta[:, 0]
        d = x[:, None] - mu[None, :]
        t = (a - b)[None, :] - (T(0.5) * (d * d)) / var[None, :]
        e = _exp_via_double(t - t.max(axis=1)[:, None], T)
        s = np.zeros(n, T)
        for i in range(k):
            s = s + e[:, i]
        g = np.zeros(n, T)
        for i in range(k):
            g = g + (e[:, i] / s) * ((x - mu[i]) / var[i])
        out[:, 0] = g
        return out
    c = np.asarray(params, np.float64).astype(T).reshape(-1, 2)
    k = c.shape[0]
    x, y = theta[:, 0], theta[:, 1]
    dx, dy = x[:, None] - c[None, :, 0], y[:, None] - c[None, :, 1]
    t = -(T(0.5) * (dx * dx + dy * dy))
    e = _exp_via_double(t - t.max(axis=1)[:, None], T)
    s = np.zeros(n, T)
    for i in range(k):
        s = s + e[:, i]
    gx, gy = np.zeros(n, T), np.zeros(n, T)
    for i in range(k):
        w = e[:, i] / s
        gx = gx + w * (x - c[i, 0])
        gy = gy + w * (y - c[i, 1])
    out[:, 0], out[:, 1] = gx, gy
    return out


def cost_grad_exact(target, params, theta, dtype, terms=False):
    """The same derivative in ``np.longdouble`` (stable logsumexp) of the target the kernel sees: ``theta`` and the
    parameters are first rounded to ``dtype``, everything after that is long double. ``terms=True`` also returns what
    the conditioned error bounds are made of: ``sum_abs[n, dim] = sum_i |r_i q_i|`` (r = responsibilities, q_i = the
    component's own gradient), ``sum_q[n, dim] = sum_i |q_i|``, ``t_max[n] = max_i |t_i|`` and, for the 1-D mixture,
    ``const = max_i (|a_i| + |b_i|)``."""
    L = np.longdouble
    T = np.dtype(dtype).type
    theta = np.asarray(theta, T).reshape(-1, DIM[target]).astype(L)
    if target == BANANA:
        x, y = theta[:, 0], theta[:, 1]
        u = (y + L(1) / L(10) * (x * x)) - L(10)
        g = np.stack([x / L(100) + u * (x / L(5)), u], axis=1)
        return (g, {}) if terms else g
    if target == GMM1D:
        k = len(params) // 3
        p = np.asarray(params, np.float64)
        mu, var, w = (p[i * k:(i + 1) * k].astype(T).astype(L) for i in range(3))
        a, b = np.log(w), L(0.5) * np.log(L(2) * L(np.pi) * var)       # pi to double: the kernel's constant
        d = theta[:, 0:1] - mu[None, :]
        t = (a - b)[None, :] - L(0.5) * d * d / var[None, :]
        q = (d / var[None, :])[:, :, None]                              # [n, k, 1]
        const = float(np.max(np.abs(a) + np.abs(b)))
    else:
        c = np.asarray(params, np.float64).astype(T).astype(L).reshape(-1, 2)
        q = theta[:, None, :] - c[None, :, :]                           # [n, k, 2]
        t = -L(0.5) * (q * q).sum(axis=2)
        const = 0.0
    e = np.exp(t - t.max(axis=1)[:, None])
    r = e / e.sum(axis=1)[:, None]
    g = (r[:, :, None] * q).sum(axis=1)
    if not terms:
        return g
    return g, {"sum_abs": np.abs(r[:, :, None] * q).sum(axis=1), "sum_q": np.abs(q).sum(axis=1),
               "t_max": np.abs(t).max(axis=1), "const": const, "k": t.shape[1]}


def tie_points(params, lo, hi):
    """Every x in [lo, hi] at which two components of a 1-D mixture have the same log-density term (roots of the
    quadratic t_i(x) = t_j(x), double precision): where the running maximum of the logsumexp changes hands."""
    k = len(params) // 3
    p = np.asarray(params, np.float64)
    mu, var, w = p[:k], p[k:2 * k], p[2 * k:]
    c0 = np.log(w) - 0.5 * np.log(_TWO_PI * var)
    roots = []
    for i in range(k):
        for j in range(i + 1, k):
            qa = -0.5 / var[i] + 0.5 / var[j]
            qb = mu[i] / var[i] - mu[j] / var[j]
            qc = (c0[i] - 0.5 * mu[i] ** 2 / var[i]) - (c0[j] - 0.5 * mu[j] ** 2 / var[j])
            if qa == 0.0:
                r = [-qc / qb] if qb != 0.0 else []
            else:
                disc = qb * qb - 4.0 * qa * qc
                r = [] if disc < 0 else [(-qb + sg * math.sqrt(disc)) / (2.0 * qa) for sg in (1.0, -1.0)]
            roots += [v for v in r if lo <= v <= hi]
    return np.array(sorted(roots), np.float64)


class NoiseTable(object):
    """``noise(chain, step)`` backed by an array ``xi[n_chains, n_steps, dim]`` whose step axis starts at ``first_step``
    (what a test fills once from the K5 stream, or from the oracle's)."""

    def __init__(self, xi, first_step):
        self.xi, self.first_step = np.asarray(xi), int(first_step)

    def __call__(self, chain, step):
        return self.xi[chain, step - self.first_step]

    def step_rows(self, step, n_chains, dim):
        return self.xi[:n_chains, step - self.first_step, :dim]


def oracle_noise(seeds, dim, dtype):
    """``noise(chain, step)`` from the oracle's own Philox stream: element i of chain c at a step is xi(seed_c, step, i)."""
    return lambda chain, step: O.c_philox_normal(int(seeds[chain]), int(step), dim, dtype)


def chain(kind, target, params, state, scalars, seed, first_step, n_steps, burn_in_steps, keep_every, noise=None,
          twin_rng=None, grad_fn=None):
    """``n_steps`` steps of all chains of ``state`` (dict of ``[n_chains, dim]`` arrays named as STATE_ROWS; rows the
    sampler does not own may be missing) on the C oracle's step functions, fed :func:`cost_grad` (or ``grad_fn(theta)``).
    ``adapt = burn_in_steps <= 0 or step < burn_in_steps``; ``noise(chain, step)`` returns the chain's ``dim`` normals of
    that step (default: the oracle's Philox stream keyed by ``seed[chain]``). ``scalars`` are the sampler's, in the
    kernel's order: SGHMC ``(eps, scale_grad, mdecay)``, SGLD ``(eps, A, scale_grad)``, relativistic
    ``(eps, mass, c, D, b_hat)``. ``twin_rng``: move every gradient one ulp up or down at random (a perturbed twin).
    Returns ``(kept[ceil(n_steps / keep_every), n_chains, dim], final state dict)``; ``state`` is left untouched."""
    theta0 = np.asarray(state["theta"])
    dt = theta0.dtype
    n, dim = theta0.shape
    assert dim == DIM[target]
    if noise is None:
        noise = oracle_noise(seed, dim, dt)
    st = O.CState(theta0, dt)
    rows = {"theta": "theta", "mom": "V" if kind == SGHMC else "p", "tau": "tau", "g": "g", "v_hat": "v_hat", "minv": "minv"}
    for name in STATE_ROWS[kind]:
        getattr(st, rows[name])[:] = np.asarray(state[name], dt).ravel()
    kept = np.empty(((n_steps + keep_every - 1) // keep_every, n, dim), dt)
    n_kept = 0
    for s in range(n_steps):
        step = first_step + s
        th = st.theta.reshape(n, dim)
        grad = cost_grad(target, params, th, dt) if grad_fn is None else np.asarray(grad_fn(th), dt).reshape(n, dim)
        if twin_rng is not None:
            grad = np.nextafter(grad, np.where(twin_rng.integers(0, 2, size=grad.shape) == 1, np.inf, -np.inf).astype(dt))
        if hasattr(noise, "step_rows"):
            xi = np.ascontiguousarray(noise.step_rows(step, n, dim), dt)
        else:
            xi = np.stack([np.asarray(noise(c, step), dt)[:dim] for c in range(n)])
        adapt = burn_in_steps <= 0 or step < burn_in_steps
        with np.errstate(all="ignore"):
            if kind == SGHMC:
                O.c_sghmc_step(st, grad, scalars[0], scalars[1], scalars[2], adapt, xi)
            elif kind == SGLD:
                O.c_sgld_step(st, grad, scalars[0], scalars[1], scalars[2], adapt, xi)
            else:
                O.c_rsghmc_step(st, grad, scalars[0], scalars[1], scalars[2], scalars[3], scalars[4], xi)
        if s % keep_every == 0:
            kept[n_kept] = st.theta.reshape(n, dim)
            n_kept += 1
    return kept, {name: getattr(st, rows[name]).reshape(n, dim).copy() for name in STATE_ROWS[kind]}


N_TWINS = 8
SPREAD_CAP = 64.0       # in units of eps_T max(1, |x|): beyond it a case is too chaotic to pin and is replaced


def _in_ulps(diff, base, chain_axis):
    """max over everything but the chain axis of |diff| / (eps_T max(1, |base|)): one figure per chain"""
    eps = np.finfo(base.dtype).eps
    r = np.abs(diff.astype(np.float64)) / (eps * np.maximum(1.0, np.abs(base.astype(np.float64))))
    return r.max(axis=tuple(a for a in range(r.ndim) if a != chain_axis))


def twin_spread(kind, target, params, state, scalars, seed, first_step, n_steps, burn_in_steps, keep_every,
                noise=None, twin_seed=0):
    """The unperturbed reference run and, per chain, the largest distance to it of N_TWINS twins whose every gradient is
    moved one ulp up or down at random (seeded), over the kept rows and every final state array, in units of
    ``eps_T max(1, |x|)``. Chains are independent, so the spread of a case with the first n chains is ``spread[:n].max()``.
    Returns ``(kept, final, spread[n_chains])``."""
    args = (kind, target, params, state, scalars, seed, first_step, n_steps, burn_in_steps, keep_every, noise)
    kept, final = chain(*args)
    spread = np.zeros(kept.shape[1])
    for t in range(N_TWINS):
        k2, f2 = chain(*args, twin_rng=np.random.default_rng([twin_seed, t]))
        spread = np.maximum(spread, _in_ulps(k2 - kept, kept, 1))
        for name in final:
            spread = np.maximum(spread, _in_ulps(f2[name] - final[name], final[name], 0))
    return kept, final, spread


def allowance(base, spread):
    """What a device run may differ from the reference ``base`` by: 4 x the largest twin spread plus 2 ulp of
    ``max(1, |x|)``. The device's gradients differ from :func:`cost_grad` by at most the twins' one-ulp perturbation (its
    double ``exp`` is within 1 ulp of libm's), and on far fewer steps; the factor 4 covers the twins being a sample of 8."""
    eps = np.finfo(base.dtype).eps
    return (4.0 * spread + 2.0) * eps * np.maximum(1.0, np.abs(base.astype(np.float64)))


def within(got, base, spread):
    """Largest ``|got - base| / allowance`` (<= 1 passes)."""
    return float(np.max(np.abs(got.astype(np.float64) - base.astype(np.float64)) / allowance(base, spread)))


# ---- the error bounds of the gradient comparisons (derivations: tests/test_toy_chains_kernel_gpu.py) ----------------

def _floor(terms, T):
    """Underflow: an ``e_i`` below the smallest normal of T carries an ABSOLUTE error of up to one subnormal spacing
    (the double exp result is rounded to a subnormal or to 0), so do ``e_i / s`` and its product with ``q_i``:
    at most ``2 tiny_T sum_i (1 + |q_i|)`` in the gradient."""
    return 2.0 * float(np.finfo(T).smallest_subnormal) * (terms["k"] + terms["sum_q"].astype(np.float64))


def bound_vs_cost_grad(terms, dtype):
    """``(k + 4) eps_T sum_i |r_i q_i|`` (+ the underflow floor): two evaluations of the same program whose ``exp`` results
    differ by at most one ulp."""
    T = np.dtype(dtype).type
    return (terms["k"] + 4) * float(np.finfo(T).eps) * terms["sum_abs"].astype(np.float64) + _floor(terms, T)


def exact_bound_constant(target, terms):
    """``c`` of ``c eps_T (1 + max_i |t_i|) sum_i |r_i q_i|`` from the op count (see the GPU test module's docstring)."""
    k = terms["k"]
    return k + 15 + 14.0 * terms["const"] if target == GMM1D else k + 13


def bound_vs_exact(target, terms, dtype):
    T = np.dtype(dtype).type
    c = exact_bound_constant(target, terms)
    cond = (1.0 + terms["t_max"].astype(np.float64))[:, None]
    return c * float(np.finfo(T).eps) * cond * terms["sum_abs"].astype(np.float64) + _floor(terms, T)


# ---- the shared cases ------------------------------------------------------------------------------------------------

N_PROBE = 4099          # chains of a gradient probe launch: 65 blocks of 64 lanes, the last one ragged


def random_mixture_1d(k=16, seed=20):
    """k components: centres in [-20, 20], variances in [1e-3, 1e3] (log-uniform), weights from 1e-30 to 1."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-20.0, 20.0, k)
    var = 10.0 ** rng.uniform(-3.0, 3.0, k)
    var[0], var[1] = 1e-3, 1e3
    w = rng.permutation(10.0 ** np.linspace(-30.0, 0.0, k))
    return list(mu) + list(var) + list(w)


def random_centres_2d(k=16, seed=21):
    return list(np.random.default_rng(seed).uniform(-10.0, 10.0, 2 * k))


def _points_1d(params, dtype):
    """x dense on [-40, 40], every mu_i exactly (as the dtype holds it) and the points where two components tie."""
    k = len(params) // 3
    special = np.concatenate([np.asarray(params[:k], np.float64), tie_points(params, -40.0, 40.0)])
    special = special[:N_PROBE // 4]
    x = np.concatenate([special, np.linspace(-40.0, 40.0, N_PROBE - special.size)])
    return x.astype(dtype).reshape(-1, 1)


def _grid_2d(half, extra, dtype):
    ax = np.linspace(-half, half, 64)
    g = np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=2).reshape(-1, 2)
    pts = np.concatenate([g, np.asarray(extra, np.float64).reshape(-1, 2)])
    assert pts.shape[0] == N_PROBE
    return pts.astype(dtype)


def probe_sets(dtype):
    """``[(name, target, params, theta[N_PROBE, dim])]``: the sweeps of the gradient probe."""
    out = []
    for name in ("gmm1", "gmm2", "gmm3"):
        out.append((name, GMM1D, BUILTIN[name][1], _points_1d(BUILTIN[name][1], dtype)))
    one = [1.7, 0.37, 1.0]
    out.append(("k1", GMM1D, one, _points_1d(one, dtype)))
    wide = random_mixture_1d()
    out.append(("k16", GMM1D, wide, _points_1d(wide, dtype)))
    c3 = BUILTIN["gmm2d"][1]
    out.append(("gmm2d", GMM2D, c3, _grid_2d(12.0, c3, dtype)))
    c16 = random_centres_2d()
    out.append(("gmm2d_k16", GMM2D, c16, _grid_2d(12.0, c16[:6], dtype)))
    out.append(("banana", BANANA, [], _grid_2d(30.0, [0.0, 0.0, 0.0, 10.0, 1.5, 8.0], dtype)))
    return out


# short free-running chains: 48 steps from step 5, burn-in switch at step 20, every third state kept
FREE = dict(first_step=5, n_steps=48, burn_in_steps=20, keep_every=3)
FREE_STARTS = {"gmm1": [0.4], "gmm2": [0.4], "gmm3": [-2.6], "banana": [0.5, 6.0], "gmm2d": [0.5, -0.5]}
FREE_SCALARS = {SGHMC: (0.05, 1.0, 0.05), SGLD: (0.05, 1.0, 1.0), RSGHMC: (0.1, 1.0, 1.0, 1.0, 0.0)}
FREE_CHAINS = 130
FREE_POOL = 192         # candidate chains of a case; the first FREE_CHAINS tame ones are used
FREE_PICK = 16.0        # a candidate whose own twin spread exceeds this many eps_T is replaced by the next one


def free_seeds(n_chains=FREE_POOL):
    return [1000 + c for c in range(n_chains)]


def free_state(kind, name, dtype, n_chains=FREE_POOL):
    """Chain c starts at the target's start + c / 128 in every coordinate, V = p = 0.3, statistics at their initial 1."""
    target = BUILTIN[name][0]
    theta = (np.asarray(FREE_STARTS[name], np.float64)[None, :] + np.arange(n_chains)[:, None] / 128.0).astype(dtype)
    st = {"theta": theta}
    for row in STATE_ROWS[kind][1:]:
        st[row] = np.full((n_chains, DIM[target]), 0.3 if row == "mom" else 1.0, dtype)
    return st


def free_case(kind, name, dtype, pool_noise, **overrides):
    """One free-running case: the reference run of the FREE_POOL candidate chains with ``pool_noise`` (a NoiseTable over
    the candidates and the FREE steps), their twin spreads, and the first FREE_CHAINS candidates whose spread is at most
    FREE_PICK. A few SGLD candidates drive v_hat towards 0 during burn-in and amplify one ulp a hundredfold: such a
    chain cannot be pinned by a tolerance and is replaced by the next candidate -- a choice made from the reference
    alone. ``overrides`` replace entries of FREE (another burn-in, say). Returns a dict: target, params, scalars, seeds, state, kept, final, spread (of the chosen chains), noise."""
    target, params = BUILTIN[name]
    state, seeds = free_state(kind, name, dtype), free_seeds()
    kept, final, spread = twin_spread(kind, target, params, state, FREE_SCALARS[kind], seeds, noise=pool_noise,
                                      **dict(FREE, **overrides))
    sel = np.flatnonzero(spread <= FREE_PICK)[:FREE_CHAINS]
    assert sel.size == FREE_CHAINS, "only %d of %d candidate chains are tame" % (sel.size, FREE_POOL)
    return dict(target=target, params=params, scalars=FREE_SCALARS[kind], seeds=[seeds[i] for i in sel],
                state={k: v[sel].copy() for k, v in state.items()}, kept=kept[:, sel].copy(),
                final={k: v[sel].copy() for k, v in final.items()}, spread=spread[sel], pool_spread=spread,
                noise=NoiseTable(pool_noise.xi[sel], pool_noise.first_step))
