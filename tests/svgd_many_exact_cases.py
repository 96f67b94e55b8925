"""Lattice clouds, small-n and translated cases of the many-particle SVGD path (csrc/sgmcmc_svgd_many.hip), shared by
``test_svgd_many_exact.py`` (no GPU) and ``test_svgd_many_exact_gpu.py``.

A LATTICE cloud has small integers in every entry and a column mean that the dtype holds exactly. Then every partial sum of
MEAN, of the centred Gram blocks, of REDUCE and of DIST is exact in any order, so ``D_ij = fl(fl(sqrt(k))^2)`` for the exact
integer ``k = |x_i - x_j|^2``: what the oracle gives in the case's own dtype, bit for bit. The median of such a cloud is
asserted with ``==``; ``test_svgd_many_exact.py`` checks the premise for every case, by exact integer arithmetic and by an
emulation of the kernels' order of summation (``emulated_sqdist``).

``python tests/svgd_many_exact_cases.py`` prints the oracle's own error at the small-n step cases (``narrow_against_wide``
of svgd_many_cases.py) and the select facts of every lattice case."""
import collections

import numpy as np

import svgd_many_cases as M                                                            # puts the repository root on sys.path

from oracle import sgmcmc_oracle as O                                                  # noqa: E402
import test_svgd_tile_walk_gpu as W                                                    # noqa: E402  (step_reference_on)

F32, F64 = M.F32, M.F64
MANTISSA = {F32: 24, F64: 53}
MEAN_CHAINS = 8                               # MANY_MEAN_CHAINS of the .hip file

# (family, n, d): what each family is there for is in ``lattice`` below
FAMILIES = ("balanced", "clusters", "offset", "sphere", "boundary")
LATTICE = [
    ("balanced", 3, 2),         # the smallest odd count
    ("balanced", 46, 5),        # the first n with two select workgroups
    ("balanced", 129, 3),       # odd n * n
    ("balanced", 130, 40),
    ("balanced", 161, 7),       # odd n * n
    ("balanced", 1024, 6),      # the capped select grid of 256 workgroups; ties of 1e5 keys
    ("clusters", 130, 3),
    ("clusters", 256, 3),
    ("offset", 256, 33),
    ("offset", 512, 5),
    ("sphere", 256, 258),
    ("boundary", 256, 258),
]
CLUSTER_POINT = (3, -1, 2)                    # |2 a|^2 = 56
OFFSET_C = {(256, 33): 4096, (512, 5): 1000}
# sphere: 2 (n r)^2 is 1.53 x 2^22 in f32 and just below 2^52 in f64 at n = 256. The issue's r = 8 in f32 puts 2 (n r)^2 on
# 2^23 itself, and fl(fl(sqrt(2^23))^2) = 2^23 - 0.5: the keys then lie on both sides of the exponent boundary and differ in
# every byte below the first, so that cloud cannot have the one-giant-bin property the family is there for (its premise
# fails on the CPU). 2 (n r)^2 = 2^17 r^2 always sits on a 2^16 edge of the key space, so r must be one whose round trip does
# not go below it: 7 is the largest that fits 24 bits (5 is the other; 1 .. 4, 6 and 8 round down). The r = 8 cloud is kept as
# a family of its own, ``boundary`` (r = 2^17 in f64: 2^51, where the round trip goes up and every key stays above).
SPHERE_R = {"sphere": {F32: 7, F64: 185363}, "boundary": {F32: 8, F64: 131072}}

# the raw entries below 64 particles and around them: smallest even and odd counts, np == n, one particle into a second
# 16-block, one and two select workgroups, three block pairs, one short of 128
SMALL = [(2, 1), (3, 2), (16, 5), (17, 33), (45, 7), (46, 7), (65, 20), (127, 3)]
# a cloud 100 away from the origin with a spread of 1 / sqrt(d) per column
TRANSLATED = [(129, 40), (257, 3)]
TRANSLATION = 100.0


def lattice(family, n, d, dtype):
    """The cloud of one case, in ``dtype``; rng seeded from (n, d, family)."""
    rng = np.random.default_rng([n, d, FAMILIES.index(family)])
    if family == "balanced":
        # every column: k entries +1, k entries -1, the rest 0, shuffled: column sums are 0 for any n, D has few distinct
        # values, so the median rank falls inside a tie
        X = np.zeros((n, d), np.int64)
        for c in range(d):
            k = int(rng.integers(1, n // 2 + 1))
            col = np.array([1] * k + [-1] * k + [0] * (n - 2 * k), np.int64)
            rng.shuffle(col)
            X[:, c] = col
    elif family == "clusters":
        # n / 2 copies of a and of -a: half of the keys are 0 and half 56', count_le == mid, the upper middle value is NEXT's
        assert n % 2 == 0 and d == len(CLUSTER_POINT)
        X = np.array([CLUSTER_POINT] * (n // 2) + [tuple(-v for v in CLUSTER_POINT)] * (n // 2), np.int64)
        rng.shuffle(X, axis=0)
    elif family == "offset":
        # c + e, e in -2 .. 2, the second half of a column the negation of the first: the mean is the integer c exactly,
        # and without MEAN's centring the f32 Gram entries would be near 5e8
        assert n & (n - 1) == 0
        e = rng.integers(-2, 3, size=(n // 2, d))
        X = OFFSET_C[(n, d)] + np.concatenate([e, -e], axis=0)
    elif family in ("sphere", "boundary"):
        # particle i has n r in column i; two more columns of integers 0 .. 11 whose second half is 11 minus the first.
        # Every off-diagonal D is 2 (n r)^2 + small: the keys agree in all but the lowest one or two bytes
        assert n & (n - 1) == 0 and d == n + 2
        X = np.zeros((n, d), np.int64)
        X[np.arange(n), np.arange(n)] = n * SPHERE_R[family][dtype]
        first = rng.integers(0, 12, size=(n // 2, 2))
        X[:, n:] = np.concatenate([first, 11 - first], axis=0)
    else:
        raise ValueError(family)
    out = X.astype(dtype)
    assert np.array_equal(out.astype(np.int64), X)
    return out


Exact = collections.namedtuple("Exact", "X D med K kg h med64")
_exact = {}


def exact_reference(family, n, d, dtype):
    """X, the oracle's D and median IN THE CASE'S DTYPE (what the kernels must reproduce bit for bit), and K, kernel
    gradients, h and the median of the f64 oracle on the same inputs. Computed once, never modified."""
    key = (family, n, d, np.dtype(dtype).name)
    if key not in _exact:
        X = lattice(family, n, d, dtype)
        D = O.svgd_kernel(X)[3]
        assert D.dtype == dtype
        K, kg, h, D64 = O.svgd_kernel(X.astype(np.float64))
        for a in (X, D, K, kg):
            a.setflags(write=False)
        _exact[key] = Exact(X, D, O.svgd_median(D), K, kg, float(h), float(O.svgd_median(D64)))
    return _exact[key]


# ---- host checks of the premise --------------------------------------------------------------------------------------------

def exact_sqdist(X):
    """|x_i - x_j|^2 in int64 from an integer-valued cloud"""
    Xi = X.astype(np.int64)
    assert np.array_equal(Xi.astype(X.dtype), X)
    sq = (Xi * Xi).sum(axis=1)
    return sq[:, None] + sq[None, :] - 2 * (Xi @ Xi.T)


def fits(values, dtype):
    """True if every integer of ``values`` (int64) is a number of ``dtype``"""
    values = np.asarray(values, np.int64)
    return bool(np.array_equal(values.astype(dtype).astype(np.int64), values))


def partial_sum_bounds(X, dtype):
    """(largest |partial sum| of a column sum, of a centred Gram entry), each in units of its quantum, for ANY order of
    summation: the sum of the absolute values of the terms. A value  m * quantum  with |m| <= 2^mantissa is a number of the
    dtype. The centred entries are multiples of 1 / s (s = 1 or 2: a column mean may be a half-integer), their products
    multiples of 1 / s^2."""
    Xi = X.astype(np.int64)
    n = X.shape[0]
    col = np.abs(Xi).sum(axis=0)
    total = Xi.sum(axis=0)
    s = 1 if np.all(total % n == 0) else 2
    assert np.all((s * total) % n == 0), "a column mean is neither an integer nor a half-integer"
    Y = s * Xi - (s * total) // n                                    # s x the centred cloud, exact
    A = np.abs(Y)
    return int(col.max()), int((A @ A.T).max()), s, Y


def roundtrip(k, dtype):
    """fl(fl(sqrt(k))^2) in ``dtype`` for exact integers k"""
    assert fits(k, dtype)
    dist = np.sqrt(np.asarray(k).astype(dtype))
    assert dist.dtype == dtype
    return dist * dist


def emulated_mean(X):
    """MEAN in X.dtype: chain k adds the rows k, k + 8, ... in ascending order, the chains are added in chain order, then
    times fl(1 / n)"""
    T = X.dtype.type
    n, d = X.shape
    chains = np.zeros((MEAN_CHAINS, d), X.dtype)
    for r in range(n):
        chains[r % MEAN_CHAINS] += X[r]
    m = chains[0].copy()
    for k in range(1, MEAN_CHAINS):
        m = m + chains[k]
    return m * (T(1) / T(n))


def emulated_sqdist(X, order):
    """D as MEAN, GRAM / REDUCE and DIST form it, in X.dtype, with the Gram columns added in the order ``order``"""
    T = X.dtype.type
    n = X.shape[0]
    Y = X - emulated_mean(X)[None, :]
    g = np.zeros((n, n), X.dtype)
    for c in order:
        g += Y[:, c][:, None] * Y[:, c][None, :]
    diag = np.diag(g)
    s = (diag[:, None] + diag[None, :]) - T(2) * g                    # symmetric, so (lo, hi) and (hi, lo) agree
    s = np.where(s > 0, s, T(0))
    dist = np.sqrt(s)
    D = dist * dist
    D[np.arange(n), np.arange(n)] = 0
    assert D.dtype == X.dtype
    return D


def keys(D):
    return np.ascontiguousarray(D).view(np.uint32 if D.dtype == F32 else np.uint64).reshape(-1)


Select = collections.namedtuple("Select", "N mid rank lo count_le next_key distinct")


def select_facts(D):
    """What SELECT, NEXT and BANDWIDTH see: the key of rank mid (odd n * n) or mid - 1 (even), how many keys are <= it, the
    smallest larger key (None if there is none), and the number of distinct keys"""
    k = np.sort(keys(D))
    N = k.shape[0]
    mid = N // 2
    rank = mid if N % 2 else mid - 1
    lo = k[rank]
    count_le = int(np.searchsorted(k, lo, side="right"))
    return Select(N, mid, rank, int(lo), count_le, int(k[count_le]) if count_le < N else None, int(np.unique(k).shape[0]))


# ---- steps on inputs that are not the table's recipe -----------------------------------------------------------------------

def lattice_step_inputs(family, n, d, dtype):
    """(X, G, H) for a step on a lattice cloud: any G will do, the header words depend on X alone"""
    rng = np.random.default_rng([n, d, FAMILIES.index(family), 1])
    X = lattice(family, n, d, dtype)
    return X, rng.normal(size=(n, d)).astype(dtype), rng.uniform(0.05, 1.0, size=(n, d)).astype(dtype)


def translated_cloud(n, d, dtype):
    """``cloud`` of svgd_many_cases.py moved 100 away from the origin, rounded to the dtype"""
    return M.cloud(n, d, dtype, seed=n * 1000 + d, offset=TRANSLATION, scale=1.0 / np.sqrt(d))


_translated = {}


def translated_kernel_reference(n, d, dtype):
    """(X, K, kernel gradients, h, median) of the f64 oracle ON THE ROUNDED INPUTS"""
    key = (n, d, np.dtype(dtype).name)
    if key not in _translated:
        X = translated_cloud(n, d, dtype)
        K, kg, h, D = O.svgd_kernel(X.astype(np.float64))
        for a in (X, K, kg):
            a.setflags(write=False)
        _translated[key] = (X, K, kg, float(h), float(O.svgd_median(D)))
    return _translated[key]


def translated_step_inputs(n, d, dtype):
    rng = np.random.default_rng([n, d, np.dtype(dtype).itemsize, 100])
    return (translated_cloud(n, d, dtype), rng.normal(size=(n, d)).astype(dtype),
            rng.uniform(0.05, 1.0, size=(n, d)).astype(dtype))


_translated_steps = {}


def translated_step_reference(n, d, dtype, sign, wide=np.float64):
    key = (n, d, np.dtype(dtype).name, sign, np.dtype(wide).name)
    if key not in _translated_steps:
        ref = W.step_reference_on(translated_step_inputs(n, d, dtype), sign, wide)
        for a in ref:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _translated_steps[key] = ref
    return _translated_steps[key]


def translated_narrow_against_wide(n, d, dtype, sign):
    """``narrow_against_wide`` of svgd_many_cases.py on the translated inputs"""
    wide = np.float64 if dtype == F32 else np.longdouble
    ref = W.step_reference_on(translated_step_inputs(n, d, dtype), sign, wide)
    Xn, Hn = ref.X.copy(), ref.H.copy()
    O.svgd_step(Xn, ref.G, Hn, M.EPS, M.ALPHA, M.FUDGE, float(sign))
    return W.bar_units(ref, dtype, Xn, Hn)


if __name__ == "__main__":
    for dtype in (F32, F64):
        name = np.dtype(dtype).name
        for family, n, d in LATTICE:
            f = select_facts(exact_reference(family, n, d, dtype).D)
            print("%-8s %-8s %4d x %-3d  %3d distinct keys, count_le - mid = %d" % (name, family, n, d, f.distinct, f.count_le - f.mid))
        if dtype == F64 and not M.LONG_DOUBLE_IS_WIDER:
            continue
        for n, d in SMALL:
            row = [u for sign in (1, -1) for u in M.narrow_against_wide(M.Case(n, d, dtype, sign))]
            print("%-8s small      %4d x %-3d  oracle units (X, H) sign +1 | -1: %.3f %.3f %.3f %.3f" % ((name, n, d) + tuple(row)))
        for n, d in TRANSLATED:
            row = [u for sign in (1, -1) for u in translated_narrow_against_wide(n, d, dtype, sign)]
            print("%-8s translated %4d x %-3d  oracle units (X, H) sign +1 | -1: %.3f %.3f %.3f %.3f" % ((name, n, d) + tuple(row)))
