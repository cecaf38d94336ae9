"""Criterion for the pair sums and the moments of csrc/metrics.hip (smd_pair_kernel_sums, smd_moments): integer lattices whose
results are exact, float64 references with derived per-pair / per-element bounds, input regimes, an fp32 emulation of the kernels'
arithmetic and planted faults.  NumPy only, no GPU.  U and worst_ratio are those of tests/_attn_ref.py, SECOND that of _ln_ref.py,
the pair d2 bound is pair_bound of _nn_search_ref.py, FLT_MIN that of _nn_metrics_ref.py and the float64 sums are kernel_sums of
_metrics_ref.py (imported, one definition each).

The kernels (csrc/metrics.hip, csrc/gram_tile.h), T = 128:
    pair sums   g_ij = <x_i, y_j> and |x_i|^2, |y_j|^2 as fp32 fma chains in k order;  d2 = max((-2 g + |x|^2) + |y|^2, 0), 0 on the
                diagonal of the symmetric mode;  kr = __expf(-gamma_rbf d2);  kp = t^degree by repeated multiplication,
                t = gamma_poly g + coef0;  the 16 accumulator values of one lane and MFMA tile are added in fp32, everything after
                that in fp64; the symmetric mode visits the tiles bi <= bj and doubles those with bi < bj.
    moments     fp64 column sums per row slab, mean = sum / n;  xc = fp32(fp64(x) - mean);  C = sum_r xc_a xc_b as fp32 fma chains
                over the rows that are added to fp64 every 32 rows (sooner at the end of a slab);  cov = C / (n - 1).

1. Lattices: conditions, not measurements.  On rows of small integers every product, every partial sum of a chain, both norms and
   (-2 g + |x|^2) + |y|^2 are integers below 2^24 in magnitude: fp32 holds them exactly, in ANY order of the additions.
   duplicates  gamma_rbf = 200: a pair with d2 >= 1 gives exp2(-200 log2e d2) = exp2(-288.5..) = 0 (below the smallest fp32
               denormal 2^-149) and d2 = 0 gives exp2(-0) = 1, so out[0] is the NUMBER of pairs at distance 0: the planted ones in
               the full mode, n + 2 (planted unordered pairs) in the symmetric one.  One missing, doubled or mis-masked pair, one
               norm read from another slot, moves that integer by at least 1.
   polynomial  gamma_poly = 1 and integer coef0: t and every power of it are integers; with |t^degree| <= 2^20 the fp32 sum of 16
               of them stays below 2^24 and is exact, the fp64 sums are sums of integers below 2^53: out[1] is the int64 sum, bit
               for bit.  Coordinates are in {-2 .. 2}; a row keeps at most (floor(2^(20 / degree)) - |coef0|) / 4 non-zero ones
               (all of them up to degree 2, 24 at degree 3, 7 at degree 4), which is what holds |t| under 2^(20 / degree).
   moments     rows in +- pairs (and one zero row for odd n): every column sums to exactly 0 in fp64, the mean is 0, the centred
               rows are the rows.  With magnitudes in [512, 724] a 32-row sum of products is at most 32 * 724^2 = 16,773,632 < 2^24
               and exact, while 64 rows of squares reach 64 * 512^2 = 2^24: a chain that is not handed to fp64 every 32 rows
               loses the low bits of the diagonal.  The fp64 sums are integers below 2^53: cov = (X^T X) / (n - 1), an exact integer
               and ONE IEEE division, bit for bit, and so equal to its transpose.

2. Bounds.  U = 2^-24; an fp32 operation costs U |result|; a fma chain of d products d U sum|products| (written d + 1).
   d2     |d2_fp32 - d2| <= m_ij = (d + 4) U (|x_i| + |y_j|)^2  (pair_bound).  Of the d + 4 units d pay for the three chains
          (2 d U |x||y| + d U |x|^2 + d U |y|^2 = d U (|x| + |y|)^2) and two for the two additions; the remaining two cover the
          second-order terms and the rounding of the PRODUCT gamma d2 in front of the exponential (U gamma d2 <= U gamma (|x| + |y|)^2),
          which is why only two roundings of the argument are counted below although three happen.
   rbf    the clamp is 1-Lipschitz and keeps the computed d2 in [max(d2 - m, 0), d2 + m]: the computed kernel value lies in
              [exp(-gamma (d2 + m)) / E,  exp(-gamma max(d2 - m, 0)) E],   E = exp(2 U gamma (d2 + m)) (1 + 2 U) (1 + 16 U):
          __expf is exp2(a log2e), the constant and the product move the argument by 2 U |a| (the model of _ln_ref.py), exp2 is
          within 1 ulp = 2 U, and the 16-term fp32 sum costs 16 U.  Both ends are at most k expm1(gamma m + ...) away from
          k = exp(-gamma d2), the symmetric form; the upper end is in addition never above E, which is what the clamp buys: a
          kernel without it returns values above 1.  FLT_MIN per pair is added for results that are flushed, n_pairs 2^-53 sum k for
          the fp64 sums.  The diagonal of the symmetric mode is exactly 1.
   poly   eg = (d + 1) U sum_k |x_k y_k|;  dt = gamma eg + U (|gamma g| + |t|);  the power carries
              (|t| + dt)^degree - |t|^degree  +  (degree - 1 + 16) U (|t| + dt)^degree.
          The first term is degree |t|^(degree - 1) dt to first order; the first-order form times SECOND = 1 + 2^-10 holds only
          while degree dt < 2^-10 |t|, and the `poly_cancel` regime puts |t| BELOW dt on purpose (there the error of t^degree is
          dt^degree, which no multiple of |t|^(degree - 1) dt covers), so the exact difference is used: it is never smaller than
          the first-order term and never larger than it times SECOND where that form is valid (the host test checks both).
   mean   fp64 sum of n fp32 values in any order and one division: dm_c = n 2^-53 mean_r |x_rc|.
   cov    e_rc = dm_c + U (|xc_rc| + dm_c) is the error of the centred, rounded value.  Per element (a, b):
              [ sum_r (|xc_ra| e_rb + |xc_rb| e_ra + e_ra e_rb)  +  (32 U + (n / 32 + 18) 2^-53) sum_r (|xc_ra| + e_ra)(|xc_rb| + e_rb) ] / (n - 1)
              + 2^-52 |cov_ab|
          (propagated input error; an fp32 chain of at most 32 products; one fp64 addition per 32 rows and per slab; the division).
          Nothing is capped and no share of the elements is excluded.  A constant column is exact: n v and every partial sum of it
          fit 53 bits, (n v) / n = v, xc = 0 -- its mean error, its row and its column of cov are asserted to be 0, not bounded.
Nothing is fitted to GPU output.
"""
import math

import numpy as np

from _attn_ref import U, worst_ratio                      # noqa: F401  (one definition, re-exported)
from _ln_ref import SECOND
from _metrics_ref import kernel_sums
from _nn_metrics_ref import FLT_MIN
from _nn_search_ref import pair_bound

MT = 128                       # tile of gram_tile.h
BK = 16                        # rows per stage of centred_gram_kernel; two stages per fp64 flush
SLAB, MAX_SPLITS = 1024, 16    # MOM_SLAB_ROWS, MOM_MAX_SPLITS
EXACT = float(2 ** 24)
F32, F64 = np.float32, np.float64
LOG2E32 = F32(1.4426950408889634)
GAMMA_COUNT = 200.0            # every d2 >= 1 underflows to 0, d2 = 0 gives 1
OLD_PAIR_REL, OLD_MOM_REL = 2e-5, 1e-6     # the whole-sum thresholds of tests/test_gpu_metrics.py

EXACT_N = (1, 127, 128, 129, 257, 513)
EXACT_D = (1, 15, 16, 17, 33)
# (nx, ny) of the full mode: the squares (1, 1, 1, 4, 9, 25 tiles) and two rectangles for 6 and 15 tiles; the symmetric mode
# launches 1, 1, 1, 3, 6, 15 tiles for EXACT_N.  9 is no triangular number: the full 257 x 257 case carries it.
FULL_SHAPES = tuple((n, n) for n in EXACT_N) + ((129, 257), (257, 513))
BIG_FULL, BIG_SYM, BIG_D = 2100, 2900, 5                 # 17 x 17 = 289 and 23 * 24 / 2 = 276 tiles: the strided loop of the reduce
POLY_COEF0 = (0, 1, -3)
POLY_DEGREES = (1, 2, 3, 4)
MOM_EXACT_N = (2, 3, 16, 17, 33, 1024, 1025, 2049, 16385, 20001)
MOM_EXACT_D = (1, 127, 128, 129, 1024)
SWEEP_N, SWEEP_D = 257, 5


def f32r(v):
    """the value a C float argument carries"""
    return float(F32(v))


def tiles_launched(nx, ny, symmetric):
    tx, ty = -(-nx // MT), -(-ny // MT)
    return tx * (tx + 1) // 2 if symmetric else tx * ty


def mom_split(n):
    """(splits, rows per slab) of smd_moments"""
    s = max(1, min(MAX_SPLITS, -(-n // SLAB)))
    return s, -(-n // s)


# ------------------------------------------------------------------------------------------------ lattices
def distinct_rows(n, d, seed):
    """n pairwise distinct integer rows (fp32): the first min(d, 8) coordinates are the digits of a drawn code in the smallest odd
    base b >= 5 with b^min(d, 8) >= n, centred; the others are drawn from {-2 .. 2}"""
    rng = np.random.default_rng(seed)
    k = min(d, 8)
    b = 5
    while b ** k < n:
        b += 2
    codes = rng.choice(b ** k, size=n, replace=False)
    x = rng.integers(-2, 3, (n, d)).astype(np.int64)
    for j in range(k):
        x[:, j] = (codes // b ** j) % b - b // 2
    assert len(np.unique(x, axis=0)) == n
    return x.astype(F32)


def assert_lattice(x, y):
    """integers, and every partial sum of g, of the norms and of (-2 g + |x|^2) + |y|^2 below 2^24 in magnitude"""
    x64, y64 = x.astype(F64), y.astype(F64)
    assert np.array_equal(x64, np.rint(x64)) and np.array_equal(y64, np.rint(y64))
    nx, ny = (x64 * x64).sum(1).max(), (y64 * y64).sum(1).max()
    g = (np.abs(x64) @ np.abs(y64).T).max()                 # bounds every partial sum of every chain
    assert max(nx, ny, g) < EXACT and 2 * g + nx + ny < EXACT


def zero_pairs(x, y):
    """the number of (i, j) with x_i = y_j, by integer arithmetic"""
    xi, yi = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
    d2 = (xi * xi).sum(1)[:, None] + (yi * yi).sum(1)[None, :] - 2 * (xi @ yi.T)
    assert d2.min() >= 0
    return int((d2 == 0).sum())


def _edge_rows(n):
    """rows on both sides of every tile edge, the ends and the middle"""
    return sorted({r for r in (0, 1, 2, 126, 127, 128, 129, 130, 255, 256, 257, n // 2, n - 3, n - 2, n - 1) if 0 <= r < n})


def dup_full(nx, ny, d, seed=0):
    """(x, y, expected count, planted (i, j)): distinct rows, then y_j = x_i at edge rows paired so that the duplicates sit in
    diagonal and off-diagonal tiles, on both sides of a tile edge and in the last ragged tile"""
    rows = distinct_rows(nx + ny, d, 1000 * seed + 7 * nx + 3 * ny + d)
    x, y = rows[:nx].copy(), rows[nx:].copy()
    ei, ej = _edge_rows(nx), _edge_rows(ny)
    ej = ej[len(ej) // 2:] + ej[:len(ej) // 2]                # rotate: row 0 meets the middle, the last rows meet the first tile
    planted = list(zip(ei, ej))
    for i, j in planted:
        y[j] = x[i]
    assert_lattice(x, y)
    assert zero_pairs(x, y) == len(planted)                   # pairwise distinct unless planted
    return x, y, float(len(planted)), planted


SYM_PAIRS = ((0, 1), (2, 127), (126, 128), (129, 130), (131, 255), (254, 256), (3, -1), (-3, -2), (5, 300), (140, 400))


def dup_symmetric(n, d, seed=0):
    """(x, expected count n + 2 planted, planted (i, j) with i < j): x_j = x_i for disjoint pairs in diagonal tiles ((0, 1), (129, 130)),
    off-diagonal tiles, across a tile edge ((126, 128), (254, 256)), at the edge inside a tile ((2, 127)) and in the last ragged tile"""
    x = distinct_rows(n, d, 1000 * seed + 11 * n + d)
    used, planted = set(), []
    for i, j in SYM_PAIRS:
        i, j = (i + n if i < 0 else i), (j + n if j < 0 else j)
        if 0 <= i < j < n and i not in used and j not in used:
            used.update((i, j))
            planted.append((i, j))
            x[j] = x[i]
    assert_lattice(x, x)
    assert zero_pairs(x, x) == n + 2 * len(planted)
    return x, float(n + 2 * len(planted)), planted


def sweep_rows():
    """the 257 distinct rows of the slot sweep (Y = roll(X, s): every row of X occurs once in Y, the count is 257 for every s)"""
    x = distinct_rows(SWEEP_N, SWEEP_D, 4711)
    assert_lattice(x, x)
    norms = (x.astype(F64) ** 2).sum(1)
    assert len(np.unique(norms)) > 4                          # a norm read from another slot is another number
    return x


def poly_nonzeros(d, degree, coef0):
    return max(1, min(d, (int(math.floor(2.0 ** (20.0 / degree))) - abs(coef0)) // 4))


def poly_rows(n, d, degree, coef0, seed):
    """n integer rows (fp32) with coordinates in {-2 .. 2}, at most poly_nonzeros of them non-zero"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (n, d))
    nz = poly_nonzeros(d, degree, coef0)
    if nz < d:
        keep = np.argsort(rng.random((n, d)), axis=1)[:, :nz]
        m = np.zeros((n, d), bool)
        np.put_along_axis(m, keep, True, 1)
        x = np.where(m, x, 0)
    return x.astype(F32)


def poly_exact(x, y, coef0, degree):
    """(the int64 sum of (g + coef0)^degree over all pairs as a float, whether a negative base occurs); asserts the preconditions"""
    assert_lattice(x, y)
    t = np.rint(x).astype(np.int64) @ np.rint(y).astype(np.int64).T + int(coef0)
    p = t ** degree
    assert np.abs(p).max() <= 2 ** 20                         # 16 of them sum exactly in fp32
    total = int(p.sum())
    assert abs(total) < 2 ** 53
    return float(total), bool((t < 0).any())


def poly_case(nx, ny, d, coef0, degree, symmetric, seed=0):
    s = 1000 * seed + 13 * nx + 5 * ny + 3 * d + 7 * degree + coef0
    x = poly_rows(nx, d, degree, coef0, s)
    y = x if symmetric else poly_rows(ny, d, degree, coef0, s + 1)
    return (x, y) + poly_exact(x, y, coef0, degree)


def moment_rows(n, d, seed=0):
    """integer rows in +- pairs with magnitudes in [512, 724] (one zero row for odd n), shuffled; asserts the 32-row condition"""
    rng = np.random.default_rng(1000 * seed + 17 * n + d)
    h = rng.integers(512, 725, (n // 2, d)) * rng.choice((-1, 1), (n // 2, d))
    x = np.concatenate([h, -h] + ([np.zeros((1, d), np.int64)] if n % 2 else []))
    x = x[rng.permutation(n)].astype(F32)
    assert 2 * BK * float(np.abs(x).max()) ** 2 < EXACT       # every 32-row fp32 sub-sum, wherever it starts
    assert not x.astype(F64).sum(0).any()
    return x


def moment_exact(x):
    x64 = x.astype(F64)
    s = x64.T @ x64                                           # integers below 2^53: exact in any order
    assert np.abs(x64).max() ** 2 * len(x) < 2 ** 53
    return s / (len(x) - 1)


# ------------------------------------------------------------------------------------------------ references and bounds
def pair_reference(x, y, same, gamma_rbf, gamma_poly, coef0, degree):
    """dict of the float64 sums (kernel_sums of _metrics_ref) and the derived limits: rbf, rbf_lo, rbf_hi (the sum must lie in
    [rbf_lo, rbf_hi]), poly, poly_bound, first_order_ok (where the first-order form times SECOND would have held), pairs"""
    gr, gp, c0 = f32r(gamma_rbf), f32r(gamma_poly), f32r(coef0)
    x64 = np.asarray(x, F64)
    y64 = x64 if same else np.asarray(y, F64)
    n, m, d = len(x64), len(y64), x64.shape[1]
    ref = kernel_sums(x64, y64, same, gr, gp, c0, degree)
    g = x64 @ y64.T
    d2 = np.maximum(-2.0 * g + (x64 * x64).sum(1)[:, None] + (y64 * y64).sum(1)[None, :], 0.0)
    if same:
        np.fill_diagonal(d2, 0.0)
    mb = pair_bound(d, x64, y64)
    if same:
        np.fill_diagonal(mb, 0.0)                             # set, not computed
    k = np.exp(-gr * d2)
    E = np.exp(np.minimum(2 * U * gr * (d2 + mb), 700.0)) * (1 + 2 * U) * (1 + 16 * U)
    lo = np.exp(-gr * (d2 + mb)) / E - FLT_MIN
    hi = np.exp(-gr * np.maximum(d2 - mb, 0.0)) * E + FLT_MIN
    f64 = n * m * 2.0 ** -53 * k.sum()
    assert abs(k.sum() - ref[0]) <= 1e-12 * ref[1]
    ag = np.abs(x64) @ np.abs(y64).T
    eg = (d + 1) * U * ag
    t = gp * g + c0
    dt = gp * eg + U * (np.abs(gp * g) + np.abs(t))
    at = np.abs(t)
    top = (at + dt) ** degree
    diff = dt * sum((at + dt) ** i * at ** (degree - 1 - i) for i in range(degree))       # (|t| + dt)^degree - |t|^degree, no cancellation
    pb = diff + (degree - 1 + 16) * U * top
    first = SECOND * degree * at ** (degree - 1) * dt + (degree - 1 + 16) * U * at ** degree
    return dict(rbf=ref[0], rbf_abs=ref[1], rbf_lo=lo.sum() - f64, rbf_hi=hi.sum() + f64, poly=ref[2], poly_abs=ref[3],
                poly_bound=pb.sum() + n * m * 2.0 ** -53 * ref[3], first_order_ok=bool((pb <= first * (1 + 1e-12)).all()),
                first_order_not_larger=bool((degree * at ** (degree - 1) * dt <= diff * (1 + 1e-12)).all()),
                pairs=n * m, min_abs_t=float(at.min()), max_dt=float(dt.max()))


def rbf_ratio(got, r):
    """signed distance of `got` from the reference in units of the room on that side: <= 1 inside [rbf_lo, rbf_hi]"""
    if not np.isfinite(got):
        return float("inf")
    room = (r["rbf_hi"] - r["rbf"]) if got >= r["rbf"] else (r["rbf"] - r["rbf_lo"])
    err = abs(got - r["rbf"])
    return err / room if room > 0 else (0.0 if err == 0 else float("inf"))


def poly_ratio(got, r):
    return worst_ratio(np.array([got]), np.array([r["poly"]]), np.array([r["poly_bound"]]))


def column_means(x64):
    """correctly rounded column means (math.fsum): the reference must not carry a summation error of its own"""
    return np.array([math.fsum(x64[:, c]) for c in range(x64.shape[1])]) / len(x64)


def moments_reference(x):
    """(mean, cov, mean bound [d], cov bound [d][d]) in float64"""
    x64 = np.asarray(x, F64)
    n = len(x64)
    mean = column_means(x64)
    xc = x64 - mean
    cov = xc.T @ xc / (n - 1)
    dm = n * 2.0 ** -53 * np.abs(x64).mean(0)
    a = np.abs(xc)
    e = dm + U * (a + dm)
    prop = a.T @ e + e.T @ a + e.T @ e
    prod = (a + e).T @ (a + e)
    bound = (prop + (2 * BK * U + (n / 32 + 18) * 2.0 ** -53) * prod) / (n - 1) + 2.0 ** -52 * np.abs(cov)
    return mean, cov, dm, bound


def mmd_reference(x, y, gamma_rbf=1.0, degree=2, gamma_poly=1.0, coef0=0.0):
    """float64 (mmd_rbf, mmd_polynomial) of the biased estimator and their composed limits: (rbf, rbf_lo, rbf_hi, poly, poly_bound)"""
    n, m = len(x), len(y)
    xx = pair_reference(x, x, True, gamma_rbf, gamma_poly, coef0, degree)
    yy = pair_reference(y, y, True, gamma_rbf, gamma_poly, coef0, degree)
    xy = pair_reference(x, y, False, gamma_rbf, gamma_poly, coef0, degree)
    f = lambda a, b, c: a / (n * n) + b / (m * m) - 2.0 * c / (n * m)
    return dict(rbf=f(xx["rbf"], yy["rbf"], xy["rbf"]), rbf_lo=f(xx["rbf_lo"], yy["rbf_lo"], xy["rbf_hi"]),
                rbf_hi=f(xx["rbf_hi"], yy["rbf_hi"], xy["rbf_lo"]), poly=f(xx["poly"], yy["poly"], xy["poly"]),
                poly_bound=xx["poly_bound"] / (n * n) + yy["poly_bound"] / (m * m) + 2.0 * xy["poly_bound"] / (n * m),
                rbf_unit=xx["rbf_abs"] / (n * n) + yy["rbf_abs"] / (m * m) + 2.0 * xy["rbf_abs"] / (n * m),
                poly_unit=xx["poly_abs"] / (n * n) + yy["poly_abs"] / (m * m) + 2.0 * xy["poly_abs"] / (n * m))


# ------------------------------------------------------------------------------------------------ regimes
PAIR_REGIMES = ("latent", "clamp", "saturate", "flat", "poly_cancel", "poly_neg")
PAIR_SHAPES = ((300, 257, 5), (300, 257, 42), (257, 300, 146), (300, 300, 512))      # (nx, ny, d); the symmetric mode uses nx
MOM_REGIMES = ("offset", "collapsed", "mixed")
MOM_SHAPES = tuple((n, d) for n in (33, 1025, 4097) for d in (42, 129))
CONST_COL, CONST_VALUE = 1, 3.3

_CACHE = {}


def clamp_gamma(d):
    """about one over the fp32 spacing at |x|^2 = 9 d: the rounding noise of the raw d2 is then of order 1 in the exponent"""
    return f32r(0.5 / (9.0 * d * U))


def pair_regime(name, nx, ny, d, seed=0):
    """dict(x, y, params): fp32 rows and the (gamma_rbf, gamma_poly, coef0, degree) launches of the regime; shared, never modified"""
    key = ("pair", name, nx, ny, d, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(100 * seed + 7 * nx + 3 * ny + d + sum(map(ord, name)))
    latent = lambda n: np.clip(0.25 * rng.standard_normal((n, d)), -1, 1)
    if name == "latent":
        x, y, params = latent(nx), latent(ny), [(1.0, 1.0, 0.0, 2), (1.0 / d, 1.0 / d, 1.0, 3)]
    elif name == "clamp":                  # near-duplicates of (3, .., 3): d2 ~ 2 d 1e-8 is far below the spacing of |x|^2 = 9 d
        x, y = 3.0 + 1e-4 * rng.standard_normal((nx, d)), 3.0 + 1e-4 * rng.standard_normal((ny, d))
        params = [(clamp_gamma(d), 1.0 / d, 0.0, 2), (1.0, 1.0 / d, -9.0, 2)]
    elif name == "saturate":               # gamma d2 ~ 50 * 2 d / 16 >> 87.3: all but the closest pairs are below FLT_MIN
        x, y, params = latent(nx), latent(ny), [(50.0, 1.0, 0.0, 2)]
    elif name == "flat":
        x, y, params = latent(nx), latent(ny), [(1e-12, 1.0, 1.0, 1)]
    elif name == "poly_cancel":            # <x, y> = 1 + O(1e-3) and coef0 = -1: t is what is left of the cancellation
        u = np.ones(d) / math.sqrt(d)
        x, y = u + 1e-3 / math.sqrt(d) * rng.standard_normal((nx, d)), u + 1e-3 / math.sqrt(d) * rng.standard_normal((ny, d))
        params = [(1.0, 1.0, -1.0, 2), (1.0, 1.0, -1.0, 3), (1.0, 2.0, -2.0, 1)]
    elif name == "poly_neg":               # t = <x, y> - 1 with |<x, y>| mostly below 1: negative bases at odd degrees
        x, y, params = latent(nx), latent(ny), [(1.0, 1.0, -1.0, 3), (1.0, 1.0, -1.0, 5)]
    else:
        raise KeyError(name)
    _CACHE[key] = dict(x=x.astype(F32), y=y.astype(F32), params=[tuple(f32r(v) for v in p[:3]) + (p[3],) for p in params])
    return _CACHE[key]


def moments_regime(name, n, d, seed=0):
    """fp32 (n, d): column CONST_COL is constant in every regime"""
    key = ("mom", name, n, d, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(100 * seed + 7 * n + d + sum(map(ord, name)))
    z = rng.standard_normal((n, d))
    offset = 100.0 + 1e-3 * z
    collapsed = z * np.geomspace(1.0, 1e-4, d)
    if name == "offset":
        x = offset
    elif name == "collapsed":
        x = collapsed
    elif name == "mixed":                  # offset | tiny spread | latent | large spread, side by side
        kinds = np.arange(d) % 4
        x = np.where(kinds == 0, offset, np.where(kinds == 1, 1e-4 * z, np.where(kinds == 2, np.clip(0.25 * z, -1, 1), 1e4 * z)))
    else:
        raise KeyError(name)
    x = x.astype(F32)
    if d > CONST_COL:
        x[:, CONST_COL] = F32(CONST_VALUE)
    _CACHE[key] = x
    return x


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
PAIR_FAULTS = ("no-clamp", "diagonal-not-zeroed", "mirror-weight-1", "padded-row-counted", "tile-dropped", "tile-twice",
               "neighbour-tile-norms")
MOM_FAULTS = ("fp32-mean", "one-pass", "slab-fp32", "n-not-n-1")


def fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)     # a b is exact in float64: one rounding


def gram32(x, y):
    """<x_i, y_j> as one fp32 fma chain in k order"""
    acc = np.zeros((len(x), len(y)), F32)
    for k in range(x.shape[1]):
        acc = fma32(x[:, k, None], y[None, :, k], acc)
    return acc


def norms32(x):
    s = np.zeros(len(x), F32)
    for k in range(x.shape[1]):
        s = fma32(x[:, k], x[:, k], s)
    return s


def raw_d2_32(x, y):
    """(-2 g + |x|^2) + |y|^2 in fp32, in front of the clamp"""
    return (F32(-2.0) * gram32(x, y) + norms32(x)[:, None]) + norms32(y)[None, :]


def expf32(a):
    """__expf: exp2(fl(a log2e)), results below FLT_MIN flushed"""
    r = np.exp2((a.astype(F32) * LOG2E32).astype(F64)).astype(F32)
    return np.where(r < F32(FLT_MIN), F32(0), r)


def powi32(t, degree):
    p = t
    for _ in range(1, degree):
        p = p * t
    return p


def tile_sums(v):
    """fp64 [tiles x][tiles y]: the values of each lane's 16 accumulator registers (column lane & 31, rows (r & 3) + 8 (r >> 2)
    + 4 (lane >> 5) of a 32 x 32 MFMA tile) added in fp32 in register order, everything else in fp64.  Masked entries are 0."""
    n, m = v.shape
    tx, ty = -(-n // MT), -(-m // MT)
    p = np.zeros((tx * MT, ty * MT), F32)
    p[:n, :m] = v
    a = p.reshape(tx, 4, 4, 2, 4, ty * MT).transpose(0, 1, 3, 2, 4, 5).reshape(tx, 4, 2, 16, ty * MT)
    s = np.zeros((tx, 4, 2, ty * MT), F32)
    for r in range(16):
        s = s + a[:, :, :, r, :]
    return s.astype(F64).sum((1, 2)).reshape(tx, ty, MT).sum(2)


_CHAINS = {}


def _chains(x, y):
    """(g, |x|^2, |y|^2) of gram32 / norms32, kept per pair of input arrays (the regimes' arrays are shared and never modified)"""
    key = (id(x), id(y))
    if key not in _CHAINS:
        if len(_CHAINS) > 16:
            _CHAINS.clear()
        _CHAINS[key] = (x, y, gram32(x, y), norms32(x), norms32(y))
    return _CHAINS[key][2:]


def emu_pair_sums(x, y, symmetric, gamma_rbf, gamma_poly, coef0, degree, fault=None, tile=(0, 0)):
    """[sum rbf, sum poly] as pair_sums_kernel forms them; `fault` plants one of PAIR_FAULTS, `tile` = (bi, bj) is where the
    tile faults strike"""
    x = np.asarray(x, F32)
    y = x if symmetric else np.asarray(y, F32)
    if fault == "padded-row-counted":                          # the zero row behind the last row of x passes the mask
        assert not symmetric and len(x) % MT
        x = np.concatenate([x, np.zeros((1, x.shape[1]), F32)])
    n, m = len(x), len(y)
    g, na, nb = _chains(x, y)
    NA =np.broadcast_to(na[:, None], (n, m)).copy()
    bi, bj = tile
    rows, cols = slice(bi * MT, min((bi + 1) * MT, n)), slice(bj * MT, min((bj + 1) * MT, m))
    if fault == "neighbour-tile-norms":                        # na[] of this tile filled from the next tile's rows
        nxt = np.zeros(MT, F32)
        src = na[(bi + 1) * MT:(bi + 2) * MT]
        nxt[:len(src)] = src
        NA[rows, cols] = nxt[:rows.stop - rows.start, None]
    d2 = (F32(-2.0) * g + NA) + nb[None, :]
    if fault != "no-clamp":
        d2 = np.maximum(d2, F32(0))
    if symmetric and fault != "diagonal-not-zeroed":
        np.fill_diagonal(d2, F32(0))
    kr = expf32(F32(-gamma_rbf) * d2)
    kp = powi32(fma32(F32(gamma_poly), g, F32(coef0)), degree)
    tr, tp = tile_sums(kr), tile_sums(kp)
    w = np.ones(tr.shape)
    if symmetric:
        w = np.triu(np.full(tr.shape, 1.0 if fault == "mirror-weight-1" else 2.0), 1) + np.eye(len(tr))
    if fault == "tile-dropped":
        w[bi, bj] = 0.0
    if fault == "tile-twice":
        w[bi, bj] *= 2.0
    return np.array([(w * tr).sum(), (w * tp).sum()])


def emu_moments(x, fault=None):
    """(mean, cov) as smd_moments forms them; `fault` plants one of MOM_FAULTS"""
    x = np.asarray(x, F32)
    n, d = x.shape
    splits, slab = mom_split(n)
    x64 = x.astype(F64)
    if fault == "fp32-mean":
        mean = (np.cumsum(x, axis=0, dtype=F32)[-1] / F32(n)).astype(F64)
    else:
        part = [np.cumsum(x64[s * slab:min(n, (s + 1) * slab)], axis=0)[-1] for s in range(splits) if s * slab < n]
        mean = np.cumsum(np.array(part), axis=0)[-1] / n
    xc = x if fault == "one-pass" else (x64 - mean).astype(F32)
    tot = np.zeros((d, d))
    for s in range(splits):
        r0, r1 = s * slab, min(n, (s + 1) * slab)
        acc64, acc = np.zeros((d, d)), np.zeros((d, d), F32)
        for r in range(r0, r1):
            acc = fma32(xc[r, :, None], xc[r, None, :], acc)
            last = r + 1 == r1
            if last or (fault != "slab-fp32" and (r + 1 - r0) % (2 * BK) == 0):
                acc64 += acc.astype(F64)
                acc = np.zeros((d, d), F32)
        tot += acc64
    if fault == "one-pass":
        tot = tot - n * np.outer(mean, mean)
    return mean, tot / (n if fault == "n-not-n-1" else n - 1)
