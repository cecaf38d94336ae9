"""float64 numpy restatement (brute force) of the k-means metrics as DESIGN.md section 15 fixes them: nearest-centre labels,
cluster means, the PRD curve (Sajjadi et al. 2018) with its F-beta summary and the NDB score (Richardson & Weiss 2018), with the
fp32 error model the GPU tests hold the kernels to."""
import numpy as np

Z95 = 1.959963984540054
U24 = 2.0 ** -24


def scores(x, c):
    """s[i, j] = -2 <x_i, c_j> + |c_j|^2 in float64: |x_i - c_j|^2 without the |x_i|^2 every j shares"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)


def pair_error(x, c):
    """e[i, j] = (d + 4) 2^-24 (2 |x_i| |c_j| + |c_j|^2): the most an fp32 s_ij differs from the exact one -- a length-d fma
    chain for the dot product (d 2^-24 |x_i| |c_j|, doubled), one chain for |c_j|^2 (d 2^-24 |c_j|^2) and one rounding of the
    add, to first order with room to spare"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    nx, nc = np.sqrt((x * x).sum(1)), np.sqrt((c * c).sum(1))
    return (x.shape[1] + 4) * U24 * (2.0 * nx[:, None] * nc[None, :] + (nc * nc)[None, :])


def labels_certain(x, c):
    """(labels, certain, s, e): the float64 arg min (ties to the lowest j) and the rows fp32 arithmetic cannot relabel: the
    float64 gap from the best centre to every other j exceeds e_i,best + e_ij"""
    s, e = scores(x, c), pair_error(x, c)
    lab = s.argmin(1)
    rows = np.arange(len(lab))
    gap = s - s[rows, lab][:, None]
    need = e + e[rows, lab][:, None]
    gap[rows, lab] = np.inf
    return lab, (gap > need).all(1), s, e


def min_d2(x, s, lab):
    """max(s_i,label + |x_i|^2, 0) in float64 for the given labels"""
    x = np.asarray(x, np.float64)
    return np.maximum(s[np.arange(len(lab)), lab] + (x * x).sum(1), 0.0)


def min_d2_bound(x, e, lab):
    """e_i,label + (d + 4) 2^-24 |x_i|^2: the error of s, the chain of |x_i|^2 and the rounding of the last add"""
    x = np.asarray(x, np.float64)
    return e[np.arange(len(lab)), lab] + (x.shape[1] + 4) * U24 * (x * x).sum(1)


def means(x, lab, prev):
    """(centres, counts): the float64 mean of every label's rows; a label without rows keeps its row of ``prev``"""
    x, prev = np.asarray(x, np.float64), np.asarray(prev, np.float64)
    k = len(prev)
    counts = np.bincount(lab, minlength=k)
    sums = np.zeros((k, x.shape[1]))
    np.add.at(sums, lab, x)
    out = prev.copy()
    out[counts > 0] = sums[counts > 0] / counts[counts > 0, None]
    return out, counts


def mean_bound(x, centres, counts):
    """2^-24 |c| + n_c 2^-52 max|x| per element: fp64 accumulation of fp32 values in any order ((n_c - 1) 2^-53 sum |x| for the
    sum, over n_c), the division and the rounding to fp32"""
    return U24 * np.abs(centres) + counts[:, None] * 2.0 ** -52 * np.abs(np.asarray(x, np.float64)).max()


def lloyd(x, c, iters):
    for _ in range(iters):
        c = means(x, scores(x, c).argmin(1), c)[0]
    return c


def histogram(lab, k):
    return np.bincount(np.asarray(lab), minlength=k).astype(np.float64) / len(lab)


def prd_curve(ref, ev, num_angles=1001, epsilon=1e-10):
    ref, ev = np.asarray(ref, np.float64), np.asarray(ev, np.float64)
    slopes = np.tan(np.linspace(epsilon, np.pi / 2 - epsilon, num_angles))
    precision = np.array([np.minimum(ref * t, ev).sum() for t in slopes])
    return np.clip(precision, 0.0, 1.0), np.clip(precision / slopes, 0.0, 1.0)


def f_beta(prd, beta=8.0, epsilon=1e-10):
    p, r = prd
    f = lambda b: ((1 + b * b) * p * r / (b * b * p + r + epsilon)).max()
    return float(f(beta)), float(f(1.0 / beta))


def ndb_z(p_r, p_s, n_r, n_s):
    """(z, se) per bin of the pooled two-proportion test; z is 0 where se is 0"""
    p_r, p_s = np.asarray(p_r, np.float64), np.asarray(p_s, np.float64)
    pooled = (n_r * p_r + n_s * p_s) / (n_r + n_s)
    se = np.sqrt(pooled * (1 - pooled) * (1 / n_r + 1 / n_s))
    return np.where(se > 0, np.abs(p_r - p_s) / np.where(se > 0, se, 1.0), 0.0), se


def ndb(p_r, p_s, n_r, n_s):
    z, se = ndb_z(p_r, p_s, n_r, n_s)
    return float(((se > 0) & (z > Z95)).sum()) / len(z)


# ---- the two input families of the GPU tests
def gaussian(rng, n, d):
    return np.clip(0.25 * rng.standard_normal((n, d)), -1, 1).astype(np.float32)


def mixture(rng, n, d, k):
    mu = np.clip(0.5 * rng.standard_normal((k, d)), -1, 1)
    return np.clip(mu[rng.integers(0, k, n)] + 0.1 * rng.standard_normal((n, d)), -1, 1).astype(np.float32)


def make_centres(rng, x, k):
    """three float64 Lloyd iterations from k seeded data rows, rounded to fp32"""
    return lloyd(x, np.asarray(x, np.float64)[rng.choice(len(x), k, replace=False)], 3).astype(np.float32)
