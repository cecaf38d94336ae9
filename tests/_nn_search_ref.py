"""float64 numpy restatement (brute force) of the nearest-neighbour search and the copy metrics as DESIGN.md section 24 fixes
them.  Sets are (n, d) rows; every distance is Euclidean and kept squared; neighbours are ordered by (d2, global index)."""
import numpy as np

from _nn_metrics_ref import sqdist


def pair_bound(d, q, x):
    """m[j, i] = (d + 4) 2^-24 (|q_j| + |x_i|)^2: the most the fp32 d2 of that pair differs from the exact one (section 14)"""
    nq, nx = (np.sqrt((np.asarray(v, np.float64) ** 2).sum(1)) for v in (q, x))
    return (d + 4) * 2.0 ** -24 * (nq[:, None] + nx[None, :]) ** 2


def nn_search(q, x, k=1, q_base=0, x_base=0, exclude_self=False, dqx=None):
    """(d2 (nq, k), idx (nq, k) int64, gap (nq,)): per query the k candidates with the smallest (d2, x_base + i), ascending, the
    tail (+inf, -1) where fewer exist; gap = the (k+1)-th smallest d2 minus the k-th (+inf where there is no (k+1)-th).  The
    pair with q_base + j == x_base + i is left out with ``exclude_self``."""
    d = np.array(sqdist(q, x) if dqx is None else dqx, np.float64)
    nq, nx = d.shape
    if exclude_self:
        j = np.arange(nq) + q_base - x_base
        ok = (j >= 0) & (j < nx)
        d[np.arange(nq)[ok], j[ok]] = np.inf
    order = np.argsort(d, axis=1, kind="stable")                 # stable: equal d2 stay in index order
    srt = np.take_along_axis(d, order, 1)
    pad = max(k + 1 - nx, 0)
    srt = np.concatenate([srt, np.full((nq, pad), np.inf)], 1)
    order = np.concatenate([order, np.full((nq, pad), -1)], 1)
    d2, idx = srt[:, :k].copy(), order[:, :k].astype(np.int64)
    idx = np.where(np.isfinite(d2), idx + x_base, -1)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(srt[:, k]), srt[:, k] - srt[:, k - 1], np.inf)
    return d2, idx, gap


def r1_sq(train, dxx=None):
    """every training row's squared distance to its nearest OTHER training row (self excluded by index), and that row"""
    d2, idx, _ = nn_search(train, train, 1, exclude_self=True, dqx=dxx)
    return d2[:, 0], idx[:, 0]


def authenticity(train, fake=None):
    """(score, per-row flags, per-row margin d2(q, x_i*) - r1_sq[i*]): Alaa et al. 2022 -- q is authentic when it is no closer to
    its nearest training row i* than i* is to its nearest other training row; the boundary counts as authentic.  fake None: the
    training set against itself, pair (i, i) excluded -- the leave-one-out score."""
    r1, _ = r1_sq(train)
    if fake is None:
        d2, idx, _ = nn_search(train, train, 1, exclude_self=True)
    else:
        d2, idx, _ = nn_search(fake, train, 1)
    margin = d2[:, 0] - r1[idx[:, 0]]
    return float((margin >= 0).mean()), margin >= 0, margin


def copy_report(train, held_out, fake, k=1):
    """the float64 copy report: authenticity, median_nn_fake, median_nn_held_out (distances, not squared), copy_gap, exact_copies
    (fake rows whose nearest d2 is at most the fp32 bound of that pair), nn_d2, nn_idx"""
    train = np.asarray(train, np.float64)
    same = fake is None
    q = train if same else np.asarray(fake, np.float64)
    d2, idx, _ = nn_search(q, train, k, exclude_self=same)
    dh = nn_search(held_out, train, 1)[0]
    r1, _ = r1_sq(train)
    m = pair_bound(train.shape[1], q, train)[np.arange(len(q)), idx[:, 0]]
    mf, mh = float(np.median(np.sqrt(d2[:, 0]))), float(np.median(np.sqrt(dh[:, 0])))
    return {"authenticity": float((d2[:, 0] >= r1[idx[:, 0]]).mean()), "median_nn_fake": mf, "median_nn_held_out": mh,
            "copy_gap": mf / mh if mh > 0 else (np.inf if mf > 0 else np.nan), "exact_copies": int((d2[:, 0] <= m).sum()),
            "nn_d2": d2, "nn_idx": idx}
