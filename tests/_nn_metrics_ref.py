"""float64 numpy restatement (brute force) of the nearest-neighbour metrics as DESIGN.md section 14 fixes them: improved
precision / recall (Kynkaanniemi et al. 2019), their F1 and the realism score.  Sets are (n, d) rows; every distance is
Euclidean and kept squared."""
import numpy as np

FLT_MIN = 2.0 ** -126


def sqdist(a, b=None):
    """D[i, j] = |a_i - b_j|^2 in float64, clamped at 0.  b None: a against itself, exactly symmetric with a zero diagonal, so
    the pair (i, j) has ONE value whichever row it is seen from (a row that is the k-th neighbour of j lies on j's sphere)."""
    a = np.asarray(a, np.float64)
    na = (a * a).sum(1)
    if b is None:
        d = np.maximum(na[:, None] + na[None, :] - 2.0 * (a @ a.T), 0.0)
        d = (d + d.T) / 2
        np.fill_diagonal(d, 0.0)
        return d
    b = np.asarray(b, np.float64)
    return np.maximum(na[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T), 0.0)


def knn_radii2(x, k=3, dxx=None):
    """r2[i]: the squared distance from row i to its k-th nearest OTHER row (self excluded by index: a duplicate gives 0)"""
    d = np.array(sqdist(x) if dxx is None else dxx, np.float64)
    assert 1 <= k <= d.shape[0] - 1
    np.fill_diagonal(d, np.inf)
    return np.partition(d, k - 1, axis=1)[:, k - 1]


def cover_margin(dqx, r2, exclude_diagonal=False):
    """s_q = max_j (r2_j - |q - x_j|^2) from D[q, j]: q is covered iff s_q >= 0"""
    s = r2[None, :] - dqx
    if exclude_diagonal:
        s = s.copy()
        np.fill_diagonal(s, -np.inf)
    return s.max(1)


def keep_mask(r2):
    """rows whose radius is at most numpy.median of the radii (the paper's pruning of the largest spheres)"""
    r = np.sqrt(np.asarray(r2, np.float64))
    return r <= np.median(r)


def realism2(dqx, r2, keep=None, exclude_diagonal=False):
    """max over the kept j of r2_j / max(D[q, j], FLT_MIN): the squared realism score of every query"""
    ratio = r2[None, :] / np.maximum(dqx, FLT_MIN)
    if keep is not None:
        ratio = np.where(np.asarray(keep, bool)[None, :], ratio, 0.0)
    if exclude_diagonal:
        np.fill_diagonal(ratio, 0.0)
    return ratio.max(1)


def f1_score(p, r):
    return 2.0 * p * r / (p + r) if p + r > 0 else 0.0


def metrics(real, fake=None, k=3):
    """dict of improved_precision, improved_recall, improved_f1, ipr_realism (+ the per-row realism scores).  fake None: the
    real set against itself, pair (i, i) excluded -- the leave-one-out scores."""
    if fake is None:
        d = sqdist(real)
        r2 = knn_radii2(real, k, d)
        p = r = float((cover_margin(d, r2, True) >= 0).mean())
        scores = np.sqrt(realism2(d, r2, keep_mask(r2), True))
    else:
        dyx = sqdist(fake, real)
        r2x, r2y = knn_radii2(real, k), knn_radii2(fake, k)
        p = float((cover_margin(dyx, r2x) >= 0).mean())
        r = float((cover_margin(dyx.T, r2y) >= 0).mean())
        scores = np.sqrt(realism2(dyx, r2x, keep_mask(r2x)))
    return {"improved_precision": p, "improved_recall": r, "improved_f1": f1_score(p, r), "ipr_realism": float(scores.mean()),
            "realism_scores": scores}


def d2_error_bound(d, a, b):
    """m = (d + 4) 2^-24 (|a|max + |b|max)^2: the most an fp32 d2 = (-2 <x,y> + |x|^2) + |y|^2 of a pair differs from the exact one"""
    na, nb = (float(np.sqrt((np.asarray(v, np.float64) ** 2).sum(1).max())) for v in (a, b))
    return (d + 4) * 2.0 ** -24 * (na + nb) ** 2


def loo_certain(dxx, r2, k, m):
    """Identity case: the rows whose leave-one-out coverage fp32 arithmetic with per-pair error m cannot change.  Either
    |s_q| > 2m, or q is the k-th neighbour of some j whose k-th distance is more than 2m away from its (k-1)-th and (k+1)-th:
    the d2 of a pair has one value from either side, so q lies exactly on j's sphere and is covered.  Returns (s, certain)."""
    n = len(r2)
    s = cover_margin(dxx, r2, exclude_diagonal=True)
    dn = np.array(dxx, np.float64)
    np.fill_diagonal(dn, np.inf)
    order = np.argsort(dn, axis=1)[:, :k + 1]
    srt = np.take_along_axis(dn, order, 1)
    below = srt[:, k - 1] - srt[:, k - 2] if k > 1 else np.full(n, np.inf)
    above = srt[:, k] - srt[:, k - 1] if k < n - 1 else np.full(n, np.inf)
    on_sphere = np.zeros(n, bool)
    on_sphere[order[np.minimum(below, above) > 2 * m, k - 1]] = True
    return s, (np.abs(s) > 2 * m) | on_sphere
