"""float64 numpy restatement of the reference's distance metrics for the metrics tests.

utils/metrics.py:24-77 of the reference, with the sklearn 0.19 kernels it calls (pinned by requirements.txt:190):
  euclidean_distances  sklearn/metrics/pairwise.py (0.19): XX = row_norms(X, squared=True)[:, None], YY likewise [None, :],
                       D = -2 X Y^T; D += XX; D += YY; np.maximum(D, 0, out=D); D.flat[::n + 1] = 0 when X is Y
  rbf_kernel           K = euclidean_distances(X, Y, squared=True); K *= -gamma; np.exp(K, K)
  polynomial_kernel    K = X Y^T; K *= gamma; K += coef0; K **= degree
  mmd_rbf / mmd_polynomial (metrics.py:57-77)  XX.mean() + YY.mean() - 2 XY.mean()
  frechet_distance (metrics.py:24-54)          |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2), np.cov ddof = 1
The sums are taken over row chunks so that no full N x N matrix is held.
"""
import numpy as np

CHUNK = 1024


def kernel_sums(x, y, same, gamma_rbf, gamma_poly, coef0, degree):
    """(sum K_rbf, sum |K_rbf|, sum K_poly, sum |K_poly|) in float64 over all pairs of x (n, d) and y (m, d)."""
    x = np.asarray(x, np.float64)
    y = x if same else np.asarray(y, np.float64)
    yy = (y * y).sum(1)[None, :]
    out = np.zeros(4)
    for i0 in range(0, len(x), CHUNK):
        xc = x[i0:i0 + CHUNK]
        g = xc @ y.T
        dist = -2.0 * g
        dist += (xc * xc).sum(1)[:, None]
        dist += yy
        np.maximum(dist, 0, out=dist)
        if same:
            r = np.arange(len(xc))
            dist[r, i0 + r] = 0.0
        kr = np.exp(-gamma_rbf * dist)
        kp = (gamma_poly * g + coef0) ** degree
        out += (kr.sum(), np.abs(kr).sum(), kp.sum(), np.abs(kp).sum())
    return out


def mmds(x, y, gamma_rbf=1.0, degree=2, gamma_poly=1.0, coef0=0.0):
    """(mmd_rbf, mmd_polynomial, scale_rbf, scale_poly): scale = mean|Kxx| + mean|Kyy| + 2 mean|Kxy| (the tolerance unit)."""
    same = y is x
    nx, ny = len(x), len(y)
    kxx = kernel_sums(x, x, True, gamma_rbf, gamma_poly, coef0, degree) / (nx * nx)
    kyy = kxx if same else kernel_sums(y, y, True, gamma_rbf, gamma_poly, coef0, degree) / (ny * ny)
    kxy = kxx if same else kernel_sums(x, y, False, gamma_rbf, gamma_poly, coef0, degree) / (nx * ny)
    m = kxx + kyy - 2 * kxy
    s = kxx + kyy + 2 * kxy
    return m[0], m[2], s[1], s[3]


def trace_sqrt_product_eig(s1, s2):
    """tr sqrtm(S1 S2) for PSD S1, S2 as sum sqrt(max(eig(S1^1/2 S2 S1^1/2), 0))."""
    w, v = np.linalg.eigh(s1)
    r = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    m = r @ s2 @ r
    return np.sqrt(np.clip(np.linalg.eigvalsh((m + m.T) / 2), 0, None)).sum()


def frechet(x, y, use_scipy=True):
    """(frechet distance, tolerance unit tr S1 + tr S2 + |dmu|^2).  scipy.linalg.sqrtm when scipy imports and n > d, as the
    reference; otherwise the eigen form (the reference's fallback branch would raise NameError: eps is undefined)."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    mu1, s1 = x.mean(0), np.cov(x, rowvar=False)
    mu2, s2 = y.mean(0), np.cov(y, rowvar=False)
    s1, s2 = np.atleast_2d(s1), np.atleast_2d(s2)
    diff = mu1 - mu2
    tr = None
    if use_scipy and len(x) > x.shape[1] and len(y) > y.shape[1]:
        try:
            import scipy.linalg
            covmean, _ = scipy.linalg.sqrtm(s1.dot(s2), disp=False)
            if np.isfinite(covmean).all():
                tr = np.trace(covmean).real
        except ImportError:
            pass
    if tr is None:
        tr = trace_sqrt_product_eig(s1, s2)
    fd = diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * tr
    return fd, np.trace(s1) + np.trace(s2) + diff.dot(diff)
