"""float64 restatement of the third-order exponential Adams sampler (predictor, and predictor with the free corrector) for the
Adams tests.  Written from DESIGN.md section 29, independently of smd_amd/schedule.py: two explicit stages and no folding.

With alpha = sqrt(ap), sigma = sqrt(1 - ap), lambda = log(alpha / sigma), t = taus[j] -> s = taus[j + 1], the exact solution is
  x_s = (sigma_s / sigma_t) x_t + alpha_s Int_{lambda_t}^{lambda_s} e^(l - lambda_s) x0(l) dl
and x0(l) is replaced by its Lagrange interpolant on a few lambdas where the network was evaluated.  The weights
W_i = Int_a^b e^(l - lambda_b) L_i(l) dl are taken here by Gauss-Legendre quadrature with 48 points, which integrates
e^u times a quadratic over an interval of a few units of lambda to rounding; the shipped closed forms are tested against it.
  predictor   nodes lambda of taus[j], taus[j-1], taus[j-2] (min(3, j + 1) of them), interval [lambda_t, lambda_s]
  corrector   (j >= 1, before predicting) the previous step u -> t redone on the nodes lambda_t, lambda_u, lambda_u':
              x_t^c = x_t + alpha_t (sum_i wc_i [x0_t, x0_u, x0_u'] - sum_i wp'_i [x0_u, x0_u', x0_u'']),  wp' = that step's weights
ap is the float32 cumulative product promoted; the last iteration takes ap_s = 1, is first order and returns x0.
"""
import numpy as np
import torch

from _strided_ref import alphas_prod, norm_metric, slots  # noqa: F401
from _multistep_ref import lambdas, logsnr_timesteps  # noqa: F401

_GL_X, _GL_W = np.polynomial.legendre.leggauss(48)


def quad_weights(lam_a, lam_b, nodes):
    """W_i by Gauss-Legendre quadrature of e^(l - lam_b) L_i(l) over [lam_a, lam_b]"""
    nodes = np.asarray(nodes, dtype=np.float64)
    half = 0.5 * (lam_b - lam_a)
    l = lam_a + half * (_GL_X + 1.0)
    w = half * _GL_W * np.exp(l - lam_b)
    out = np.empty(len(nodes))
    for i in range(len(nodes)):
        L = np.ones_like(l)
        for m in range(len(nodes)):
            if m != i:
                L = L * (l - nodes[m]) / (nodes[i] - nodes[m])
        out[i] = np.sum(w * L)
    return out


def coefficients(betas, taus, clip=1.0):
    """float64 per-iteration quantities of the descending walk: dict of arrays of len(taus); wp / wc are [n][3], zero where a
    node is missing, and wc is zero on the first and on the last iteration"""
    ap = alphas_prod(betas)
    lam_all = lambdas(betas)
    t = np.asarray(taus)
    n = len(t)
    lam = lam_all[t]
    at = ap[t]
    as_ = np.append(ap[t[1:]], 1.0)
    wp, wc = np.zeros((n, 3)), np.zeros((n, 3))
    for j in range(n):
        q = min(3, j + 1)
        nodes = [lam[j - i] for i in range(q)]
        if j == n - 1:
            wp[j, 0] = 1.0
            continue
        wp[j, :q] = quad_weights(lam[j], lam[j + 1], nodes)
        if j >= 1:
            wc[j, :q] = quad_weights(lam[j - 1], lam[j], nodes)
    return dict(t=t, next_t=np.append(t[1:], -1), sqrt_recip=1 / np.sqrt(at), sqrt_m1=np.sqrt(1 - at) / np.sqrt(at),
                ratio=np.sqrt(1 - as_) / np.sqrt(1 - at), alpha_t=np.sqrt(at), alpha_s=np.sqrt(as_), wp=wp, wc=wc,
                sqrt_as=np.sqrt(as_), sqrt_1m_as=np.sqrt(1 - as_), ap_t=at, sqrt_ap_t=np.sqrt(at), clip=np.full(n, float(clip)))


def _scalars(co, j, dt):
    row = {}
    for k, v in co.items():
        if k in ("t", "next_t"):
            row[k] = int(v[j])
        elif np.ndim(v[j]) == 0:
            row[k] = torch.tensor(float(v[j]), dtype=torch.float64).to(dt)
        else:
            row[k] = torch.tensor(np.asarray(v[j], dtype=np.float64)).to(dt)
    return row


def _blend(nx, row, T, masks, samples, iz):
    if masks is None:
        return nx, None
    y = row["sqrt_as"] * samples + row["sqrt_1m_as"] * iz if 0 <= row["next_t"] < T else samples
    return nx * (1 - masks) + y * masks, y


def walk(model, co, init, T, corrector, masks=None, samples=None, infill_noises=None, collect=None):
    """the two-stage walk ``co`` (coefficients()) in the dtype of init: corrector (when asked, from the second iteration on, not on
    the last), then predictor.  Returns (state, {slot: state}, metrics (4, iterations)) like _multistep_ref.walk."""
    dt = init.dtype
    x = init
    n = len(co["t"])
    met = torch.zeros((4, n), dtype=dt)
    coll = {}
    hist = []                                                   # x0_j, x0_{j-1}, ... newest first
    prev_wp = None
    for j in range(n):
        row = _scalars(co, j, dt)
        cond = row["sqrt_ap_t"] * torch.ones((x.shape[0], *([1] * (x.dim() - 1))), dtype=dt)
        eh = model(x, cond)
        x0 = torch.clamp(row["sqrt_recip"] * x - row["sqrt_m1"] * eh, -row["clip"], row["clip"])
        hist.insert(0, x0)
        q = min(3, j + 1)
        xc = x
        if corrector and 1 <= j < n - 1:
            new = sum(row["wc"][i] * hist[i] for i in range(q))
            old = sum(prev_wp[i] * hist[1 + i] for i in range(min(3, j)))
            xc = x + row["alpha_t"] * (new - old)
        nx = row["ratio"] * xc + row["alpha_s"] * sum(row["wp"][i] * hist[i] for i in range(q))
        iz = infill_noises(row["t"]).to(dt) if (masks is not None and 0 <= row["next_t"] < T) else None
        nx, _ = _blend(nx, row, T, masks, samples, iz)
        met[0, j], met[1, j], met[2, j], met[3, j] = norm_metric(eh), norm_metric(x - nx), row["ap_t"], norm_metric(torch.zeros_like(x))
        if collect is not None and collect[j] >= 0:
            coll[collect[j]] = nx
        prev_wp = row["wp"]
        hist = hist[:4]
        x = nx
    return x, coll, met


# ------------------------------------------------------------------ on the shipped tables
def table_rows(coef, plan, taus, betas):
    """per-iteration dict from a shipped pair of tables (float32 [T][12], int32 [T][4]): the folded update
    x' = b x + A0 x0 + A1 h1 + A2 h2 + A3 h3 with the float32 numbers the kernel reads, promoted"""
    ap = alphas_prod(betas)
    t = np.asarray(taus)
    c = coef[t].astype(np.float64)
    return dict(t=t, next_t=plan[t, 0].astype(np.int64), sqrt_recip=c[:, 0], sqrt_m1=c[:, 1], A=c[:, [2, 8, 9, 10]], b=c[:, 3],
                sqrt_as=c[:, 6], sqrt_1m_as=c[:, 7], ap_t=ap[t], sqrt_ap_t=np.sqrt(ap[t]), clip=c[:, 5])


def update(x, eh, hist, row, T, masks=None, samples=None, iz=None):
    """one folded update in the dtype of x from a row (a dict of scalars and the four A): ``hist`` = (h1, h2, h3), read only where
    its coefficient is not zero.  Returns (new state, the clamped x0, y or None)."""
    c = {k: (v if k in ("t", "next_t") else torch.as_tensor(v, dtype=x.dtype)) for k, v in row.items()}
    x0 = torch.clamp(c["sqrt_recip"] * x - c["sqrt_m1"] * eh, -c["clip"], c["clip"])
    nx = c["b"] * x + c["A"][0] * x0
    for i in (1, 2, 3):
        if float(c["A"][i]) != 0:
            nx = nx + c["A"][i] * hist[i - 1]
    nx, y = _blend(nx, c, T, masks, samples, iz)
    return nx, x0, y


def table_walk(model, rows, init, T, masks=None, samples=None, infill_noises=None, collect=None):
    """the walk ``rows`` (table_rows()) in the dtype of init, with the kernel's ring of three histories"""
    dt = init.dtype
    x = init
    n = len(rows["t"])
    met = torch.zeros((4, n), dtype=dt)
    coll = {}
    hist = [None, None, None]
    for j in range(n):
        row = _scalars(rows, j, dt)
        cond = row["sqrt_ap_t"] * torch.ones((x.shape[0], *([1] * (x.dim() - 1))), dtype=dt)
        eh = model(x, cond)
        iz = infill_noises(row["t"]).to(dt) if (masks is not None and 0 <= row["next_t"] < T) else None
        nx, x0, _ = update(x, eh, hist, row, T, masks, samples, iz)
        met[0, j], met[1, j], met[2, j], met[3, j] = norm_metric(eh), norm_metric(x - nx), row["ap_t"], norm_metric(torch.zeros_like(x))
        if collect is not None and collect[j] >= 0:
            coll[collect[j]] = nx
        hist = [x0, hist[0], hist[1]]
        x = nx
    return x, coll, met
