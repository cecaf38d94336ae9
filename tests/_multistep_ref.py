"""float64 restatement of the second-order multistep sampler DPM-Solver++(2M) and of the lambda-uniform timestep grid for the
multistep tests.

Written from Lu et al. 2022 ("DPM-Solver++"), Algorithm 2 (data prediction), independently of smd_amd/schedule.py.  With
alpha_t = sqrt(ap_t), sigma_t = sqrt(1 - ap_t), lambda_t = log(alpha_t / sigma_t), t = t_{i-1} -> s = t_i, h_i = lambda_s - lambda_t and
r_i = h_{i-1} / h_i:
  D_i = (1 + 1 / (2 r_i)) x0_i - (1 / (2 r_i)) x0_{i-1}         (D_1 = x0_1: the first step has no history)
  x_s = (sigma_s / sigma_t) x_t - alpha_s (exp(-h_i) - 1) D_i
x0_i = clamp((x_t - sigma_t eps_hat) / alpha_t, -clip, clip) is the data prediction at x_t.  ap is the float32 cumulative product
of (1 - beta), promoted; the last iteration takes ap_s = 1 (sigma_s = 0, h = inf): it is first order, D = x0, and returns x0.
Order 1 is D_i = x0_i everywhere (DDIM at eta = 0).  The walks run any callable ``model(x, cond)`` in the dtype of ``init``.
"""
import numpy as np
import torch

from _strided_ref import alphas_prod, norm_metric, slots  # noqa: F401  (the schedule's products and the collection bookkeeping)


def lambdas(betas):
    ap = alphas_prod(betas)
    return np.log(np.sqrt(ap) / np.sqrt(1 - ap))


def logsnr_timesteps(T, K, betas):
    """K lambdas evenly spaced from lambda[T-1] to lambda[0], each replaced by the timestep whose lambda is nearest; descending set"""
    lam = lambdas(betas)
    out = set()
    for i in range(K):
        target = lam[T - 1] + (lam[0] - lam[T - 1]) * i / (K - 1)
        out.add(int(np.argmin(np.abs(lam - target))))
    return sorted(out, reverse=True)


def coefficients(betas, taus, order, clip=1.0):
    """float64 per-iteration quantities of the descending walk, in the paper's variables: dict of arrays of len(taus)"""
    ap = alphas_prod(betas)
    lam = lambdas(betas)
    t = np.asarray(taus)
    n = len(t)
    at = ap[t]
    as_ = np.append(ap[t[1:]], 1.0)
    h = np.append(lam[t[1:]] - lam[t[:-1]], np.inf)
    inv2r = np.zeros(n)                                         # 1 / (2 r_i) = h_i / (2 h_{i-1})
    if order == 2:
        for i in range(1, n - 1):
            inv2r[i] = h[i] / (2 * h[i - 1])
    return dict(t=t, next_t=np.append(t[1:], -1), sqrt_recip=1 / np.sqrt(at), sqrt_m1=np.sqrt(1 - at) / np.sqrt(at),
                ratio=np.sqrt(1 - as_) / np.sqrt(1 - at), gain=-np.sqrt(as_) * np.expm1(-h), inv2r=inv2r, h=h,
                sqrt_as=np.sqrt(as_), sqrt_1m_as=np.sqrt(1 - as_), ap_t=at, sqrt_ap_t=np.sqrt(at), clip=np.full(n, float(clip)))


def table_rows(coef, plan, taus, betas):
    """the same dict from a shipped pair of tables (float32 [T][12], int32 [T][4]): gain (1 + inv2r) = a0, -gain inv2r = a1, so
    gain = a0 + a1 and inv2r = -a1 / gain -- the walk below then runs ON the shipped numbers"""
    ap = alphas_prod(betas)
    t = np.asarray(taus)
    c = coef[t].astype(np.float64)
    gain = c[:, 2] + c[:, 8]
    return dict(t=t, next_t=plan[t, 0].astype(np.int64), sqrt_recip=c[:, 0], sqrt_m1=c[:, 1], ratio=c[:, 3], gain=gain,
                inv2r=-c[:, 8] / gain, sqrt_as=c[:, 6], sqrt_1m_as=c[:, 7], ap_t=ap[t], sqrt_ap_t=np.sqrt(ap[t]), clip=c[:, 5])


def update(x, eh, x0_prev, row, T, masks=None, samples=None, iz=None):
    """one update in the dtype of x from a row (a dict of scalars): (new state, the x0 it used and stores as history, y or None)"""
    c = {k: (v if k in ("t", "next_t") else torch.as_tensor(v, dtype=x.dtype)) for k, v in row.items()}
    x0 = torch.clamp(c["sqrt_recip"] * x - c["sqrt_m1"] * eh, -c["clip"], c["clip"])
    D = x0 if float(c["inv2r"]) == 0 else (1 + c["inv2r"]) * x0 - c["inv2r"] * x0_prev
    nx = c["ratio"] * x + c["gain"] * D
    y = None
    if masks is not None:
        y = c["sqrt_as"] * samples + c["sqrt_1m_as"] * iz if 0 <= int(c["next_t"]) < T else samples
        nx = nx * (1 - masks) + y * masks
    return nx, x0, y


def walk(model, co, init, T, masks=None, samples=None, infill_noises=None, collect=None):
    """the walk ``co`` (coefficients() or table_rows()) in the dtype of init, coefficients rounded to that dtype.
    Returns (state, {slot: state} for the iterations ``collect`` (a slot list) names, metrics (4, iterations))."""
    dt = init.dtype
    x = init
    n = len(co["t"])
    met = torch.zeros((4, n), dtype=dt)
    coll = {}
    x0_prev = None
    for j in range(n):
        row = {k: (int(v[j]) if k in ("t", "next_t") else torch.tensor(float(v[j]), dtype=torch.float64).to(dt)) for k, v in co.items()}
        cond = row["sqrt_ap_t"] * torch.ones((x.shape[0], *([1] * (x.dim() - 1))), dtype=dt)
        eh = model(x, cond)
        iz = infill_noises(row["t"]).to(dt) if (masks is not None and 0 <= row["next_t"] < T) else None
        nx, x0_prev, _ = update(x, eh, x0_prev, row, T, masks, samples, iz)
        met[0, j], met[1, j], met[2, j], met[3, j] = norm_metric(eh), norm_metric(x - nx), row["ap_t"], norm_metric(torch.zeros_like(x))
        if collect is not None and collect[j] >= 0:
            coll[collect[j]] = nx
        x = nx
    return x, coll, met
