"""float64 restatement of the strided (DDIM) sampler and of its inversion for the strided tests.

Written from Song et al. 2021, eq. 12, independently of smd_amd/schedule.py.  With eps_hat = (x_t - sqrt(ap_t) x0) / sqrt(1 - ap_t):
  x_s = sqrt(ap_s) x0 + sqrt(1 - ap_s - sigma^2) eps_hat + sigma z = a x0 + b x_t + sigma z
  sigma = eta sqrt((1 - ap_s) / (1 - ap_t)) sqrt(1 - ap_t / ap_s),  b = sqrt(1 - ap_s - sigma^2) / sqrt(1 - ap_t),  a = sqrt(ap_s) - b sqrt(ap_t)
ap is the float32 cumulative product of (1 - beta) (what every table of the engine starts from), promoted; the last
iteration of a descending walk takes ap_s = 1 (the clean sample).  The walks run ``O.make_model``'s network in the dtype
of ``init``: float64 is the reference, float32 the measure of what float32 arithmetic costs the same computation (g32).
"""
import numpy as np
import torch


def alphas_prod(betas):
    return np.cumprod(np.float32(1) - np.asarray(betas, np.float32), dtype=np.float32).astype(np.float64)


def timesteps(T, K):
    return sorted({int(np.round(v)) for v in np.linspace(0, T - 1, K)}, reverse=True)


def slots(K):
    """the reference's collection bookkeeping (utils/ebm_utils.py:324-325, 387-394) for a walk of K iterations: iteration j
    (0-based) is image_idx = j + 2; repeated linspace entries add up and a sum past row 40 is dropped."""
    idx = np.linspace(np.float32(1), np.float32(K), 40, dtype=np.float32).astype(np.int32)
    out = []
    for j in range(K):
        hit = np.nonzero(idx == j + 2)[0]
        s = int(hit.sum()) + 1 if hit.size else -1
        out.append(s if s <= 40 else -1)
    return out


def descending(betas, taus, eta):
    """float64 per-iteration coefficients of the descending walk: dict of arrays of len(taus)"""
    ap = alphas_prod(betas)
    t = np.asarray(taus)
    at = ap[t]
    as_ = np.append(ap[t[1:]], 1.0)
    sigma = eta * np.sqrt((1 - as_) / (1 - at)) * np.sqrt(1 - at / as_)
    b = np.sqrt(np.maximum(1 - as_ - sigma * sigma, 0)) / np.sqrt(1 - at)
    return dict(t=t, next_t=np.append(t[1:], -1), sqrt_recip=np.sqrt(1 / at), sqrt_m1=np.sqrt(1 - at) * np.sqrt(1 / at),
                a=np.sqrt(as_) - b * np.sqrt(at), b=b, sigma=sigma, sqrt_as=np.sqrt(as_), sqrt_1m_as=np.sqrt(1 - as_),
                ap_t=at, sqrt_ap_t=np.sqrt(at), clip=np.full(len(t), 1.0))


def ascending(betas, taus):
    """the inversion: taus ascending, t_j -> t_{j+1}, sigma = 0, no clamp; len(taus) - 1 iterations"""
    ap = alphas_prod(betas)
    asc = np.asarray(sorted(taus))
    t, s = asc[:-1], asc[1:]
    b = np.sqrt(1 - ap[s]) / np.sqrt(1 - ap[t])
    return dict(t=t, next_t=np.append(s[:-1], len(betas)), sqrt_recip=np.sqrt(1 / ap[t]), sqrt_m1=np.sqrt(1 - ap[t]) * np.sqrt(1 / ap[t]),
                a=np.sqrt(ap[s]) - b * np.sqrt(ap[t]), b=b, sigma=np.zeros(len(t)), sqrt_as=np.sqrt(ap[s]), sqrt_1m_as=np.sqrt(1 - ap[s]),
                ap_t=ap[t], sqrt_ap_t=np.sqrt(ap[t]), clip=np.full(len(t), np.inf))


def update(x, eh, z, row, T, masks=None, samples=None, iz=None):
    """one update in the dtype of x from a row of coefficients (a dict of scalars): (new state, x0, y or None)"""
    c = {k: (v if k in ("t", "next_t") else torch.as_tensor(v, dtype=x.dtype)) for k, v in row.items()}
    x0 = torch.clamp(c["sqrt_recip"] * x - c["sqrt_m1"] * eh, -c["clip"], c["clip"])
    nx = c["a"] * x0 + c["b"] * x + (c["sigma"] * z if float(c["sigma"]) != 0 else torch.zeros_like(x))
    y = None
    if masks is not None:
        y = c["sqrt_as"] * samples + c["sqrt_1m_as"] * iz if 0 <= int(c["next_t"]) < T else samples
        nx = nx * (1 - masks) + y * masks
    return nx, x0, y


def norm_metric(v):
    """utils/ebm_utils.py:381-383: sqrt(sum(v^2, axis=1) + 1e-10).mean()"""
    return torch.sqrt((v * v).sum(dim=1) + 1e-10).mean()


def walk(model, co, init, T, noises=None, masks=None, samples=None, infill_noises=None, collect=None):
    """the walk ``co`` (descending() or ascending()) in the dtype of init, coefficients rounded to that dtype.
    Returns (state, {slot: state} for the iterations ``collect`` (a slot list) names, metrics (4, iterations))."""
    dt = init.dtype
    x = init
    n = len(co["t"])
    met = torch.zeros((4, n), dtype=dt)
    coll = {}
    for j in range(n):
        row = {k: (int(v[j]) if k in ("t", "next_t") else torch.tensor(float(v[j]), dtype=torch.float64).to(dt)) for k, v in co.items()}
        t = row["t"]
        cond = row["sqrt_ap_t"] * torch.ones((x.shape[0], *([1] * (x.dim() - 1))), dtype=dt)
        eh = model(x, cond)
        z = noises(t).to(dt) if (noises is not None and float(row["sigma"]) != 0) else torch.zeros_like(x)
        iz = infill_noises(t).to(dt) if (masks is not None and 0 <= row["next_t"] < T) else None
        nx, _, _ = update(x, eh, z, row, T, masks, samples, iz)
        met[0, j], met[1, j], met[2, j], met[3, j] = norm_metric(eh), norm_metric(x - nx), row["ap_t"], norm_metric(row["sigma"] * z)
        if collect is not None and collect[j] >= 0:
            coll[collect[j]] = nx
        x = nx
    return x, coll, met
