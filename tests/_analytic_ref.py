"""float64 restatement of the analytic (optimal) reverse variance of Bao et al. 2022 (Analytic-DPM) for the analytic tests.

Written from the paper's Theorem 1 in the notation of tests/_strided_ref.py, independently of smd_amd/schedule.py.  A walk step
t -> s with lam = sigma_eta has the mean sqrt(ap_s) x0_hat + sqrt(bb_s - lam^2) eps_hat, i.e. x_t sqrt(ap_s / ap_t) - h eps_hat,
  h = sqrt(bb_t ap_s / ap_t) - sqrt(bb_s - lam^2),  bb = 1 - ap,
and the optimal state-independent variance is sig2 = lam^2 + h^2 (1 - g), g = E[eps_hat^2] (per element, or its mean).
"""
import numpy as np
import torch

import _strided_ref as R


def variance(betas, taus, eta, g, clip=np.inf):
    """sig2 per iteration, float64; g [K] or [K][...]; the last iteration keeps 0"""
    co = R.descending(betas, taus, eta)
    ap = R.alphas_prod(betas)
    t = np.asarray(taus)
    at, as_ = ap[t], np.append(ap[t[1:]], 1.0)
    lam2 = co["sigma"] ** 2
    h = np.sqrt((1 - at) * as_ / at) - np.sqrt(np.maximum(1 - as_ - lam2, 0))
    g = np.clip(np.asarray(g, dtype=np.float64), 0, 1)
    ex = (slice(None),) + (None,) * (g.ndim - 1)
    s2 = lam2[ex] + h[ex] ** 2 * (1 - g)
    if np.isfinite(clip):
        s2 = np.minimum(s2, lam2[ex] + (co["a"][ex] * clip) ** 2)
    s2[-1] = 0
    return s2


def eps_units(kind, ap_t, x_t, out):
    """the network's output in eps units, float64, from the closed forms per kind"""
    if kind == "eps":
        return out
    if kind == "x0":
        return (x_t - np.sqrt(ap_t) * out) / np.sqrt(1 - ap_t)
    return np.sqrt(1 - ap_t) * x_t + np.sqrt(ap_t) * out           # v = sqrt(ap) eps - sqrt(1 - ap) x0


def gaussian_g(ap_t, v):
    """E[eps_hat^2] of the exact score of x0 ~ N(0, diag(v)): eps_hat = sqrt(bb) x_t / (ap v + bb)"""
    return (1 - ap_t) / (ap_t * v + 1 - ap_t)


def gaussian_walk_variances(betas, taus, eta, v, sig2):
    """Var(x_s) per element after every iteration of the walk started from Var(x_T) = ap_T v + bb_T, x0 ~ N(0, diag(v)), with the
    exact score and the noise variances sig2 [K][len(v)]: everything is linear in x_t, so the variance propagates in closed
    form.  Returns (got [K][len(v)], want [K][len(v)] = ap_s v + bb_s)."""
    co = R.descending(betas, taus, eta)
    ap = R.alphas_prod(betas)
    t = np.asarray(taus)
    as_ = np.append(ap[t[1:]], 1.0)
    V = ap[t[0]] * v + 1 - ap[t[0]]
    got, want = [], []
    for j in range(len(t)):
        at = ap[t[j]]
        k = np.sqrt(1 - at) / (at * v + 1 - at)                    # eps_hat = k x_t
        m = co["a"][j] * (1 - np.sqrt(1 - at) * k) / np.sqrt(at) + co["b"][j]
        V = m * m * V + sig2[j]
        got.append(V)
        want.append(as_[j] * v + 1 - as_[j])
    return np.array(got), np.array(want)


def estimate(model, betas, x0, ts, eps_of, dtype=torch.float64):
    """g [len(ts)][...] = mean over the examples of eps_hat^2 on the CPU oracle's eps network ``model`` in ``dtype``: x_t is formed
    from the float32-rounded table entries the kernels read (sqrt(ap), sqrt(1 - ap)), in ``dtype``."""
    ap = R.alphas_prod(betas)
    out = []
    with torch.no_grad():
        for t in ts:
            sa = torch.tensor(float(np.float32(np.sqrt(ap[t]))), dtype=dtype)
            s1 = torch.tensor(float(np.float32(np.sqrt(1 - ap[t]))), dtype=dtype)
            xt = sa * x0.to(dtype) + s1 * eps_of(t).to(dtype)
            if dtype == torch.float64:                               # the kernel's x_t is one fp32 FMA of fp32 inputs
                xt = xt.float().double()
            cond = torch.tensor(float(np.sqrt(ap[t])), dtype=dtype) * torch.ones((x0.shape[0], *([1] * (x0.dim() - 1))), dtype=dtype)
            eh = model(xt, cond)
            out.append((eh.double() ** 2).mean(dim=0).numpy())
    return np.array(out)


def walk(model, betas, taus, eta, sig, init, noises, T, collect=None):
    """the strided walk in the dtype of ``init`` with the per-element noise scale ``sig`` [K][...] (float32 table values,
    promoted) in place of sigma_eta: (state, {slot: state})"""
    co = R.descending(betas, taus, eta)
    dt = init.dtype
    x = init
    coll = {}
    for j in range(len(co["t"])):
        c = {k: torch.tensor(float(co[k][j]), dtype=torch.float64).to(dt) for k in ("sqrt_recip", "sqrt_m1", "a", "b", "sqrt_ap_t")}
        t = int(co["t"][j])
        cond = c["sqrt_ap_t"] * torch.ones((x.shape[0], *([1] * (x.dim() - 1))), dtype=dt)
        eh = model(x, cond)
        x0 = torch.clamp(c["sqrt_recip"] * x - c["sqrt_m1"] * eh, -1.0, 1.0)
        sg = torch.as_tensor(np.asarray(sig[j], dtype=np.float64)).to(dt)
        nx = c["a"] * x0 + c["b"] * x
        if bool((sg != 0).any()):
            nx = nx + sg * noises(t).to(dt)
        if collect is not None and collect[j] >= 0:
            coll[collect[j]] = nx
        x = nx
    return x, coll
