"""Float64 NumPy restatement of the per-timestep variational bound (Ho et al. 2020, eq. 5): the tables,
the three per-example sums, the terms, the prior and the total.  Independent of smd_amd.schedule.bound_tables: the weights are
written in their second form, beta_t ap_{t-1} / (2 (1-ap_t)(1-ap_{t-1})).  ``walk`` runs oracle/ddpm_oracle.py's float64
network (imported, not modified) on explicit eps."""
import numpy as np


def alphas(betas):
    """(beta, ap, ap_prev) in float64; ap is the float32 cumulative product promoted, ap_prev[0] = 1"""
    b32 = np.asarray(betas, dtype=np.float32)
    ap = np.cumprod((np.float32(1) - b32).astype(np.float32), dtype=np.float32).astype(np.float64)
    return b32.astype(np.float64), ap, np.concatenate([np.ones(1), ap[:-1]])


def tables(betas):
    """dict of float64 per-timestep arrays: w (w[0] = 1 / (2 var_0)), var_0, decoder_const (per dimension), prior_a, prior_c, and the
    four columns of the kernels' table BEFORE rounding"""
    beta, ap, app = alphas(betas)
    w = np.empty_like(ap)
    w[1:] = beta[1:] * app[1:] / (2 * (1 - ap[1:]) * (1 - app[1:]))
    var_0 = beta[1] * (1 - app[1]) / (1 - ap[1])
    w[0] = 1 / (2 * var_0)
    return dict(w=w, var_0=var_0, decoder_const=0.5 * np.log(2 * np.pi * var_0), prior_a=ap[-1], prior_c=-ap[-1] - np.log(1 - ap[-1]),
                table=np.stack([np.sqrt(ap), np.sqrt(1 - ap), np.sqrt(1 / ap), np.sqrt(1 / ap - 1)], axis=1))


def x_t(x0, eps, row):
    """row = (sqrt_ap, sqrt_1m_ap, sqrt_recip, sqrt_m1), any float type: promoted"""
    r = np.asarray(row, dtype=np.float64)
    return r[0] * np.asarray(x0, np.float64) + r[1] * np.asarray(eps, np.float64)


def x0_hat(x0, eps, eps_hat, row, clip=1.0):
    """(clamped reconstruction, share of clipped elements)"""
    r = np.asarray(row, dtype=np.float64)
    raw = r[2] * x_t(x0, eps, row) - r[3] * np.asarray(eps_hat, np.float64)
    return np.clip(raw, -clip, clip), float(np.mean(np.abs(raw) > clip))


def three_sums(x0, eps, eps_hat, row, clip=1.0):
    """[B][3] float64 (q, e, n) from the definition, on whatever inputs and table row it is given (promoted to float64)"""
    x0, eps, eps_hat = (np.asarray(v, np.float64) for v in (x0, eps, eps_hat))
    rec, _ = x0_hat(x0, eps, eps_hat, row, clip)
    ax = tuple(range(1, x0.ndim))
    return np.stack([((x0 - rec) ** 2).sum(ax), ((eps - eps_hat) ** 2).sum(ax), (x0 ** 2).sum(ax)], axis=1)


def term(tab, t, q, D):
    """L_t in nats per example from q_t [B]"""
    return tab["w"][t] * q + (D * tab["decoder_const"] if t == 0 else 0.0)


def prior(tab, n, D):
    return 0.5 * (tab["prior_a"] * n + D * tab["prior_c"])


def walk(model64, betas, x0, eps_of_t, timesteps, clip=1.0):
    """model64(x, s): ddpm_oracle.make_model's float64 network.  Returns dict(terms [K][B], eps_mse [K][B], prior [B], total [B] or None)."""
    import torch
    tab = tables(betas)
    x0 = np.asarray(x0, np.float64)
    B, D = x0.shape[0], int(np.prod(x0.shape[1:]))
    terms, mse, n = [], [], None
    for t in timesteps:
        row = tab["table"][t]
        eps = np.asarray(eps_of_t(t), np.float64)
        xt = x_t(x0, eps, row)
        s = torch.full((B,) + (1,) * (x0.ndim - 1), float(row[0]), dtype=torch.float64)
        with torch.no_grad():
            eh = model64(torch.from_numpy(xt), s).numpy()
        sums = three_sums(x0, eps, eh, row, clip)
        terms.append(term(tab, t, sums[:, 0], D))
        mse.append(sums[:, 1] / D)
        n = sums[:, 2]
    terms = np.stack(terms)
    pr = prior(tab, n, D)
    full = len(timesteps) == len(np.asarray(betas))
    return dict(terms=terms, eps_mse=np.stack(mse), prior=pr, total=pr + terms.sum(0) if full else None)
