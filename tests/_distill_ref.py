"""float64 reference of the three distillation kernels (csrc/distill.hip), working from the fp32 inputs and
the fp32 [N][16] table the kernels read, so that a comparison measures the kernels' own roundings and nothing else.  Every
function takes ``steps`` int [B]; a step outside [0, N) marks a no-op sample, whose rows come back as NaN.

Also the quotient form of the target (Salimans & Ho 2022, eq. of section 3), which the kernels do NOT use, for the host test of
the convex form.
"""
import numpy as np

U = 2.0 ** -24          # one fp32 rounding, relative

COLS = dict(c0_t=0, c1_t=1, a=2, b=3, clip=4, alpha_t=5, sigma_t=6, alpha_m=7, c0_m=8, c1_m=9, w1=10, w2=11, weight=12,
            inv_sigma_t=13)


def rows(table, steps):
    """float64 rows [B][16] of the fp32 table for ``steps``; live [B] bool"""
    table = np.asarray(table, dtype=np.float32).astype(np.float64)
    steps = np.asarray(steps, dtype=np.int64)
    live = (steps >= 0) & (steps < len(table))
    return table[np.where(live, steps, 0)], live


def _col(r, name, ndim):
    return r[:, COLS[name]].reshape((-1,) + (1,) * (ndim - 1))


def _mask(out, live):
    out = np.array(out, dtype=np.float64)
    out[~live] = np.nan
    return out


def noise(x0, eps, table, steps):
    """(z_t, level)"""
    x0, eps = np.asarray(x0, np.float64), np.asarray(eps, np.float64)
    r, live = rows(table, steps)
    z = _col(r, "alpha_t", x0.ndim) * x0 + _col(r, "sigma_t", x0.ndim) * eps
    return _mask(z, live), _mask(r[:, COLS["alpha_t"]], live)


def x_hat(z, out, c0, c1, clip):
    return np.clip(c0 * z - c1 * out, -clip, clip)


def mid(z_t, out1, table, steps):
    """(x1, z_m, level_m, raw): raw is the unclamped estimate (how close an element is to the clamp's kink)"""
    z_t, out1 = np.asarray(z_t, np.float64), np.asarray(out1, np.float64)
    r, live = rows(table, steps)
    n = z_t.ndim
    raw = _col(r, "c0_t", n) * z_t - _col(r, "c1_t", n) * out1
    x1 = np.clip(raw, -_col(r, "clip", n), _col(r, "clip", n))
    z_m = _col(r, "a", n) * x1 + _col(r, "b", n) * z_t
    return _mask(x1, live), _mask(z_m, live), _mask(r[:, COLS["alpha_m"]], live), _mask(raw, live)


def kind_target(kind, x, z_t, alpha_t, inv_sigma_t):
    """what a network of ``kind`` (0 eps, 1 x0, 2 v) must output at z_t for its x0 estimate to be x"""
    if kind == 1:
        return x
    if kind == 0:
        return (z_t - alpha_t * x) * inv_sigma_t
    return (alpha_t * z_t - x) * inv_sigma_t


def loss(x1, z_m, out2, z_t, pred, kind, table, steps, iw, inv_global_count):
    """dict(x2, raw2, xs (x~), target, loss [B], weight [B], dpred) in float64"""
    x1, z_m, out2, z_t, pred = (np.asarray(v, np.float64) for v in (x1, z_m, out2, z_t, pred))
    r, live = rows(table, steps)
    n = x1.ndim
    raw2 = _col(r, "c0_m", n) * z_m - _col(r, "c1_m", n) * out2
    x2 = np.clip(raw2, -_col(r, "clip", n), _col(r, "clip", n))
    xs = _col(r, "w1", n) * x1 + _col(r, "w2", n) * x2
    target = kind_target(kind, xs, z_t, _col(r, "alpha_t", n), _col(r, "inv_sigma_t", n))
    d = pred - target
    w = r[:, COLS["weight"]] * (1.0 if iw is None else np.asarray(iw, np.float32).astype(np.float64))
    per = (d * d).reshape(len(d), -1).mean(axis=1)
    dpred = 2.0 * w.reshape((-1,) + (1,) * (n - 1)) * d * float(np.float32(inv_global_count))
    return dict(x2=_mask(x2, live), raw2=_mask(raw2, live), xs=_mask(xs, live), target=_mask(target, live), loss=_mask(per, live),
                weight=_mask(w, live), dpred=_mask(dpred, live))


# ------------------------------------------------------------------ host-only forms
def quotient_target(z_t, z_u, alpha_t, sigma_t, alpha_u, sigma_u):
    """x~ = (z_u - r z_t) / (alpha_u - r alpha_t), r = sigma_u / sigma_t: the form the kernels avoid"""
    r = sigma_u / sigma_t
    return (z_u - r * z_t) / (alpha_u - r * alpha_t)


def exact_output(kind, x, z, ap):
    """the output of an ideal network of ``kind`` at the state z of level ap whose x0 estimate is exactly x"""
    alpha, sigma = np.sqrt(ap), np.sqrt(1.0 - ap)
    return kind_target(kind, x, z, alpha, 1.0 / sigma)
