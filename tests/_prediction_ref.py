"""Float64 NumPy reference of x0- / v-parameterised training and sampling: the target of the network's
output, the min-SNR weight of each kind, the weighted loss gradient, the x0 a sampler table recovers from the output, and the
output each kind would emit for a given eps_hat.  Everything is evaluated ON THE STORED fp32 noise level s, as the kernel does:
ap = s^2 and sb = sqrt((1 - s)(1 + s)) in float64.

kind 0 eps, 1 x0, 2 v = s eps - sb x0.
"""
import numpy as np

import _timestep_ref as TR

U = TR.U
KINDS = {"eps": 0, "x0": 1, "v": 2}


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _per_sample(v, ndim):
    return np.asarray(v, np.float64).reshape(-1, *([1] * (ndim - 1)))


def levels(s):
    """(s, sb) float64 from the fp32 noise levels"""
    s = _f64(s)
    return s, np.sqrt((1.0 - s) * (1.0 + s))


def target(kind, eps, x0, s):
    """what the network's output is compared with, float64 [B]..."""
    e, x = _f64(eps), _f64(x0)
    if kind == 0:
        return e
    if kind == 1:
        return x
    s64, sb = levels(s)
    return _per_sample(s64, e.ndim) * e - _per_sample(sb, e.ndim) * x


def weight(kind, s, iw, gamma):
    """w_b = iw_b * (eps: min(1, gamma / SNR); x0: min(SNR, gamma); v: min(SNR, gamma) / (SNR + 1)), SNR = ap / (1 - ap); without
    an SNR factor (gamma <= 0 or inf) iw_b alone.  ap = 1: eps 0, x0 gamma, v 0; ap = 0: eps 1, x0 0, v 0."""
    s64 = _f64(s)
    w = np.ones_like(s64) if iw is None else _f64(iw)
    if not TR.snr_on(gamma):
        return w
    ap = s64 * s64
    om = (1.0 - s64) * (1.0 + s64)
    g = float(gamma)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = ap / om                                        # ap + om = 1: never 0 / 0; om = 0 gives inf
        if kind == 0:
            f = np.minimum(1.0, np.where(ap > 0.0, g / snr, np.inf))
        elif kind == 1:
            f = np.minimum(snr, g)
        else:
            f = np.where(np.isinf(snr), 0.0, np.minimum(snr, g) / (np.where(np.isinf(snr), 0.0, snr) + 1.0))
    return w * f


def param_grad(kind, pred, eps, x0, s, iw, gamma, inv_global_count):
    """(dpred float64, loss_per_sample float64 [B] -- the UNWEIGHTED mean of (out - target)^2 --, w float64 [B]); inv_global_count:
    the fp32 value the kernel gets"""
    p = _f64(pred)
    d = p - target(kind, eps, x0, s)
    w = weight(kind, s, iw, gamma)
    g = 2.0 * float(np.float32(inv_global_count)) * _per_sample(w, d.ndim) * d
    return g, (d * d).reshape(d.shape[0], -1).mean(axis=1), w


def bf16_ulp(r):
    """one unit in the last place of the bf16 value r (8 significant bits), float64; the smallest normal's below 2^-126"""
    a = np.maximum(np.abs(np.asarray(r, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def check_dpred(got, g64):
    """dpred against the reference ROUNDED to bf16: (number of elements more than one bf16 ulp away, worst distance in ulps)"""
    r = TR.to_bf16(g64)
    err = np.abs(np.asarray(got, np.float64) - r) / bf16_ulp(r)
    return int((err > 1.0).sum()), float(err.max())


# ---------------------------------------------------------------------------------------------------- sampling side
def x0_coefficients(kind, ap):
    """float64 (c0, c1) of x0 = c0 x_t - c1 out, written out here independently of schedule.x0_coefficients"""
    ap = np.asarray(ap, np.float64)
    if kind == 0:
        return 1.0 / np.sqrt(ap), np.sqrt(1.0 - ap) / np.sqrt(ap)
    if kind == 1:
        return np.zeros_like(ap), -np.ones_like(ap)
    return np.sqrt(ap), np.sqrt(1.0 - ap)


def output_of(kind, x_t, eps_hat, ap):
    """the output a network of ``kind`` emits when its belief about the noise in x_t is eps_hat (float64; ap scalar or
    broadcastable): x0_hat = (x_t - sqrt(1 - ap) eps_hat) / sqrt(ap), v_hat = sqrt(ap) eps_hat - sqrt(1 - ap) x0_hat"""
    x_t, eps_hat, ap = np.asarray(x_t, np.float64), np.asarray(eps_hat, np.float64), np.asarray(ap, np.float64)
    if kind == 0:
        return eps_hat
    x0_hat = (x_t - np.sqrt(1.0 - ap) * eps_hat) / np.sqrt(ap)
    if kind == 1:
        return x0_hat
    return np.sqrt(ap) * eps_hat - np.sqrt(1.0 - ap) * x0_hat


def eps_of(kind, x_t, out, ap):
    """the inverse of ``output_of``: the eps_hat equivalent to the output ``out`` of a network of ``kind``"""
    x_t, out, ap = np.asarray(x_t, np.float64), np.asarray(out, np.float64), np.asarray(ap, np.float64)
    if kind == 0:
        return out
    c0, c1 = x0_coefficients(kind, ap)
    x0_hat = c0 * x_t - c1 * out
    return (x_t - np.sqrt(ap) * x0_hat) / np.sqrt(1.0 - ap)


def loss_in_eps_units(kind, loss_per_sample, s):
    """mean_b f_b loss_b with f = 1 (eps), ap / (1 - ap) (x0; samples with ap = 1 left out), ap (v)"""
    loss = np.asarray(loss_per_sample, np.float64)
    ap = _f64(s) ** 2
    if kind == 0:
        return float(loss.mean())
    if kind == 2:
        return float((ap * loss).mean())
    keep = ap < 1.0
    if not keep.any():
        return 0.0
    return float((ap[keep] / (1.0 - ap[keep]) * loss[keep]).mean())
