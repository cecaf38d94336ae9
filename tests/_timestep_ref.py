"""Float64 NumPy reference of weighted training: the per-sample loss weight, the weighted loss gradient
rounded to bf16, the ten-deep loss ring per timestep written as the obvious sequential loop, and the tables p / cdf with the
inverse-CDF draw -- plus the comparisons the GPU tests make (``check_*``), so that tests/test_timestep_host.py can show on the
CPU that each of them catches a planted fault (``fault=...``).

The bound on one element of dpred
---------------------------------
The kernel forms, in fp32, d = pred - eps (1 rounding), w = iw * min(1, (gamma * ((1 - s) * (1 + s))) / (s * s)) (1 - s is exact
for s in [1/2, 2], else 1 rounding; 1 + s: 1; their product: 1; gamma *: 1; s * s: 1; the division: 1, or up to 2.5 ulp where the
compiler does not round it correctly; iw *: 1), gscale = (2 inv) * w (1; 2 inv is exact and the reference below takes the same
fp32 inv) and g = d * gscale (1): at most 11.5 roundings of relative size 2^-24 each, taken as FP32_ROUNDINGS = 16 to first
order.  g is then rounded to bf16 (8 significant bits): half an ulp of bf16 AT THE fp32 VALUE.  So for the float64 value x

    |dpred - x| <= half_ulp_bf16(|x| (1 + 16 * 2^-24)) + 16 * 2^-24 |x|      (+ 2^-134, half the smallest bf16 denormal)

on every element; nothing is averaged over the tensor.
"""
import numpy as np
import torch

import bf16_emulation as E

U = 2.0 ** -24
FP32_ROUNDINGS = 16
DEPTH = 10
MIX = np.float32(1e-3)            # the kernel receives uniform_mix as an fp32 argument and widens it


# ---------------------------------------------------------------------------------------------------- weight
def snr_on(gamma):
    return bool(gamma > 0.0 and np.isfinite(gamma))


def weight(s, iw, gamma, fault=None):
    """w_b = iw_b min(1, gamma (1 - ap) / ap), ap = s_b^2, from the fp32 noise levels; float64"""
    s = np.asarray(s, dtype=np.float32).astype(np.float64)
    w = np.ones_like(s) if iw is None else np.asarray(iw, dtype=np.float32).astype(np.float64)
    if snr_on(gamma):
        ap = s * s
        with np.errstate(divide="ignore", invalid="ignore"):
            f = ap / (float(gamma) * (1.0 - ap)) if fault == "snr_inverted" else float(gamma) * (1.0 - ap) / ap
        f = np.where(np.isnan(f), np.inf, f)
        w = w * np.minimum(1.0, f)
    return w


def weighted_grad(pred, eps, s, iw, gamma, inv_global_count, fault=None):
    """(dpred float64 [B][S][C], loss_per_sample float64 [B], w float64 [B]); inv_global_count: the fp32 value the kernel gets"""
    p, q = np.asarray(pred, np.float32).astype(np.float64), np.asarray(eps, np.float32).astype(np.float64)
    d = p - q
    w = weight(s, iw, gamma, fault)
    g = 2.0 * float(np.float32(inv_global_count)) * w.reshape(-1, *([1] * (d.ndim - 1))) * d
    return g, (d * d).reshape(d.shape[0], -1).mean(axis=1), w


def to_bf16(x):
    """round-to-nearest-even to bf16 as the engine stores it (oracle/bf16_emulation.py rb on the fp32 value), as float64"""
    return E.rb(torch.from_numpy(np.asarray(x, np.float64).astype(np.float32))).numpy().astype(np.float64)


def grad_bound(g64):
    a = np.abs(g64)
    mag = np.maximum(a * (1.0 + FP32_ROUNDINGS * U), 2.0 ** -126)
    half_ulp = 2.0 ** (np.floor(np.log2(mag)) - 8)
    return half_ulp + FP32_ROUNDINGS * U * a + 2.0 ** -134


def check_grad(got, g64):
    """number of elements of dpred (any float array) outside the bound, and the worst excess ratio"""
    err = np.abs(np.asarray(got, np.float64) - g64)
    b = grad_bound(g64)
    return int((err > b).sum()), float((err / b).max())


# ---------------------------------------------------------------------------------------------------- ring
def ring_update(history, counts, labels, loss, label_base, fault=None):
    """the samples in order: a row fills front to back, a full row shifts left and appends; labels outside the table dropped"""
    h, c = np.array(history, dtype=np.float32, copy=True), np.array(counts, dtype=np.int32, copy=True)
    n = h.shape[0]
    for lab, l in zip(np.asarray(labels).tolist(), np.asarray(loss, np.float32).tolist()):
        i = lab - label_base
        if i < 0 or i >= n:
            continue
        if c[i] < DEPTH:
            h[i, c[i]] = l
            c[i] += 1
        elif fault == "ring_overwrite":
            h[i, -1] = l
        else:
            h[i, :-1] = h[i, 1:].copy()
            h[i, -1] = l
    return h, c


def tables(history, counts, mix=MIX, fault=None):
    """(p float64 [n], p fp32, cdf fp32 = the inclusive prefix sums of the fp32 p in float64 rounded once, warmed)"""
    h = np.asarray(history, np.float32).astype(np.float64)
    n = h.shape[0]
    warmed = bool((np.asarray(counts) >= DEPTH).all())
    raw = np.sqrt((h * h).mean(axis=1))
    m = float(np.float32(mix))
    if warmed and raw.sum() > 0 and np.isfinite(raw.sum()):
        p = raw / raw.sum() * (1.0 - m) + m / n
    else:
        p = np.full(n, 1.0 / n)
    p32 = p.astype(np.float32)
    c = np.cumsum(p32.astype(np.float64))
    if fault == "cdf_exclusive":
        c = c - p32.astype(np.float64)
    return p, p32, c.astype(np.float32), warmed


def draw(cdf, p, u, label_base, fault=None):
    """labels = label_base + (first i with cdf[i] > u, the last index when there is none); iw = 1 / (n p[i]) float64"""
    cdf, p, u = np.asarray(cdf, np.float32), np.asarray(p, np.float32), np.asarray(u, np.float32)
    n = cdf.shape[0]
    i = np.minimum(np.searchsorted(cdf, u, side="right"), n - 1)
    iw = 1.0 / ((1.0 if fault == "iw_no_n" else float(n)) * p[i].astype(np.float64))
    return (label_base + i).astype(np.int32), iw


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def check_draw(labels, iw, cdf, p, u, label_base):
    """labels exact, iw within 1 ulp of 1 / (n p): (number of wrong labels, number of iw outside)"""
    rl, riw = draw(cdf, p, u, label_base)
    bad_iw = np.abs(np.asarray(iw, np.float64) - riw) > ulp32(riw)
    return int((np.asarray(labels) != rl).sum()), int(bad_iw.sum())


def check_tables(p, cdf, history, counts, ulps=4):
    """p within `ulps` ulp of float64; cdf non-decreasing with |cdf[n-1] - 1| <= n 2^-24: list of what fails"""
    rp, _p32, _c, _w = tables(history, counts)
    p, cdf = np.asarray(p, np.float32), np.asarray(cdf, np.float32)
    bad = []
    if (np.abs(p.astype(np.float64) - rp) > ulps * ulp32(rp)).any():
        bad.append("p")
    if (np.diff(cdf) < 0).any():
        bad.append("cdf decreases")
    if abs(float(cdf[-1]) - 1.0) > cdf.shape[0] * U:
        bad.append("cdf end")
    return bad


# ---------------------------------------------------------------------------------------------------- chi-square
def chi2_quantile(df, tail=1e-6):
    """x with P(chi2_df > x) = tail, by bisection on the regularised upper incomplete gamma function (float64)"""
    sf = lambda x: float(torch.special.gammaincc(torch.tensor(df / 2.0, dtype=torch.float64), torch.tensor(x / 2.0, dtype=torch.float64)))
    lo, hi = float(df), float(df) + 100.0 * np.sqrt(2.0 * df) + 100.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if sf(mid) > tail else (lo, mid)
    return hi


def chi2_stat(labels, p, label_base, n_draws):
    counts = np.bincount(np.asarray(labels) - label_base, minlength=len(p)).astype(np.float64)
    e = n_draws * np.asarray(p, np.float64)
    return float(((counts - e) ** 2 / e).sum())
