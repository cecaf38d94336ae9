"""Element-wise criterion for the objective and sampler kernels of csrc/diffusion.hip: float64 restatements of each operation taken
from the float32 tables and inputs the kernel read, a per-element error bound built from the kernel's own operation order, an fp32
numpy emulation of that order (the check that the bound is attainable) and planted faults.  numpy on the CPU only.

Bound.  U = 2^-24: one fp32 operation costs U |result| (half an ulp).  A bf16 store of a value v that carries the error e adds
BF (|v| + e), BF = 2^-8 (round to nearest even: half a bf16 ulp is at most 2^-8 |v|); a product or square that can fall below the
smallest normal fp32 adds FL = 2^-126 (flushed, or rounded on the denormal grid).  Reads are exact.  Contracting a b + c into one
fma only removes a rounding, so one bound serves both forms.  No element is left out of any comparison; nothing is fitted to GPU output.

  q_sample      sa = sqrt(alpha), sb = sqrt(1 - alpha): one rounding of 1 - alpha (U, halved by the root) and a root within 1 ulp
                (2 U): each within 3 U relative, which is the bound of s_out.  xt before the store: 4 U (|sa x0| + |sb eps|) -- hipcc
                rounds sqrtf correctly (U / 2 + U = 1.5 U for sb), the product U, the sum U: 3.5 U.  eps_out is bit-equal to eps_in.
                dsm: sa = 1 and sb = sigma exactly, so the coefficient share is zero and the same 4 U holds.
  mse_loss_grad d = pred - eps carries U |d|; on the dsm form d = sigma pred + eps carries 2 U (|sigma pred| + |eps|).  The gradient
                d gscale carries one more U for the scale (dsm: gscale = (sigma inv) SC is two roundings more: 3 U), then the store.
                The loss is a sum of non-negative terms: each thread sums n_t = VEC ceil(SC / (1024 VEC)) terms, six shuffle levels,
                sixteen adds; with the difference (2 U on the square), the square and the final scale (n_t + 26) U relative, plus
                SC FL for flushed squares; on the dsm form the absolute share of d, sum (2 |d| e_d + e_d^2) / 2, comes on top.
  reverse_step  r = sr x - sm eh: e_r = 2 U (|sr x| + |sm eh|).  The clamp is 1-Lipschitz and exact once both sides saturate:
                e_c = e_r where |r_ref| <= 1 + e_r, else 0.  x' = mu1 c + mu2 x + sigma z: e_x = |mu1| e_c + 3 U (|mu1 c| + |mu2 x| +
                |sigma z|) (+ |sigma| NORMAL_ABS where z is drawn in the kernel).  Infill y = sa s + sb z_i: e_y = 2 U (|sa s| + |sb z_i|)
                (+ |sb| NORMAL_ABS), y = s exactly at t = 0; blend |1 - m| e_x + |m| e_y + 3 U (|x' (1 - m)| + |y m|).  The bf16 copy
                is the RNE of the fp32 state that was written (bit for bit, against the kernel's own x), the collection slot is
                bit-equal to x.  Metrics, trips = ceil(C / (128 VEC)): the summation costs (S / RG + RG + VEC trips + 12) U relative
                (column walk, row-group combine, the thread's own columns; the square, the root, the floor, six shuffle levels, one
                add and the subtraction x - x' make up the 12); the carried error goes through the triangle inequality,
                sum_cols ||e_x[:, col]||_2 for the step norm and U relative on sigma z for the noise norm.  The 1e-10 floor sits
                inside the reference; S = 1 is sum-then-sqrt over the channels.
  langevin_step x' = x + alpha g + c z carries 3 U (|x| + |alpha g| + |c z|); infill y = s + sigma_i z_i carries 2 U (|s| + |sigma_i z_i|),
                blend and metrics as above with one row group and trips = ceil(C / 256).
  normals       float64 Box-Muller of the same Philox bits (oracle philox4x32 is bit-exact, u01 is restated exactly); the criterion
                is the one csrc/rng.h promises: |dz| <= NORMAL_ABS = 2e-6 per element.
  noise_embed   float64 sin / cos of arg = (5000 s) f_i, f_i = exp(e_i) with the fp32 exponent e_i the kernel forms; expf within 1 ulp
                (2 U) and two products: 3 U |arg|, + 2^-22 for sincosf, then the bf16 store.
"""
import math

import numpy as np

import ddpm_oracle as O

U = 2.0 ** -24
BF = 2.0 ** -8
FL = 2.0 ** -126
NORMAL_ABS = 2e-6                      # csrc/rng.h: "Absolute error of a normal <= 2e-6"
F32, F64 = np.float32, np.float64
FLOOR = float(F32(1e-10))
STREAM_EPS, STREAM_LABEL, STREAM_Z, STREAM_INIT, STREAM_INFILL = 0, 1, 2, 3, 4
OLD_STATE_REL, OLD_XT_REL, OLD_WALK_REL = 1e-5, 3e-3, 1e-2      # the whole-array rel-L2 criteria this file replaces
Q_FORMS = ("quads QPT 4", "quads QPT 1", "scalar VEC4", "scalar tail")


# ---------------------------------------------------------------------------------------------- number formats
def bf16_bits(x, truncate=False):
    """fp32 -> bf16 bit pattern (uint16), round to nearest even (or truncated: a planted fault)"""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    if truncate:
        return (b >> np.uint32(16)).astype(np.uint16)
    r = b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))
    return (r >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(F32).astype(F64)


def stored_bf16_bound(v, e):
    """bound of a bf16 store of the value v (float64 reference) that carries the error e"""
    return e + BF * (np.abs(v) + e) + FL


def ftz(x):
    """fp32 array with denormals flushed to zero"""
    x = np.asarray(x, dtype=F32)
    return np.where(np.abs(x) < F32(FL), F32(0) * x, x).astype(F32)


def fma32(a, b, c):
    """fp32 fma(a, b, c): the product is exact in float64, one rounding of the float64 sum first (harmless here)"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def rel_l2(a, b):
    a, b = np.asarray(a, F64).ravel(), np.asarray(b, F64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def worst_ratio(got, ref, bound):
    """largest |got - ref| / bound over ALL elements (a non-finite difference counts as infinite)"""
    d = np.abs(np.asarray(got, F64) - np.asarray(ref, F64))
    bound = np.broadcast_to(np.asarray(bound, F64), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / bound)
    q = np.where(np.isfinite(q), q, np.inf)
    return float(q.max()) if q.size else 0.0


def butterfly(v):
    """wave_sum / cross-wave order on an fp32 vector whose length is a power of two: xor offsets n/2 .. 1, returns lane 0"""
    v = np.asarray(v, dtype=F32).copy()
    o = v.size // 2
    while o:
        v = (v + v[np.arange(v.size) ^ o]).astype(F32)
        o //= 2
    return v[0]


# ---------------------------------------------------------------------------------------------- Philox normals
def philox_ctr(n4, sample, stream, step):
    c = np.zeros((n4, 4), np.uint32)
    c[:, 0] = np.arange(n4, dtype=np.uint32)
    c[:, 1], c[:, 2], c[:, 3] = np.uint32(sample), np.uint32(stream), np.uint32(step)
    return c


def philox_normals(B, per_sample, key, stream, step=0, sample_offset=0):
    """float64 Box-Muller of the kernel's Philox bits: [B][per_sample], element e of sample b from counter (e / 4, b + offset, stream, step)"""
    n4 = (per_sample + 3) // 4
    out = np.empty((B, per_sample), F64)
    k = np.array(key, np.uint32)
    for b in range(B):
        out[b] = O.philox_normal4(philox_ctr(n4, b + sample_offset, stream, step), k).reshape(-1)[:per_sample]
    return out


def label_draw_alpha_candidates(alphas_prod_ext, T, bglob, key, step=0):
    """label 0 without explicit alphas: alpha = max(lo, u (1 - lo) + lo), u from word 1 of the label block; the two fp32 values
    the expression can take (separate product and sum, or one fma)"""
    r = O.philox4x32(np.array([[0, bglob, STREAM_LABEL, step]], np.uint32), np.array(key, np.uint32))[0]
    u = (np.array([(r[1] >> np.uint32(9)) | np.uint32(0x3F800000)], np.uint32).view(F32) - F32(1))[0]
    lo = F32(alphas_prod_ext[T])
    w = F32(F32(1) - lo)
    return (np.maximum(lo, F32(F32(u * w) + lo)), np.maximum(lo, fma32(u, w, lo)))


# ---------------------------------------------------------------------------------------------- q_sample
def q_form(B, S, C, Cp):
    """the launcher's rule, restated for the host test only (the GPU test takes the form from the lab entry)"""
    groups = (S * C + 3) // 4
    if C % 4 == 0 and Cp % 4 == 0 and S * C < (1 << 22):
        return 0 if B * ((groups + 1023) // 1024) >= 1024 else 1
    return 2 if (S * C) % 4 == 0 else 3


def q_alpha_from_labels(labels, alphas_prod_ext, T):
    lab = np.clip(np.asarray(labels, np.int64), 0, T)
    assert (lab > 0).all(), "label 0 draws its alpha: label_draw_alpha_candidates"
    return np.asarray(alphas_prod_ext, F32)[lab - 1]


def q_sample_ref(x0, eps, alpha, dsm=False):
    """x0, eps [B][S][C] fp32; alpha [B] fp32 (dsm: the sigmas).  -> xt (float64, before the store), e_pre, s_out, e_s"""
    x0, eps = np.asarray(x0, F32).astype(F64), np.asarray(eps, F32).astype(F64)
    a = np.asarray(alpha, F32).astype(F64)
    sa, sb = (np.ones_like(a), a) if dsm else (np.sqrt(a), np.sqrt(1.0 - a))
    sh = (-1,) + (1,) * (x0.ndim - 1)
    p, q = sa.reshape(sh) * x0, sb.reshape(sh) * eps
    s = sb if dsm else sa
    return p + q, 4 * U * (np.abs(p) + np.abs(q)) + FL, s, (0.0 if dsm else 3 * U) * np.abs(s)


def q_sample_emu(x0, eps, alpha, dsm=False, fma=True, fault=None):
    """fp32 in the kernel's order.  fma: the explicit fma of the quads form (or a contracted scalar form), else product + product + sum"""
    x0, eps, a = np.asarray(x0, F32), np.asarray(eps, F32), np.asarray(alpha, F32)
    sa = np.ones_like(a) if dsm else np.sqrt(a).astype(F32)
    sb = a.copy() if dsm else np.sqrt((F32(1) - a).astype(F32)).astype(F32)
    if fault == "sb_is_one_minus_alpha" and not dsm:
        sb = (F32(1) - a).astype(F32)
    sh = (-1,) + (1,) * (x0.ndim - 1)
    p = ftz(sa.reshape(sh) * x0)
    xt = fma32(sb.reshape(sh), eps, p) if fma else (p + ftz(sb.reshape(sh) * eps)).astype(F32)
    return xt, (sb if dsm else sa)


def q_layout(xt, Cp, fill, fault=None):
    """bf16 bits of xt [B][S][C] in the [B*S][Cp] image pre-filled with `fill`; fault 'row_index': the quad that starts each row
    but the first is placed with the previous row's index (column C .. C+3: the padding of that row, or the next row's head)"""
    B, S, C = xt.shape
    img = np.full((B * S, Cp), fill, np.uint16)
    bits = bf16_bits(xt).reshape(B * S, C)
    img[:, :C] = bits
    if fault == "row_index":
        flat = img.reshape(-1)
        for r in range(1, B * S):
            if r % S:                                   # srow one too small: c = e - (srow - 1) C = C .. C + 3
                flat[(r - 1) * Cp + C:(r - 1) * Cp + C + 4] = bits[r, :4]
                img[r, :4] = fill
    return img


# ---------------------------------------------------------------------------------------------- mse_loss_grad
def loss_vec(C, Cp):
    return 4 if C % 4 == 0 and Cp % 4 == 0 else 1


def loss_grad_ref(pred, eps, inv, sigma=None, vec=1):
    """pred, eps [B][S][C] fp32, inv = the fp32 inv_global_count, sigma [B] fp32 or None.  -> grad, e_grad (before the store), loss, e_loss"""
    p, q = np.asarray(pred, F32).astype(F64), np.asarray(eps, F32).astype(F64)
    B, SC = p.shape[0], int(np.prod(p.shape[1:]))
    inv = float(F32(inv))
    n_t = vec * math.ceil(SC / (1024 * vec))
    ax = tuple(range(1, p.ndim))
    if sigma is None:
        d = p - q
        e_d = U * np.abs(d)
        g, e_g = d * (2.0 * inv), (e_d * 2.0 * inv + U * np.abs(d * 2.0 * inv))
        loss = (d * d).sum(ax) / SC
        e_loss = (n_t + 26) * U * loss + SC * FL
    else:
        sg = np.asarray(sigma, F32).astype(F64).reshape((-1,) + (1,) * (p.ndim - 1))
        d = sg * p + q
        e_d = 2 * U * (np.abs(sg * p) + np.abs(q)) + FL
        gs = sg * inv * SC
        g, e_g = d * gs, e_d * np.abs(gs) + 3 * U * np.abs(d * gs)
        loss = 0.5 * (d * d).sum(ax)
        e_loss = (n_t + 26) * U * loss + SC * FL + 0.5 * (2 * np.abs(d) * e_d + e_d * e_d).sum(ax)
    return g, e_g + FL, loss, e_loss


def loss_grad_emu(pred, eps, inv, sigma=None, vec=1, fault=None):
    """fp32 in the kernel's order: 1024 threads, VEC consecutive elements per trip, xor butterfly per wave, 16 sequential adds"""
    p, q = np.asarray(pred, F32), np.asarray(eps, F32)
    B, SC = p.shape[0], int(np.prod(p.shape[1:]))
    p, q = p.reshape(B, SC), q.reshape(B, SC)
    inv = F32(inv)
    if sigma is None:
        d = (p - q).astype(F32)
        gs = np.full((B, 1), F32(2) * inv if fault != "grad_factor_2" else inv, F32)
    else:
        sg = np.asarray(sigma, F32).reshape(B, 1)
        d = (ftz(sg * p) + q).astype(F32)
        gs = (F32(F32(sg * inv) * F32(SC))).astype(F32)
    grad = ftz(d * gs)
    sq = ftz(d * d)
    step = 1024 * vec
    trips = math.ceil(SC / step)
    pad = np.zeros((B, trips * step), F32)
    pad[:, :SC] = sq
    pad = pad.reshape(B, trips, 1024, vec)
    loss = np.empty(B, F32)
    for b in range(B):
        acc = np.zeros(1024, F32)
        for k in range(trips):
            for v in range(vec):
                acc = (acc + pad[b, k, :, v]).astype(F32)
        waves = [butterfly(acc[w * 64:(w + 1) * 64]) for w in range(16)]
        if fault == "loss_drops_a_wave":
            waves[15] = F32(0)
        t = F32(0)
        for w in waves:
            t = F32(t + w)
        loss[b] = F32(t / F32(SC)) if sigma is None else F32(F32(0.5) * t)
    return grad.reshape(np.asarray(pred).shape), loss


# ---------------------------------------------------------------------------------------------- reverse step / Langevin
def step_form(S, C, Cp=None, with_bf16=False):
    vec = 4 if C % 4 == 0 and (not with_bf16 or Cp % 4 == 0) else 1
    return vec, (4 if S >= 4 else 1)


def _clip(r):
    return np.minimum(np.maximum(r, -1.0), 1.0)


def reverse_step_ref(x, eh, z, cf, t, mask=None, samples=None, zi=None, z_abs=0.0, zi_abs=0.0):
    """x, eh, z [B][S][C] fp32 (z / zi may be float64 references of in-kernel draws that carry z_abs / zi_abs); cf = coef[t] (8 fp32).
    -> new state (float64), its bound, and (sigma z, e_sigma_z) for the noise metric"""
    x, eh = np.asarray(x, F32).astype(F64), np.asarray(eh, F32).astype(F64)
    sr, sm, mu1, mu2, sigma, _, sa, sb = (float(v) for v in np.asarray(cf, F32))
    noisy = t > 0
    a, b = sr * x, sm * eh
    r = a - b
    e_r = 2 * U * (np.abs(a) + np.abs(b)) + FL
    c = _clip(r)
    e_c = np.where(np.abs(r) <= 1 + e_r, e_r, 0.0)
    sz = sigma * np.asarray(z, F64) if noisy else np.zeros_like(x)
    e_sz = (U * np.abs(sz) + abs(sigma) * z_abs + FL) if noisy else np.zeros_like(x)
    nx = mu1 * c + mu2 * x + sz
    e_x = abs(mu1) * e_c + 3 * U * (np.abs(mu1 * c) + np.abs(mu2 * x) + np.abs(sz)) + (abs(sigma) * z_abs if noisy else 0.0) + FL
    if mask is not None:
        m, s = np.asarray(mask, F32).astype(F64), np.asarray(samples, F32).astype(F64)
        if noisy:
            y = sa * s + sb * np.asarray(zi, F64)
            e_y = 2 * U * (np.abs(sa * s) + np.abs(sb * np.asarray(zi, F64))) + abs(sb) * zi_abs + FL
        else:
            y, e_y = s, np.zeros_like(s)
        u, v = nx * (1 - m), y * m
        nx, e_x = u + v, np.abs(1 - m) * e_x + np.abs(m) * e_y + 3 * U * (np.abs(u) + np.abs(v)) + FL
    return nx, e_x, sz, e_sz


def langevin_step_ref(x, g, z, alpha, coef, mask=None, samples=None, zi=None, infill_sigma=0.0, z_abs=0.0, zi_abs=0.0):
    x, g, z = np.asarray(x, F32).astype(F64), np.asarray(g, F32).astype(F64), np.asarray(z, F64)
    alpha, coef, isg = float(F32(alpha)), float(F32(coef)), float(F32(infill_sigma))
    stp, nz = alpha * g, coef * z
    nx = x + stp + nz
    e_x = 3 * U * (np.abs(x) + np.abs(stp) + np.abs(nz)) + abs(coef) * z_abs + FL
    if mask is not None:
        m, s = np.asarray(mask, F32).astype(F64), np.asarray(samples, F32).astype(F64)
        y = s + isg * np.asarray(zi, F64)
        e_y = 2 * U * (np.abs(s) + np.abs(isg * np.asarray(zi, F64))) + abs(isg) * zi_abs + FL
        u, v = nx * (1 - m), y * m
        nx, e_x = u + v, np.abs(1 - m) * e_x + np.abs(m) * e_y + 3 * U * (np.abs(u) + np.abs(v)) + FL
    return nx, e_x, (stp, U * np.abs(stp) + FL), (nz, U * np.abs(nz) + abs(coef) * z_abs + FL)


def norm_metric_ref(v, e_v, depth):
    """v, e_v [B][S][C] float64: per sample sum_c sqrt(sum_s v^2 + 1e-10), or sqrt(sum_c v^2 + 1e-10) for S == 1, with its bound:
    depth U relative for the summation, the carried error through the triangle inequality, S FL per column for flushed squares"""
    B, S, C = v.shape
    if S > 1:
        col = np.sqrt((v * v).sum(1) + FLOOR)
        m = col.sum(1)
        carried = np.sqrt((e_v * e_v).sum(1)).sum(1)
        flush = (S * FL / (2 * np.sqrt(FLOOR))) * C
    else:
        m = np.sqrt((v * v).sum((1, 2)) + FLOOR)
        carried = np.sqrt((e_v * e_v).sum((1, 2)))
        flush = C * FL / (2 * np.sqrt(FLOOR))
    return m, depth * U * m + carried + flush


def reverse_depth(S, C, vec, rg):
    return S / rg + rg + vec * math.ceil(C / (128 * vec)) + 12


def langevin_depth(S, C):
    return S + 1 + math.ceil(C / 256) + 12


def reverse_metrics_ref(x, eh, nx, e_x, sz, e_sz, vec, rg):
    """[B][3] (eps_hat norm, step norm, noise norm) and bounds, from the float64 state reference"""
    x, eh = np.asarray(x, F32).astype(F64), np.asarray(eh, F32).astype(F64)
    depth = reverse_depth(x.shape[1], x.shape[2], vec, rg)
    out = [norm_metric_ref(eh, np.zeros_like(eh), depth), norm_metric_ref(x - nx, e_x, depth), norm_metric_ref(sz, e_sz, depth)]
    return np.stack([o[0] for o in out], 1), np.stack([o[1] for o in out], 1)


def langevin_metrics_ref(g, stp, nz):
    g = np.asarray(g, F32).astype(F64)
    depth = langevin_depth(g.shape[1], g.shape[2])
    out = [norm_metric_ref(g, np.zeros_like(g), depth), norm_metric_ref(stp[0], stp[1], depth), norm_metric_ref(nz[0], nz[1], depth)]
    return np.stack([o[0] for o in out], 1), np.stack([o[1] for o in out], 1)


def _metric_emu(cols32, S, threads, vec, fault=None):
    """cols32 [3][C] fp32 column sums of one sample -> the three metrics in the kernel's order: per column sqrt (S > 1), the thread's
    own columns (col = trip threads vec + thread vec + v), butterfly over the first 128 threads' two waves (threads = 128) or the
    256 threads' four waves (Langevin), one (three) adds"""
    C = cols32.shape[1]
    per = threads * vec
    trips = math.ceil(C / per)
    res = []
    for k in range(3):
        v = cols32[k].astype(F32)
        per_col_sqrt = S > 1 or fault == "sqrt_per_column"
        if per_col_sqrt:
            v = np.sqrt((v + F32(1e-10)).astype(F32)).astype(F32)
        pad = np.zeros(trips * per, F32)
        pad[:C] = v
        pad = pad.reshape(trips, threads, vec)
        acc = np.zeros(threads, F32)
        for tr in range(trips):
            for j in range(vec):
                acc = (acc + pad[tr, :, j]).astype(F32)
        waves = [butterfly(acc[w * 64:(w + 1) * 64]) for w in range(threads // 64)]
        tot = F32(waves[0] + waves[1]) if threads == 128 else F32(F32(waves[0] + waves[1]) + F32(waves[2] + waves[3]))
        res.append(tot if per_col_sqrt else F32(np.sqrt(F32(tot + F32(1e-10)))))
    return np.array(res, F32)


def reverse_step_emu(x, eh, z, cf, t, vec, rg, mask=None, samples=None, zi=None, fma=False, fault=None, cf_row=None):
    """fp32 in the kernel's order -> new state [B][S][C] fp32, metrics [B][3] fp32.  fma: contracted products (both forms must sit in
    the bound).  cf_row: the row the infill coefficients are taken from (fault 'blend_at_level_t' passes another row)."""
    x, eh = np.asarray(x, F32), np.asarray(eh, F32)
    B, S, C = x.shape
    sr, sm, mu1, mu2, sigma, _, sa, sb = (F32(v) for v in np.asarray(cf, F32))
    if fault == "blend_at_level_t":
        sa, sb = F32(cf_row[6]), F32(cf_row[7])
    noisy = t > 0 or fault == "z_at_t0"
    zz = np.asarray(z, F32)
    sz = ftz(zz * (sigma if fault != "z_unscaled" else F32(1))) if noisy else np.zeros_like(x)
    if fma:
        r = fma32(sr, x, -ftz(sm * eh))
    else:
        r = (ftz(sr * x) - ftz(sm * eh)).astype(F32)
    if fault == "clamp_after_mu1":
        nx0 = np.minimum(np.maximum(ftz(mu1 * r), F32(-1)), F32(1))
    else:
        c = np.minimum(r, F32(1)) if fault == "no_negative_clamp" else np.minimum(np.maximum(r, F32(-1)), F32(1))
        nx0 = ftz(mu1 * c)
    nx = (fma32(mu2, x, nx0) + sz).astype(F32) if fma else ((nx0 + ftz(mu2 * x)).astype(F32) + sz).astype(F32)
    if mask is not None:
        m, s, zi32 = np.asarray(mask, F32), np.asarray(samples, F32), (np.asarray(zi, F32) if zi is not None else None)
        if fault == "mask_inverted":
            m = (F32(1) - m).astype(F32)
        if t > 0:
            ca, cb = (sb, sa) if fault == "infill_coef_swapped" else (sa, sb)
            y = fma32(ca, s, ftz(cb * zi32)) if fma else (ftz(ca * s) + ftz(cb * zi32)).astype(F32)
        else:
            y = s
        nx = (ftz(nx * (F32(1) - m).astype(F32)) + ftz(y * m)).astype(F32)
    if fault == "stale_last_column":
        nx[:, :, C - 1] = x[:, :, C - 1]
    st = (x - nx).astype(F32)
    met = np.empty((B, 3), F32)
    for b in range(B):
        cols = np.zeros((3, C), F32)
        for k, v in enumerate((eh[b], st[b], sz[b])):
            sq = ftz(v * v)
            parts = []
            for g in range(rg):
                acc = np.zeros(C, F32)
                for s_ in range(g, S, rg):
                    acc = (acc + sq[s_]).astype(F32)
                parts.append(acc)
            if fault == "drops_a_row_group" and rg > 1:
                parts[(S - 1) % rg] = np.zeros(C, F32)                      # the partial of the group that holds the last row is lost
            tot = np.zeros(C, F32)
            for pacc in parts:
                tot = (tot + pacc).astype(F32)
            cols[k] = tot
        met[b] = _metric_emu(cols, S, 128, vec, fault)
    return nx, met


def langevin_step_emu(x, g, z, alpha, coef, mask=None, samples=None, zi=None, infill_sigma=0.0, fault=None):
    x, g, z = np.asarray(x, F32), np.asarray(g, F32), np.asarray(z, F32)
    B, S, C = x.shape
    alpha, coef, isg = F32(alpha), F32(coef), F32(infill_sigma)
    noise = ftz(coef * z)
    stp = ftz(alpha * g)
    if fault == "noise_coef_on_gradient":
        noise, stp = z.copy(), ftz(coef * g)
    nx = ((x + stp).astype(F32) + noise).astype(F32)
    if mask is not None:
        m, s = np.asarray(mask, F32), np.asarray(samples, F32)
        y = (s + ftz(isg * np.asarray(zi, F32))).astype(F32)
        nx = (ftz(nx * (F32(1) - m).astype(F32)) + ftz(y * m)).astype(F32)
    met = np.empty((B, 3), F32)
    for b in range(B):
        cols = np.zeros((3, C), F32)
        for k, v in enumerate((g[b], stp[b], noise[b])):
            sq = ftz(v * v)
            acc = np.zeros(C, F32)
            for s_ in range(S):
                acc = (acc + sq[s_]).astype(F32)
            cols[k] = acc
        met[b] = _metric_emu(cols, S, 256, 1)
    return nx, met


# ---------------------------------------------------------------------------------------------- noise embedding
def noise_embed_ref(s, channels):
    """-> values [n][channels] float64 and the bound of the stored bf16"""
    s = np.asarray(s, F32)
    half = channels // 2
    k32 = F32(F32(9.210340371976184) / F32(half - 1))
    e32 = (np.arange(half, dtype=F32) * F32(-k32)).astype(F32)
    arg = (5000.0 * s.astype(F64))[:, None] * np.exp(e32.astype(F64))[None, :]
    v = np.zeros((s.size, channels), F64)
    v[:, :half], v[:, half:2 * half] = np.sin(arg), np.cos(arg)
    e = np.zeros_like(v)
    e[:, :half] = e[:, half:2 * half] = 3 * U * np.abs(arg) + 2.0 ** -22
    return v, stored_bf16_bound(v, e)


def noise_embed_emu(s, channels):
    s = np.asarray(s, F32)
    half = channels // 2
    k32 = F32(F32(9.210340371976184) / F32(half - 1))
    f = np.exp((np.arange(half, dtype=F32) * F32(-k32)).astype(F32)).astype(F32)
    arg = ((F32(5000) * s).astype(F32)[:, None] * f[None, :]).astype(F32)
    v = np.zeros((s.size, channels), F32)
    v[:, :half], v[:, half:2 * half] = np.sin(arg.astype(F64)).astype(F32), np.cos(arg.astype(F64)).astype(F32)
    return bf16_value(bf16_bits(v))


# ---------------------------------------------------------------------------------------------- regimes
def ulp_nudge(v, k):
    """fp32 array moved by k ulps"""
    b = np.ascontiguousarray(v, dtype=F32).view(np.int32)
    return (b + np.where(b >= 0, k, -k).astype(np.int32)).view(F32)


REVERSE_REGIMES = ("normal", "clamped", "edge", "cancel", "tiny", "huge")


def reverse_regime(name, shape, cf, rng):
    """(x, eps_hat) fp32 of a value regime of the reverse step at the coefficients cf"""
    sr, sm = F32(cf[0]), F32(cf[1])
    x = rng.standard_normal(shape).astype(F32)
    if name == "normal":
        eh = rng.standard_normal(shape).astype(F32)
    elif name == "clamped":                                  # |r| >> 1, both signs
        sign = np.where(rng.random(shape) < 0.5, F32(-1), F32(1))
        x = (sign * (F32(3) + np.abs(x)) / sr).astype(F32)
        eh = (-sign * F32(2) / np.maximum(sm, F32(1e-3))).astype(F32)
    elif name == "edge":                                     # r within +-4 ulp of +-1
        sign = np.where(rng.random(shape) < 0.5, F32(-1), F32(1))
        if sm > F32(1e-6):
            eh = ((sr * x - sign) / sm).astype(F32)
            eh = ulp_nudge(eh, rng.integers(-4, 5, shape))
        else:
            x, eh = ulp_nudge((sign / sr).astype(F32), rng.integers(-4, 5, shape)), np.zeros(shape, F32)
    elif name == "cancel":                                   # r ~ 0: the two products agree to rounding
        eh = (sr * x / np.maximum(sm, F32(1e-6))).astype(F32) if sm > F32(1e-6) else np.zeros(shape, F32)
        if sm <= F32(1e-6):
            x = np.zeros(shape, F32)
    elif name == "tiny":
        x, eh = (x * F32(1e-20)).astype(F32), (rng.standard_normal(shape) * 1e-20).astype(F32)
    elif name == "huge":
        x, eh = (x * F32(1e15)).astype(F32), rng.standard_normal(shape).astype(F32)
    else:
        raise KeyError(name)
    return x, eh


MASKS = ("none", "zeros", "ones", "binary", "quarter")


def make_mask(name, shape, rng):
    if name == "none":
        return None
    if name == "zeros":
        return np.zeros(shape, F32)
    if name == "ones":
        return np.ones(shape, F32)
    if name == "binary":
        return (rng.random(shape) < 0.5).astype(F32)
    return np.full(shape, 0.25, F32)


LOSS_REGIMES = ("normal", "equal", "huge", "tiny", "spike")


def loss_regime(name, shape, rng):
    pred = rng.standard_normal(shape).astype(F32)
    eps = rng.standard_normal(shape).astype(F32)
    if name == "equal":
        pred = ulp_nudge(eps, rng.integers(-3, 4, shape))
    elif name == "huge":
        pred, eps = (pred * F32(1e15)).astype(F32), (eps * F32(1e15)).astype(F32)
    elif name == "tiny":
        pred, eps = (pred * F32(1e-25)).astype(F32), (eps * F32(1e-25)).astype(F32)
    elif name == "spike":
        pred, eps = (pred * F32(1e-3)).astype(F32), (eps * F32(1e-3)).astype(F32)
        pred.reshape(pred.shape[0], -1)[:, pred[0].size // 2] = F32(3e4)
    return pred, eps


# shapes of the issue (B, S, C[, Cp]) per form
REVERSE_SHAPES = {
    (4, 4): [(3, 32, 512), (2, 5, 516), (2, 4, 1024), (2, 7, 8)],
    (1, 4): [(3, 32, 42), (2, 6, 130), (2, 4, 1), (2, 32, 8, 10)],
    (4, 1): [(5, 1, 512), (3, 1, 1028), (2, 3, 64)],
    (1, 1): [(5, 1, 42), (3, 1, 146), (2, 3, 42), (4, 1, 1)],
}
Q_SHAPES = {
    0: [(512, 32, 132), (1024, 3, 44), (1, 349525, 12)],        # the last: the row index at its limit, S C = 2^22 - 12 (1024 blocks)
    1: [(9, 32, 512), (9, 1, 4)],
    2: [(1, 1048576, 4), (9, 2, 42), (9, 32, 8, 10)],
    3: [(9, 1, 42), (9, 3, 42), (9, 1, 1)],
}
LOSS_SHAPES = [(5, 32, 512), (3, 1, 512), (5, 3, 42), (2, 1, 1), (2, 5, 516)]
LANGEVIN_SHAPES = [(3, 32, 42), (2, 32, 512), (2, 5, 300), (5, 1, 42), (3, 1, 600), (4, 1, 1)]


T = 1000


def tables():
    """the linear schedule the other tests use: betas, coef [T][8], slot [T], alphas_prod_ext [T + 1] (all as the kernels read them)"""
    import smd_amd.schedule as S
    betas = S.create_noise_schedule(1e-6, 0.01, T, "linear")
    ap_ext = np.concatenate([np.ones(1, F32), S.alphas_cumprod(betas)]).astype(F32)
    return betas, S.reverse_coefficient_table(betas), S.collection_slot_table(T).astype(np.int32), ap_ext


def reverse_timesteps(slot):
    """T - 1, a t with a collection slot, one without, 1, 0"""
    mid = np.arange(2, T - 1)
    with_slot = int(mid[(slot[mid] >= 0) & (slot[mid] <= 40)][len(mid) // 80])
    without = int(mid[slot[mid] < 0][len(mid) // 3])
    return (T - 1, with_slot, without, 1, 0)


def reverse_cases(slot):
    """(shape, t, regime, mask) of every reverse-step case: every regime without infill and every mask on N(0,1), at every timestep"""
    for form, shapes in REVERSE_SHAPES.items():
        for shape in shapes:
            for t in reverse_timesteps(slot):
                for regime in REVERSE_REGIMES:
                    yield form, padded(shape), t, regime, "none"
                for mask in MASKS[1:]:
                    yield form, padded(shape), t, "normal", mask


def case_rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def padded(shape):
    """(B, S, C, Cp): Cp defaults to C rounded up to a multiple of 8 plus nothing for C % 4 == 0, else C + 6 (an odd stride)"""
    if len(shape) == 4:
        return shape
    B, S, C = shape
    return B, S, C, (C + 8 if C % 4 == 0 else C + 6)
