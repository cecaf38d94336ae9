"""Element-wise criterion for the LayerNorm kernels of csrc/norm.hip (and the same one-pass statistics in ln128.hip / net_f32.hip):
float64 model of the op and its backward, derived per-element bounds, row regimes that are built exactly, FiLM and dout regimes,
an fp32 emulation of the kernels' arithmetic and planted faults.  torch float64 / float32 on the CPU only, no GPU.  U, hulp,
worst_ratio, rel and ln_fwd_bound are those of tests/_attn_ref.py (imported, one definition).

The op, as oracle/ddpm_oracle.py defines it (layer_norm, FeaturewiseAffine, swish), n = D columns, eps = 1e-6:
    m = mean(x)   var = mean(x^2) - m^2 (biased)   rs = 1 / sqrt(var + eps)   xh = (x - m) rs   y0 = xh gamma + beta
    pre = scale y0 + shift  (FiLM: the row's sample, or with t_ptr the one table row clamp(*t_ptr, 0, film_rows - 1))   out = swish(pre)
    d = dout swish'(pre);  dscale (= | +=) sum_rows d y0;  dshift (= | +=) sum_rows d;  d2 = d scale;  dgamma = sum d2 xh;  dbeta = sum d2
    dxh = d2 gamma;  dx = rs (dxh - mean(dxh) - xh mean(dxh xh)) + dres;      saved statistics (m, rs) per row
    e4m3 copy: q = e4m3(out 2^-ex), ex = e4m3_row_exponent(max_row |out|) (smd_common.h), dequantised q 2^ex

Contract: |x| < 2^55, so that sum x^2 over 4096 columns stays finite in fp32 (2^110 * 2^12 < 2^128); the regimes use at most 2^40.

Bound.  U = 2^-24; an fp32 operation costs U |result|; products of two first-order terms are covered by the factor SECOND = 1 + 2^-10.
  sums      A sum of n terms in ANY order is off by at most (n - 1) U sum|terms|; n + 2 is used (as ln_fwd_bound does): the kernels of
            this family sum a row in three different layouts (64 lanes x D / 64 values, 16 lanes x 8, and the fp32 kernel's strided
            walk), so no single path depth applies.  tests/test_gpu_ln_saved_stats.py derives "at most 38 roundings" for ONE layout,
            the 2048-wide row on 64 lanes (32 sequential + 6 shuffle steps); that count is right for that kernel and is used there
            for the saved statistics of that kernel only.  Here n + 2 is used everywhere: it is 54 times looser at D = 2048 but
            holds for every kernel, every D and the sequential emulation.
  mean      dm = (n + 2) U mean|x|   (1 / D is a power of two: the scaling is exact)
  variance  the kernels form E[x^2] - mean^2 in fp32 in one pass:
            dvar = (n + 3) U E[x^2] + 2 |m| dm + dm^2 + 3 U (E[x^2] + m^2) + 2 U eps
            (squares and their sum; the error of the computed mean, squared; product, difference and the addition of fp32(eps)).
  rstd      as an INTERVAL, finite on every row: the kernel's argument is fl(var + eps) within dvar of the true one and, by the clamp
            in smd_ln_rstd, never below eps, and v_rsq_f32 is within 1 ulp (2 U) + the argument's rounding:
            rs in [rsqrt(var + eps + dvar) (1 - 3 U), rsqrt(max(var + eps - dvar, eps (1 - 2 U))) (1 + 3 U)] = [lo, hi],
            drs = max(hi - rs, rs - lo).  Without the clamp the upper end does not exist (argument <= 0: inf or NaN).
  xh        row kernel fl(fl(x - m^) rs^), wide kernels fma(x, rs^, fl(-m^ rs^)).  With c = x - m:
            exh = |c| drs + (dm + U (|m| + |c|)) hi + U |xh|.  The U |m| hi term is the wide form's rounded offset; the row form has
            U |c| hi instead.  Both are far below dm hi >= (n + 2) U |m| hi, so ONE bound serves both at a cost below 1 / n.
  y0, pre   unfolded (row kernel): fl(fl(xh g) + b), fl(fl(sc y0) + sh); folded (wide): A = fl(sc g), C = fma(sc, b, sh), fma(xh, A, C).
            epre = |sc| |g| exh + U (2 |sc g xh| + 2 |sc y0| + |sc b + sh| + |pre|): the sum of both forms' roundings; all of them are
            U-sized against an exh of n U, so again one bound (cost far below a factor of two).
  sigmoid   sigmoidf_(x) = rcp(1 + __expf(-x)), __expf = exp2(x log2e): constant and product move the argument by 2 U |x| log2e, i.e.
            e relatively by 2 U |x|; exp2 is within 1 ulp: eps_e = expm1(2 U |x|) + 2 U.  d = 1 + e costs U d ABSOLUTE, rcp 2 U:
            ds = s (1 - s) eps_e + 3 U s.  Where e (1 + eps_e) < 2^-25, fl(1 + e) = 1 and rcp(1) = 1: the kernel's s IS 1, ds = 1 - s.
            Where x < -87 the kernel's e overflows (or 1 / d is a denormal that may be flushed): its s is 0 or below 2^-126, ds = s.
            TINY = 2^-100 absolute is added for flushed results.
  swish     |swish''| <= 1/2 (at 0; the host test measures it): eout = (|swish'(pre)| + epre / 2) epre + |pre| ds + U |out|,
            + hulp(|out| + eout) for the bf16 store.
  swish'    swish_gradf_ = s (1 + x (1 - s)), 1 - s from the SAME rounded s: d/ds = 1 + x (1 - 2 s), so
            esg = |1 + x (1 - 2 s)| ds + |x| ds^2 + U (2 s (1 - s) |x| + 2 |sg|) + (|swish''(pre)| + S3 epre) epre, S3 = 1/2 >= max |swish'''|.
  d, dxh    ed = |dout| esg + U |d|;  edxh = (ed |sc| + 2 U |d2|) |g|
  dx        t1 = mean(dxh), t2 = mean(dxh xh): et1 = mean(edxh) + (n + 2) U mean|dxh|,
            et2 = mean(edxh |xh| + |dxh| exh) + (n + 3) U mean|dxh xh|;  inner = dxh - t1 - xh t2,
            einner = edxh + et1 + exh |t2| + (|xh| + exh) et2 + 3 U (|dxh| + |t1| + |xh t2|)   (exh et2 and the like are kept: on a
            constant row exh is NOT small -- dm hi is 1000 dm -- and the products of two errors are the leading terms);
            edx = drs |inner| + hi einner + 3 U rs^2 |t2| (|x| + |m|) + 2 U (|rs inner| + |dres| + |dx|)
            (the third term: the 8-wave kernel evaluates rs dxh - (rs^2 t2) x - rs (t1 - m rs t2), whose last two products cancel
            at the size rs^2 |t2| |m|); + hulp for a bf16 dx.  Saved and recomputed statistics obey the same interval.
  columns   dgamma, dbeta, dscale, dshift are sums over rows in three stages (rows inside a wave, waves through LDS, groups in the
            reduce kernel): (terms + 3 + 3) U sum|terms| (3 stages, 3 roundings of the factors) + the propagated error of every term.
            The wide kernels build dscale as gamma P + beta Q and dgamma as scale P (P = sum d xh, Q = sum d); the bound is written
            on |d| (|g xh| + |b|) >= |d y0| so that it holds for both.
  e4m3      half an e4m3 spacing at the scaled value (2^(floor(log2 v) - 4), 2^-10 below 2^-6) times 2^ex, + the fp32 error of the
            value.  ex must be e4m3_row_exponent of the reference row maximum; only where that maximum lies within its own bound of a
            step of the exponent (mantissa 1.75) the neighbouring value is admissible: ex(max - bound) <= ex <= ex(max + bound).
Nothing is fitted to GPU output.
"""
import math

import torch

from _attn_ref import U, F64, bf, hulp, worst_ratio, rel, ln_fwd_bound      # noqa: F401  (one definition, re-exported)

EPS = 1e-6
SECOND = 1.0 + 2.0 ** -10
TINY = 2.0 ** -100
S2, S3 = 0.5, 0.5
XMAX = 2.0 ** 55
OLD_BF16_REL, OLD_F32_REL, OLD_E4M3_REL = 4e-3, 1e-4, 4e-2       # the whole-tensor thresholds of tests/test_gpu_kernels.py / test_gpu_fp8.py

ROW_KINDS = ("unit", "offset", "edge", "tiny", "zero", "const3", "const10", "const100", "nearconst", "outlier", "huge")
CONST = {"const3": 3.3, "const10": 10.1, "const100": 100.3}
FILM_KINDS = ("near1", "zero", "neg", "sat30", "sat100")
DOUT_KINDS = ("unit", "zero", "big", "comb")


def group_rows(film, rps):
    return rps if film else 32


# ------------------------------------------------------------------------------------------------ closed forms
def swish(x):
    return x * torch.sigmoid(x)


def swish_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * torch.sigmoid(-x))


def swish_grad2(x):
    s, o = torch.sigmoid(x), torch.sigmoid(-x)
    return s * o * (2 + x * (o - s))


def e4m3_row_exponent(amax):
    """smd_common.h: floor(log2 amax) - 8, + 1 when the mantissa exceeds 1.75; 0 for amax == 0 (float64 tensor in, int64 out)"""
    a = amax.double().float().double()
    m, e = torch.frexp(a.clamp_min(2.0 ** -140))              # a = m 2^e, m in [0.5, 1)
    ex = e - 1 - 8 + (m * 2 > 1.75).long()
    return torch.where(a > 0, ex.clamp_min(-126), torch.zeros_like(ex))


def e4m3_half_spacing(v):
    """half the spacing of e4m3 at |v| (already scaled, <= 448)"""
    v = v.abs().clamp_min(2.0 ** -6)
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e - 1 - 4)


def e4m3_round(v):
    """round to nearest e4m3 (ties to even), saturating at 448: through torch's float8_e4m3fn"""
    return v.clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn).float().double()


# ------------------------------------------------------------------------------------------------ row statistics and their bounds
def stats(x):
    x = x.double()
    n = x.shape[-1]
    mean = lambda t: t.mean(-1, keepdim=True)
    m, q, a = mean(x), mean(x * x), mean(x.abs())
    var = mean((x - m) ** 2)                                  # two passes in float64: no cancellation
    dm = (n + 2) * U * a
    dvar = SECOND * ((n + 3) * U * q + 2 * m.abs() * dm + dm * dm + 3 * U * (q + m * m) + 2 * U * EPS)
    A = var + EPS
    rs = A.rsqrt()
    lo = (A + dvar).rsqrt() * (1 - 3 * U)
    hi = torch.maximum(A - dvar, torch.full_like(A, EPS * (1 - 2 * U))).rsqrt() * (1 + 3 * U)
    return dict(n=n, m=m, q=q, var=var, dm=dm, dvar=dvar, rs=rs, lo=lo, hi=hi, drs=torch.maximum(hi - rs, rs - lo))


def xh_err(x, st):
    c = x.double() - st["m"]
    xh = c * st["rs"]
    return xh, SECOND * (c.abs() * st["drs"] + (st["dm"] + U * (st["m"].abs() + c.abs())) * st["hi"] + U * xh.abs())


def sig_err(x):
    s, o = torch.sigmoid(x), torch.sigmoid(-x)
    eps_e = torch.expm1(2 * U * x.abs().clamp_max(1e6)) + 2 * U
    ds = s * o * eps_e + 3 * U * s
    one = torch.exp(-x.clamp(-700.0, 700.0)) * (1 + eps_e) < 2.0 ** -25
    ds = torch.where(one, o, ds)
    ds = torch.where(x < -87.0, torch.maximum(ds, s), ds)
    return s, o, ds


def film_rows_of(pr, fault=None):
    """(scale, shift) [rows][D] float64 as each row reads them, or (None, None)"""
    if not pr["film"]:
        return None, None
    D, rows = pr["D"], pr["rows"]
    ss = pr["ss"].double()
    if pr.get("t") is not None:
        T, t = ss.shape[0], pr["t"]
        idx = torch.full((rows,), (t % T) if fault == "t-unclamped" else min(max(t, 0), T - 1))
    else:
        idx = torch.arange(rows) // pr["rps"]
        if fault == "film-neighbour-sample":
            idx = (idx + 1) % ss.shape[0]
    return ss[idx, :D], ss[idx, D:]


# ------------------------------------------------------------------------------------------------ the model (reference and faults)
FWD_FAULTS = ("no-eps", "unbiased-variance", "rsqrt-unclamped", "film-neighbour-sample", "C-beta-plus-shift", "t-unclamped",
              "ragged-last-row-dropped", "columns-swapped", "e4m3-exponent-off-by-one")
BWD_FAULTS = ("dx-missing-mean-term", "dres-twice", "dgamma-missing-last-group", "dscale-overwritten", "rstd-of-previous-row")
FAULTS = FWD_FAULTS + BWD_FAULTS


def model(pr, fault=None, backward=True):
    """float64 model of the op on the problem `pr` (see problem()); `fault` plants one of FAULTS.  Without one it is the reference."""
    x, g, b = pr["x"].double(), pr["gamma"].double(), pr["beta"].double()
    rows, D = x.shape
    m = x.mean(-1, keepdim=True)
    var = ((x - m) ** 2).mean(-1, keepdim=True)
    if fault == "unbiased-variance":
        var = var * D / (D - 1)
    arg = var + (0.0 if fault == "no-eps" else EPS)
    if fault == "rsqrt-unclamped":                           # the one-pass fp32 argument as the 64-lane kernels form it, not clamped
        arg = emu_stats(pr["x"], "wave", clamp=False)[2].double()
    rs = arg.rsqrt()
    xh = (x - m) * rs
    y0 = xh * g + b
    sc, sh = film_rows_of(pr, fault)
    pre = y0
    if sc is not None:
        pre = sc * xh * g + (b + sh) if fault == "C-beta-plus-shift" else sc * y0 + sh
    out = swish(pre) if pr["swish"] else pre
    if fault == "ragged-last-row-dropped" and rows % group_rows(pr["film"] and pr.get("t") is None, pr["rps"]) != 0:
        out = out.clone()
        out[-1] = 0.0
    if fault == "columns-swapped":                            # lane 5, second 256-column chunk (or the only one): its columns 1 and 2
        c0 = (256 if D > 256 else 0) + (20 if D > 128 else 10)
        out = out.clone()
        out[:, [c0 + 1, c0 + 2]] = out[:, [c0 + 2, c0 + 1]]
    r = dict(m=m[:, 0], rs=rs[:, 0], xh=xh, y0=y0, pre=pre, out=out, sc=sc, sh=sh)
    amax = out.abs().max(-1, keepdim=True).values
    ex = e4m3_row_exponent(amax) + (1 if fault == "e4m3-exponent-off-by-one" else 0)
    r.update(amax=amax[:, 0], ex=ex[:, 0], deq=torch.ldexp(e4m3_round(torch.ldexp(out, -ex)), ex))
    if not backward or pr.get("dout") is None or pr.get("t") is not None:
        return r
    dout = pr["dout"].double()
    d = dout * swish_grad(pre) if pr["swish"] else dout
    gr = group_rows(pr["film"], pr["rps"])
    if sc is not None:
        ns = rows // pr["rps"]
        dsc = (d * y0).view(ns, pr["rps"], D).sum(1)
        dsh = d.view(ns, pr["rps"], D).sum(1)
        dss = torch.cat([dsc, dsh], 1)
        if pr["accumulate"] and fault != "dscale-overwritten":
            dss = dss + pr["dss0"].double()
        r["dss"] = dss
        d2 = d * sc
    else:
        d2 = d
    rsb, xhb = rs, xh
    if fault == "rstd-of-previous-row":
        rsb = torch.roll(rs, 1, 0)
        xhb = (x - m) * rsb
    keep = rows - (rows - 1) % gr - 1 if fault == "dgamma-missing-last-group" else rows      # rows in front of the last group
    r["dgamma"], r["dbeta"] = (d2 * xhb)[:keep].sum(0), d2[:keep].sum(0)
    dxh = d2 * g
    t1 = 0.0 if fault == "dx-missing-mean-term" else dxh.mean(-1, keepdim=True)
    t2 = (dxh * xhb).mean(-1, keepdim=True)
    dx = rsb * (dxh - t1 - xhb * t2)
    if pr.get("dres") is not None:
        dx = dx + pr["dres"].double() * (2.0 if fault == "dres-twice" else 1.0)
    r.update(d=d, d2=d2, dxh=dxh, t1=t1, t2=t2, dx=dx)
    return r


# ------------------------------------------------------------------------------------------------ bounds
def bounds(pr, ref):
    """per-element bounds of every output of the reference `ref` = model(pr): mean, rstd (lo / hi), out (bf16 store), y (the fp32
    value in front of the store), dx_f32, dx_bf16, dgamma, dbeta, dss"""
    x, g, b = pr["x"].double(), pr["gamma"].double(), pr["beta"].double()
    rows, D = x.shape
    st = stats(x)
    xh, exh = xh_err(x, st)
    ag, ab = g.abs(), b.abs()
    y0 = ref["y0"]
    sc, sh = ref["sc"], ref["sh"]
    if sc is not None:
        pre = sc * y0 + sh
        asc = sc.abs()
        epre = SECOND * (asc * ag * exh + U * (2 * (sc * g * xh).abs() + 2 * (sc * y0).abs() + (sc * b + sh).abs() + pre.abs()))
    else:
        pre, asc = y0, torch.ones_like(y0)
        epre = SECOND * (ag * exh + U * ((xh * g).abs() + y0.abs()))
    if pr["swish"]:
        s, o, ds = sig_err(pre)
        out = pre * s
        ey = SECOND * ((swish_grad(pre).abs() + S2 * epre) * epre + pre.abs() * ds + U * out.abs()) + TINY
    else:
        out, ey = pre, epre
    B = dict(mean=st["dm"][:, 0] + U * st["m"][:, 0].abs(), rs_lo=st["lo"][:, 0], rs_hi=st["hi"][:, 0], y=ey, out=ey + hulp(out.abs() + ey), st=st)
    B["amax_err"] = ey.max(-1).values
    if "dx" not in ref:
        return B
    dout = pr["dout"].double()
    if pr["swish"]:
        sg = swish_grad(pre)
        esg = SECOND * ((1 + pre * (o - s)).abs() * ds + pre.abs() * ds * ds + U * (2 * s * o * pre.abs() + 2 * sg.abs())
                        + (swish_grad2(pre).abs() + S3 * epre) * epre) + TINY
        d = dout * sg
        ed = SECOND * (dout.abs() * esg + U * d.abs())
    else:
        d, ed = dout, torch.zeros_like(dout) + pr.get("dout_err", 0.0)      # dout_err: dout is itself a rounded sum (ln128_bwd_parts)
    d2 = d * sc if sc is not None else d
    ed2 = ed * asc + U * d2.abs()
    nterm = rows + 6
    B["dgamma"] = SECOND * ((ed2 * (xh.abs() + exh) + d2.abs() * exh).sum(0) + nterm * U * (d2 * xh).abs().sum(0))
    B["dbeta"] = SECOND * (ed2.sum(0) + nterm * U * d2.abs().sum(0))
    if sc is not None:
        rps = pr["rps"]
        ns = rows // rps
        G = lambda t: t.view(ns, rps, D).sum(1)
        w = ag * xh.abs() + ab
        esc = SECOND * (G(ed * (w + ag * exh) + d.abs() * ag * exh) + (rps + 6) * U * G(d.abs() * w))
        esh = SECOND * (G(ed) + (rps + 6) * U * G(d.abs()))
        e = torch.cat([esc, esh], 1)
        if pr["accumulate"]:
            e = e + U * (pr["dss0"].double().abs() + ref["dss"].abs())
        B["dss"] = e
    mean = lambda t: t.mean(-1, keepdim=True)
    dxh = d2 * g
    edxh = SECOND * (ed * asc + 2 * U * d2.abs()) * ag
    t1, t2 = mean(dxh), mean(dxh * xh)
    et1 = mean(edxh) + (D + 2) * U * mean(dxh.abs())
    et2 = mean(edxh * (xh.abs() + exh) + dxh.abs() * exh) + (D + 3) * U * mean((dxh * xh).abs())
    inner = dxh - t1 - xh * t2
    einner = edxh + et1 + exh * t2.abs() + (xh.abs() + exh) * et2 + 3 * U * (dxh.abs() + t1.abs() + (xh * t2).abs())
    rs = st["rs"]
    res = pr["dres"].double().abs() if pr.get("dres") is not None else 0.0
    edx = SECOND * (st["drs"] * inner.abs() + st["hi"] * einner + 3 * U * rs * rs * t2.abs() * (x.abs() + st["m"].abs())
                    + 2 * U * ((rs * inner).abs() + res + ref["dx"].abs())) + TINY
    B["dx_f32"] = edx
    B["dx_bf16"] = edx + hulp(ref["dx"].abs() + edx)
    return B


def rstd_ratio(got, B, ref):
    """worst of (got - rs) / (hi - rs) above and (rs - got) / (rs - lo) below the reference: <= 1 inside the interval; inf for NaN"""
    got, rs = got.double().cpu(), ref["rs"]
    up, dn = (got - rs) / (B["rs_hi"] - rs).clamp_min(1e-300), (rs - got) / (rs - B["rs_lo"]).clamp_min(1e-300)
    r = torch.maximum(up, dn)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return float(r.max())


def f8_check(q, scale, ref, B):
    """(worst |dequantised - out| / bound with the kernel's OWN exponent, number of rows whose exponent is not admissible).
    q uint8 [rows][D] (e4m3 bytes), scale int [rows] (E8M0 byte = ex + 127)"""
    ex = (scale.cpu().to(torch.int64) & 0xFF) - 127
    deq = torch.ldexp(q.cpu().view(torch.float8_e4m3fn).float().double(), ex[:, None])
    return f8_check_values(deq, ex, ref, B)


def f8_check_values(deq, ex, ref, B):
    a, ea = ref["amax"], B["amax_err"]
    # the exponent is monotone in the maximum: the reference's own, or, only where the maximum is within its bound of a step, up to
    # that of maximum +- bound (on an ill-conditioned row -- constant x -- the bound spans more than one step)
    ok = (ex >= e4m3_row_exponent((a - ea).clamp_min(TINY))) & (ex <= e4m3_row_exponent(a + ea))
    scaled = torch.ldexp(ref["out"].abs() + B["y"], -ex[:, None]).clamp_max(448.0)
    bound = B["y"] + torch.ldexp(e4m3_half_spacing(scaled), ex[:, None])
    return worst_ratio(deq, ref["out"], bound), int((~ok).sum())


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
F32 = torch.float32


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()     # a b is exact in float64: one rounding, as the fp32 fma


def _butterfly(v):
    """xor-shuffle all-reduce over the last axis (a power of two): every lane ends with the same bits"""
    n = v.shape[-1]
    idx = torch.arange(n)
    o = n // 2
    while o:
        v = v + v[..., idx ^ o]
        o //= 2
    return v[..., 0]


def sum32(x, order):
    """fp32 sums (sum x, sum x^2) of the rows of x in the order of `order`:
    wave    64 lanes; lane owns columns k 256 + 4 lane + e (2 lane + e at D = 128), sequential in (k, e), then six xor steps -- the row
            kernel and the wide kernels (one layout);
    narrow  16 lanes x D / 16 contiguous columns, sequential, then four xor steps -- layernorm_bwd_narrow128_kernel;
    seq     one accumulator, ascending columns"""
    x = x.float()
    rows, D = x.shape
    if order == "seq":
        lanes = x.view(rows, 1, D)
    elif order == "narrow":
        lanes = x.view(rows, 16, D // 16)
    elif D == 128:
        lanes = x.view(rows, 64, 2)
    else:
        lanes = x.view(rows, D // 256, 64, 4).permute(0, 2, 1, 3).reshape(rows, 64, D // 64)
    s = torch.zeros(lanes.shape[:2], dtype=F32)
    s2 = torch.zeros(lanes.shape[:2], dtype=F32)
    for i in range(lanes.shape[2]):
        v = lanes[:, :, i]
        s = s + v
        s2 = s2 + v * v
    return _butterfly(s), _butterfly(s2)


def emu_stats(x, order, clamp=True):
    """(mean, rstd, argument of the rsqrt) [rows][1] fp32"""
    D = x.shape[1]
    s, s2 = sum32(x, order)
    inv = torch.tensor(1.0 / D, dtype=F32)
    mean = s * inv
    arg = s2 * inv - mean * mean + torch.tensor(EPS, dtype=F32)
    a = torch.maximum(arg, torch.tensor(EPS, dtype=F32)) if clamp else arg
    return mean[:, None], a.rsqrt()[:, None], arg[:, None]


def _sigmoid32(x):
    one = torch.tensor(1.0, dtype=F32)
    return one / (one + torch.exp2(-x * torch.tensor(1.4426950408889634, dtype=F32)))


def emu_forward(pr, order, folded, clamp=True):
    """out bf16, y fp32 (in front of the store), mean, rstd: the row kernel's (unfolded) or the wide kernels' (folded) arithmetic"""
    x, g, b = pr["x"].float(), pr["gamma"].float(), pr["beta"].float()
    mean, rstd, _ = emu_stats(x, order, clamp)
    sc, sh = film_rows_of(pr)
    if folded:
        xh = _fma32(x, rstd.expand_as(x), (-mean * rstd).expand_as(x))
        if sc is not None:
            A, C = sc.float() * g, _fma32(sc.float(), b.expand_as(x), sh.float())
        else:
            A, C = g.expand_as(x), b.expand_as(x)
        y = _fma32(xh, A, C)
    else:
        y = (x - mean) * rstd * g + b
        if sc is not None:
            y = sc.float() * y + sh.float()
    if pr["swish"]:
        y = y * _sigmoid32(y)
    return dict(out=bf(y), y=y, mean=mean[:, 0], rstd=rstd[:, 0])


def _colsum32(t, gr):
    """fp32 column sums: rows of a group in ascending order, then the groups in ascending order; also per group"""
    rows, D = t.shape
    per = []
    for r0 in range(0, rows, gr):
        acc = torch.zeros(D, dtype=F32)
        for r in range(r0, min(r0 + gr, rows)):
            acc = acc + t[r]
        per.append(acc)
    tot = torch.zeros(D, dtype=F32)
    for p in per:
        tot = tot + p
    return tot, torch.stack(per)


def emu_backward(pr, order, folded, stats_in=None):
    """dx (fp32; bf() it for the bf16 output), dgamma, dbeta, dss: the register kernel's arithmetic (unfolded) or the 8-wave kernel's
    (folded constants, P / Q column sums, dx = rs dxh - (rs^2 t2) x - rs (t1 - m rs t2)); stats_in: saved (mean, rstd) or None"""
    x, g, b = pr["x"].float(), pr["gamma"].float(), pr["beta"].float()
    rows, D = x.shape
    mean, rstd, _ = emu_stats(x, order) if stats_in is None else (stats_in[0][:, None], stats_in[1][:, None], None)
    sc, sh = film_rows_of(pr)
    dy = pr["dout"].float()
    one = torch.tensor(1.0, dtype=F32)
    inv = torch.tensor(1.0 / D, dtype=F32)

    def sgrad(p):
        s = _sigmoid32(p)
        return s * (one + p * (one - s))

    gr = group_rows(pr["film"], pr["rps"])
    out = {}
    if folded:
        nmr = -mean * rstd
        xh = _fma32(x, rstd.expand_as(x), nmr.expand_as(x))
        A = sc.float() * g if sc is not None else g.expand_as(x)
        d = dy
        if pr["swish"]:
            C = _fma32(sc.float(), b.expand_as(x), sh.float()) if sc is not None else b.expand_as(x)
            d = dy * sgrad(_fma32(xh, A, C))
        dh = d * A
        _, Pg = _colsum32(d * xh, gr)
        _, Qg = _colsum32(d, gr)
        scg = sc.float()[::gr] if sc is not None else torch.ones(Pg.shape, dtype=F32)
        out["dgamma"], out["dbeta"] = _colsum32(scg * Pg, 1 << 30)[0], _colsum32(scg * Qg, 1 << 30)[0]
        if sc is not None:
            out["dss"] = torch.cat([g * Pg + b * Qg, Qg], 1)
        s1 = sum32x(dh, order)[:, None] * inv
        s2 = sum32x(dh * xh, order)[:, None] * inv
        m2, c0 = rstd * rstd * s2, rstd * _fma32(nmr, s2, s1)
        dx = rstd * dh - m2 * x - c0
    else:
        xh = (x - mean) * rstd
        n = xh * g + b
        d = dy
        if sc is not None:
            pre = sc.float() * n + sh.float()
            if pr["swish"]:
                d = d * sgrad(pre)
            out["dss"] = torch.cat([_colsum32(d * n, gr)[1], _colsum32(d, gr)[1]], 1)
            d = d * sc.float()
        elif pr["swish"]:
            d = d * sgrad(n)
        out["dgamma"], out["dbeta"] = _colsum32(d * xh, gr)[0], _colsum32(d, gr)[0]
        dh = d * g
        s1 = sum32x(dh, order)[:, None] * inv
        s2 = sum32x(dh * xh, order)[:, None] * inv
        dx = rstd * (dh - s1 - xh * s2)
    if pr.get("dres") is not None:
        dx = dx + pr["dres"].float()
    if "dss" in out and pr["accumulate"]:
        out["dss"] = pr["dss0"].float() + out["dss"]
    out["dx"] = dx
    return out


def sum32x(t, order):
    return sum32(t, order)[0]


# ------------------------------------------------------------------------------------------------ regimes
def outlier_cols(D):
    """columns the outlier visits: lane j of chunk j % NV for every lane (element j % 4 of its quad), then both ends of the row"""
    if D == 128:
        return [2 * j + (j % 2) for j in range(64)] + [0, D - 1]
    nv = D // 256
    return [256 * (j % nv) + 4 * j + (j % 4) for j in range(64)] + [0, D - 1]


_EDGE = {}


def edge_mean(D, xbf):
    """the largest mean mu (to 1 %) at which a row mu + N(0, 1) still has dvar <= (var + eps) / 8 by stats(): found by bisection on
    the derived bound, on the row as the kernel reads it (rounded to fp32, or to bf16)"""
    key = (D, xbf)
    if key not in _EDGE:
        z = torch.randn(D, generator=torch.Generator().manual_seed(4242 + D), dtype=F64)
        row = lambda mu: (bf(mu + z).double() if xbf else (mu + z).float().double())[None]
        ok = lambda mu: bool((stats(row(mu))["dvar"] <= (stats(row(mu))["var"] + EPS) / 8).all())
        lo, hi = 0.0, 1e4
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if ok(mid) else (lo, mid)
        while not ok(lo):
            lo *= 0.99
        _EDGE[key] = lo
    return _EDGE[key]


def make_rows(kinds, D, xbf, g):
    """x fp32 [len(kinds)][D] (bf16-representable when xbf): row r in the regime kinds[r], built exactly"""
    rn = lambda: torch.randn(D, generator=g, dtype=F64)
    cols = outlier_cols(D)
    rows, k_out = [], 0
    for kind in kinds:
        if kind == "unit":
            r = 1.5 * rn() + 0.3
        elif kind == "offset":
            r = 8.0 + 0.25 * rn()
        elif kind == "edge":
            r = edge_mean(D, xbf) + torch.randn(D, generator=torch.Generator().manual_seed(4242 + D), dtype=F64)
        elif kind == "tiny":
            r = 1e-4 * rn()
        elif kind == "zero":
            r = torch.zeros(D, dtype=F64)
        elif kind in CONST:
            r = torch.full((D,), CONST[kind], dtype=F64)
        elif kind == "nearconst":
            r = 10.1 + 1e-3 * rn()
        elif kind == "outlier":
            r = 1.5 * rn() + 0.3
            r[cols[k_out % len(cols)]] = 1024.0
            k_out += 1
        elif kind == "huge":
            r = rn() * 2.0 ** 40
        else:
            raise KeyError(kind)
        rows.append(r)
    x = torch.stack(rows)
    return bf(x).float() if xbf else x.float()


def make_film(kinds, D, g):
    """[len(kinds)][2 D] fp32: scale | shift of each sample (or table row)"""
    rn = lambda: torch.randn(D, generator=g, dtype=F64)
    alt = torch.where(torch.arange(D) % 2 == 0, 1.0, -1.0).double()
    alt3 = torch.where((torch.arange(D) // 2) % 2 == 0, 1.0, -1.0).double()
    out = []
    for kind in kinds:
        if kind == "near1":
            sc, sh = 1 + 0.3 * rn(), 0.2 * rn()
        elif kind == "zero":
            sc, sh = torch.zeros(D, dtype=F64), rn()
        elif kind == "neg":
            sc, sh = -(1 + 0.3 * rn().abs()), 0.2 * rn()
        elif kind == "sat30":
            sc, sh = 16.0 * (1 + 0.1 * rn()) * alt, 5.0 * rn()
        elif kind == "sat100":
            sc, sh = 30.0 * alt, 40.0 * alt3
        else:
            raise KeyError(kind)
        out.append(torch.cat([sc, sh]))
    return torch.stack(out).float()


def make_dout(kinds, D, g):
    rows = len(kinds)
    out = []
    for r, kind in enumerate(kinds):
        v = torch.randn(D, generator=g, dtype=F64)
        if kind == "zero":
            v = torch.zeros(D, dtype=F64)
        elif kind == "big":
            v = v * 2.0 ** 20
        elif kind == "comb":                                 # non-zero where column % rows == r: every column gets ONE term, from row c % rows
            v = torch.where(torch.arange(D) % rows == r, v + torch.sign(v), torch.zeros(D, dtype=F64))
        out.append(v)
    return bf(torch.stack(out))


_PROBLEMS = {}


def problem(D, rows, rps, film=False, swish=False, xbf=False, rot=0, kinds=None, film_kinds=None, dout="mix", res=None,
            accumulate=0, t=None, film_rows=7, seed=0):
    """One problem, shared between tests and never modified.  Row r is in regime ROW_KINDS[(r + rot) % 11] (or kinds[r % len]), sample s
    has FiLM kind FILM_KINDS[(s + rot) % 5]; with `t` (an int, the value at *t_ptr) the FiLM table has `film_rows` rows of kinds
    FILM_KINDS[i % 5] and every row reads row clamp(t).  dout: "mix" (row r of DOUT_KINDS[r % 4]) or one kind for every row.
    res: None / "f32" / "bf16" residual gradient."""
    key = (D, rows, rps, film, swish, xbf, rot, tuple(kinds or ()), tuple(film_kinds or ()), dout, res, accumulate, t, film_rows, seed)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    g = torch.Generator().manual_seed(10007 * seed + 31 * D + 7 * rows + rps + 3 * rot + int(film) + 2 * int(xbf))
    rk = [(kinds[r % len(kinds)] if kinds else ROW_KINDS[(r + rot) % len(ROW_KINDS)]) for r in range(rows)]
    x = make_rows(rk, D, xbf, g)
    gamma = (1 + 0.2 * torch.randn(D, generator=g)).float()
    beta = (0.1 * torch.randn(D, generator=g)).float()
    pr = dict(D=D, rows=rows, rps=rps, film=film, swish=swish, xbf=xbf, kinds=rk, x=x, gamma=gamma, beta=beta, t=t, accumulate=accumulate, res=res)
    if film:
        if t is not None:
            fk = [FILM_KINDS[i % len(FILM_KINDS)] for i in range(film_rows)]
        else:
            ns = rows // rps
            fk = [(film_kinds[s % len(film_kinds)] if film_kinds else FILM_KINDS[(s + rot) % len(FILM_KINDS)]) for s in range(ns)]
        pr.update(ss=make_film(fk, D, g), film_kinds=fk)
        if t is None:
            pr["dss0"] = torch.randn(rows // rps, 2 * D, generator=g).float()
    dk = [DOUT_KINDS[r % len(DOUT_KINDS)] if dout == "mix" else dout for r in range(rows)]
    pr.update(dout=make_dout(dk, D, g), dout_kinds=dk)
    if res is not None:
        dres = torch.randn(rows, D, generator=g)
        pr["dres"] = bf(dres).float() if res == "bf16" else dres.float()
    assert float(x.abs().max()) < XMAX and bool(torch.isfinite(x).all())
    _PROBLEMS[key] = pr
    return pr


def rows_of(pr, kind):
    return [r for r, k in enumerate(pr["kinds"]) if k == kind or (kind == "constant" and k in CONST)]
