"""Element-wise criterion for the NT GEMM  C = A Bt^T  on bf16 operands with the fused epilogue of GemmEpilogue (no GPU needed).

Reference (``reference``): float64 of the bf16 operands, stage by stage in the order written above GemmEpilogue (smd_kernels.h):

    v = alpha acc + bias[col];  pre_bf16 <- v;  v = act(v);  v *= aux'(aux[row][col]);  v += res_f32[row % mod][col];
    v += res_bf16[row][col];  out_f32 <- (old +) v;  out_bf16 <- v          (out_bf16 never holds the accumulated value)

GELU is the tanh form of the oracle (ddpm_oracle.gelu), written as x / (1 + exp(-2 w)), w = k0 (x + k1 x^3): the same function,
without the cancellation of 1 + tanh(w) that costs float64 its digits in the negative tail (tests/test_nt_ref_host.py holds the
two together); gelu' and swish' are written with sigmoid(-z) for 1 - sigmoid(z) for the same reason.

Bound, per element (``reference`` carries it along as `e`, next to the value `v`).  u = 2^-24 (fp32 unit roundoff), ulp = 2^-23 (one
unit in the last place, relative), ub = 2^-8 (bf16 unit roundoff), floor = 2^-126 (a result or operand flushed as a denormal).

  Accumulator.  A product of two bf16 numbers has 16 significant bits and is exact in fp32; only the additions round.  K products and
  the KG partial sums of the K-groups: |err| <= gamma_{K+KG} sum|term| for ANY order of summation (Higham, Accuracy and Stability of
  Numerical Algorithms, section 4.2).  The matrix core's adder is not specified to round to nearest after every addition, a
  truncating adder loses 2 u per addition:                      e = 2 (K + KG) u (|A| |Bt|^T) + floor
  fp32 stages.  r = fl(a op b) adds u |r|:   alpha: e = |alpha| e + u |v|;   bias, res_f32, res_bf16, accumulate: e += u |v| (the
  operand itself is exact: fp32 data, or bf16 data whose conversion to fp32 is exact -- reading aux / res_bf16 costs nothing).
  act.  e = |act'(v)| e + E_act(v), first order in e, act' in float64;  aux.  v *= g:  e = |g| e + |v| E_g + u |v g|.
  bf16 stores (pre_bf16, out_bf16): round to nearest even of the computed value:   e_store = e + ub (|v| + e) + floor.
  Activation functions (smd_common.h), E_act / E_g.  AMD documents v_exp_f32 and v_rcp_f32 at 1 ulp; both flush denormals.  With
  t the exponent's argument and dt its error:
      s = rcp(1 + exp2(t)):  de = e (expm1(ln2 dt) + ulp) + floor;  d = 1 + e, dd = de + u d;  ds = dd / (d (d - dd)) + ulp s + floor
      geluf_:   t = x fma(Bc, x^2, A), A = -2 k0 log2(e) (three roundings in the constant: 3 u), Bc = A k1 (5 u), x^2 (u), fma (u):
                dw = 3 u |A| + 6 u |Bc| x^2 + u |w|,  dt = |x| dw + u |t|;   gelu = x s:  E = |x| ds + u |x s| + floor
                (dt grows like |t| ~ |x|^3: the relative error of exp2 in the tails is that of its ARGUMENT, not 1 ulp)
      swishf_:  t = fl(-x log2e): dt = 2 u |t|;  E = |x| ds + u |x s| + floor
      swish_gradf_ = s (1 + x (1 - s)):  a = 1 - s: da = ds + u |a|;  b = x a: db = |x| da + u |b|;  c = 1 + b: dc = db + u |c|;
                E = |c| ds + s dc + u |s c| + floor        (1 - s cancels for large x: |x| ds, as the kernel computes it)
      gelu_gradf_ = 0.5 (1 + T) + 0.5 x (1 - T^2) du,  T = 1 - 2 / (exp(2 w) + 1):
                w = k0 (x + k1 x x x): dw = k0 (4 u k1 |x|^3 + u |x + k1 x^3|) + 2 u |w|;  t = fl(2 w log2e): dt = 2 log2e dw + 2 u |t|;
                q = 2 / (e + 1) by IEEE division: dq = 2 dd / (d (d - dd)) + u q;  dT = dq + u |T|;  du = k0 (1 + 3 k1 x^2): 7 u |du|;
                h = 1 + T: dh = dT + u |h|;  p = T^2: dp = 2 |T| dT + u p;  m = 1 - p: dm = dp + u |m|;  g1 = 0.5 x m: dg1 = 0.5 |x| dm
                + u |g1|;  g2 = g1 du: dg2 = |g1| 7 u |du| + |du| dg1 + u |g2|;   E = 0.5 dh + dg2 + u |gelu'| + floor
                (1 - T^2 cancels in both tails and is multiplied by 0.5 |x| du ~ 0.05 |x|^3: the bound is wide there because the
                expression is; contraction into FMAs only removes roundings)
Nothing here is fitted to GPU output, and nothing is to be widened.  ``emulate`` -- the same expressions in fp32 numpy, one fp32
addition per 16-wide K step, the K-groups added afterwards, exp2 / rcp / division correctly rounded -- is inside the bound
everywhere, and its accumulator inside 0.01 of the accumulator's (tests/test_nt_ref_host.py).  It is NOT inside half of the whole
bound at every output, and cannot be: u |v| and ub |v| are the half-spacing of fp32 / bf16 at the bottom of a binade, one correctly
rounded operation reaches them wherever it dominates (0.97 for the bf16 store of the plain bias epilogue).  Room is left where the
hardware is not specified to round correctly: the matrix core's adder (factor 2) and exp2 / rcp (1 ulp).

``plant``: the mistakes an epilogue or planner rewrite makes, planted into a correctly rounded result.
"""
import math
from dataclasses import dataclass, replace

import numpy as np
import torch

from _wgrad_ref import U, rel, worst_ratio  # noqa: F401  (re-exported for the tests)

ULP = 2.0 ** -23
UB = 2.0 ** -8
FLOOR = 2.0 ** -126
K0, K1 = math.sqrt(2.0 / math.pi), 0.044715
LOG2E, LN2 = 1.0 / math.log(2.0), math.log(2.0)
GA = -2.0 * K0 * LOG2E            # geluf_: exp(-2 w) = exp2(x (GA + GB x^2))
GB = GA * K1
NAN = float("nan")


def bf(x):
    return x.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ epilogues and cases
@dataclass(frozen=True)
class Ep:
    name: str
    alpha: float = 1.0
    bias: bool = False
    pre: bool = False
    act: int = 0
    aux: int = 0                  # aux_mode
    res: bool = False             # res_f32
    mod: int = 0                  # res_row_mod
    inplace: bool = False         # out_f32 is the res_f32 buffer
    resb: bool = False
    f32: bool = False
    acc: bool = False             # accumulate onto known data
    b16: bool = False

    @property
    def oct_stages(self):         # alpha == 1 and no accumulate: the 256 x 256 kernel's epilogue applies
        return self.alpha == 1.0 and not self.acc


EPILOGUES = [
    Ep("bias->f32", bias=True, f32=True),
    Ep("bias->bf16", bias=True, b16=True),                                   # the packed path of the 256 x 256 kernel
    Ep("film-f1", bias=True, pre=True, act=2, b16=True),
    Ep("gelu+pre", bias=True, pre=True, act=1, b16=True),
    Ep("dgrad-gelu", aux=1, b16=True),
    Ep("dgrad-swish", aux=2, b16=True),
    Ep("pos-mod32", res=True, mod=32, f32=True),
    Ep("pos-mod96", res=True, mod=96, f32=True),
    Ep("bf16-trunk", resb=True, b16=True, f32=True),
    Ep("in-place", bias=True, res=True, inplace=True, f32=True),
    Ep("pre-only", bias=True, pre=True),
    Ep("alpha", alpha=-0.5, bias=True, f32=True),
    Ep("accumulate", acc=True, f32=True),
    Ep("everything8", bias=True, pre=True, act=1, aux=2, res=True, mod=96, resb=True, f32=True, b16=True),
    Ep("everything", alpha=-0.5, bias=True, pre=True, act=2, aux=1, res=True, mod=96, resb=True, f32=True, acc=True, b16=True),
]
EP = {e.name: e for e in EPILOGUES}


@dataclass(frozen=True)
class Case:
    M: int
    N: int
    K: int
    ld: str                       # "tight": every ld = the width; "pad": + 8 (vector paths stay); "odd": odd lds (scalar epilogue)
    knobs: tuple = ()             # ((key, value), ...) on top of the defaults
    expect: tuple = ()            # (kernel, BM, NS, KG) the plan must report
    seed: int = 0

    @property
    def id(self):
        k = ",".join(f"{a.replace('gemm_', '')}={b}" for a, b in self.knobs)
        return f"{self.M}x{self.N}x{self.K}-{self.ld}" + (f"-{k}" if k else "") + "-<%d:%d,%d,%d>" % self.expect


KNOB_DEFAULTS = {"gemm_nt_form": 0, "gemm_nt256": 1, "gemm_nt256_variant": 0, "gemm_nt256_pk": 1}
FORMS = {1: (64, 2, 1), 2: (128, 2, 1), 3: (128, 2, 2), 4: (64, 2, 2), 5: (128, 3, 1), 6: (64, 3, 2)}      # gemm_nt_form (gemm_plan.h)
NT256_VARIANTS = (0, 1, 2, 3)     # every schedule variant launch_gemm_nt256 has without -DSMD_ABLATIONS


def _cases():
    out = []
    # by shape (smd_plan::nt_plan): the three 32-row forms at their smallest shapes, and from M = 200 (ragged against 32 too)
    for (M, N, K, ld), form in (((32, 128, 64, "pad"), (32, 2, 1)), ((32, 128, 512, "pad"), (32, 4, 1)), ((32, 128, 1024, "pad"), (32, 3, 2)),
                                ((32, 128, 64, "odd"), (32, 2, 1)), ((200, 136, 64, "tight"), (32, 2, 1)), ((200, 134, 512, "odd"), (32, 4, 1)),
                                ((200, 136, 1024, "pad"), (32, 3, 2)), ((200, 134, 1024, "pad"), (32, 3, 2))):
        out.append(Case(M, N, K, ld, (), (128,) + form))
    # forced forms: M = 200 is ragged against 64 and 128; N = 136 leaves a ragged last tile on the vector path, N = 134 with odd
    # lds takes the scalar path everywhere, N = 134 with aligned lds the vector path with a scalar last quad.
    # K: nk = 1 (< NS - 1 for <128,3,1>; one K-tile per group for the two-group forms) and nk = 3
    for f, (bm, ns, kg) in FORMS.items():
        k1, k3 = (64, 192) if kg == 1 else (128, 384)
        for N, K, ld in ((136, k1, "tight"), (136, k3, "pad"), (134, k1, "odd"), (134, k3, "odd"), (134, k1, "pad")):
            out.append(Case(200, N, K, ld, (("gemm_nt_form", f),), (128, bm, ns, kg)))
    # a two-group form asked for at K = 192 (an odd number of K-tiles) falls through to the default form
    for f in (3, 4, 6):
        out.append(Case(200, 136, 192, "pad", (("gemm_nt_form", f),), (128, 32, 2, 1)))
    # the 256 x 256 kernel, forced onto small grids: one tile with nk = 2, and 2 x 2 tiles (row and column offsets non-zero)
    for v in NT256_VARIANTS:
        out.append(Case(256, 256, 128, "tight", (("gemm_nt256", 2), ("gemm_nt256_variant", v)), (256, 256, 2, 1)))
        out.append(Case(512, 512, 256, "pad", (("gemm_nt256", 2), ("gemm_nt256_variant", v)), (256, 256, 2, 1)))
    return [replace(c, seed=100 + 7 * c.M + 3 * c.N + c.K + len(c.ld)) for c in out]       # one problem per shape: shared between forms


CASES = _cases()


def epilogues_for(case):
    """the list of section "Epilogues per form": on the 256 x 256 kernel alpha / accumulate leave it (checked apart)"""
    if case.expect[0] == 256:
        return [e for e in EPILOGUES if e.oct_stages]
    return [e for e in EPILOGUES if e.name != "everything8"]


# ------------------------------------------------------------------------------------------------ problems
def lds(case):
    """leading dimensions (lda, ldb, ld_pre, ld_aux, ld_res, ld_resb, ld_out, ld_outb)"""
    N, K = case.N, case.K
    if case.ld == "tight":
        return dict(a=K, b=K, pre=N, aux=N, res=N, resb=N, out=N, outb=N)
    n8 = (N + 7) // 8 * 8
    if case.ld == "pad":              # multiples of 8 (fp32 residual: of 4): every vector path stays open
        return dict(a=K + 8, b=K + 16, pre=n8 + 8, aux=n8 + 16, res=n8 + 4, resb=n8 + 24, out=n8 + 8, outb=n8 + 32)
    return dict(a=K + 8, b=K + 8, pre=n8 + 1, aux=n8 + 3, res=n8 + 5, resb=n8 + 7, out=n8 + 9, outb=n8 + 11)


def _padded(g, rows, width, ld, scale, shift, garbage):
    """[rows][ld] float32: data in the logical columns, finite garbage of another magnitude behind them"""
    t = garbage + torch.randn(rows, ld, generator=g)
    t[:, :width] = torch.randn(rows, width, generator=g) * scale + shift
    return t


def make_problem(case):
    """CPU tensors of one case, shared by its epilogues.  A ~ N(0, 1), Bt ~ N(0, 4 / K) (z ~ N(0, 4): both tails of the
    activations), bias, residuals ~ N(0, 1), aux ~ N(0, 4) in bf16, `old` = what an accumulating launch finds in out_f32.
    Padding columns: about +-50 .. 70.  res: max(M, 96) rows; a launch with res_row_mod gets its first `mod` rows only."""
    M, N, K = case.M, case.N, case.K
    ld = lds(case)
    g = torch.Generator().manual_seed(case.seed)
    p = dict(case=case, ld=ld)
    p["A"] = bf(_padded(g, M, K, ld["a"], 1.0, 0.0, 50.0))
    p["Bt"] = bf(_padded(g, N, K, ld["b"], 2.0 / math.sqrt(K), 0.0, -50.0))
    p["bias"] = torch.randn(N, generator=g)
    p["aux"] = bf(_padded(g, M, N, ld["aux"], 2.0, 0.0, 60.0))
    p["res"] = _padded(g, max(M, 96), N, ld["res"], 1.0, 0.1, -60.0)          # at least the 96 rows of the larger table
    p["resb"] = bf(_padded(g, M, N, ld["resb"], 1.0, -0.1, 70.0))
    p["old"] = _padded(g, M, N, ld["out"], 1.0, 0.5, -70.0)
    Ad, Bd = p["A"][:, :K].double(), p["Bt"][:, :K].double()
    p["acc"], p["absacc"] = Ad @ Bd.t(), Ad.abs() @ Bd.abs().t()
    return p


def problem_from(A, Bt, bias=None, res=None):
    """a problem of the caller's own tensors (CPU, unpadded) for `reference`: the older tests of tests/test_gpu_kernels.py"""
    M, K = A.shape
    c = Case(M, Bt.shape[0], K, "tight")
    Ad, Bd = A.double(), Bt.double()
    return dict(case=c, ld=lds(c), A=A, Bt=Bt, bias=bias, res=res, acc=Ad @ Bd.t(), absacc=Ad.abs() @ Bd.abs().t())


# ------------------------------------------------------------------------------------------------ activations: value and error
def _sig(z):
    return torch.sigmoid(z)


def gelu_w(x):
    return K0 * (x + K1 * x ** 3)


def gelu(x):
    return x * _sig(2.0 * gelu_w(x))


def swish(x):
    return x * _sig(x)


def gelu_grad(x):
    w = gelu_w(x)
    s, c = _sig(2.0 * w), _sig(-2.0 * w)                       # c = 1 - s without the cancellation
    return s + 2.0 * x * s * c * K0 * (1.0 + 3.0 * K1 * x * x)


def swish_grad(x):
    s, c = _sig(x), _sig(-x)
    return s * (1.0 + x * c)


def _exp2(t):
    return torch.exp2(t.clamp(-1100.0, 1000.0))


def _err_s(t, dt):
    """(s, ds) of s = rcp(1 + exp2(t)) as the kernels evaluate it (module docstring)"""
    e = _exp2(t)
    de = e * (torch.expm1((LN2 * dt).clamp(max=50.0)) + ULP) + FLOOR
    d = 1.0 + e
    dd = de + U * d
    s = 1.0 / d
    ds = (dd / d) / (d - dd).clamp_min(0.5) + ULP * s + FLOOR      # d - dd >= 0.5: d >= 1 and dd / d is far below 1 / 2
    ds = torch.where(dd < 0.5 * d, ds, torch.ones_like(ds))       # (were it not: s lies in [0, 1], so does what rcp returns)
    return s, ds


def err_gelu(x):
    x2 = x * x
    w = GA + GB * x2
    t = x * w
    dw = 3 * U * abs(GA) + 6 * U * abs(GB) * x2 + U * w.abs()
    dt = x.abs() * dw + U * t.abs()
    s, ds = _err_s(t, dt)
    return x.abs() * ds + U * (x * s).abs() + FLOOR


def err_swish(x):
    t = -x * LOG2E
    s, ds = _err_s(t, 2 * U * t.abs())
    return x.abs() * ds + U * (x * s).abs() + FLOOR


def err_swish_grad(x):
    t = -x * LOG2E
    s, ds = _err_s(t, 2 * U * t.abs())
    a = _sig(-x)                                                  # 1 - s, without float64's cancellation
    da = ds + U * a
    b = x * a
    db = x.abs() * da + U * b.abs()
    c = 1.0 + b
    dc = db + U * c.abs()
    return c.abs() * ds + s * dc + U * (s * c).abs() + FLOOR


def err_gelu_grad(x):
    ax = x.abs()
    x3 = K1 * ax ** 3
    w = gelu_w(x)
    dw = K0 * (4 * U * x3 + U * (ax + x3)) + 2 * U * w.abs()
    t = 2.0 * w * LOG2E
    dt = 2.0 * LOG2E * dw + 2 * U * t.abs()
    e = _exp2(t)
    de = e * (torch.expm1((LN2 * dt).clamp(max=50.0)) + ULP) + FLOOR
    d = e + 1.0
    dd = de + U * d
    q = 2.0 / d
    dq = 2.0 * (dd / d) / (d - dd).clamp_min(0.5) + U * q + FLOOR
    dq = torch.where(dd < 0.5 * d, dq, torch.full_like(dq, 2.0))                   # q lies in [0, 2] whatever e is
    T = _sig(2.0 * w) - _sig(-2.0 * w)                                              # tanh(w)
    dT = dq + U * T.abs()
    du = K0 * (1.0 + 3.0 * K1 * x * x)
    ddu = 7 * U * du
    h = 1.0 + T
    dh = dT + U * h
    m = 4.0 * _sig(2.0 * w) * _sig(-2.0 * w)                                        # 1 - T^2
    dp = 2.0 * T.abs() * dT + U * T * T
    dm = (dp + U * m).clamp(max=1.0)                                                # T in [-1, 1] in the kernel too: m in [0, 1]
    g1 = 0.5 * ax * m
    dg1 = 0.5 * ax * dm + U * g1
    g2 = g1 * du
    dg2 = g1 * ddu + du * dg1 + U * g2
    return 0.5 * dh + dg2 + U * gelu_grad(x).abs() + FLOOR


ACT = {1: (gelu, gelu_grad, err_gelu), 2: (swish, swish_grad, err_swish)}
AUX = {1: (gelu_grad, err_gelu_grad), 2: (swish_grad, err_swish_grad)}


# ------------------------------------------------------------------------------------------------ reference and bound
def res_rows(p, ep):
    """the [M][N] residual each output row reads: row % mod of the table's first `mod` rows"""
    N, M = p["case"].N, p["case"].M
    r = p["res"][:, :N].double()
    return r[torch.arange(M) % ep.mod] if ep.mod else r[:M]


def reference(p, ep, KG=1, fault=None, where=None):
    """float64 outputs and per-element bounds of one launch: dict with pre / f32 / b16 -> (value, bound, bound of the fp32 value in
    front of the store) for the outputs `ep` has.
    `fault` plants one of FAULTS into the computation (the bound is that of the correct one: do not use it)."""
    c = p["case"]
    M, N, K = c.M, c.N, c.K
    acc = p["acc"]
    if fault == "kgroup-dropped":                 # the odd K-tiles (second K-group) missing from one 32 x 32 sub-tile
        r0, c0 = where
        Ad, Bd = p["A"][:, :K].double(), p["Bt"][:, :K].double()
        odd = torch.cat([torch.arange(k, k + 64) for k in range(64, K, 128)])
        acc = acc.clone()
        acc[r0:r0 + 32, c0:c0 + 32] -= Ad[r0:r0 + 32][:, odd] @ Bd[c0:c0 + 32][:, odd].t()
    e = 2.0 * (K + KG) * U * p["absacc"] + FLOOR
    v = acc
    if ep.alpha != 1.0:
        v = ep.alpha * v
        e = abs(ep.alpha) * e + U * v.abs()
    if ep.bias:
        b = p["bias"].double()
        if fault == "bias-one-right":             # within a quad: columns 0..2 of it read their right neighbour's bias
            col = torch.arange(N)
            b = b[torch.where((col % 4 < 3) & (col + 1 < N), col + 1, col)]
        v = v + b
        e = e + U * v.abs()
    out = {}
    pre_v, pre_e = v, e
    if ep.act:
        f, df, ef = ACT[ep.act]
        e = df(v).abs() * e + ef(v)
        v = f(v)
    if ep.pre:
        if fault == "pre-after-act":
            pre_v = v
        out["pre"] = (pre_v, pre_e + UB * (pre_v.abs() + pre_e) + FLOOR, pre_e)
    if ep.aux:
        z = p["aux"][:, :N].double()
        if fault == "aux-ld-out":                 # element (row, col) read at row * ld_out + col of the aux buffer
            flat = p["aux"].reshape(-1).double()
            idx = (torch.arange(M)[:, None] * p["ld"]["out"] + torch.arange(N)[None, :]).clamp(max=flat.numel() - 1)
            z = flat[idx]
        dg, eg = AUX[ep.aux]
        g = dg(z)
        e = g.abs() * e + v.abs() * eg(z)
        v = v * g
        e = e + U * v.abs()
    if ep.res:
        r = res_rows(p, ep)
        if fault == "row-not-reduced":            # rows >= mod read on behind the table: whatever lies there (here: other data)
            r = p["res"][:M, :N].double()
        if fault == "second-tile-first-residual":
            r = r[torch.arange(M) % 256]
        v = v + r
        e = e + U * v.abs()
    if ep.resb:
        v = v + p["resb"][:, :N].double()
        e = e + U * v.abs()
    if ep.b16:
        out["b16"] = (v, e + UB * (v.abs() + e) + FLOOR, e)
    if ep.f32:
        if ep.acc and fault != "accumulate-overwrites":
            v = v + p["old"][:, :N].double()
            e = e + U * v.abs()
        out["f32"] = (v, e + FLOOR, e + FLOOR)
    return out


def rounded(ref):
    """a correct kernel's outputs: every value correctly rounded to its format"""
    return {k: (bf(v.float()).double() if k in ("pre", "b16") else v.float().double()) for k, (v, _, _) in ref.items()}


def check(got, ref, what=""):
    """asserts |got - ref| <= bound at every element of every output; -> {output: worst ratio}"""
    ratios = {k: worst_ratio(got[k], v, b) for k, (v, b, _) in ref.items()}
    for k, r in ratios.items():
        assert r <= 1.0, f"{what}: {k} leaves the element-wise bound, worst |err| / bound = {r:.3g}"
    return ratios


def flagged(got, ref):
    try:
        check(got, ref)
    except AssertionError:
        return True
    return False


OLD_F32, OLD_B16, OLD_ACT = 2e-5, 4e-3, 1e-4          # tests/test_gpu_kernels.py: fp32 out, bf16 out, fp32 out behind an activation


def old_criteria_hold(got, ref, ep):
    """the whole-matrix relative-L2 criteria of the older tests, on every output"""
    ok = True
    for k, (v, _, _) in ref.items():
        tol = OLD_B16 if k in ("pre", "b16") else (OLD_ACT if ep.act or ep.aux else OLD_F32)
        ok = ok and rel(got[k], v) < tol              # a NaN compares false: not ok
    return ok


# ------------------------------------------------------------------------------------------------ fault planters
# name -> (epilogue, case filter).  Each is planted where it applies: the case must have what the fault needs.
FAULTS = {
    "bias-one-right": "bias->f32",
    "row-not-reduced": "pos-mod32",
    "aux-ld-out": "dgrad-gelu",                        # needs ld_out != ld_aux: a "pad" or "odd" case
    "pre-after-act": "film-f1",
    "kgroup-dropped": "bias->f32",                     # needs a two-group case
    "accumulate-overwrites": "accumulate",
    "ragged-columns-stale": "bias->bf16",              # needs N % 4 != 0
    "second-tile-first-residual": "in-place",          # needs M > 256
}


def plant(p, fault, KG=1, where=(32, 64), stale=0.0):
    """the outputs of a launch with `fault` in it, correctly rounded otherwise -> (got, ref, ep)"""
    ep = EP[FAULTS[fault]]
    ref = reference(p, ep, KG)
    if fault == "ragged-columns-stale":               # the columns behind the last full quad keep what the buffer held
        got = rounded(ref)
        N = p["case"].N
        assert N % 4
        for k in got:
            got[k] = got[k].clone()
            got[k][:, N // 4 * 4:] = stale
        return got, ref, ep
    return rounded(reference(p, ep, KG, fault=fault, where=where)), ref, ep


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def _f(x):
    return np.asarray(x, dtype=np.float32)


def _bf_np(x):
    return bf(torch.from_numpy(np.ascontiguousarray(x))).float().numpy()


def _rn(x64):
    """float64 -> float32, round to nearest: a correctly rounded exp2 / rcp / division / fma"""
    with np.errstate(over="ignore"):
        return np.asarray(x64, dtype=np.float64).astype(np.float32)


def _rcp(d):
    with np.errstate(divide="ignore"):
        return _rn(1.0 / d.astype(np.float64))


def _exp2f(t):
    with np.errstate(over="ignore", under="ignore"):
        return _rn(np.exp2(np.clip(t.astype(np.float64), -1100.0, 1100.0)))


_GA32 = np.float32(np.float32(-2.0) * np.float32(K0) * np.float32(LOG2E))
_GB32 = np.float32(_GA32 * np.float32(K1))
_L2E32, _K032, _K132 = np.float32(LOG2E), np.float32(K0), np.float32(K1)


def geluf(x):
    w = _rn(_GB32.astype(np.float64) * (x * x).astype(np.float64) + _GA32.astype(np.float64))      # fmaf(Bc, x * x, A)
    return x * _rcp(np.float32(1.0) + _exp2f(x * w))


def _sigmoidf(x):
    return _rcp(np.float32(1.0) + _exp2f(-x * _L2E32))


def swishf(x):
    return x * _sigmoidf(x)


def swish_gradf(x):
    s = _sigmoidf(x)
    return s * (np.float32(1.0) + x * (np.float32(1.0) - s))


def gelu_gradf(x):
    with np.errstate(over="ignore", invalid="ignore"):
        w = _K032 * (x + _K132 * x * x * x)
        e = _exp2f(np.float32(2.0) * w * _L2E32)
        T = np.float32(1.0) - _rn(2.0 / (e.astype(np.float64) + 1.0).astype(np.float32).astype(np.float64))
        du = _K032 * (np.float32(1.0) + np.float32(3.0) * _K132 * x * x)
        return np.float32(0.5) * (np.float32(1.0) + T) + np.float32(0.5) * x * (np.float32(1.0) - T * T) * du


ACTF = {1: geluf, 2: swishf}
AUXF = {1: gelu_gradf, 2: swish_gradf}


def emulate_acc(p, KG):
    """the fp32 accumulator tile: K-group kg takes the K-tiles kt * KG + kg (64 wide), one fp32 addition per 16-wide MFMA step, the
    groups are added afterwards (stage_tile_add)"""
    K = p["case"].K
    A, Bt = p["A"][:, :K].double().numpy(), p["Bt"][:, :K].double().numpy()
    parts = []
    for kg in range(KG):
        acc = np.zeros((A.shape[0], Bt.shape[0]), np.float32)
        for kt in range(kg, K // 64, KG):
            for k in range(kt * 64, kt * 64 + 64, 16):
                acc = acc + _rn(A[:, k:k + 16] @ Bt[:, k:k + 16].T)
        parts.append(acc)
    return parts[0] if KG == 1 else parts[0] + parts[1]


def emulate(p, ep, KG=1, acc=None):
    """the launch in fp32 numpy, expression by expression as gemm_epilogue.h writes it -> {output: float64 tensor}; "pre:f32" and
    "b16:f32" are the fp32 values in front of the two bf16 stores"""
    N = p["case"].N
    v = emulate_acc(p, KG) if acc is None else acc
    v = np.float32(ep.alpha) * v
    if ep.bias:
        v = v + _f(p["bias"].numpy())
    out = {}
    if ep.pre:
        out["pre"], out["pre:f32"] = _bf_np(v), v
    if ep.act:
        v = ACTF[ep.act](v)
    if ep.aux:
        v = v * AUXF[ep.aux](_f(p["aux"][:, :N].float().numpy()))
    if ep.res:
        v = v + _f(res_rows(p, ep).float().numpy())
    if ep.resb:
        v = v + _f(p["resb"][:, :N].float().numpy())
    if ep.b16:
        out["b16"], out["b16:f32"] = _bf_np(v), v
    if ep.f32:
        out["f32"] = v + _f(p["old"][:, :N].numpy()) if ep.acc else v
    return {k: torch.from_numpy(np.ascontiguousarray(x)).double() for k, x in out.items()}


# ------------------------------------------------------------------------------------------------ activation sweep
def all_bf16():
    """every bf16 bit pattern as a [65536] bf16 tensor, the non-finite ones replaced by 0"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16).clone()
    x[~torch.isfinite(x.float())] = 0.0
    return x


SWEEP_RANGE = 65536.0
SWEEP = {"gelu": (gelu, err_gelu, geluf), "swish": (swish, err_swish, swishf),
         "gelu'": (gelu_grad, err_gelu_grad, gelu_gradf), "swish'": (swish_grad, err_swish_grad, swish_gradf)}
