"""Element-wise criterion for the encoder MLP half-layers (encoder_fused.hip: mlp_block_fwd, mlp_hs_fwd, mlp_hs_bwd; ln128.hip:
ln128_parts): float64 reference, derived bounds, regimes of the pre-activation z that are set exactly, selector weights that make
every hidden unit visible on its own, and planted faults.  torch float64 only, no GPU.  U, hulp, worst_ratio, gemm_bound and the
LayerNorm bounds are those of tests/_attn_ref.py.

    z = a2 W1 + b1        u = gelu(z) = z s(z),  s = sigmoid(2 k0 (z + k1 z^3))  (tanh form, k0 = sqrt(2 / pi), k1 = 0.044715)
    gz = gelu'(z) = s + xd s (1 - s),  xd = 2 k0 z (1 + 3 k1 z^2)                  (closed form)
    du = dh W2^T          dz = du gz          da2 = dz W1^T          h_out = h + u W2 + b2
Hidden quarter q holds the units [q M/4, (q + 1) M/4); tile q of h_out is the contraction over that quarter, quarter 0 alone carries
b2 and the residual h; tile q of da2 is the contraction of dz over the quarter.  h_out = (p0 + p1) + (p2 + p3).

Bound.  u = 2^-24 (written U below), hulp(x) = half the spacing of bf16 at x; an fp32 operation costs U |result|, a sum of n products
on the matrix cores 2 (n + 2) U sum |terms| in any order (gemm_bound).  First-order terms are multiplied by 1 + 2^-10 for the
products of two of them that the derivation drops.

  z     ez = 2 (128 + 2) U (|a2| |W1|) + 2 U |z|: the contraction over the stream width, one fp32 addition of b1 (and one more in the
        four-wave fused kernel, which adds two accumulators).  With selector W1 one product is non-zero and z is representable, so
        the kernel's z is exact; the same formula is kept (it is then ~1.5e-5 |z|, a hundredth of a bf16 step).
  s     geluf_ (smd_common.h): t = x fma(Bc, x^2, A) with A = -2 k0 log2(e), Bc = A k1.  A and Bc are fp32 constants folded from
        fp32 factors (3 and 5 roundings), x^2, the fma and the product round once each: |dt| <= 8 U |t| (A and Bc have one sign, so
        |t| = |x| (|A| + |Bc| x^2) and nothing cancels).  e = exp2(t) is within 1 ulp = 2 U: relative error of e
        eps_e = expm1(8 U ln2 |t|) + 2 U.  d = 1 + e costs U d, ABSOLUTE (not relative to e); rcp is within 1 ulp (2 U):
            ds = s (1 - s) eps_e + 3 U s.
        Where e (1 + eps_e) < 2^-25, fl(1 + e) is 1 and rcp(1) is 1 (a power of two: exact), so the kernel's s IS 1 and ds = 1 - s.
        Where t >= 128, exp2 gives +inf, rcp(inf) = 0 and the kernel's s IS 0: ds = s < 2^-128; results below the smallest normal
        number may be flushed: TINY = 2^-100 absolute is added to every result.
  u     dg = |x| ds + U |g|;  the argument carries ez: |gelu(z') - gelu(z)| <= (|gelu'(z)| + G2 ez) ez on [z - ez, z + ez], G2 = 1 >=
        max |gelu''| (0.80 at 0; the host test measures it);  eu = (|gz| + ez) ez + dg, and a bf16 store adds hulp(|u| + eu).
  gz    gelu_fwd_grad_: xd = x fma(6 k0 k1, x^2, 2 k0) (8 U |xd| as t), dg = fma(xd, s (1 - s), s).  1 - s is formed from the SAME
        rounded s, so the error of s (1 - s) is |1 - 2 s| ds + 2 U s (1 - s): ABSOLUTE in ds, it does not shrink as s -> 1:
            egz = |xd| (|1 - 2 s| ds + 2 U s (1 - s) + ds^2) + 8 U |xd| s (1 - s) + ds + U |gz| + G2 ez.
        The term |xd| |1 - 2 s| ds is largest where 1 + e last differs from 1, e ~ 2^-25: z = 5.06, xd = 35.8, term 6.4e-6 (six times
        gelu' - 1 = 1.0e-6 there; test_gelu_closed_forms... prints it).  Beyond, s is exactly 1 and gelu' exactly 1.
  dz    du carries edu = 2 (128 + 2) U (|dh| |W2|^T);  edz = edu (|gz| + egz) + |du| egz + U |dz|, + hulp(|dz| + edz).
  tiles fp32 stores.  da2 tile q from the kernel's own dz: 2 (M/4 + 2) U (|dz_q| |W1_q|^T).  Forward tile q, hidden-split kernel:
        u is not observable, so its whole uncertainty is carried through W2: sum_h (eu_h + hulp_h) |W2_hn| + 2 (M/4 + 2) U
        sum_h (|u_h| + eu_h) |W2_hn|, and in quarter 0 the two additions v += (b2 + h): 2 U (|acc| + |b2| + |h|).
        Fused kernel, h_out from its own saved u: every wave contracts M/4 units, three additions (p0 + p1) + (p2 + p3) through LDS,
        two more for b2 and h: (2 (M/4 + 2) + 3) U (|u| |W2|) + 2 U (|acc| + |b2| + |h| + |h_out|).
Nothing is fitted to GPU output.

Contract on z.  gelu_fwd_grad_ forms xd = x (2 k0 + 6 k0 k1 x^2) in fp32: it overflows for |x| > 1.17e13 and inf * 0 is NaN.  a2 is a
LayerNorm output (|a2| <= sqrt(127) |gamma| + |beta|) and the weights are bf16 of a trained network, so |z| stays many orders below:
ZMAX = 2^42 is the largest magnitude the regimes use (xd = 2^124.4 there: finite).

Selector weights.  Through a dense W2 the propagated tile bound (~ sum of M/4 half-spacings) is looser than any single-unit fault.
  selector W1: column h of W1 has one non-zero 2^k(h) in row PI(h), b1(h) a multiple of 2^-16: z[t][h] = 2^k a2[t][PI(h)] + b1[h]
               is representable in fp32, hence exact in the kernel.
  selector W2, phase p of M / 512: for each quarter q and output column n the ONE live hidden unit q M/4 + 128 p + perm(n) with
               weight +-2^j; the phases are disjoint and cover every unit once.  Tile q is then +-2^j bf16(gelu(z[t][h])) exactly
               (+ b2 + h in quarter 0).  Its transpose serves as the backward's fc1 dgrad pack (each da2 tile element is one dz
               element), the sum over the phases as the backward's fc2 dgrad pack (du = +-2^j dh[t][n(h)], exact).
"""
import math

import torch

from _attn_ref import U, F64, bf, hulp, worst_ratio, rel, gemm_bound, ln_fwd_bound      # noqa: F401  (one definition, re-exported)

K0, K1 = math.sqrt(2.0 / math.pi), 0.044715
LOG2E = 1.0 / math.log(2.0)
TINY = 2.0 ** -100
G2 = 1.0
SECOND = 1.0 + 2.0 ** -10
ZMAX = 2.0 ** 42
E = 128
OLD_HOUT_REL, OLD_U_REL, OLD_DZ_REL = 3e-3, 4e-3, 6e-3        # the whole-matrix thresholds of tests/test_gpu_kernels.py


# ------------------------------------------------------------------------------------------------ closed forms
def _t(z, cubic=True):
    return 2 * K0 * (z + (K1 if cubic else 0.0) * z ** 3)


def gelu(z, cubic=True):
    return z * torch.sigmoid(_t(z, cubic))


def gelu_grad(z, full=True):
    t = _t(z)
    s = torch.sigmoid(t)
    if not full:
        return s
    return s + 2 * K0 * z * (1 + 3 * K1 * z * z) * (s * torch.sigmoid(-t))


def quarter(M, q):
    return slice(q * (M // 4), (q + 1) * (M // 4))


# ------------------------------------------------------------------------------------------------ the model (reference and faults)
FAULT_UNIT = 37            # the hidden unit of b1-one-unit; units 37 and 41 lie in one 32-unit group
FAULTS = ("b1-one-unit", "units-swapped", "b2-in-every-quarter", "residual-missing", "last-chunk-into-next-tile",
          "sample3-reads-sample0", "no-cubic-term", "grad-without-xd-term", "du-of-neighbour-token")


def model(pr, fault=None, rounded=False):
    """float64 model of the half-layer and its backward on the problem `pr`; `fault` plants one of FAULTS; rounded: u and dz as the
    bf16 values a kernel stores (and contracts), the tiles as fp32.  Without either it is the reference."""
    a2, W1, b1, W2, b2, h = (pr[k].double() for k in ("a2", "W1", "b1", "W2", "b2", "h"))
    rows, M = a2.shape[0], W1.shape[1]
    HQ = M // 4
    a2z = a2
    if fault == "sample3-reads-sample0":                     # in every group of four samples, tokens 16 .. 31
        a2z = a2.clone()
        for g0 in range(0, rows - 127, 128):
            a2z[g0 + 112:g0 + 128] = a2[g0 + 16:g0 + 32]
    if fault == "b1-one-unit":
        b1 = b1.clone()
        b1[FAULT_UNIT] += pr.get("b1_step", 2.0 ** -8)       # one bf16 step of z in [0.5, 1): the typical |z| of the dense problem
    z = a2z @ W1 + b1
    u = gelu(z, cubic=fault != "no-cubic-term")
    gz = gelu_grad(z, full=fault != "grad-without-xd-term")
    uo = bf(u).double() if rounded else u
    uc = uo
    if fault == "units-swapped":
        uc = uo.clone()
        for q in range(4):                                   # in every quarter, two units of one 32-unit group of every chunk
            for c0 in range(q * HQ, (q + 1) * HQ, 128):
                uc[:, [c0 + 37, c0 + 41]] = uo[:, [c0 + 41, c0 + 37]]
    tiles = []
    for q in range(4):
        tiles.append(uc[:, quarter(M, q)] @ W2[quarter(M, q)])
    if fault == "last-chunk-into-next-tile":
        c = slice(2 * HQ - 128, 2 * HQ)                      # the last chunk of quarter 1 lands in tile 2
        moved = uc[:, c] @ W2[c]
        tiles[1] = tiles[1] - moved
        tiles[2] = tiles[2] + moved
    acc0 = tiles[0]
    for q in range(4):
        if q == 0 or fault == "b2-in-every-quarter":
            tiles[q] = tiles[q] + b2
    if fault != "residual-missing":
        tiles[0] = tiles[0] + h
    out = dict(z=z, u=uo, gz=gz, tiles=torch.stack(tiles), acc0=acc0, h_out=(tiles[0] + tiles[1]) + (tiles[2] + tiles[3]))
    if pr.get("dh") is not None:
        dh, W2b, W1d = pr["dh"].double(), pr["W2b"].double(), pr["W1d"].double()
        du = dh @ W2b.t()
        if fault == "du-of-neighbour-token":
            du = torch.roll(du, 1, 0)
        dz = du * gz
        dzo = bf(dz).double() if rounded else dz
        out.update(du=du, dz=dzo, da2_tiles=torch.stack([dzo[:, quarter(M, q)] @ W1d[quarter(M, q)] for q in range(4)]))
    if rounded:
        out["tiles"] = out["tiles"].float().double()
    return out


# ------------------------------------------------------------------------------------------------ bounds
def z_err(a2, W1, z):
    return 2 * (E + 2) * U * (a2.double().abs() @ W1.double().abs()) + 2 * U * z.abs()


def s_err(z):
    """(s, ds): the sigmoid factor and what geluf_ / gelu_fwd_grad_ may be off by at the exact argument z"""
    t = _t(z)
    s = torch.sigmoid(t)
    tt = (-t * LOG2E).clamp(-200.0, 200.0)                   # the exp2 argument; beyond +-200 both branches below are negligible / exact
    eps = torch.expm1(8 * U * math.log(2.0) * tt.abs()) + 2 * U
    ds = s * torch.sigmoid(-t) * eps + 3 * U * s
    one = torch.exp2(tt) * (1 + eps) < 2.0 ** -25            # fl(1 + e) = 1, rcp(1) = 1: the kernel's s is exactly 1
    return s, torch.where(one, torch.sigmoid(-t), ds)


def u_err(z, ez, store=True):
    """what u = gelu(z') may be off by, z' within ez of z; store: + the bf16 store"""
    s, ds = s_err(z)
    g = z * s
    e = SECOND * ((gelu_grad(z).abs() + G2 * ez) * ez + z.abs() * ds + U * g.abs()) + TINY
    return e + hulp(g.abs() + e) if store else e


def xd_of(z):
    return 2 * K0 * z * (1 + 3 * K1 * z * z)


def one_minus_s_term(z):
    """|xd| |1 - 2 s| ds: the part of the gelu' error that is absolute in ds"""
    s, ds = s_err(z)
    return xd_of(z).abs() * (1 - 2 * s).abs() * ds


def gz_err(z, ez):
    s, ds = s_err(z)
    xd = xd_of(z).abs()
    p = s * torch.sigmoid(-_t(z))
    return SECOND * (xd * ((1 - 2 * s).abs() * ds + 2 * U * p + ds * ds) + 8 * U * xd * p + ds + U * gelu_grad(z).abs() + G2 * ez) + TINY


def dz_err(z, ez, du, edu):
    gz, egz = gelu_grad(z), gz_err(z, ez)
    dz = du * gz
    e = SECOND * (edu * (gz.abs() + egz) + du.abs() * egz + U * dz.abs()) + TINY
    return e + hulp(dz.abs() + e)


def du_err(dh, W2b):
    return 2 * (E + 2) * U * (dh.double().abs() @ W2b.double().abs().t())


def bounds(pr, ref):
    """per-element bounds of u, dz (bf16 stores) and of the four forward tiles of the hidden-split kernel, from the inputs"""
    M = pr["W1"].shape[1]
    ez = z_err(pr["a2"], pr["W1"], ref["z"])
    eu = u_err(ref["z"], ez)
    W2a = pr["W2"].double().abs()
    tb = []
    for q in range(4):
        sl = quarter(M, q)
        e = eu[:, sl] @ W2a[sl] + 2 * (M // 4 + 2) * U * ((ref["u"][:, sl].abs() + eu[:, sl]) @ W2a[sl])
        if q == 0:
            e = e + 2 * U * (ref["acc0"].abs() + pr["b2"].double().abs() + pr["h"].double().abs())
        tb.append(e)
    out = dict(ez=ez, u=eu, tiles=torch.stack(tb))
    if "du" in ref:
        out["dz"] = dz_err(ref["z"], ez, ref["du"], du_err(pr["dh"], pr["W2b"]))
    return out


def base_quantities(pr):
    """z, u, gz, ez, eu of a problem: they do not depend on W2, so the copies made by with_selector_w2 share them (pr["_base"])"""
    c = pr["_base"]
    if not c:
        z = pr["a2"].double() @ pr["W1"].double() + pr["b1"].double()
        ez = z_err(pr["a2"], pr["W1"], z)
        c.update(z=z, u=gelu(z), gz=gelu_grad(z), ez=ez, eu=u_err(z, ez))
    return c


def fwd_tiles(pr):
    """(reference, bound) [4][rows][128] of the hidden-split forward's tiles for the W2 of `pr` (as model / bounds, the W2-free part cached)"""
    c = base_quantities(pr)
    M = pr["W1"].shape[1]
    W2, W2a = pr["W2"].double(), pr["W2"].double().abs()
    val, bnd = [], []
    for q in range(4):
        sl = quarter(M, q)
        acc = c["u"][:, sl] @ W2[sl]
        e = c["eu"][:, sl] @ W2a[sl] + 2 * (M // 4 + 2) * U * ((c["u"][:, sl].abs() + c["eu"][:, sl]) @ W2a[sl])
        if q == 0:
            e = e + 2 * U * (acc.abs() + pr["b2"].double().abs() + pr["h"].double().abs())
            acc = acc + pr["b2"].double() + pr["h"].double()
        val.append(acc)
        bnd.append(e)
    return torch.stack(val), torch.stack(bnd)


def bwd_u_dz(pr):
    """(u, bound, dz, bound, du, z) of the recompute backward from its inputs a2, dh"""
    c = base_quantities(pr)
    du = pr["dh"].double() @ pr["W2b"].double().t()
    return c["u"], c["eu"], du * c["gz"], dz_err(c["z"], c["ez"], du, du_err(pr["dh"], pr["W2b"])), du, c["z"]


def da2_tiles_from_dz(dz, W1d, M):
    """(value, bound) [4][rows][128] of the backward's partial tiles from the kernel's own stored dz"""
    d, W = dz.double(), W1d.double()
    val = torch.stack([d[:, quarter(M, q)] @ W[quarter(M, q)] for q in range(4)])
    bnd = torch.stack([gemm_bound(d[:, quarter(M, q)].abs() @ W[quarter(M, q)].abs(), M // 4) for q in range(4)])
    return val, bnd


def fused_z1_from_a2(sa, W1, b1):
    """(value, bound) of the fused kernel's saved z1 (bf16) from its own saved a2"""
    val = sa.double() @ W1.double() + b1.double()
    return val, gemm_bound(sa.double().abs() @ W1.double().abs(), E, val, extra_adds=2)


def fused_u_from_a2(sa, W1, b1):
    z = sa.double() @ W1.double() + b1.double()
    return gelu(z), u_err(z, z_err(sa, W1, z))


def fused_hout_from_u(su, W2, b2, h):
    acc = su.double() @ W2.double()
    val = acc + b2.double() + h.double()
    M = W2.shape[0]
    e = (2 * (M // 4 + 2) + 3) * U * (su.double().abs() @ W2.double().abs()) + 2 * U * (acc.abs() + b2.double().abs() + h.double().abs() + val.abs())
    return val, e


# ------------------------------------------------------------------------------------------------ fp32 emulation of the arithmetic
def seq_matmul(a, b, descending=False):
    """a [r][K] b [K][n] in fp32, one product at a time in ascending or descending k: two of the orders a kernel may sum in"""
    a, b = a.float(), b.float()
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    ks = range(a.shape[1] - 1, -1, -1) if descending else range(a.shape[1])
    for k in ks:
        acc += a[:, k:k + 1] * b[k:k + 1]
    return acc


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()     # a b is exact in float64: one rounding, as the fp32 fma


def emu_gelu(x):
    """geluf_ / gelu_fwd_grad_ operation by operation in fp32 (exp2 and the reciprocal evaluated in fp32): g, dg"""
    f = torch.float32
    k0, k1 = torch.tensor(0.7978845608028654, dtype=f), torch.tensor(0.044715, dtype=f)
    Ac = torch.tensor(-2.0, dtype=f) * k0 * torch.tensor(1.4426950408889634, dtype=f)
    Bc = Ac * k1
    x = x.float()
    x2 = x * x
    e = torch.exp2(x * _fma32(Bc.expand_as(x), x2, Ac.expand_as(x)))
    s = torch.tensor(1.0, dtype=f) / (torch.tensor(1.0, dtype=f) + e)
    xd = x * _fma32((torch.tensor(6.0, dtype=f) * k0 * k1).expand_as(x), x2, (torch.tensor(2.0, dtype=f) * k0).expand_as(x))
    return x * s, _fma32(xd, s * (torch.tensor(1.0, dtype=f) - s), s)


def emulate(pr, descending=False):
    """the hidden-split forward and backward in fp32 with bf16 exactly where the kernels round: u, dz, forward tiles, da2 tiles"""
    M = pr["W1"].shape[1]
    z = seq_matmul(pr["a2"], pr["W1"], descending) + pr["b1"].float()
    g, dg = emu_gelu(z)
    u = bf(g)
    tiles = []
    for q in range(4):
        t = seq_matmul(u[:, quarter(M, q)], pr["W2"][quarter(M, q)], descending)
        if q == 0:
            t = t + (pr["b2"].float() + pr["h"].float())
        tiles.append(t)
    out = dict(z=z, u=u, tiles=torch.stack(tiles))
    if pr.get("dh") is not None:
        du = seq_matmul(pr["dh"], pr["W2b"].t(), descending)
        dz = bf(du * dg)
        out.update(dz=dz, da2_tiles=torch.stack([seq_matmul(dz[:, quarter(M, q)], pr["W1d"][quarter(M, q)], descending) for q in range(4)]))
    return out


# ------------------------------------------------------------------------------------------------ selector weights
def PI(M):
    """stream column that feeds hidden unit h: a permutation inside every 128-unit chunk, shifted from chunk to chunk"""
    h = torch.arange(M)
    return (37 * h + 11 * (h // 128)) % E


def selector_w1(M, k, b1):
    """W1 [128][M] bf16 with W1[PI(h)][h] = 2^k[h]; b1 [M] fp32 as given"""
    W = torch.zeros(E, M, dtype=F64)
    W[PI(M), torch.arange(M)] = torch.ldexp(torch.ones(M, dtype=F64), k)
    return bf(W), b1.float()


def n_phases(M):
    return M // 512


def selector_w2(M, phase):
    """S [M][128] bf16: for every quarter q and column n one live unit q M/4 + 128 phase + (29 n + 5) % 128, weight +-2^j"""
    n = torch.arange(E)
    S = torch.zeros(M, E, dtype=F64)
    w = torch.ldexp(torch.where((n // 3) % 2 == 0, 1.0, -1.0).double(), (n % 3) - 1)
    for q in range(4):
        S[q * (M // 4) + 128 * phase + (29 * n + 5 + 7 * q) % E, n] = w
    return bf(S)


def selector_w2_all(M):
    S = selector_w2(M, 0).double()
    for p in range(1, n_phases(M)):
        S = S + selector_w2(M, p).double()
    return bf(S)


# ------------------------------------------------------------------------------------------------ regimes of z
Z_REGIMES = ("core", "zero", "dcross", "neg", "neg_sat", "pos", "pos_sat", "mixed")
REGIMES = Z_REGIMES + ("random",)
DCROSS = -0.7518                                            # zero of gelu'


def _vals(name):
    """(a2 values: bf16-representable, b1 values: multiples of 2^-16 (2^-20 in `zero`), shifts k)"""
    r = lambda lo, hi, step: [lo + step * i for i in range(int(round((hi - lo) / step)) + 1)]
    if name == "core":       # the grid of bf16 values of step 2^-5 on [-4, 4]; b1 puts z next to the bf16 rounding boundaries of its binade
        b = [0.0] + [sg * v for sg in (1, -1) for v in (2.0 ** -7 - 2.0 ** -16, 2.0 ** -8 + 2.0 ** -16, 2.0 ** -9 - 2.0 ** -16, 3 * 2.0 ** -12)]
        return r(-4.0, 4.0, 2.0 ** -5), b, [0]
    if name == "zero":
        return [0.0, 2.0 ** -20, -2.0 ** -20, 0.0], [0.0], [0]
    if name == "dcross":     # bf16 values around -0.75 (spacing 2^-8), refined by b1 to 2^-12
        return r(-0.765625, -0.734375, 2.0 ** -8), [i * 2.0 ** -12 for i in range(-8, 9)], [0]
    if name == "neg":
        return r(-12.0, -4.0, 2.0 ** -4), [i * 2.0 ** -8 for i in range(-4, 5)], [0]
    if name == "neg_sat":
        return [-20.0, -24.0, -32.0, -50.0, -64.0, -100.0, -1000.0, -2.0 ** 20, -2.0 ** 30, -ZMAX / 4], [0.0], [0, 0, 1, 2]
    if name == "pos":
        return r(4.0, 8.0, 2.0 ** -5), [i * 2.0 ** -8 for i in range(-4, 5)], [0]
    if name == "pos_sat":
        return [30.0, 32.0, 50.0, 64.0, 100.0, 128.0, 150.0, 200.0, 40.0, 80.0], [0.0], [0]
    if name == "mixed":
        return [-ZMAX, 0.5, -0.75, 200.0, -20.0, 0.0, 5.0625, -8.0, 2.0 ** -20, 30.0, -1000.0, 3.0, -0.0625, 100.0, -4.5, 1.0, -2.0, 7.5, -12.0, -0.7421875], [0.0], [0]
    raise KeyError(name)


_PROBLEMS = {}


def problem(name, rows, M, seed=0):
    """inputs of one regime, W2 dense (random): a2 bf16 [rows][128], W1 bf16 [128][M], b1, W2 bf16 [M][128], b2, h fp32, dh bf16 and
    the backward's packs W2b (= W2) and W1d (= W1^T).  Shared between tests: never modified (with_selector_w2 returns a copy)."""
    key = (name, rows, M, seed)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    g = torch.Generator().manual_seed(7919 * seed + 31 * rows + M + 1000003 * REGIMES.index(name))
    rn = lambda *s: torch.randn(*s, generator=g)
    h, b2, dh = rn(rows, E) * 1.5 + 0.3, 0.1 * rn(E), bf(rn(rows, E) * 0.05)
    W2 = bf(rn(M, E) / math.sqrt(M))
    if name == "random":                                   # the inputs of tests/test_gpu_kernels.py
        a2, W1, b1 = bf(rn(rows, E)), bf(rn(E, M) * 0.09), 0.1 * rn(M)
    else:
        vals, bs, ks = _vals(name)
        v = torch.tensor(vals, dtype=F64)
        t, c = torch.arange(rows)[:, None], torch.arange(E)[None, :]
        want = v[(7 * t + 3 * c + 5 * (t // 32)) % len(vals)]
        if name == "zero":
            want[0::4] = 0.0                               # all-zero rows
        a2 = bf(want)
        assert torch.equal(a2.double(), want)              # representable in bf16
        hid = torch.arange(M)
        W1, b1 = selector_w1(M, torch.tensor(ks)[(hid // 2) % len(ks)], torch.tensor(bs, dtype=F64)[(hid * 5 + hid // 128) % len(bs)])
        z = a2.double() @ W1.double() + b1.double()
        assert torch.equal(z.float().double(), z) and float(z.abs().max()) <= ZMAX      # representable: exact in the kernel
    pr = dict(name=name, a2=a2, W1=W1, b1=b1, W2=W2, b2=b2, h=h, dh=dh, W2b=W2, W1d=W1.t().contiguous(), phase=None, _base={})
    _PROBLEMS[key] = pr
    return pr


def with_selector_w2(pr, phase):
    M = pr["W1"].shape[1]
    S = selector_w2(M, phase)
    out = dict(pr)
    out.update(W2=S, W2b=selector_w2_all(M), W1d=S, phase=phase)
    return out


# ------------------------------------------------------------------------------------------------ LayerNorm regimes (fused kernel, ln128_parts)
LN_REGIMES = ("unit", "offset", "const")


def ln_rows(name, rows, seed=0):
    """x fp32 [rows][128]: unit (mean 0.3, std 1.5), offset (row mean 200 >> row std 1), const (every fourth row constant:
    variance exactly 0, eps decides; the other rows unit)"""
    g = torch.Generator().manual_seed(100 * seed + rows + LN_REGIMES.index(name))
    x = torch.randn(rows, E, generator=g) * 1.5 + 0.3
    if name == "offset":
        x = torch.randn(rows, E, generator=g) + 200.0
    if name == "const":
        x[0::4] = torch.tensor([3.0, -0.625, 0.0, 100.0])[torch.arange(rows // 4) % 4, None]
    return x
