"""Element-wise criterion for the fp32 Dense GEMM (csrc/gemm_f32.hip, smd_gemm_f32): integer lattices whose results are exact,
selector weights that make the activation epilogues visible on their own, derived per-element bounds, regimes of the
pre-activation z that are set exactly, an fp32 emulation of the kernel's walk and planted faults.  torch float64 / float32 / int64
on the CPU only, no GPU.  U, worst_ratio and rel are those of tests/_attn_ref.py; the geluf_ derivation (s_err, u_err, G2, SECOND,
TINY, ZMAX, emu_gelu) is that of tests/_mlp_ref.py and the sigmoidf_ derivation (sig_err, S2) that of tests/_ln_ref.py: imported,
one definition each.

The op:   z = A W + b   (A [M][K], W [K][N], fp32)      out = act(z) + res[m % row_mod or m]      act: none | tanh-GELU | swish
The kernel: tiles of 128 x 128 for N > 512 and 32 x 128 for N <= 512; k walks in stages of 16 through LDS, inside a stage the
32x32x2 MFMA takes the k pairs (0,1), (2,3), ... in order into ONE accumulator per element; rows, columns and k past the edge
load zeros (16-byte loaders: a group of four is inside or outside as a whole, and they run only where that is the same thing);
accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of its 32 x 32 tile (cd_row).

1. Lattices: a condition, not a measurement.  A, W, bias and residual hold small non-zero integers with
       max_mn (sum_k |a_mk| |w_kn|) + max |b| + max |r| < 2^24                                 (asserted by lattice()).
   Every product, every partial sum in ANY order, the bias add and the residual add are then integers below 2^24 in magnitude:
   fp32 holds them exactly, so with act = none the output equals the int64 result bit for bit, and the tolerance is zero.  The
   values are random, so a swapped, dropped or duplicated row, column or k changes the result; they are never 0, so a dropped
   element always changes it.

2. Selector weights.  K = 128; column n of W has ONE non-zero entry sg(n) 2^j(n) in row perm(n) (a permutation inside every 128
   columns), b[n] is a multiple of a power of two chosen per regime so that
       z[m][n] = sg 2^j A[m][perm(n)] + b[n]
   is representable in fp32 (asserted).  In the kernel 127 products are 0, one is exact (a power-of-two scaling) and the bias add
   is exact: the kernel's z IS z, and an output element is act(z) (+ res) of one known argument.

3. Bounds.  U = 2^-24; an fp32 operation costs U |result|; products of two first-order terms are covered by SECOND = 1 + 2^-10.
   z (dense W)  ez = (K + 2) U (|A| |W| + |b|): a length-K dot product in any order (K + 1) U sum|a w| (Higham 3.5), one more
                rounding for the bias add: the bound tests/test_gpu_fp32_kernels.py uses for act = none.  Selector W: ez = 0.
   GELU         _mlp_ref.s_err / u_err(store=False): eg = (|gelu'(z)| + G2 ez) ez + |z| ds + U |g| (+ TINY), ds from the constant
                folding (8 U |t|), exp2 at 1 ulp, the absolute rounding of 1 + e, rcp at 1 ulp.  Exact places: where
                e (1 + eps_e) < 2^-25 the kernel's sigmoid IS 1 and the output IS z; where the exp2 argument is at least 128 for
                every admissible rounding, t (1 - 8 U) >= 128, exp2 gives +inf, rcp 0 and the output IS -0 / +0.
   swish        _ln_ref.sig_err: sigmoidf_ = rcp(1 + __expf(-x)), __expf = exp2(x log2e) with two roundings of the argument:
                eps_e = expm1(2 U |x|) + 2 U, ds = s (1 - s) eps_e + 3 U s;  es = (|swish'(z)| + S2 ez) ez + |z| ds + U |out|
                (+ TINY), S2 = 1/2 >= max |swish''|.  Exact places: e (1 + eps_e) < 2^-25 gives z itself (x > 17.33);
                |x| log2e (1 - 2 U) >= 128 (x < -88.72) gives exp2 = +inf and the output -0.
   act(0)       0 times a finite sigmoid: exactly 0.
   residual     one more rounding: (1 + U) e_act + U |act(z) + res|.  In the exact places the output is the ONE correctly rounded
                sum fl(v + res) with v = z or 0; the residuals are multiples of 2^-10 below 4 in magnitude, so that float64 holds
                z + res exactly there (asserted) and its conversion to fp32 is that one rounding.
   Nothing is fitted to GPU output.  TINY = 2^-100 absolute covers results (or sigmoids) below the smallest normal number, which
   v_rcp_f32 / v_exp_f32 may flush.

   What the bound cannot see: the GELU constant A = -2 k0 log2e one ulp off moves t by at most 2 U |t|, inside the 8 U |t| that the
   derivation grants the folded constants (each of A's three roundings is granted U, so a fourth fits).  It is kept as the
   documented limit BEYOND (the host test asserts that it stays inside the bound).  The same fault in swish's __expf (log2e one ulp
   away from the true value: 1.64 U |x| where the derivation grants the constant U) IS seen, in the negative tail where the
   relative error of the sigmoid is |x| times that of the argument.

4. Regimes of z (SEL_REGIMES), each used with both activations.  Operands stay at or above 2^-60 in magnitude (x^2 = 2^-120 is a
   normal number): fp32 denormals are kept OUT of A, W, b and z, because whether the fp32 MFMA flushes them has not been measured.
       zero       +-0 in A and b                           tiny       +-{1, 3, 5, 2^10, 2^20} 2^-60, shifts 0..2
       gelu_min   around -0.7518 on a 2^-12 grid           swish_min  around -1.2785 on a 2^-12 grid
       sweep      every multiple of 2^-10 in [-12, 12), four parts of 64 rows
       one_gelu   both sides of 5.06 (1 + e becomes 1)     one_swish  both sides of 17.33
       exp2_ovf   both sides of -10.07 (t = 128)           expf_ovf   [-89.5, -86]: both sides of -88.72, and of -87.34 where the
                                                                      sigmoid leaves the normal numbers
       neg_tail   [-64, -16] on a 2^-8 grid, two parts: swish's sigmoid runs from 1e-7 to 1e-28, above TINY, where its relative
                  error is |x| times that of the exp2 argument (the sharpest place for the __expf constant); GELU is exactly -0
       big        +-2^20, +-2^30, +-ZMAX = +-2^42 (t of geluf_ stays finite up to there, _mlp_ref)
   Columns alternate in sign in groups of three, so every regime also runs mirrored.

5. Emulation (emulate): the walk in fp32, operation for operation where IEEE defines it: tile form from N, zero fill, stages of 16,
   k pairs as two fma in order (a model: on a lattice every order gives the same bits, elsewhere the bound covers any order),
   cd_row, bias, activation (exp2 and the reciprocal evaluated in fp32), residual.  fast=True replaces the k walk by one float64
   matrix product: for the large old shapes, where only the size of a fault's effect is wanted.  FAULTS are planted in it.
"""
import math

import torch

import _ln_ref as LN
import _mlp_ref as MLP
from _attn_ref import U, F64, worst_ratio, rel                      # noqa: F401  (one definition, re-exported)
from _mlp_ref import SECOND, TINY, G2, ZMAX, LOG2E

S2 = LN.S2
F32 = torch.float32
EXACT = 2 ** 24
OLD_REL = 1e-5                                   # the whole-matrix threshold of tests/test_gpu_fp32_kernels.py
ACT = {"none": 0, "gelu": 1, "swish": 2}
BN, BK = 128, 16

# ------------------------------------------------------------------------------------------------ closed forms
gelu, gelu_grad = MLP.gelu, MLP.gelu_grad
swish, swish_grad = LN.swish, LN.swish_grad


def act_ref(z, act):
    return gelu(z) if act == "gelu" else swish(z) if act == "swish" else z


def form_rows(N):
    """rows of the workgroup tile: 128 x 128 above N = 512, 32 x 128 up to it"""
    return 128 if N > 512 else 32


def cd_row(reg, half):
    return (reg & 3) + 8 * (reg >> 2) + 4 * half


# ------------------------------------------------------------------------------------------------ lattices
SWEEP_M = (1, 31, 32, 33, 127, 128, 129, 257)
SWEEP_N = (1, 3, 4, 127, 128, 129, 131, 512, 513, 516, 641)
SWEEP_K = (1, 2, 3, 4, 15, 16, 17, 20, 31, 32, 33, 47)
MODES = ("none", "full", 1, 7, 32)               # residual: none, one row each, or row m % row_mod of a table
MAXM = max(SWEEP_M)
AMAX, BMAX = 255, 4095
_LATTICES = {}


def _ints(g, shape, hi):
    """random integers with magnitudes 1 .. hi: never 0"""
    mag = torch.randint(1, hi + 1, shape, generator=g)
    return torch.where(torch.randint(0, 2, shape, generator=g) == 1, mag, -mag)


def lattice(N, K, seed=0):
    """int64 operands of the (N, K) lattice for every M <= MAXM (slice the rows): A [MAXM][K], W [K][N], b [N], r [MAXM][N] and
    z = A W + b.  Shared between tests: never modified."""
    key = (N, K, seed)
    if key not in _LATTICES:
        g = torch.Generator().manual_seed(1000003 * seed + 641 * K + N)
        A, W = _ints(g, (MAXM, K), AMAX), _ints(g, (K, N), AMAX)
        b, r = _ints(g, (N,), BMAX), _ints(g, (MAXM, N), BMAX)
        mag = int((A.abs() @ W.abs()).max()) + int(b.abs().max()) + int(r.abs().max())
        assert mag < EXACT, (N, K, mag)                        # every partial sum in any order is exact in fp32
        _LATTICES[key] = dict(A=A, W=W, b=b, r=r, z=A @ W + b, mag=mag)
    return _LATTICES[key]


def mode_ok(M, mode):
    return mode in ("none", "full") or mode == 1 or M % mode != 0


def sweep_cases():
    """(M, N, K, mode): the cross product of SWEEP_M, SWEEP_N, SWEEP_K, each with one residual mode, rotated so that every
    mode meets every M, N and K; a row_mod that divides M (other than 1) gives way to the next mode"""
    out = []
    for iN, N in enumerate(SWEEP_N):
        for iK, K in enumerate(SWEEP_K):
            for iM, M in enumerate(SWEEP_M):
                i = iM + 2 * iN + 3 * iK
                while not mode_ok(M, MODES[i % len(MODES)]):
                    i += 1
                out.append((M, N, K, MODES[i % len(MODES)]))
    return out


def reduced_cases():
    """24 (M, N, K) that hold every value of the three lists at least twice (in two different pairings)"""
    out = [(SWEEP_M[i % 8], SWEEP_N[i % 11], SWEEP_K[i]) for i in range(12)]
    out += [(SWEEP_M[(3 * i + 5) % 8], SWEEP_N[(7 * i + 4) % 11], SWEEP_K[(5 * i + 6) % 12]) for i in range(12)]
    return out


def res_rows(M, mode):
    """row of the residual table that output row m reads"""
    m = torch.arange(M)
    return m if mode == "full" else m % mode


def lattice_want(lat, M, mode):
    """int64 [M][N]: the exact result of act = none"""
    z = lat["z"][:M]
    return z if mode == "none" else z + lat["r"][res_rows(M, mode)]


# ------------------------------------------------------------------------------------------------ bounds
def z_err(A, W, b, K):
    mag = A.double().abs() @ W.double().abs()
    return (K + 2) * U * (mag + (0.0 if b is None else b.double().abs()))


def gelu_zones(z):
    """(the kernel's sigmoid is exactly 1: output z;  exactly 0: output +-0) for geluf_ at the exact argument z: the conditions
    of _mlp_ref.s_err, the second with the 8 U |t| the argument may be off by"""
    tt = (-MLP._t(z) * LOG2E).clamp(-200.0, 200.0)
    eps = torch.expm1(8 * U * math.log(2.0) * tt.abs()) + 2 * U
    return torch.exp2(tt) * (1 + eps) < 2.0 ** -25, tt * (1 - 8 * U) >= 128.0


def swish_zones(z):
    eps = torch.expm1(2 * U * z.abs().clamp_max(1e6)) + 2 * U
    return torch.exp(-z.clamp(-700.0, 700.0)) * (1 + eps) < 2.0 ** -25, -z * LOG2E * (1 - 2 * U) >= 128.0


def zones(z, act):
    one, zero = gelu_zones(z) if act == "gelu" else swish_zones(z)
    return one, zero | (z == 0)


def act_err(z, act, ez=None):
    """what act(z') may be off by, z' within ez of the exact z (ez None: z' = z)"""
    z = z.double()
    if act == "none":
        return torch.zeros_like(z) if ez is None else ez
    e0 = torch.zeros_like(z) if ez is None else ez
    if act == "gelu":
        e = MLP.u_err(z, e0, store=False)
    else:
        s, _, ds = LN.sig_err(z)
        e = SECOND * ((swish_grad(z).abs() + S2 * e0) * e0 + z.abs() * ds + U * (z * s).abs()) + TINY
    return torch.where(z == 0, torch.zeros_like(e), e) if ez is None else e


def out_ref_bound(z, act, ez=None, res=None):
    """(reference, bound) float64 of act(z) + res"""
    z = z.double()
    v, e = act_ref(z, act), act_err(z, act, ez)
    if res is None:
        return v, e
    ref = v + res.double()
    return ref, (1 + U) * e + U * ref.abs()


def exact_want(z, act, res=None):
    """(mask, fp32 values): where the derivation says the output is exact, and what it is: z where the sigmoid is 1, 0 where it
    is 0, and with a residual the one correctly rounded sum"""
    z = z.double()
    one, zero = zones(z, act)
    v = torch.where(one, z, torch.zeros_like(z))
    if res is not None:
        s = v + res.double()
        m = one | zero
        assert torch.equal((s - res.double())[m], v[m]) and torch.equal((s - v)[m], res.double()[m])     # float64 holds the sum
        v = s
    return one | zero, v.float()


def judge(out, z, act, res=None, ez=None):
    """the criterion on one output [M][N] whose exact pre-activation is z (float64): (worst |err| / bound, the same outside the
    exact places, every element finite, equal to z / 0 / fl(v + res) where the derivation says so).  In the places where the output
    is z itself the bound IS the distance z (1 - s) from the reference, so the first figure reads 1 / SECOND there by construction;
    the second is the one that measures the arithmetic.  With a residual the last addition's rounding leads, and a correctly rounded
    sum just above a power of two is at 1 - 2^-23 of its bound U |result|: figures near 1 are then the format, not the kernel."""
    out = out.detach().float().cpu()
    ref, bound = out_ref_bound(z, act, ez, res)
    ratio = (out.double() - ref).abs() / bound.clamp_min(1e-300)
    ratio = torch.where((bound == 0) & (out.double() == ref), torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    if ez is not None or act == "none":
        return float(ratio.max()), float(ratio.max()), bool(torch.isfinite(out).all()), True
    mask, want = exact_want(z, act, res)
    inner = float(ratio[~mask].max()) if bool((~mask).any()) else 0.0
    return float(ratio.max()), inner, bool(torch.isfinite(out).all()), torch.equal(out[mask], want[mask])


# ------------------------------------------------------------------------------------------------ selector problems
SEL_M, SEL_K = 64, 128
SEL_N = (128, 640)
SEL_REGIMES = ("zero", "tiny", "gelu_min", "swish_min", "sweep", "one_gelu", "one_swish", "exp2_ovf", "neg_tail", "expf_ovf", "big")
SWISH_MIN = -1.2785                                         # zero of swish'
ONE_GELU, ONE_SWISH, EXP2_OVF, EXPF_OVF = 5.06, 17.33, -10.07, -88.72


def _vals(name):
    """(values of A, values of b, shifts j) of a regime"""
    r = lambda lo, hi, step: [lo + step * i for i in range(int(round((hi - lo) / step)) + 1)]
    pm = lambda v: [s * x for x in v for s in (1.0, -1.0)]
    fine = [i * 2.0 ** -12 for i in range(-8, 9)]
    if name == "zero":
        return [0.0, -0.0, 0.0, 0.0, -0.0], [0.0, -0.0], [0, 1]
    if name == "tiny":
        t = 2.0 ** -60
        return pm([t, 3 * t, 5 * t, 2.0 ** -50, 2.0 ** -40]), [0.0, 4 * t, -2 * t], [0, 1, 2]
    if name == "gelu_min":
        return r(-0.765625, -0.734375, 2.0 ** -8), fine, [0]
    if name == "swish_min":
        return r(-1.296875, -1.265625, 2.0 ** -8), fine, [0]
    if name == "sweep":
        return r(-12.0, 12.0, 2.0 ** -3), [i * 2.0 ** -10 for i in range(128)], [0]
    if name == "one_gelu":
        return r(4.875, 5.25, 2.0 ** -6), fine, [0]
    if name == "one_swish":
        return r(17.0, 17.75, 2.0 ** -5), [2 * f for f in fine], [0]
    if name == "exp2_ovf":
        return r(-10.25, -9.875, 2.0 ** -6), fine, [0]
    if name == "neg_tail":
        return r(-64.0, -16.0, 0.5), [16 * f for f in fine], [0]
    if name == "expf_ovf":
        return r(-89.5, -86.0, 2.0 ** -4), [4 * f for f in fine], [0]
    if name == "big":
        return pm([2.0 ** 20, 2.0 ** 30, ZMAX, 2.0 ** 20 + 0.125, 3.0 * 2.0 ** 19]), [0.0], [0]
    raise KeyError(name)


def n_parts(name):
    return -(-len(_vals(name)[0]) // SEL_M)


def sel_perm(N):
    n = torch.arange(N)
    return (37 * n + 11 * (n // 128)) % SEL_K


_SELECTORS = {}


def selector_problem(name, N, part=0, res=False):
    """fp32 operands of one regime: A [64][128] carries the regime's values, W [128][N] selects, b [N]; z float64 is what the kernel
    forms exactly.  res: a residual [64][N] of non-zero multiples of 2^-10 below 4.  Shared between tests: never modified."""
    key = (name, N, part, res)
    if key in _SELECTORS:
        return _SELECTORS[key]
    av, bv, jv = (torch.tensor(v, dtype=F64) for v in _vals(name))
    m, p, n = torch.arange(SEL_M)[:, None], torch.arange(SEL_K)[None, :], torch.arange(N)
    A = av[(SEL_M * part + m + 7 * p) % len(av)]
    sg = torch.where((n // 3) % 2 == 0, 1.0, -1.0).double()
    w = torch.ldexp(sg, jv[(n // 2) % len(jv)].long())
    b = bv[(5 * n + n // 128) % len(bv)]
    W = torch.zeros(SEL_K, N, dtype=F64)
    W[sel_perm(N), n] = w
    z = w * A[:, sel_perm(N)] + b
    for t in (A, b, z):
        assert torch.equal(t.float().double(), t)              # representable: the kernel's z is exact
    nz = torch.cat([A.flatten(), b, z.flatten()])
    nz = nz[nz != 0].abs()
    assert (nz.numel() == 0 or float(nz.min()) >= 2.0 ** -60) and float(z.abs().max()) <= ZMAX        # no denormal operands
    pr = dict(name=name, M=SEL_M, K=SEL_K, N=N, A=A.float(), W=W.float(), b=b.float(), z=z, res=None, row_mod=0)
    if res:
        g = torch.Generator().manual_seed(97 * SEL_REGIMES.index(name) + N + part)
        pr["res"] = (_ints(g, (SEL_M, N), 4095).double() * 2.0 ** -10).float()
    _SELECTORS[key] = pr
    return pr


def selector_list():
    return [(name, N, part) for name in SEL_REGIMES for N in SEL_N for part in range(n_parts(name))]


# ------------------------------------------------------------------------------------------------ dense problems
DENSE_SHAPES = ((96, 146, 128), (160, 128, 640))             # M, K, N: one per tile form


def dense_problem(M, K, N, seed=0, sigma=2.0):
    """N(0, 1) A, W scaled so that z has standard deviation sigma: |z| reaches about 3 sigma = 6, both tails populated"""
    g = torch.Generator().manual_seed(7919 * seed + M + 3 * K + 7 * N)
    A = torch.randn(M, K, generator=g)
    W = sigma * torch.randn(K, N, generator=g) / math.sqrt(K)
    b = 0.1 * torch.randn(N, generator=g)
    return dict(name="dense", M=M, K=K, N=N, A=A, W=W, b=b, z=A.double() @ W.double() + b.double(), res=None, row_mod=0)


def old_problem(M, K, N, epi, cap=True):
    """the inputs of tests/test_gpu_fp32_kernels.py (N(0, 1) A, W / sqrt(K), 0.1 N(0, 1) bias).  cap: M above 384 is cut to
    256 + M % 128 rows, which keeps M mod 32 and mod 128 (the raggedness of both tile forms); the share of a faulty edge row or
    tile in the rel-L2 only grows by that, so a fault that passes the old threshold on the cut problem passes on the full one"""
    if cap and M > 384:
        M = 256 + M % 128
    g = torch.Generator().manual_seed(M + 3 * K + 7 * N)
    pr = dict(name="old", M=M, K=K, N=N, A=torch.randn(M, K, generator=g), W=torch.randn(K, N, generator=g) / math.sqrt(K),
              b=0.1 * torch.randn(N, generator=g), res=None, row_mod=0, act="none")
    if epi == "residual":
        pr["res"] = torch.randn(M, N, generator=g)
    elif epi == "posenc":
        pr["res"], pr["row_mod"] = torch.randn(32, N, generator=g), 32
    elif epi in ACT:
        pr["act"] = epi
    return pr


# ------------------------------------------------------------------------------------------------ fp32 emulation with planted faults
FAULTS = ("odd-k-last-pair-dropped", "k-tail-of-partial-stage-dropped", "group-of-four-on-ragged-k-dropped",
          "group-of-four-on-ragged-k-read", "last-row-dropped", "last-row-duplicated", "last-col-dropped", "last-col-duplicated",
          "form-switch-at-512", "row-and-instead-of-mod", "residual-before-activation", "act-codes-swapped", "sigmoid-arg-1ulp",
          "cd-row-permuted")
BEYOND = ("gelu-constant-1ulp",)                              # inside the derivation's allowance: section 3 of the docstring

_L2E32 = torch.tensor(1.4426950408889634, dtype=F32)
# one ulp AWAY from the true value (the fp32 constant lies above log2(e) by 0.25 U: the next one up is off by 1.64 U)
_L2E32_OFF = torch.nextafter(_L2E32, torch.tensor(2.0 if float(_L2E32) > 1.4426950408889634 else 1.0, dtype=F32))


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emu_swish(x, l2e=_L2E32):
    """swishf_ operation by operation in fp32: x rcp(1 + exp2(-x log2e))"""
    x = x.float()
    one = torch.tensor(1.0, dtype=F32)
    return x * (one / (one + torch.exp2(-x * l2e)))


def _emu_act(v, act, fault, fast):
    if act == "none":
        return v
    if fault == "act-codes-swapped":
        act = "swish" if act == "gelu" else "gelu"
    if fast:
        if act == "gelu":
            return v * torch.sigmoid(MLP._t(v) * ((1 + 2.0 ** -23) if fault == "gelu-constant-1ulp" else 1.0))
        return v * torch.sigmoid(v * (float(_L2E32_OFF) / float(_L2E32) if fault == "sigmoid-arg-1ulp" else 1.0))
    if act == "gelu":
        if fault == "gelu-constant-1ulp":
            return _emu_gelu_off(v)
        return MLP.emu_gelu(v)[0]
    return emu_swish(v, _L2E32_OFF if fault == "sigmoid-arg-1ulp" else _L2E32)


def _emu_gelu_off(x):
    """geluf_ with the folded constant A one ulp larger in magnitude (Bc = A k1 follows it)"""
    k0, k1 = torch.tensor(0.7978845608028654, dtype=F32), torch.tensor(0.044715, dtype=F32)
    Ac = torch.tensor(-2.0, dtype=F32) * k0 * _L2E32
    Ac = torch.nextafter(Ac, torch.tensor(-4.0, dtype=F32))
    Bc = Ac * k1
    x = x.float()
    e = torch.exp2(x * _fma32(Bc.expand_as(x), x * x, Ac.expand_as(x)))
    return x * (torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) + e))


def emulate(pr, act="none", fault=None, fast=False, vec=True, a_pad=None):
    """the kernel's walk on the problem `pr` (A, W, b, res, row_mod as tensors of fp32 values): fp32 [M][N], NaN where nothing is
    written.  vec: the operands are 16-byte aligned (the vector loaders run where K % 4 == 0 / N % 4 == 0).  a_pad: what lies behind
    the K values of a row of A (lda > K); None: the next row, and zeros behind the last.  fast: float64 arithmetic and one matrix
    product in place of the k walk."""
    A, W = pr["A"].float(), pr["W"].float()
    M, K = A.shape
    N = W.shape[1]
    BM = form_rows(N)
    tiles_m, tiles_n = -(-M // BM), -(-N // BN)
    if fault == "form-switch-at-512" and N == 512:            # the launcher counts 128-row tiles from N >= 512, the kernel has 32
        tiles_m = -(-M // 128)
    Mp, Np = tiles_m * BM, tiles_n * BN
    stages = K // BK if fault == "k-tail-of-partial-stage-dropped" else -(-K // BK)
    Kp = stages * BK
    # ---- loaders: zero fill past the edges
    mem = torch.zeros(max(M, Mp) * K + Kp + 4, dtype=F32)     # A as it lies in memory behind its K columns
    if a_pad is None:
        mem[:M * K] = A.flatten()
        ext = torch.stack([mem[m * K:m * K + Kp + 4] for m in range(M)])
    else:
        ext = torch.full((M, max(K, Kp) + 4), float(a_pad), dtype=F32)
        ext[:, :K] = A
    k = torch.arange(Kp)
    inside = k < K
    if fault == "group-of-four-on-ragged-k-dropped":          # "outside as a whole" whatever K % 4
        inside = (k // 4) * 4 + 3 < K
    elif fault == "group-of-four-on-ragged-k-read":           # "inside as a whole" whatever K % 4
        inside = (k // 4) * 4 < K
    elif fault == "odd-k-last-pair-dropped":
        inside = (k // 2) * 2 + 1 < K
    rows = min(M, Mp)
    Ap = torch.zeros(Mp, Kp, dtype=F32)
    Ap[:rows] = torch.where(inside[None, :], ext[:rows, :Kp], torch.zeros((), dtype=F32))
    Wp = torch.zeros(Kp, Np, dtype=F32)
    kk = min(K, Kp)
    Wp[:kk, :N] = W[:kk]
    if M % BM and M >= 2 and rows == M:
        if fault == "last-row-dropped":
            Ap[M - 1] = 0.0
        elif fault == "last-row-duplicated":
            Ap[M - 1] = Ap[M - 2]
    if N % BN and N >= 2:
        if fault == "last-col-dropped":
            Wp[:, N - 1] = 0.0
        elif fault == "last-col-duplicated":
            Wp[:, N - 1] = Wp[:, N - 2]
    # ---- the k walk: one accumulator per element, k pairs in order
    if fast:
        acc = Ap.double() @ Wp.double()
    else:
        acc = torch.zeros(Mp, Np, dtype=F32)
        for k0 in range(0, Kp, 2):
            acc = _fma32(Ap[:, k0:k0 + 1], Wp[k0:k0 + 1], acc)
            acc = _fma32(Ap[:, k0 + 1:k0 + 2], Wp[k0 + 1:k0 + 2], acc)
    # ---- epilogue: register r of lane half h holds row cd_row(r, h) of its 32 x 32 tile and is written to the row the kernel names
    src = torch.zeros(32, dtype=torch.int64)
    for reg in range(16):
        for h in range(2):
            dst = (reg & 3) + 4 * (reg >> 2) + 16 * h if fault == "cd-row-permuted" else cd_row(reg, h)
            src[dst] = cd_row(reg, h)
    acc = acc.view(Mp // 32, 32, Np)[:, src, :].reshape(Mp, Np)
    v = acc[:rows, :N]
    if pr.get("b") is not None:
        v = v + (pr["b"].double() if fast else pr["b"].float())
    res = pr.get("res")
    r = None
    if res is not None:
        m, rm = torch.arange(rows), pr.get("row_mod", 0)
        idx = m if rm == 0 else (m & (rm - 1)) if fault == "row-and-instead-of-mod" else m % rm
        r = res.double()[idx] if fast else res.float()[idx]
    if r is not None and fault == "residual-before-activation":
        v = _emu_act(v + r, act, fault, fast)
    else:
        v = _emu_act(v, act, fault, fast)
        if r is not None:
            v = v + r
    out = torch.full((M, N), float("nan"), dtype=F64 if fast else F32)
    out[:rows] = v
    return out


def lattice_problem(M, N, K, mode):
    """the fp32 operands of one exact case, as emulate and the GPU test take them"""
    lat = lattice(N, K)
    pr = dict(name="lattice", M=M, K=K, N=N, A=lat["A"][:M].float(), W=lat["W"].float(), b=lat["b"].float(), res=None, row_mod=0)
    if mode != "none":
        pr["res"] = lat["r"][:M].float() if mode == "full" else lat["r"][:mode].float()
        pr["row_mod"] = 0 if mode == "full" else mode
    return pr


def bits_equal(got, want):
    """fp32 tensors equal bit for bit (a NaN that was never overwritten fails, and so does a zero of the wrong sign)"""
    return torch.equal(got.float().contiguous().view(torch.int32), want.float().contiguous().view(torch.int32))
