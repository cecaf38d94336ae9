"""Element-wise criterion for the e4m3 path: the row quantiser (quantize_rows_e4m3_kernel in csrc/norm.hip, e4m3_row_exponent /
pack4_e4m3 in csrc/smd_common.h) and the scaled-MFMA GEMM (gemm_nt256_kernel<V, true> in csrc/gemm_nt256.hip).  torch float64 and
integers on the CPU only, no GPU, and no torch.float8_e4m3fn: the encoder and the decode table are written out here, and
tests/test_e4m3_ref_host.py checks them against torch's cast.

1. The format.  OCP e4m3 "fn": sign, 4 exponent bits (bias 7), 3 mantissa bits, no infinity, 0x7F / 0xFF are NaN, the largest
   finite value is 0x7E = 1.75 * 2^8 = 448.  Normal numbers 2^E (1 + m / 8), E = -6 .. 8, spacing 2^(E - 3); subnormals m 2^-9
   below 2^-6.  encode() rounds to nearest, ties to even, with frexp and integer rounding: |v| = q * spacing with q exact in
   float64, n = rne(q), byte = 8 (E + 6) + n (n = 16 carries into the next binade by itself; E = -6 covers the subnormals).

2. The quantiser.  amax = max |x| over the K columns of a row (bf16 -> fp32, exact); e = row_exponent(amax) = the smallest e with
   amax 2^-e <= 448: floor(log2 amax) - 8, plus one when the mantissa of amax exceeds 1.75 (field > 0x600000), at least -126, 0 for
   a zero row; the scale dword is e + 127; byte = encode(clamp(x 2^-e, -448, 448)).  x 2^-e is a power-of-two scaling: exact in
   fp32 unless it falls below 2^-126, where every value rounds to a zero byte anyway (the first non-zero midpoint is 2^-10).  The
   only freedom left to the hardware conversion is the SIGN of a zero it rounded to: same_value() holds 0x00 and 0x80 equal and
   nothing else.

3. The exact GEMM.  Operands are bytes that decode to the integers -4 .. 4 (never 0: a dropped element always shows), the E8M0
   row exponents lie in [-8, 8] and differ between rows m and m ^ 1, m and m + 32 (a scale read from either neighbour shows).
   For output (m, n) every product is an integer of magnitude <= 16, every partial sum in ANY order an integer of magnitude
   <= 16 K <= 2^15, times ONE power of two 2^(sa[m] + sb[n]) in [2^-16, 2^16]: fp32 holds all of them exactly whether the
   hardware scales the products or the operands, adds in a tree or a chain, truncates or rounds.  The fp32 output therefore equals
   gemm_exact() bit for bit (exact_condition() asserts the premises by bounding the integer sums).
   One-hot operands (ONEHOT_*): row m of A holds a single 1 at column (37 m + 11) % K, B[n][k] = (n + 3 k) % 9 - 4: output (m, n)
   NAMES the k that was multiplied.

4. Bounds.  U = 2^-24.
   exact operands, bias and fp32 residual:  2 U (|acc| + |bias| + |res|): two fp32 roundings;
   bf16 output: plus half a bf16 ulp of the result (RNE, 8 significant bits): 2^(floor(log2 |result|) - 8), which is between
   2^-9 and 2^-8 of |result| (half_ulp_bf16);
   bf16 residual: read exactly (bf16 -> fp32), one more fp32 addition;
   quantised random operands: 2 (K + 2) U sum_k |a_k b_k| (products of two e4m3 values are exact in fp32: 4 + 4 significant bits;
   (K + 1) U sum |a b| is the any-order bound of a length-K sum with a rounding adder, Higham 3.5; the factor 2 admits a truncating
   adder, which loses up to a whole ulp = 2 U per addition where rounding loses U).

5. Planted faults (QUANT_FAULTS, GEMM_FAULTS): small transformations of the reference that the cases must see; the host test
   asserts that each changes the reference result on the cases the GPU tests run."""
import math

import torch

F64 = torch.float64
U = 2.0 ** -24
FMAX = 448.0


# ------------------------------------------------------------------------------------------------ the format
def _decode_table():
    t = []
    for b in range(256):
        s, ex, m = b >> 7, (b >> 3) & 15, b & 7
        if ex == 15 and m == 7:
            v = float("nan")
        elif ex == 0:
            v = m * 2.0 ** -9
        else:
            v = (8 + m) * 2.0 ** (ex - 7 - 3)
        t.append(-v if s else v)
    return torch.tensor(t, dtype=F64)


DECODE = _decode_table()                                       # -0.0 at 0x80
FINITE_CODES = [b for b in range(256) if (b & 0x7F) != 0x7F]   # 254


def decode(b):
    """uint8 tensor -> float64"""
    return DECODE[torch.as_tensor(b).long()]


def encode(v, ties="even"):
    """float64 tensor, |v| <= 448 -> uint8 e4m3 bytes, round to nearest, ties to even (ties="away": the planted fault)"""
    v = torch.as_tensor(v, dtype=F64)
    a = v.abs()
    assert bool((a <= FMAX).all()), "encode: |v| above 448"
    _, ex = torch.frexp(a)                                     # a = m 2^ex, m in [0.5, 1)
    E = (ex.long() - 1).clamp(-6, 8)
    E = torch.where(a == 0, torch.full_like(E, -6), E)         # frexp(0) gives ex = 0
    q = torch.ldexp(a, 3 - E)                              # a / spacing: exact (a power of two), in [0, 16)
    lo = torch.floor(q)
    fr = q - lo
    lo = lo.long()
    if ties == "even":
        up = (fr > 0.5) | ((fr == 0.5) & (lo % 2 == 1))
    else:
        up = fr >= 0.5
    n = lo + up.long()
    code = 8 * (E + 6) + n
    assert bool(((code >= 0) & (code <= 0x7E)).all())
    code = code | (torch.signbit(v).long() << 7)
    return code.to(torch.uint8)


def same_value(a, b):
    """bool tensor: bytes equal, 0x00 and 0x80 equal to each other"""
    a, b = torch.as_tensor(a).long(), torch.as_tensor(b).long()
    return (a == b) | (((a & 0x7F) == 0) & ((b & 0x7F) == 0))


def zero_sign_diffs(a, b):
    """number of places where one holds 0x00 and the other 0x80"""
    a, b = torch.as_tensor(a).long(), torch.as_tensor(b).long()
    return int(((a != b) & ((a & 0x7F) == 0) & ((b & 0x7F) == 0)).sum())


# ------------------------------------------------------------------------------------------------ the quantiser
def row_exponent(amax, bump=True):
    """e4m3_row_exponent on the fp32 bit pattern: int64 tensor.  amax: float32 tensor, >= 0"""
    amax = torch.as_tensor(amax, dtype=torch.float32).contiguous()
    bits = amax.view(torch.int32).long() & 0xFFFFFFFF
    e = ((bits >> 23) & 0xFF) - 127 - 8
    if bump:
        e = e + ((bits & 0x7FFFFF) > 0x600000).long()
    e = e.clamp_min(-126)
    return torch.where(amax > 0, e, torch.zeros_like(e))


def quantize_rows(x_bf16, fault=None):
    """(bytes uint8 [rows][K], exponents int64 [rows]) as the kernel defines them; the scale dword is exponent + 127"""
    assert x_bf16.dtype == torch.bfloat16
    x = x_bf16.double()
    K = x.shape[1]
    span = x[:, :512] if fault == "amax-first-pass-only" else x
    amax = span.abs().amax(1).float()
    e = row_exponent(amax, bump=fault != "exponent-without-bump")
    y = torch.ldexp(x, -e.unsqueeze(1).expand(-1, K)).clamp(-FMAX, FMAX)
    return encode(y, ties="away" if fault == "round-half-away" else "even"), e


QUANT_FAULTS = ("exponent-without-bump", "round-half-away", "amax-first-pass-only")

QUANT_SHAPES = ((1, 8, 8), (5, 520, 520), (4, 512, 512), (7, 2048, 2048), (6, 1024, 1032), (9, 2048, 2056))     # rows, K, ld
REGIMES = ("randn", "zero", "m175", "m175_next", "one", "bf16_max", "denormal", "neg_amax",
           "slot0", "slot1", "slot2", "slot3", "slot4", "slot5", "slot6", "slot7", "last_col", "ties", "sub_mid")
RANDN_EXP = (-30, -17, -3, 0, 9, 22, 30)
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127
PAD_VALUE = 3.0e38                                             # finite garbage behind the K columns of a row (ld > K)


def tie_values():
    """every e4m3 midpoint up to 448, both ranges: odd multiples of half a spacing"""
    t = [(n + 0.5) * 2.0 ** -9 for n in range(8)]
    t += [(8 + j + 0.5) * 2.0 ** (E - 3) for E in range(-6, 9) for j in range(8)]
    return [v for v in t if v < FMAX]


def _bf16_exact(v):
    b = v.to(torch.bfloat16)
    assert torch.equal(b.double(), v), "regime value is not a bf16 number"
    return b


def _fill(g, K, amax, at, sign=1.0):
    """N(0,1) numbers scaled below amax / 4.4 (two binades down: an amax that misses column `at` gives another exponent), and
    +-amax itself at column `at`"""
    z = torch.randn(K, generator=g, dtype=F64)
    z = z / (float(z.abs().max()) * 4.4) * amax
    row = z.to(torch.bfloat16).double()
    assert float(row.abs().max()) < amax or K == 1
    row[at] = sign * amax
    return _bf16_exact(row)


def regime_row(name, K, salt):
    """one bf16 row [K] of regime `name`; salt varies the draw (row index, call index)"""
    g = torch.Generator().manual_seed(7919 * REGIMES.index(name) + 31 * K + salt)
    if name == "randn":
        f = RANDN_EXP[salt % len(RANDN_EXP)]
        return (torch.randn(K, generator=g, dtype=F64) * 2.0 ** f).to(torch.bfloat16)
    if name == "zero":
        row = torch.zeros(K, dtype=F64)
        row[1::2] = -0.0
        return row.to(torch.bfloat16)
    if name == "m175":
        return _fill(g, K, 1.75 * 2.0 ** (salt % 5 - 2), (3 * salt + 1) % K)
    if name == "m175_next":
        return _fill(g, K, (1.75 + 2.0 ** -7) * 2.0 ** (salt % 5 - 2), (5 * salt + 2) % K)
    if name == "one":
        return _fill(g, K, 1.0, (7 * salt + 3) % K)
    if name == "bf16_max":
        return _fill(g, K, BF16_MAX, (11 * salt + 4) % K, sign=-1.0 if salt % 2 else 1.0)
    if name == "denormal":                                     # k 2^-133, k = 1 .. 127: every bf16 denormal magnitude
        k = (torch.arange(K) * 37 + salt) % 127 + 1
        sg = torch.where(torch.arange(K) % 3 == 0, -1.0, 1.0).double()
        return _bf16_exact(sg * k.double() * 2.0 ** -133)
    if name == "neg_amax":
        return _fill(g, K, 1.5 * 2.0 ** (salt % 7 - 3), (13 * salt + 5) % K, sign=-1.0)
    if name.startswith("slot"):                                # amax in element slot j of a lane's 8, the lane (and pass) varying
        j = int(name[4:])
        lane = (7 * j + 3 + 61 * salt) % (K // 8)
        return _fill(g, K, 1.25 * 2.0 ** (j - 4), 8 * lane + j)
    if name == "last_col":
        return _fill(g, K, 1.875 * 2.0 ** 3, K - 1)
    if name == "ties":                                         # e = 5: x = tie 2^5, amax = 448 2^5 in column 0
        t = torch.tensor(tie_values(), dtype=F64)
        c = torch.arange(K)
        row = t[(c * 5 + 3 * salt) % len(t)] * torch.where(c % 2 == 1, -1.0, 1.0).double()
        row[0] = FMAX
        return _bf16_exact(row * 2.0 ** 5)
    if name == "sub_mid":                                      # e = -3: just below the first midpoint 2^-10, either sign
        c = torch.arange(K)
        below = 2.0 ** -10 * (1 - 2.0 ** -8)
        row = torch.where(c % 2 == 1, -below, below) * torch.where(c % 4 < 2, 1.0, 0.5).double()
        row[K - 1] = -FMAX if salt % 2 else FMAX
        return _bf16_exact(row * 2.0 ** -3)
    raise KeyError(name)


def quant_calls(rows):
    """regime offsets of the calls one shape needs so that every regime meets it: row r of call c is REGIMES[(c + r) % n]"""
    return list(range(0, len(REGIMES), rows))


_QUANT = {}


def quant_case(rows, K, ld, call):
    """dict(x bf16 [rows][ld] with PAD_VALUE behind column K, names, q uint8 [rows][K], e int64 [rows]).  Shared: never modified."""
    key = (rows, K, ld, call)
    if key not in _QUANT:
        names = [REGIMES[(call + r) % len(REGIMES)] for r in range(rows)]
        x = torch.full((rows, ld), PAD_VALUE, dtype=torch.bfloat16)
        for r, name in enumerate(names):
            x[r, :K] = regime_row(name, K, call + r)
        q, e = quantize_rows(x[:, :K].contiguous())
        _QUANT[key] = dict(x=x, names=names, q=q, e=e)
    return _QUANT[key]


# ------------------------------------------------------------------------------------------------ the exact GEMM
GEMM_SHAPES = ((256, 256, 256, 256, 256), (512, 256, 512, 512, 512), (256, 512, 2048, 2048, 2048), (512, 512, 256, 272, 288),
               (768, 1280, 512, 512, 512))                     # M, N, K, lda, ldb
ONEHOT_SHAPE = (256, 256, 512)
PAD_BYTE = 0x7E                                                # 448 behind the K columns of an operand row (ld > K)
ONE = 0x38                                                     # 1.0
_INT_CODES = encode(torch.arange(-4, 5, dtype=F64))            # bytes of -4 .. 4


def row_exponents(rows, g):
    """int64 [rows] in [-8, 8]; rows r and r ^ 1, r and r + 32 never share one"""
    e = torch.zeros(rows, dtype=torch.int64)
    draw = torch.randint(-8, 9, (rows, 4), generator=g)
    for r in range(rows):
        bad = {int(e[r ^ 1])} if (r ^ 1) < r else set()
        if r >= 32:
            bad.add(int(e[r - 32]))
        e[r] = next(int(v) for v in list(draw[r]) + [-8, 0, 8] if int(v) not in bad)
    i = torch.arange(rows)
    assert bool((e != e[i ^ 1]).all()) and bool((e[32:] != e[:-32]).all()) and int(e.min()) >= -8 and int(e.max()) <= 8
    return e


def int_bytes(shape, g):
    """uint8 bytes of random non-zero integers -4 .. 4"""
    v = torch.randint(1, 5, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)
    return _INT_CODES[v + 4]


def _padded(b, ld):
    out = torch.full((b.shape[0], ld), PAD_BYTE, dtype=torch.uint8)
    out[:, :b.shape[1]] = b
    return out


_GEMM = {}


def gemm_case(M, N, K, lda=None, ldb=None, kind="random"):
    """dict(A8 [M][lda], B8 [N][ldb] uint8 with PAD_BYTE behind column K, sa [M], sb [N] int64 exponents, bias [N] / res [M][N]
    float32 integers times a power of two, want float64 [M][N] = gemm_exact).  kind: "random", "onehot_a", "onehot_b".
    Shared between tests: never modified."""
    lda, ldb = lda or K, ldb or K
    key = (M, N, K, lda, ldb, kind)
    if key in _GEMM:
        return _GEMM[key]
    g = torch.Generator().manual_seed(1000003 * ("random", "onehot_a", "onehot_b").index(kind) + 7 * M + 11 * N + 13 * K)

    def onehot(rows):
        b = torch.zeros(rows, K, dtype=torch.uint8)
        r = torch.arange(rows)
        b[r, (37 * r + 11) % K] = ONE
        return b

    def named(rows):
        n, k = torch.arange(rows)[:, None], torch.arange(K)[None, :]
        return _INT_CODES[(n + 3 * k) % 9]                      # value (n + 3 k) % 9 - 4

    if kind == "random":
        A8, B8 = int_bytes((M, K), g), int_bytes((N, K), g)
    elif kind == "onehot_a":
        A8, B8 = onehot(M), named(N)
    else:
        A8, B8 = named(M), onehot(N)
    sa, sb = row_exponents(M, g), row_exponents(N, g)
    want = gemm_exact(A8, sa, B8, sb)
    exact_condition(A8, sa, B8, sb)
    bias = (torch.randint(-2047, 2048, (N,), generator=g).double() * 2.0 ** -6).float()
    res = (torch.randint(-2047, 2048, (M, N), generator=g).double() * 2.0 ** -6).float()
    _GEMM[key] = dict(M=M, N=N, K=K, lda=lda, ldb=ldb, A8=_padded(A8, lda), B8=_padded(B8, ldb), sa=sa, sb=sb, bias=bias, res=res,
                      want=want)
    return _GEMM[key]


def gemm_exact(A8, sa, B8, sb):
    """float64 [M][N]: the integer sum of products of the decoded operands (in units of 2^-18: an e4m3 value is a multiple of
    2^-9) times 2^(sa + sb).  The products are summed as integers held in float64 (asserted to stay below 2^53: exact), so no
    rounding happens anywhere."""
    a, b = torch.ldexp(decode(A8), torch.tensor(9)), torch.ldexp(decode(B8), torch.tensor(9))
    assert torch.equal(a, a.round()) and torch.equal(b, b.round())
    assert float(a.abs().max()) * float(b.abs().max()) * a.shape[1] < 2.0 ** 53
    acc = (a @ b.t()).to(torch.int64)
    sh = (sa.long()[:, None] + sb.long()[None, :] - 18)
    return torch.ldexp(acc.double(), sh)


def exact_condition(A8, sa, B8, sb):
    """the premises of section 3, asserted: integer operands in [-4, 4], sum_k |a b| <= 16 K <= 2^15, exponents in [-8, 8]"""
    a, b = decode(A8), decode(B8)
    K = a.shape[1]
    assert torch.equal(a, a.round()) and torch.equal(b, b.round()) and float(a.abs().max()) <= 4 and float(b.abs().max()) <= 4
    mag = a.abs() @ b.abs().t()
    assert float(mag.max()) <= 16 * K <= 2 ** 15
    assert int(sa.min()) >= -8 and int(sa.max()) <= 8 and int(sb.min()) >= -8 and int(sb.max()) <= 8
    return float(mag.max())


def scale_dwords(e):
    """E8M0 dwords (int32) of int64 exponents"""
    return (e + 127).to(torch.int32)


def epilogue_ref(acc, bias=None, res=None, bf16_out=False):
    """(reference float64, bound float64) of acc (+ bias) (+ res) with acc exact: section 4"""
    ref = acc.clone()
    mag = acc.abs()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if res is not None:
        ref, mag = ref + res.double(), mag + res.double().abs()
    bound = 2 * U * mag if (bias is not None or res is not None) else torch.zeros_like(acc)
    if bf16_out:
        bound = bound + half_ulp_bf16(ref)
    return ref, bound


def half_ulp_bf16(x):
    """half a bf16 ulp at x (8 significant bits): |x| = m 2^ex, m in [0.5, 1) -> ulp 2^(ex - 8); 0 at 0"""
    m, ex = torch.frexp(x.abs())
    return torch.where(x == 0, torch.zeros_like(m), torch.ldexp(torch.ones_like(m), ex - 9))


def worst_ratio(out, ref, bound):
    """max |out - ref| / bound; 0 where both are 0, inf where the output is not finite or misses a zero bound"""
    out = out.detach().double().cpu()
    err = (out - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(out), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def bits_equal(got, want):
    """fp32 tensors equal bit for bit (a NaN that was never overwritten fails)"""
    return torch.equal(got.float().contiguous().view(torch.int32), want.float().contiguous().view(torch.int32))


# ---- planted faults: each returns the float64 result a kernel with that fault would give on the case
def _fault_scale_neighbour(c):
    i = torch.arange(c["M"])
    return gemm_exact(c["A8"][:, :c["K"]], c["sa"][i ^ 1], c["B8"][:, :c["K"]], c["sb"])


def _fault_b_kblocks(c):
    B = c["B8"][:, :c["K"]].clone()
    s = 64 * (c["K"] // 64 - 2)                                 # one 64-wide step, every row of B
    B[:, s:s + 32], B[:, s + 32:s + 64] = c["B8"][:, s + 32:s + 64], c["B8"][:, s:s + 32]
    return gemm_exact(c["A8"][:, :c["K"]], c["sa"], B, c["sb"])


def _fault_last_step(c):
    K = c["K"]
    out = c["want"].clone()
    r0, c0 = c["M"] - 64, c["N"] - 96                           # one 32 x 32 tile
    out[r0:r0 + 32, c0:c0 + 32] = gemm_exact(c["A8"][r0:r0 + 32, :K - 64], c["sa"][r0:r0 + 32], c["B8"][c0:c0 + 32, :K - 64],
                                             c["sb"][c0:c0 + 32])
    return out


def _fault_rows_32(c):
    out = c["want"].clone()
    m = c["M"] - 256 + 70                                       # inside the last 256-row tile
    out[[m, m + 32]] = c["want"][[m + 32, m]]
    return out


GEMM_FAULTS = {"scale-from-row-m^1": _fault_scale_neighbour, "b-k-blocks-of-a-step-swapped": _fault_b_kblocks,
               "last-64-step-dropped-in-one-tile": _fault_last_step, "a-rows-m-and-m+32-swapped": _fault_rows_32}


# ------------------------------------------------------------------------------------------------ quantised random operands
RANDOM_SHAPE = (256, 512, 2048)


def random_operands(M=RANDOM_SHAPE[0], N=RANDOM_SHAPE[1], K=RANDOM_SHAPE[2]):
    """bf16 A [M][K], B [N][K]: N(0,1) times per-row factors 2^-10 .. 2^10"""
    g = torch.Generator().manual_seed(M + N + K)
    fa = torch.exp2(torch.randint(-10, 11, (M, 1), generator=g).double() + torch.rand(M, 1, generator=g, dtype=F64))
    fb = torch.exp2(torch.randint(-10, 11, (N, 1), generator=g).double() + torch.rand(N, 1, generator=g, dtype=F64))
    return ((torch.randn(M, K, generator=g, dtype=F64) * fa).to(torch.bfloat16),
            (torch.randn(N, K, generator=g, dtype=F64) * fb).to(torch.bfloat16))


def dequant(q, e):
    return torch.ldexp(decode(q), e.long().unsqueeze(1).expand(-1, q.shape[1]))


def random_ref(qa, ea, qb, eb):
    """(float64 reference, bound) on the dequantised operands: section 4"""
    a, b = dequant(qa, ea), dequant(qb, eb)
    K = a.shape[1]
    return a @ b.t(), 2 * (K + 2) * U * (a.abs() @ b.abs().t())
