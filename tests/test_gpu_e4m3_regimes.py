"""The e4m3 row quantiser and the scaled-MFMA GEMM through the C ABI, element by element against tests/_e4m3_ref.py
(tests/test_e4m3_ref_host.py checks that reference, and that its cases see every planted fault, without a GPU).

Quantiser (smd_quantize_rows_e4m3): every byte by same_value (equal, or both a zero of either sign), every scale dword exactly,
nothing written behind rows * K bytes / rows dwords, the output pitch K with finite garbage in the input's padding columns, at
six shapes (one lane, a ragged second pass, exactly one pass, four passes, ld > K, a ragged last workgroup), each meeting all 19
row regimes of _e4m3_ref.REGIMES; two calls give the same bytes.

GEMM (smd_gemm_e4m3_nt, smd_gemm_e4m3_nt_lab): operands built as bytes that decode to small integers with row exponents that
differ between the rows a wrong index would confuse -- every partial sum is exact in fp32, so the fp32 output without an epilogue
must EQUAL the integer result bit for bit; with bias / residual / bf16 output the bound is the two fp32 additions and the bf16
rounding (section 4 of _e4m3_ref).  One case through the quantiser with row factors 2^-10 .. 2^10 is judged per element against
float64 on the dequantised operands under the derived bound 2 (K + 2) 2^-24 sum |a b|.  The launcher's refusals launch nothing.

Observed on MI355X (gfx950): 0 sign-of-zero differences in 143 672 quantiser bytes -- the hardware conversion keeps the sign of a
negative value it rounds to zero (0x80), as IEEE rounding does, so the bytes equal the reference outright; the count is printed,
not asserted.  Quantised random case: worst |err| / bound 0.0108 (rel-L2 1.25e-05).  Exact cases: the fp32 output without an
epilogue is bitwise equal at every shape; bias + fp32 residual reaches 1.000 of its bound (a correctly rounded sum just above a
power of two is at 1 - 2^-23 of 2^-23 |result|: the format, not the kernel)."""
import ctypes

import pytest
import torch

import _e4m3_ref as R

pytestmark = pytest.mark.gpu

DEAD = 0xDEADBEEF - (1 << 32)                                 # the scale buffer's fill as an int32
P = lambda t: None if t is None else t.data_ptr()
st = lambda: torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


def ck(rc, what=""):
    import smd_amd.lib as lib
    lib.check(rc, what)


def quantize(L, dev, x, K, tail=64):
    """x bf16 [rows][ld] on the host -> (bytes [rows * K + tail] over a 0xA5 fill, dwords [rows + 8] over 0xDEADBEEF), on the host"""
    rows, ld = x.shape
    xd = x.to(dev)
    q = torch.full((rows * K + tail,), 0xA5, dtype=torch.uint8, device=dev)
    s = torch.full((rows + 8,), DEAD, dtype=torch.int32, device=dev)
    ck(L.smd_quantize_rows_e4m3(P(xd), ld, rows, K, P(q), P(s), st()), "quantize_rows_e4m3")
    torch.cuda.synchronize()
    return q.cpu(), s.cpu()


@pytest.mark.parametrize("rows,K,ld", R.QUANT_SHAPES)
def test_quantiser_every_byte_and_exponent(L, dev, rows, K, ld):
    flips = total = 0
    for call in R.quant_calls(rows):
        c = R.quant_case(rows, K, ld, call)
        q, s = quantize(L, dev, c["x"], K)
        got = q[:rows * K].view(rows, K)
        bad = ~R.same_value(got, c["q"])
        where = [(c["names"][r], r, int(torch.nonzero(bad[r])[0]), int(got[r][bad[r]][0]), int(c["q"][r][bad[r]][0]))
                 for r in torch.nonzero(bad.any(1)).flatten().tolist()]
        assert not where, f"call {call}: (regime, row, first column, got, want) {where}"
        assert torch.equal(s[:rows].long(), c["e"] + 127), (call, c["names"], s[:rows].tolist(), (c["e"] + 127).tolist())
        assert bool((q[rows * K:] == 0xA5).all()) and bool((s[rows:] == DEAD).all())       # nothing behind the outputs
        flips += R.zero_sign_diffs(got, c["q"])
        total += rows * K
        q2, s2 = quantize(L, dev, c["x"], K)
        assert torch.equal(q2, q) and torch.equal(s2, s)                                    # two calls: the same bytes
    print(f"quantize_rows_e4m3 rows={rows} K={K} ld={ld}: {total} bytes equal the reference, {flips} of them a zero of the other sign "
          f"(0x00 vs 0x80); two calls bitwise equal")


def gemm(L, dev, c, bias=None, res=None, f32=False, bf16=False, over=None):
    """smd_gemm_e4m3_nt on a case of _e4m3_ref.gemm_case; outputs start as NaN.  over: arguments replaced for the refusals"""
    o = dict(M=c["M"], N=c["N"], K=c["K"], lda=c["lda"], ldb=c["ldb"], sa=True, sb=True)
    o.update(over or {})
    M, N = c["M"], c["N"]
    d = dict(A=c["A8"].to(dev), B=c["B8"].to(dev), sa=R.scale_dwords(c["sa"]).to(dev), sb=R.scale_dwords(c["sb"]).to(dev),
             bias=None if bias is None else bias.to(dev), res=None if res is None else res.to(dev),
             of=torch.full((M, N), float("nan"), device=dev) if f32 else None,
             ob=torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev) if bf16 else None)
    rc = L.smd_gemm_e4m3_nt(P(d["A"]), o["lda"], P(d["sa"]) if o["sa"] else None, P(d["B"]), o["ldb"], P(d["sb"]) if o["sb"] else None,
                            o["M"], o["N"], o["K"], P(d["bias"]), P(d["res"]), N, P(d["of"]), N, P(d["ob"]), N, st())
    torch.cuda.synchronize()
    return rc, d["of"], d["ob"]


def _first_bad(got, want):
    bad = torch.nonzero(got.double().cpu() != want)
    return [(int(m), int(n), float(got[m, n]), float(want[m, n])) for m, n in bad[:4].tolist()], len(bad)


def _exact_forms(L, dev, c, tag):
    # no epilogue, fp32: bit for bit
    rc, of, _ = gemm(L, dev, c, f32=True)
    ck(rc, tag)
    assert R.bits_equal(of.cpu(), c["want"].float()), f"{tag}: first (m, n, got, want), count: {_first_bad(of, c['want'])}"
    # bias + fp32 residual -> fp32 and bf16 at once
    rc, of, ob = gemm(L, dev, c, bias=c["bias"], res=c["res"], f32=True, bf16=True)
    ck(rc, tag)
    ref, bound = R.epilogue_ref(c["want"], c["bias"], c["res"])
    r_f = R.worst_ratio(of, ref, bound)
    ref, bound = R.epilogue_ref(c["want"], c["bias"], c["res"], bf16_out=True)
    r_b = R.worst_ratio(ob, ref, bound)
    # bias -> bf16 alone (fc1 of a DenseResBlock: the packed epilogue)
    rc, _, ob = gemm(L, dev, c, bias=c["bias"], bf16=True)
    ck(rc, tag)
    ref, bound = R.epilogue_ref(c["want"], c["bias"], bf16_out=True)
    r_p = R.worst_ratio(ob, ref, bound)
    print(f"{tag}: fp32 without epilogue bitwise equal; |err| / bound: bias + residual fp32 {r_f:.3f}, its bf16 copy {r_b:.3f}, "
          f"bias -> bf16 {r_p:.3f}")
    assert r_f <= 1.0 and r_b <= 1.0 and r_p <= 1.0


@pytest.mark.parametrize("M,N,K,lda,ldb", R.GEMM_SHAPES)
def test_gemm_exact_operands(L, dev, M, N, K, lda, ldb):
    _exact_forms(L, dev, R.gemm_case(M, N, K, lda, ldb), f"gemm_e4m3_nt exact {M}x{N}x{K} lda={lda} ldb={ldb}")


@pytest.mark.parametrize("kind", ["onehot_a", "onehot_b"])
def test_gemm_one_hot_names_the_k_index(L, dev, kind):
    M, N, K = R.ONEHOT_SHAPE
    _exact_forms(L, dev, R.gemm_case(M, N, K, kind=kind), f"gemm_e4m3_nt {kind} {M}x{N}x{K}")


def test_gemm_quantised_random_per_element(L, dev):
    M, N, K = R.RANDOM_SHAPE
    a, b = R.random_operands()
    (qa, sa), (qb, sb) = quantize(L, dev, a, K, tail=0), quantize(L, dev, b, K, tail=0)
    qa, qb, ea, eb = qa.view(M, K), qb.view(N, K), sa[:M].long() - 127, sb[:N].long() - 127
    for q, e, x in ((qa, ea, a), (qb, eb, b)):
        wq, we = R.quantize_rows(x)
        assert bool(R.same_value(q, wq).all()) and torch.equal(e, we)
    c = dict(M=M, N=N, K=K, lda=K, ldb=K, A8=qa, B8=qb, sa=ea, sb=eb)
    rc, of, _ = gemm(L, dev, c, f32=True)
    ck(rc, "quantised random")
    ref, bound = R.random_ref(qa, ea, qb, eb)
    ratio = R.worst_ratio(of, ref, bound)
    print(f"gemm_e4m3_nt quantised random {M}x{N}x{K}, row factors 2^-10 .. 2^10: worst |err| / bound {ratio:.4f} "
          f"(bound 2 (K + 2) 2^-24 sum |a b|), rel-L2 {float((of.double().cpu() - ref).norm() / ref.norm()):.2e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("what,over", [("M = 255", dict(M=255)), ("N = 128", dict(N=128)), ("K = 192", dict(K=192)),
                                       ("lda = K + 8", dict(lda=264)), ("null scale_a", dict(sa=False)), ("null scale_b", dict(sb=False))])
def test_gemm_refusals_launch_nothing(L, dev, what, over):
    c = R.gemm_case(256, 256, 256, 272, 272)
    rc, of, ob = gemm(L, dev, c, bias=c["bias"], f32=True, bf16=True, over=over)
    assert rc < 0 and L.smd_last_error(), what
    with pytest.raises(ValueError):
        ck(rc, what)
    assert bool(torch.isnan(of).all()) and bool(torch.isnan(ob).all())


def test_gemm_without_an_output_is_refused(L, dev):
    c = R.gemm_case(256, 256, 256, 272, 272)
    rc, _, _ = gemm(L, dev, c, bias=c["bias"])
    assert rc < 0 and b"no output" in L.smd_last_error()


def test_engine_epilogue_forms(L, dev):
    """the forms only the engine reaches: no bias -> bf16 (every dgrad: the packed epilogue), and bias + bf16 residual -> bf16
    (the second Dense of a DenseResBlock on the bf16 trunk), through smd_gemm_e4m3_nt_lab on the exact operands"""
    import smd_amd.lib as lib
    M = N = K = 256
    c = R.gemm_case(M, N, K)
    A, B = c["A8"].to(dev), c["B8"].to(dev)
    sa, sb = R.scale_dwords(c["sa"]).to(dev), R.scale_dwords(c["sb"]).to(dev)
    res = c["res"].to(torch.bfloat16)                          # the residual IS its bf16 rounding: read exactly by the kernel
    bias, resb = c["bias"].to(dev), res.to(dev)
    for tag, with_epi in (("no bias -> bf16", False), ("bias + bf16 residual -> bf16", True)):
        out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
        e = lib.GemmEpilogue(alpha=1.0, out_bf16=P(out), ld_outb=N)
        if with_epi:
            e.bias, e.res_bf16, e.ld_resb = P(bias), P(resb), N
        ck(L.smd_gemm_e4m3_nt_lab(P(A), K, P(sa), P(B), K, P(sb), M, N, K, ctypes.byref(e), st()), tag)
        torch.cuda.synchronize()
        ref, bound = R.epilogue_ref(c["want"], c["bias"] if with_epi else None, res.float() if with_epi else None, bf16_out=True)
        ratio = R.worst_ratio(out, ref, bound)
        print(f"gemm_e4m3_nt_lab {tag}: worst |err| / bound {ratio:.3f}")
        assert ratio <= 1.0
        if not with_epi:                                        # one RNE rounding of an exact accumulator
            assert torch.equal(out.cpu(), c["want"].to(torch.bfloat16))
    e = lib.GemmEpilogue(alpha=1.0)
    assert L.smd_gemm_e4m3_nt_lab(P(A), K, P(sa), P(B), K, P(sb), M, N, K, ctypes.byref(e), st()) < 0      # no output
    e = lib.GemmEpilogue(alpha=2.0, out_bf16=P(out), ld_outb=N)
    assert L.smd_gemm_e4m3_nt_lab(P(A), K, P(sa), P(B), K, P(sb), M, N, K, ctypes.byref(e), st()) < 0      # alpha != 1
