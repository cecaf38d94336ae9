"""GPU parity tests of the reference-precision (fp32) kernels through the C-ABI (include/smd_hip.h): smd_gemm_f32,
smd_layernorm_f32, smd_attention_f32, smd_noise_embed_f32, each against float64 on its own inputs.

Bounds: SURVEY section 8(c) "fp32 kernels <= 1e-5 (fwd)" rel-L2, and for the GEMM an elementwise bound from first principles:
a length-K fp32 dot product accumulated in any order has |error| <= (K + 1) u sum_k |a_k w_k| with u = 2^-24 (Higham, Accuracy
and Stability, eq. 3.5, gamma_n ~ n u); the bias add costs one more rounding, a residual add one more on the result.
"""
import math

import pytest
import torch

import ddpm_oracle as O

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ACT = {"none": 0, "gelu": 1, "swish": 2}


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def gemm(L, A, W, bias=None, act="none", res=None, row_mod=0, out=None):
    import smd_amd.lib as lib
    M, K = A.shape
    N = W.shape[1]
    out = torch.full((M, N), float("nan"), device=A.device) if out is None else out
    lib.check(L.smd_gemm_f32(P(A), A.stride(0), P(W), W.stride(0), M, N, K, P(bias), ACT[act], P(res),
                             0 if res is None else res.stride(0), row_mod, P(out), out.stride(0), st()), "smd_gemm_f32")
    return out


def ref_epilogue(z, act):
    if act == "gelu":
        return O.gelu(z)
    if act == "swish":
        return O.swish(z)
    return z


CASES = [  # M, K, N, epilogue
    (8192, 2048, 2048, "bias"), (8192, 2048, 2048, "residual"), (8192, 128, 2048, "gelu"), (8192, 2048, 128, "residual"),
    (8192, 2048, 510, "bias"), (4064, 512, 128, "swish"), (4064, 42, 128, "posenc"), (1000, 146, 128, "posenc"),
    (4, 512, 4096, "bias"), (5, 128, 512, "swish"), (160, 2048, 42, "bias"), (160, 2048, 146, "bias"),
]


@pytest.mark.parametrize("M,K,N,epi", CASES)
def test_gemm_f32_against_float64(L, dev, M, K, N, epi):
    g = torch.Generator(device=dev).manual_seed(M + 3 * K + 7 * N)
    A = torch.randn(M, K, generator=g, device=dev)
    W = torch.randn(K, N, generator=g, device=dev) / math.sqrt(K)
    b = 0.1 * torch.randn(N, generator=g, device=dev)
    res, row_mod, act = None, 0, "none"
    if epi == "residual":
        res = torch.randn(M, N, generator=g, device=dev)
    elif epi == "posenc":
        res, row_mod = torch.randn(32, N, generator=g, device=dev), 32
    elif epi in ACT:
        act = epi
    got = gemm(L, A, W, b, act, res, row_mod)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all())            # every element written (the buffer started as NaN)
    z = A.double() @ W.double() + b.double()
    want = ref_epilogue(z, act)
    if res is not None:
        want = want + (res.double() if row_mod == 0 else res.double().repeat((M + 31) // 32, 1)[:M])
    e = rel(got, want)
    err = (got.double() - want).abs()
    print(f"gemm_f32 {M}x{K}x{N} {epi}: rel-L2 {e:.3e}, max abs {float(err.max()):.3e}")
    assert e <= 1e-5
    if act == "none":
        mag = A.double().abs() @ W.double().abs() + b.double().abs()
        bound = (K + 2) * U * mag + 2 * U * want.abs()
        worst = float((err / bound).max())
        print(f"  worst error / first-principles bound: {worst:.3f}")
        assert worst <= 1.0


def test_gemm_f32_rows_do_not_depend_on_the_problem_and_calls_repeat_bitwise(L, dev):
    g = torch.Generator(device=dev).manual_seed(11)
    for K, N in ((2048, 2048), (2048, 128), (128, 384)):
        A = torch.randn(8192, K, generator=g, device=dev)
        W = torch.randn(K, N, generator=g, device=dev) / math.sqrt(K)
        b = torch.randn(N, generator=g, device=dev)
        big = gemm(L, A, W, b, "gelu")
        again = gemm(L, A, W, b, "gelu")
        small = gemm(L, A[4096:4352].contiguous(), W, b, "gelu")
        ragged = gemm(L, A[37:37 + 99], W, b, "gelu")              # unaligned row offset is still a 16-byte multiple; ragged M
        # the scalar loaders (operands that are only 4-byte aligned) give the bits of the 16-byte vector loaders
        Av, Wv = A[100:130, 4:K], W[4:K]                           # 16-byte aligned views: vector loads
        abuf, wbuf = torch.empty(30 * (K - 4) + 1, device=dev), torch.empty((K - 4) * N + 1, device=dev)
        Am, Wm = abuf[1:].view(30, K - 4), wbuf[1:].view(K - 4, N)
        Am.copy_(Av); Wm.copy_(Wv)
        assert Av.data_ptr() % 16 == 0 and Am.data_ptr() % 16 == 4 and Wm.data_ptr() % 16 == 4
        vec, odd = gemm(L, Av, Wv, b, "gelu"), gemm(L, Am, Wm, b, "gelu")
        torch.cuda.synchronize()
        assert torch.equal(big, again)
        assert torch.equal(small, big[4096:4352])
        assert torch.equal(ragged, big[37:37 + 99])
        assert torch.equal(odd, vec)


def test_gemm_f32_rejects_bad_arguments(L, dev):
    A = torch.zeros(64, 64, device=dev)
    W = torch.zeros(64, 64, device=dev)
    out = torch.zeros(64, 64, device=dev)
    ok = lambda **kw: dict(dict(A=P(A), lda=64, W=P(W), ldw=64, M=64, N=64, K=64, bias=None, act=0, res=None, ld_res=0, row_mod=0,
                                out=P(out), ld_out=64), **kw)
    call = lambda a: L.smd_gemm_f32(a["A"], a["lda"], a["W"], a["ldw"], a["M"], a["N"], a["K"], a["bias"], a["act"], a["res"],
                                    a["ld_res"], a["row_mod"], a["out"], a["ld_out"], st())
    assert call(ok()) == 0
    for bad in (dict(A=None), dict(W=None), dict(out=None), dict(M=-1), dict(N=0), dict(K=-5), dict(lda=63), dict(ldw=32),
                dict(ld_out=8), dict(res=P(out), ld_res=10), dict(act=7), dict(A=P(A) + 2), dict(bias=P(out) + 1),
                dict(res=P(out), ld_res=64, row_mod=-1)):
        assert call(ok(**bad)) < 0, bad
        assert L.smd_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows,D,film", [(8192, 128, None), (4064, 2048, "sample"), (8192, 2048, "table"), (96, 1024, "sample"),
                                         (33, 130, None), (7, 2048, "dense")])
def test_layernorm_f32(L, dev, rows, D, film):
    import smd_amd.lib as lib
    g = torch.Generator(device=dev).manual_seed(rows + D)
    x = 0.3 + 1.7 * torch.randn(rows, D, generator=g, device=dev)
    p = {"n.scale": 1 + 0.1 * torch.randn(D, generator=g, device=dev), "n.bias": 0.1 * torch.randn(D, generator=g, device=dev)}
    rps = 1 if film == "dense" else 32
    nfilm = 1000 if film == "table" else (rows + rps - 1) // rps
    ss = torch.randn(nfilm, 2 * D, generator=g, device=dev) if film else None
    t_ptr = torch.tensor([417], dtype=torch.int32, device=dev) if film == "table" else None
    out = torch.full((rows, D), float("nan"), device=dev)
    lib.check(L.smd_layernorm_f32(P(x), rows, D, P(p["n.scale"]), P(p["n.bias"]), P(ss), None if ss is None else P(ss) + 4 * D,
                                  2 * D, rps, P(t_ptr), 1000, 1 if film else 0, P(out), st()), "smd_layernorm_f32")
    torch.cuda.synchronize()
    want = O.layer_norm(x.double(), {k: v.double() for k, v in p.items()}, "n")
    if film:
        row = torch.full((rows,), 417, device=dev) if film == "table" else torch.arange(rows, device=dev) // rps
        want = O.swish(ss.double()[row, :D] * want + ss.double()[row, D:])
    e = rel(out, want)
    print(f"layernorm_f32 rows {rows} D {D} film {film}: rel-L2 {e:.3e}")
    assert bool(torch.isfinite(out).all()) and e <= 1e-5


@pytest.mark.parametrize("H", [4, 8, 16])
def test_attention_f32(L, dev, H):
    import smd_amd.lib as lib
    B, S, E = 37, 32, 128
    d = E // H
    g = torch.Generator(device=dev).manual_seed(H)
    qkv = 1.5 * torch.randn(B * S, 3 * E, generator=g, device=dev)
    out = torch.full((B * S, E), float("nan"), device=dev)
    lib.check(L.smd_attention_f32(P(qkv), P(out), B, S, E, H, st()), "smd_attention_f32")
    torch.cuda.synchronize()
    q, k, v = qkv.double().view(B, S, 3 * E).split(E, dim=-1)
    q = q.reshape(B, S, H, d) / math.sqrt(d)
    w = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k.reshape(B, S, H, d)), dim=-1)       # oracle self_attention's core
    want = torch.einsum("bhqk,bkhd->bqhd", w, v.reshape(B, S, H, d)).reshape(B * S, E)
    e = rel(out, want)
    print(f"attention_f32 H {H} (d {d}): rel-L2 {e:.3e}")
    assert e <= 1e-5
    assert L.smd_attention_f32(P(qkv), P(out), B, 16, E, H, st()) < 0 and L.smd_attention_f32(P(qkv), P(out), B, S, E, 2, st()) < 0


def test_noise_embed_f32(L, dev):
    """NoiseEncoding at noise levels up to 1: arguments (5000 s) f_i up to 5000 rad.  Tolerance, from the fp32 format: write
    ulp_a for the ulp of the largest argument 5000 s (4.9e-4 at s = 1).  Against the float64 oracle ON THE SAME fp32 noise level the
    fp32 ARGUMENT differs by: the product 5000 s (<= 0.5 ulp_a), the product with f_i (<= 0.5 ulp_a), f_i = exp(-i c) whose
    exponent carries two roundings (c and i c: relative 2^-23 x with x = i c, times f = e^-x: x e^-x <= 0.37, i.e. <= 0.74 ulp_a)
    and expf's own ulp (<= 1 ulp_a): 2.74 ulp_a in the worst case, about 1.3e-3 rad at s = 1.  sin / cos have slope <= 1, and
    sincosf with full range reduction adds ~1e-7.  The fast hardware sine (no range reduction, error growing with the argument)
    would miss this at 5000 rad; measured values are printed."""
    import smd_amd.lib as lib
    s = torch.tensor([1.0, 0.9999995, 0.6, 0.0814, 0.3, 1e-3], device=dev)
    n, F = s.numel(), 128
    out = torch.full((n, F), float("nan"), device=dev)
    lib.check(L.smd_noise_embed_f32(P(s), n, F, P(out), F, st()), "smd_noise_embed_f32")
    torch.cuda.synchronize()
    sc = s.double().cpu()
    want = O.noise_encoding(sc[:, None], F)
    err = (out.double().cpu() - want).abs().max(dim=1).values
    ulp_a = 2.0 ** (torch.floor(torch.log2(5000.0 * sc)) - 23)
    tol = 2.74 * ulp_a + 1e-6
    print("noise_embed_f32: level: max abs error / tolerance  " + "  ".join(f"{float(a):.4g}: {float(e):.2e} / {float(t):.2e}" for a, e, t in zip(sc, err, tol)))
    assert bool((err <= tol).all())
