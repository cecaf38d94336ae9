"""Footprint tests of the C-ABI (include/smd_hip.h): every kernel writes only its documented outputs and ignores padding.

Each case puts the outputs and workspaces of one entry point into guarded arenas (tests/_footprint.py: red zones in front
and behind, the columns between the logical width and the leading dimension, all filled with a NaN sentinel) and its
strided inputs into arenas whose padding is poisoned the same way, runs the call under two different sentinels, and asserts
  1. no sentinel byte around an output changed,              4. the outputs are finite,
  2. every logical output element was written,               5. they meet the fp64 reference of the entry point's own
  3. the two runs agree bitwise (nothing read the poison;       parity test at that test's tolerance,
     an unwritten element would differ: it IS the poison),   6. every input (padding included) is bitwise unchanged.
Every byte a kernel is allowed to touch is allocated and owned by the test: a stray store fails an assertion.

Entry point -> case (every entry of include/smd_hip.h that enqueues a kernel):
  smd_gemm_bf16_nt                               test_gemm_bf16_nt, test_gemm_bf16_nt_256_forced, ..._refuses_a_leading_dimension...
  smd_gemm_bf16_tn, smd_gemm_tn_slab_elems       test_gemm_bf16_tn, test_gemm_bf16_tn_256_forced
  smd_wgrad_lab_launch (smd_hip_lab.h)           test_wgrad_lab_launch_grouped
  smd_quantize_rows_e4m3, smd_gemm_e4m3_nt       test_quantize_rows_e4m3_ragged, test_gemm_e4m3_nt
  smd_layernorm_fwd_e4m3                         test_layernorm_fwd_e4m3
  smd_layernorm_fwd_lab (smd_hip_lab.h)          test_layernorm_fwd_lab_table_row
  smd_gemm_f32, smd_layernorm_f32                test_gemm_f32, test_layernorm_f32
  smd_attention_f32, smd_noise_embed_f32         test_attention_f32, test_noise_embed_f32_and_bf16
  smd_noise_embed                                test_noise_embed_f32_and_bf16
  smd_mlp_block_fwd / _fwd_hs / _bwd_hs          test_mlp_block_fwd, test_mlp_block_fwd_hs_..., test_mlp_block_bwd_hs_...
  smd_attn_block_fwd / _fwd_ex                   test_attn_block_fwd_and_fwd_ex
  smd_attn_block_bwd / _bwd_ln                   test_attn_block_bwd_and_bwd_ln
  smd_ln128_parts, smd_ln128_bwd_parts           test_ln128_parts_and_bwd_parts_with_poisoned_gaps
  smd_layernorm_fwd / _fwd_ex / _bwd / _bwd_ex / _bwd_film      test_layernorm_fwd_and_bwd_forms
  smd_attention_fwd, smd_attention_bwd           test_attention_fwd_bwd
  smd_cast_pad_bf16                              test_cast_pad_bf16_writes_zero_padding_and_nothing_behind_the_last_row
  smd_q_sample, smd_mse_fwd_bwd                  test_q_sample_and_mse_leave_the_pad_columns_alone
  smd_rng_normal                                 test_rng_normal_ragged_row_length
  smd_threefry_bits / _uniform / _normal / _randint             test_threefry_windows
  smd_adam_clip_ema                              test_adam_clip_ema
  smd_set_timestep                               test_set_timestep_writes_one_word
  smd_ddpm_reverse_step                          test_ddpm_reverse_step_touches_one_slot_and_one_metrics_row
  smd_langevin_step                              test_langevin_step_direct, test_langevin_step_table_mode
  smd_pair_kernel_sums, smd_moments              test_pair_kernel_sums, test_moments
  smd_knn_radii, smd_ball_cover                  test_knn_radii_and_ball_cover
  smd_kmeans_assign, smd_kmeans_update           test_kmeans_assign, test_kmeans_update_counts_a_label_outside_the_range_nowhere
  smd_engine_refresh_weights / _forward / _forward_level / _loss_backward / _forward_train / _backward_from / _optimizer_step /
  _prepare_sampler / _init_state / _load_state / _sample_step / _sample_step_part            test_engine_stays_inside_its_buffers
Left out: the entries that enqueue no kernel (create / destroy / queries / set_option / bind_* / set_used_alphas, and
smd_engine_wait_grad_bucket / _join_update, which only make a stream wait).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import _cluster_metrics_ref as RC
import _footprint as F
import _metrics_ref as RM
import _nn_metrics_ref as RN
import ddpm_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def ck(rc, what=""):
    import smd_amd.lib as lib
    lib.check(rc, what)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bf(x):
    return x.to(torch.bfloat16)


def bits(t):
    return t.detach().contiguous().view(torch.uint8)


def is_poison(t, fill):
    """every 32-bit word of ``t`` still holds the sentinel: the kernel left it alone"""
    word = torch.from_numpy(np.array([fill | fill << 16], np.uint32).view(np.int32))
    return bool((t.contiguous().view(torch.int32) == word).all())


class Run:
    """The arenas of one call under one sentinel."""

    def __init__(self, dev, fill):
        self.dev, self.fill = dev, fill
        self.ins, self.outs = [], {}

    def inp(self, t, ld=None, **kw):
        """guarded copy of a CPU tensor; checked bitwise (padding included) after the call"""
        view, h = F.guarded_like(t, self.dev, ld=ld, fill=self.fill, **kw)
        self.ins.append((h, h.snapshot()))
        return view

    def out(self, name, shape, dtype=torch.float32, ld=None, init=None, **kw):
        """guarded output: starts as the sentinel (NaN for floats) unless ``init`` (a CPU tensor: an in-place operand)"""
        view, h = F.guarded(shape, dtype, self.dev, ld=ld, fill=self.fill, **kw)
        if init is not None:
            view.copy_(init)
        self.outs[name] = h
        return view

    def finish(self):
        torch.cuda.synchronize()
        for name, h in self.outs.items():
            h.assert_untouched(name)
        for i, (h, snap) in enumerate(self.ins):
            h.assert_same(snap, f"input {i}")
        return {name: h.logical().clone() for name, h in self.outs.items()}


def both(dev, body, unwritten=()):
    """body(run) under the two sentinels -> the outputs of the first run (CPU tensors), after checks 1, 2, 3, 4 and 6.
    ``unwritten``: outputs the contract leaves (partly) alone; their bits legitimately differ between the sentinels."""
    res = []
    for fill in F.PATTERNS:
        r = Run(dev, fill)
        body(r)
        res.append(r.finish())
    for name in res[0]:
        if name in unwritten:
            continue
        a, b = res[0][name], res[1][name]
        assert torch.equal(bits(a), bits(b)), f"{name}: differs between the two poison patterns (padding was read, or an element was not written)"
        if a.is_floating_point():
            assert bool(torch.isfinite(a.float()).all()), f"{name}: not finite"
    return {k: v.cpu() for k, v in res[0].items()}, {k: v.cpu() for k, v in res[1].items()}


# ================================================================================================ bf16 NT GEMM
_NT = {}


def nt_case(M, N, K):
    if (M, N, K) not in _NT:
        g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
        A, Bt = bf(torch.randn(M, K, generator=g)), bf(torch.randn(N, K, generator=g) * 0.5)
        bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        z = A.double() @ Bt.double().t() + bias.double()
        _NT[(M, N, K)] = (A, Bt, bias, res, z)
    return _NT[(M, N, K)]


@pytest.mark.parametrize("pad_out,pad_outb", [(3, 1), (4, 8)])
@pytest.mark.parametrize("M,N,K", [(300, 42, 192), (96, 200, 1024), (64, 512, 2048), (2080, 510, 2048)],
                         ids=["tile128-ragged", "rows32", "rows64-2kgroups", "out_proj-ragged"])
def test_gemm_bf16_nt(L, dev, M, N, K, pad_out, pad_outb):
    """lda = K + 8, ldb = K + 16, ld_res = N + 5, ld_out = N + 3 / N + 4, ld_outb = N + 1 / N + 8: the scalar tail and the
    quad epilogue next to poisoned gaps; bias -> fp32 + bf16, bias + residual -> fp32, and the in-place residual stream."""
    A, Bt, bias, res, z = nt_case(M, N, K)
    ldo, ldb16 = N + pad_out, N + pad_outb

    def body(r):
        a, b = r.inp(A, ld=K + 8, gemm=True), r.inp(Bt, ld=K + 16, gemm=True)
        bd, rd = r.inp(bias), r.inp(res, ld=N + 5, gemm=True)
        o = r.out("out", (M, N), ld=ldo, gemm=True)
        ob = r.out("outb", (M, N), torch.bfloat16, ld=ldb16, gemm=True)
        ck(L.smd_gemm_bf16_nt(P(a), K + 8, P(b), K + 16, M, N, K, P(bd), 0, None, 0, P(o), ldo, P(ob), ldb16, st()))
        o2 = r.out("out_res", (M, N), ld=ldo, gemm=True)
        ck(L.smd_gemm_bf16_nt(P(a), K + 8, P(b), K + 16, M, N, K, P(bd), 0, P(rd), N + 5, P(o2), ldo, None, 0, st()))
        o3 = r.out("inplace", (M, N), ld=ldo, gemm=True, init=res)
        ck(L.smd_gemm_bf16_nt(P(a), K + 8, P(b), K + 16, M, N, K, P(bd), 0, P(o3), ldo, P(o3), ldo, None, 0, st()))

    got, _ = both(dev, body)
    e, eb = rel(got["out"], z), rel(got["outb"].float(), z)
    e2, e3 = rel(got["out_res"], z + res.double()), rel(got["inplace"], z + res.double())
    print(f"gemm_nt {M}x{N}x{K} ld_out N+{pad_out} ld_outb N+{pad_outb}: fp32 {e:.2e} bf16 {eb:.2e} +res {e2:.2e} in place {e3:.2e}")
    assert e < 2e-5 and eb < 4e-3            # test_gemm_nt_plain
    assert e2 < 2e-5 and e3 < 2e-5           # test_gemm_nt_epilogues (in-place residual stream)
    assert torch.equal(got["out_res"], got["inplace"])


@pytest.mark.parametrize("pk", [0, 1])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 768, 256)])
def test_gemm_bf16_nt_256_forced(L, dev, M, N, K, variant, pk):
    """The 256x256 kernel (forced) with every leading dimension padded by what its 8-column epilogue accepts (N + 8): the fp32
    staged, the bias + gelu + residual and the packed-bf16 (bf16 output only) epilogues."""
    import smd_amd.lib as lib
    A, Bt, bias, res, z = nt_case(M, N, K)
    ld = N + 8

    def body(r):
        a, b = r.inp(A, ld=K + 8, gemm=True), r.inp(Bt, ld=K + 16, gemm=True)
        bd, rd = r.inp(bias), r.inp(res, ld=ld, gemm=True)
        o, ob = r.out("out", (M, N), ld=ld, gemm=True), r.out("outb", (M, N), torch.bfloat16, ld=ld, gemm=True)
        ck(L.smd_gemm_bf16_nt(P(a), K + 8, P(b), K + 16, M, N, K, P(bd), 0, None, 0, P(o), ld, P(ob), ld, st()))
        o2 = r.out("gelu_res", (M, N), ld=ld, gemm=True)
        ck(L.smd_gemm_bf16_nt(P(a), K + 8, P(b), K + 16, M, N, K, P(bd), 1, P(rd), ld, P(o2), ld, None, 0, st()))
        o3 = r.out("bf16_only", (M, N), torch.bfloat16, ld=ld, gemm=True)
        ck(L.smd_gemm_bf16_nt(P(a), K + 8, P(b), K + 16, M, N, K, P(bd), 0, None, 0, None, 0, P(o3), ld, st()))

    lib.check(L.smd_set_tuning(b"gemm_nt256", 2))
    lib.check(L.smd_set_tuning(b"gemm_nt256_variant", variant))
    lib.check(L.smd_set_tuning(b"gemm_nt256_pk", pk))
    try:
        got, _ = both(dev, body)
    finally:
        lib.check(L.smd_set_tuning(b"gemm_nt256", 1))
        lib.check(L.smd_set_tuning(b"gemm_nt256_variant", 0))
        lib.check(L.smd_set_tuning(b"gemm_nt256_pk", 1))
    e, eb, e2 = rel(got["out"], z), rel(got["outb"].float(), z), rel(got["gelu_res"], O.gelu(z) + res.double())
    assert e < 2e-5 and eb < 4e-3 and e2 < 1e-4                   # test_gemm_nt256_forced
    assert rel(got["bf16_only"].float(), z) < 4e-3                # test_gemm_nt256_packed_bf16_epilogue_is_bitwise_the_staged_one
    assert torch.equal(got["bf16_only"], got["outb"])


def test_gemm_bf16_nt_refuses_a_leading_dimension_that_is_no_multiple_of_8(L, dev):
    """lda / ldb must be multiples of 8 (16-byte rows for the LDS DMA): refused, nothing written"""
    A, Bt, bias, res, z = nt_case(300, 42, 192)
    for lda, ldb in ((192 + 4, 192), (192, 192 + 2)):
        r = Run(dev, F.PATTERNS[0])
        a, b = r.inp(A, ld=lda, gemm=True), r.inp(Bt, ld=ldb, gemm=True)
        o = r.out("out", (300, 42), ld=45, gemm=True)
        assert L.smd_gemm_bf16_nt(P(a), lda, P(b), ldb, 300, 42, 192, None, 0, None, 0, P(o), 45, None, 0, st()) < 0
        assert bool(torch.isnan(r.finish()["out"]).all())


# ================================================================================================ weight-gradient GEMM
_TN = {}


def tn_case(M, Kd, N):
    if (M, Kd, N) not in _TN:
        g = torch.Generator().manual_seed(M + Kd + N)
        X, Y = bf(torch.randn(M, Kd, generator=g)), bf(torch.randn(M, N, generator=g) * 0.1 + 0.01)
        _TN[(M, Kd, N)] = (X, Y, X.double().t() @ Y.double(), Y.double().sum(0))
    return _TN[(M, Kd, N)]


def run_tn(L, dev, M, Kd, N, ldx, ldy, ldo, tr_path):
    X, Y, ref, refb = tn_case(M, Kd, N)
    slab_elems = int(L.smd_gemm_tn_slab_elems())
    scratch_elems = (Kd + N) * ((M + 63) // 64 * 64) if not tr_path else 128

    def body(r):
        # rows M .. roundup(M, 256) are the back red zone (poison), the columns Kd .. ldx / N .. ldy the poisoned gaps
        x, y = r.inp(X, ld=ldx, gemm=True), r.inp(Y, ld=ldy, gemm=True)
        zero = r.inp(torch.zeros(128, dtype=torch.bfloat16))
        dw, db = r.out("dW", (Kd, N), ld=ldo, gemm=True), r.out("db", (N,))
        slab = r.out("slab", (slab_elems,), gemm=True)
        scratch = r.out("scratch", (scratch_elems,), torch.bfloat16, gemm=True)
        ck(L.smd_gemm_bf16_tn(P(x), ldx, P(y), ldy, M, Kd, N, P(dw), ldo, P(db), P(zero), P(slab), slab_elems,
                              P(scratch), scratch_elems, tr_path, st()))

    got, _ = both(dev, body, unwritten=("slab", "scratch"))
    e, eb = rel(got["dW"], ref), rel(got["db"], refb)
    print(f"gemm_tn tr={tr_path} M={M} Kd={Kd} N={N} ldx={ldx} ldy={ldy} ldo={ldo}: dW {e:.2e} db {eb:.2e}")
    assert e < 3e-5 and eb < 3e-5            # test_gemm_tn / test_gemm_tn256


@pytest.mark.parametrize("tr_path", [1, 0])
@pytest.mark.parametrize("M,Kd,N,ldx,ldy", [(1000, 42, 128, 64, 128), (300, 128, 146, 128, 192)])
def test_gemm_bf16_tn(L, dev, M, Kd, N, ldx, ldy, tr_path):
    run_tn(L, dev, M, Kd, N, ldx, ldy, N, tr_path)


def test_gemm_bf16_tn_256_forced(L, dev):
    import smd_amd.lib as lib
    lib.check(L.smd_set_tuning(b"gemm_tn256", 2))
    try:
        run_tn(L, dev, 1000, 512, 256, 512, 320, 256 + 4, 1)
    finally:
        lib.check(L.smd_set_tuning(b"gemm_tn256", 1))


def test_wgrad_lab_launch_grouped(L, dev):
    """A grouped launch of the 128-wide kernel (include/smd_hip_lab.h) writes its gradients, its bias rows and the first
    nsplit * sum(stride) floats of the slab, nothing else: in_proj of C = 42 (Kd = 42, ldx = 64), out_proj of C = 42 (N = 42,
    ldy = 64: the rows of dW are 42 floats, nothing behind the last one) and a 128 x 128 peer without a bias, over 1000 rows,
    with a slab of exactly three splits' partials (the planner asks for more: the capacity binds)."""
    import smd_amd.lib as lib
    import _wgrad_ref as WR
    Mrows, nsplit = 1000, 3
    specs = [(42, 128, 64, 128, True), (256, 42, 256, 64, True), (128, 128, 128, 128, False)]
    data = [tn_case(Mrows, Kd, N) for Kd, N, *_ in specs]
    slab_elems = nsplit * sum((Kd * N + N + 3) // 4 * 4 for Kd, N, *_ in specs)
    plans = []

    def body(r):
        arr = (lib.WgradProblem * len(specs))()
        for i, (a, (Kd, N, ldx, ldy, wb), (X, Y, _, _)) in enumerate(zip(arr, specs, data)):
            x, y = r.inp(X, ld=ldx, gemm=True), r.inp(Y, ld=ldy, gemm=True)
            dw = r.out(f"dW{i}", (Kd, N), gemm=True)
            db = r.out(f"db{i}", (N,)) if wb else None
            a.X, a.dY, a.out, a.bias_out = P(x), P(y), P(dw), P(db)
            a.ldx, a.ldy, a.ldo, a.Mrows, a.Kd, a.N = ldx, ldy, N, Mrows, Kd, N
        zero = r.inp(torch.zeros(128, dtype=torch.bfloat16))
        slab = r.out("slab", (slab_elems,), gemm=True)
        plan, count = (ctypes.c_int32 * 6)(), ctypes.c_int32(0)
        ck(L.smd_wgrad_lab_launch(arr, len(specs), 0, P(zero), P(slab), slab_elems, plan, 6, ctypes.byref(count), st()))
        plans.append((count.value, tuple(plan[:3])))

    got, _ = both(dev, body, unwritten=("slab",))        # the slab's rounding gaps and the bias row of problem 2 stay unwritten
    assert plans == [(1, (1 + 2 + 1, nsplit, 6))] * 2, plans
    for i, ((Kd, N, ldx, ldy, wb), (X, Y, ref, refb)) in enumerate(zip(specs, data)):
        e = rel(got[f"dW{i}"], ref)
        assert e < 3e-5                                  # test_gemm_tn
        if wb:
            assert rel(got[f"db{i}"], refb) < 3e-5
        WR.check(got[f"dW{i}"], got[f"db{i}"] if wb else None, WR.reference(X, Y), Mrows, nsplit, what=f"problem {i}")


# ================================================================================================ fp32 kernels
@pytest.mark.parametrize("row_mod", [0, 32])
@pytest.mark.parametrize("M,N,K,pads,mis", [(37, 45, 67, (1, 3, 1, 3), 1), (130, 132, 128, (4, 4, 4, 4), 0)], ids=["scalar", "vector"])
def test_gemm_f32(L, dev, M, N, K, pads, mis, row_mod):
    g = torch.Generator().manual_seed(M + 3 * K + 7 * N)
    A, W = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) / math.sqrt(K)
    b = 0.1 * torch.randn(N, generator=g)
    res = torch.randn(row_mod or M, N, generator=g)
    lda, ldw, ldo, ldr = K + pads[0], N + pads[1], N + pads[2], N + pads[3]

    def body(r):
        a, w = r.inp(A, ld=lda, gemm=True, misalign=mis), r.inp(W, ld=ldw, gemm=True, misalign=mis)
        bd, rd = r.inp(b, misalign=mis), r.inp(res, ld=ldr, gemm=True, misalign=mis)
        o = r.out("out", (M, N), ld=ldo, gemm=True, misalign=mis)
        assert (P(a) % 16 == 4) == bool(mis)
        ck(L.smd_gemm_f32(P(a), lda, P(w), ldw, M, N, K, P(bd), 0, P(rd), ldr, row_mod, P(o), ldo, st()), "smd_gemm_f32")

    got, _ = both(dev, body)
    want = A.double() @ W.double() + b.double() + (res.double() if not row_mod else res.double().repeat((M + 31) // 32, 1)[:M])
    err = (got["out"].double() - want).abs()
    bound = (K + 2) * U * (A.double().abs() @ W.double().abs() + b.double().abs()) + 2 * U * want.abs()
    assert rel(got["out"], want) <= 1e-5 and float((err / bound).max()) <= 1.0          # test_gemm_f32_against_float64


@pytest.mark.parametrize("rows,D,film", [(33, 130, False), (7, 2048, True)])
def test_layernorm_f32(L, dev, rows, D, film):
    g = torch.Generator().manual_seed(rows + D)
    x = 0.3 + 1.7 * torch.randn(rows, D, generator=g)
    p = {"n.scale": 1 + 0.1 * torch.randn(D, generator=g), "n.bias": 0.1 * torch.randn(D, generator=g)}
    ss = torch.randn(rows, 2 * D, generator=g) if film else None

    def body(r):
        xd, gd, bd = r.inp(x), r.inp(p["n.scale"]), r.inp(p["n.bias"])
        sd = r.inp(ss) if film else None
        o = r.out("out", (rows, D))
        ck(L.smd_layernorm_f32(P(xd), rows, D, P(gd), P(bd), P(sd), P(sd) + 4 * D if film else None, 2 * D, 1, None, 1000,
                               int(film), P(o), st()), "smd_layernorm_f32")

    got, _ = both(dev, body)
    want = O.layer_norm(x.double(), {k: v.double() for k, v in p.items()}, "n")
    if film:
        want = O.swish(ss.double()[:, :D] * want + ss.double()[:, D:])
    assert rel(got["out"], want) <= 1e-5                                                # test_layernorm_f32


def test_attention_f32(L, dev):
    B, S, E, H = 3, 32, 128, 8
    d = E // H
    qkv = 1.5 * torch.randn(B * S, 3 * E, generator=torch.Generator().manual_seed(H))

    def body(r):
        q, o = r.inp(qkv), r.out("out", (B * S, E))
        ck(L.smd_attention_f32(P(q), P(o), B, S, E, H, st()), "smd_attention_f32")

    got, _ = both(dev, body)
    q, k, v = qkv.double().view(B, S, 3 * E).split(E, dim=-1)
    w = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q.reshape(B, S, H, d) / math.sqrt(d), k.reshape(B, S, H, d)), dim=-1)
    want = torch.einsum("bhqk,bkhd->bqhd", w, v.reshape(B, S, H, d)).reshape(B * S, E)
    assert rel(got["out"], want) <= 1e-5                                                # test_attention_f32


def test_noise_embed_f32_and_bf16(L, dev):
    s = torch.tensor([1.0, 0.9999995, 0.6, 0.0814, 1e-3])
    n, C = s.numel(), 128

    def body(r):
        sd = r.inp(s)
        o = r.out("f32", (n, C), ld=C + 4)
        ck(L.smd_noise_embed_f32(P(sd), n, C, P(o), C + 4, st()), "smd_noise_embed_f32")
        ob = r.out("bf16", (n, C), torch.bfloat16, ld=C + 8)
        ck(L.smd_noise_embed(P(sd), n, C, P(ob), C + 8, st()), "smd_noise_embed")

    got, _ = both(dev, body)
    err = (got["f32"].double() - O.noise_encoding(s.double()[:, None], C)).abs().max(dim=1).values
    tol = 2.74 * 2.0 ** (torch.floor(torch.log2(5000.0 * s.double())) - 23) + 1e-6      # test_noise_embed_f32
    assert bool((err <= tol).all())
    assert float((got["bf16"].float() - O.noise_encoding(s[:, None], C)).abs().max()) < 1.2e-2   # test_noise_embed_and_rng


# ================================================================================================ elementwise and RNG
T = 1000
BETAS = O.create_noise_schedule(1e-6, 0.01, T, "linear")
APE = np.concatenate([np.ones(1, np.float32), O.alphas_cumprod(BETAS)]).astype(np.float32)


def test_cast_pad_bf16_writes_zero_padding_and_nothing_behind_the_last_row(L, dev):
    x = torch.randn(5, 42, generator=torch.Generator().manual_seed(1))

    def body(r):
        xd, o = r.inp(x), r.out("out", (5, 64), torch.bfloat16)         # the pad columns ARE output here: [rows][ld_out] is written
        ck(L.smd_cast_pad_bf16(P(xd), 5, 42, P(o), 64, st()))

    got, _ = both(dev, body)
    assert torch.equal(got["out"][:, :42], bf(x))
    assert bool((got["out"][:, 42:].contiguous().view(torch.int16) == 0).all())         # exactly +0


@pytest.mark.parametrize("B,S,C,Cp", [(5, 3, 42, 64), (1, 1, 1, 8)])
def test_q_sample_and_mse_leave_the_pad_columns_alone(L, dev, B, S, C, Cp):
    """xt_bf16 and dpred_bf16 are [B*S][Cp] with only the columns < C written (the arenas' pad columns are the sentinel)"""
    g = torch.Generator().manual_seed(B + C)
    x0 = torch.clamp(0.25 * torch.randn(B, S, C, generator=g), -1, 1)
    eps, pred = torch.randn(B, S, C, generator=g), torch.randn(B, S, C, generator=g)
    labels = torch.randint(1, T + 1, (B,), generator=g)
    inv = 1.0 / (B * S * C)

    def body(r):
        xd, ed, pd, ld_, ape = r.inp(x0), r.inp(eps), r.inp(pred), r.inp(labels.int()), r.inp(torch.from_numpy(APE))
        xt = r.out("xt", (B * S, C), torch.bfloat16, ld=Cp)
        eo, so = r.out("eps_out", (B, S, C)), r.out("level", (B,))
        ck(L.smd_q_sample(P(xd), B, S, C, Cp, T, P(ape), P(ld_), 1, None, P(ed), 7, 9, None, 0, P(xt), P(eo), P(so), st()))
        loss, dp = r.out("loss", (B,)), r.out("dpred", (B * S, C), torch.bfloat16, ld=Cp)
        ck(L.smd_mse_fwd_bwd(P(pd), P(ed), B, S, C, Cp, inv, P(loss), P(dp), st()))

    got, _ = both(dev, body)
    a = torch.from_numpy(O.used_alphas_from_labels(BETAS, labels.numpy())).view(B, 1, 1)
    want = torch.sqrt(a) * x0 + torch.sqrt(1 - a) * eps
    xt = got["xt"].float().view(B, S, C)
    assert torch.equal(got["eps_out"], eps) and torch.allclose(got["level"], torch.sqrt(a).flatten(), rtol=1e-6)
    assert torch.equal(xt, bf(want).float()) or rel(xt, want) < 3e-3                    # test_q_sample_matches_the_oracle_on_any_row_length
    assert torch.allclose(got["loss"], ((eps - pred) ** 2).mean(dim=(1, 2)), rtol=1e-5)
    assert rel(got["dpred"].float().view(B, S, C), 2 * (pred - eps) * inv) < 3e-3       # test_mse_and_adam_entries_match_the_oracle


def test_rng_normal_ragged_row_length(L, dev):
    B, per = 3, 126

    def body(r):
        ck(L.smd_rng_normal(P(r.out("z", (B, per))), B, per, 1234, 77, 3, 10, st()))

    got, _ = both(dev, body)
    ctr = np.zeros((B, 32, 4), np.uint32)
    ctr[..., 0], ctr[..., 1], ctr[..., 2] = np.arange(32)[None, :], (np.arange(B) + 10)[:, None], 3
    ref = O.philox_normal4(ctr, np.array([1234, 77], np.uint32)).reshape(B, 128)[:, :per]
    assert np.abs(got["z"].numpy() - ref).max() < 5e-5                                  # test_noise_embed_and_rng


@pytest.mark.parametrize("count", [7, 1])
def test_threefry_windows(L, dev, count):
    n, off, k0, k1 = 10, 3, 0x1234, 0xABCD
    key = (np.uint32(k0), np.uint32(k1))

    def body(r):
        ck(L.smd_threefry_bits(P(r.out("bits", (count,), torch.int32)), n, off, count, k0, k1, st()))
        ck(L.smd_threefry_uniform(P(r.out("uniform", (count,))), n, off, count, k0, k1, -0.25, 3.5, st()))
        ck(L.smd_threefry_normal(P(r.out("normal", (count,))), n, off, count, k0, k1, None, None, 0, 0, st()))
        ck(L.smd_threefry_randint(P(r.out("randint", (count,), torch.int32)), n, off, count, k0, k1, 1, 1001, st()))

    got, _ = both(dev, body)
    w = slice(off, off + count)
    assert np.array_equal(got["bits"].numpy().view(np.uint32), O.jax_random_bits(key, n)[w])
    assert np.array_equal(got["uniform"].numpy(), O.jax_uniform(key, n, -0.25, 3.5)[w])
    assert np.array_equal(got["randint"].numpy(), O.jax_randint(key, n, 1, 1001)[w])
    want = np.asarray(O.jax_normal(key, n), np.float64)[w]
    assert np.max(np.abs(got["normal"].double().numpy() - want) / (1 + np.abs(want))) <= 4e-7   # test_gpu_jax_random.close_normal


@pytest.mark.parametrize("with_ema", [True, False])
def test_adam_clip_ema(L, dev, with_ema):
    import smd_amd.lib as lib
    n = 1027
    g = torch.Generator().manual_seed(6)
    w, gr = torch.randn(n, generator=g, dtype=torch.float64), 0.01 * torch.randn(n, generator=g, dtype=torch.float64)
    h = lib.TrainHyper(1e-3, 0.98, 10000, 0.9, 0.999, 1e-8, 1.0, 0.999, 1.0)

    def body(r):
        gd = r.inp(gr.float())
        wd = r.out("w", (n,), init=w.float())
        m, v = r.out("m", (n,), init=torch.zeros(n)), r.out("v", (n,), init=torch.zeros(n))
        e = r.out("ema", (n,), init=w.float()) if with_ema else None
        step = r.out("step", (1,), torch.int32, init=torch.zeros(1, dtype=torch.int32))
        scratch, metrics = r.out("norm_partial", (1024,)), r.out("metrics", (4,))
        ck(L.smd_adam_clip_ema(P(wd), P(gd), P(m), P(v), P(e), n, ctypes.byref(h), P(step), P(scratch), P(metrics), st()))

    got, _ = both(dev, body, unwritten=("norm_partial",))
    clipped, norm = O.clip_grads({"w": gr}, 1.0)
    params = O.adam_update({"w": w.clone()}, clipped, O.AdamState(), O.stepped_lr(1e-3, 0, 10000, 0.98))
    assert rel(got["w"], params["w"]) < 1e-6 and int(got["step"]) == 1                  # test_mse_and_adam_entries_match_the_oracle
    if with_ema:
        assert rel(got["ema"], O.ema_update({"w": w.clone()}, params, 0.999)["w"]) < 1e-6
    assert abs(float(got["metrics"][0]) - float(torch.sqrt((gr * gr).sum()))) < 1e-4


def test_set_timestep_writes_one_word(L, dev):
    def body(r):
        ck(L.smd_set_timestep(P(r.out("t", (1,), torch.int32)), 417, st()))

    got, _ = both(dev, body)
    assert int(got["t"]) == 417


@pytest.mark.parametrize("mode", ["slot", "no-slot", "t=-1", "t=T"])
def test_ddpm_reverse_step_touches_one_slot_and_one_metrics_row(L, dev, mode):
    import smd_amd.schedule as S
    B, Sq, C, t = 5, 32, 42, 500
    coef = torch.from_numpy(S.reverse_coefficient_table(BETAS))
    g = torch.Generator().manual_seed(C)
    x, eh, z = (torch.randn(B, Sq, C, generator=g) for _ in range(3))
    slot = torch.full((T,), -1, dtype=torch.int32)
    if mode == "slot":
        slot[t] = 1
    slot[t - 1], slot[t + 1] = 0, 2                          # the neighbours' slots must stay untouched
    tv = {"t=-1": -1, "t=T": T}.get(mode, t)
    state, _, met = O.diffusion_dynamics(lambda s_, c_: eh.double(), BETAS, x.double(), lambda tt: z.double(), t_start=t, t_stop=t)
    handles = []

    def body(r):
        cd, ed, zd, sd = r.inp(coef), r.inp(eh), r.inp(z), r.inp(slot)
        tp = r.inp(torch.tensor([tv], dtype=torch.int32))
        xd = r.out("x", (B, Sq, C), init=x)
        mp, cl = r.out("metrics", (T, B, 3)), r.out("collection", (3, B, Sq, C))
        ck(L.smd_ddpm_reverse_step(P(xd), P(ed), B, Sq, C, P(cd), T, P(tp), P(zd), 0, 0, 0, P(mp), P(cl), P(sd), st()))
        handles.append(r)

    got, got2 = both(dev, body, unwritten=("metrics", "collection"))
    for res, fill in ((got, F.PATTERNS[0]), (got2, F.PATTERNS[1])):
        poisoned = lambda v: is_poison(v, fill)
        if mode in ("t=-1", "t=T"):                          # a no-op: nothing changes at all
            assert torch.equal(res["x"], x) and poisoned(res["metrics"]) and poisoned(res["collection"])
            continue
        assert rel(res["x"], state) < 1e-5                   # test_reverse_step_kernel
        assert poisoned(res["metrics"][:t]) and poisoned(res["metrics"][t + 1:])
        m = res["metrics"][t].sum(0).double() / (B * C)
        row = T - 1 - t
        assert abs(m[0] - met[0, row, 0]) / met[0, row, 0] < 1e-5 and abs(m[1] - met[1, row, 0]) / met[1, row, 0] < 1e-4
        assert abs(m[2] - met[3, row, 0]) / (met[3, row, 0] + 1e-12) < 1e-4
        assert poisoned(res["collection"][0]) and poisoned(res["collection"][2])
        if mode == "slot":
            assert torch.equal(res["collection"][1], res["x"])
        else:
            assert poisoned(res["collection"][1])
    assert torch.equal(got["x"], got2["x"])


# ================================================================================================ metric kernels
def latent(n, d, seed, scale=1.0, shift=0.0):
    rng = np.random.default_rng(seed)
    return np.clip(scale * 0.25 * rng.standard_normal((n, d)) + shift, -1, 1).astype(np.float32)


def ws_arena(r, nbytes):
    return r.out("workspace", (max(int(nbytes), 8),), torch.uint8)


@pytest.mark.parametrize("symmetric", [0, 1])
def test_pair_kernel_sums(L, dev, symmetric):
    nx, ny, d = 130, (130 if symmetric else 77), 42
    x = np.random.default_rng(1).uniform(-1, 1, (nx, d)).astype(np.float32)
    y = x if symmetric else np.random.default_rng(2).uniform(-0.9, 1, (ny, d)).astype(np.float32)
    gamma, degree, coef0 = 1.0 / d, 2, 0.5
    need = L.smd_pair_kernel_sums_workspace_bytes(nx, ny, symmetric)

    def body(r):
        xd = r.inp(torch.from_numpy(x), ld=d + 3)
        yd = None if symmetric else r.inp(torch.from_numpy(y), ld=d + 3)
        ws, o = ws_arena(r, need), r.out("out", (2,), torch.float64)
        ck(L.smd_pair_kernel_sums(P(xd), d + 3, nx, P(yd), d + 3, ny, d, symmetric, gamma, 1.0, coef0, degree, P(ws), need, P(o), st()))

    got, _ = both(dev, body, unwritten=("workspace",))
    ref = RM.kernel_sums(x, y, bool(symmetric), gamma, 1.0, coef0, degree)
    out = got["out"].numpy()
    assert abs(out[0] - ref[0]) <= 2e-5 * ref[1] + nx * ny * 2.0 ** -126 and abs(out[1] - ref[2]) <= 2e-5 * ref[3]   # test_pair_kernel_sums_match_float64


def test_moments(L, dev):
    n, d = 130, 42
    rng = np.random.default_rng(n)
    x = (rng.uniform(-1, 1, (n, d)) * rng.uniform(0.1, 1.0, d) + rng.uniform(-0.5, 0.5, d)).astype(np.float32)
    need = L.smd_moments_workspace_bytes(n, d)

    def body(r):
        xd, ws = r.inp(torch.from_numpy(x), ld=d + 3), ws_arena(r, need)
        mu, cov = r.out("mean", (d,), torch.float64), r.out("cov", (d, d), torch.float64)
        ck(L.smd_moments(P(xd), d + 3, n, d, P(ws), need, P(mu), P(cov), st()))

    got, _ = both(dev, body, unwritten=("workspace",))
    rmu, rcov = x.astype(np.float64).mean(0), np.cov(x.astype(np.float64), rowvar=False)
    mu, cov = got["mean"].numpy(), got["cov"].numpy()
    assert np.linalg.norm(mu - rmu) <= 1e-6 * np.linalg.norm(rmu) and np.linalg.norm(cov - rcov) <= 1e-6 * np.linalg.norm(rcov)   # test_moments_match_np_cov
    assert np.array_equal(cov, cov.T)


def test_knn_radii_and_ball_cover(L, dev):
    from test_gpu_nn_metrics import check_cover, check_radii, check_realism
    n, nq, d, k = 130, 77, 42, 3
    x, q = latent(n, d, 0), latent(nq, d, 1, 0.9, 0.05)
    need = L.smd_knn_radii_workspace_bytes(n, k)

    def knn(r):
        xd, ws = r.inp(torch.from_numpy(x), ld=d + 3), ws_arena(r, need)
        ck(L.smd_knn_radii(P(xd), d + 3, n, d, k, P(ws), need, P(r.out("r2", (n,))), st()))

    r2_gpu = both(dev, knn, unwritten=("workspace",))[0]["r2"]
    r2 = check_radii(x, k, r2_gpu.numpy())
    keep = torch.from_numpy(RN.keep_mask(r2).astype(np.uint8))
    for excl in (0, 1):
        qq, nqq = (x, n) if excl else (q, nq)
        bneed = L.smd_ball_cover_workspace_bytes(nqq, n)

        def cover(r):
            qd, xd = r.inp(torch.from_numpy(qq), ld=d + 3), r.inp(torch.from_numpy(x), ld=d + 3)
            rd, kd, ws = r.inp(r2_gpu), r.inp(keep), ws_arena(r, bneed)
            cov, re2 = r.out("covered", (nqq,), torch.uint8), r.out("realism2", (nqq,))
            ck(L.smd_ball_cover(P(qd), d + 3, nqq, P(xd), d + 3, n, d, P(rd), P(kd), excl, P(ws), bneed, P(cov), P(re2), st()))

        got, _ = both(dev, cover, unwritten=("workspace",))
        m = RN.d2_error_bound(d, qq, x)
        dqx = RN.sqdist(x) if excl else RN.sqdist(qq, x)
        if excl:
            s, certain = RN.loo_certain(dqx, r2, k, m)
        else:
            s = RN.cover_margin(dqx, r2)
            certain = np.abs(s) > 2 * m
        check_cover(f"exclude_diagonal={excl}", s, certain, got["covered"].numpy())
        check_realism(dqx, r2, keep.numpy(), m, got["realism2"].numpy(), exclude_diagonal=bool(excl))


@pytest.mark.parametrize("k", [5, 128])
def test_kmeans_assign(L, dev, k):
    from test_gpu_kmeans import check_labels, check_min_d2
    n, d = 130, 42
    rng = np.random.default_rng([n, d, k])
    x = RC.mixture(rng, n, d, max(k, 2))
    c = RC.make_centres(rng, x, k)
    lab, certain, s, e = RC.labels_certain(x, c)
    need = L.smd_kmeans_assign_workspace_bytes(n, k)

    def body(r):
        xd, cd, ws = r.inp(torch.from_numpy(x), ld=d + 3), r.inp(torch.from_numpy(c)), ws_arena(r, need)
        lb, md = r.out("labels", (n,), torch.int32), r.out("min_d2", (n,))
        inertia, changed = r.out("inertia", (1,), torch.float64), r.out("changed", (1,), torch.int64)
        ck(L.smd_kmeans_assign(P(xd), d + 3, n, d, P(cd), k, 0, P(ws), need, P(lb), P(md), P(inertia), P(changed), st()))

    got, _ = both(dev, body, unwritten=("workspace",))
    lab_gpu = got["labels"].numpy()
    assert lab_gpu.max() < k and int(got["changed"]) == n
    check_labels(f"k={k}", lab_gpu, lab, certain)
    check_min_d2(f"k={k}", x, s, e, lab_gpu, got["min_d2"].numpy(), float(got["inertia"]))


def test_kmeans_update_counts_a_label_outside_the_range_nowhere(L, dev):
    n, d, k = 300, 42, 5
    rng = np.random.default_rng(9)
    x = RC.mixture(rng, n, d, k)
    c = RC.make_centres(rng, x, k)
    lab = RC.scores(x, c).argmin(1).astype(np.int32)
    lab[17], lab[290] = -1, k
    valid = (lab >= 0) & (lab < k)
    need = L.smd_kmeans_update_workspace_bytes(n, d, k)

    def body(r):
        xd, ld_, cd = r.inp(torch.from_numpy(x), ld=d + 3), r.inp(torch.from_numpy(lab)), r.inp(torch.from_numpy(c))
        ws, new, counts = ws_arena(r, need), r.out("centres", (k, d)), r.out("counts", (k,), torch.int64)
        ck(L.smd_kmeans_update(P(xd), d + 3, n, d, P(ld_), P(cd), k, P(ws), need, P(new), P(counts), st()))

    got, _ = both(dev, body, unwritten=("workspace",))
    ref, ref_counts = RC.means(x[valid], lab[valid], c)
    counts = got["counts"].numpy()
    assert np.array_equal(counts, ref_counts) and counts.sum() == n - 2
    err = np.abs(got["centres"].double().numpy() - ref)
    assert (err <= RC.mean_bound(x[valid], ref, ref_counts)).all()                       # test_update_against_float64


# ================================================================================================ LayerNorm, attention, partial tiles
def ln64(v, gm, bt):
    mu, var = v.mean(-1, keepdim=True), v.var(-1, unbiased=False, keepdim=True)
    return (v - mu) / torch.sqrt(var + 1e-6) * gm.double() + bt.double()


def ln_partial_min(rows, D, group):
    """the documented minimum of partial_elems: one [2][D] pair of column sums per row group (rows_per_sample rows with FiLM, else 32)"""
    return -(-rows // group) * 2 * D


@pytest.mark.parametrize("D,film", [(128, False), (1024, True), (2048, True)])
def test_layernorm_fwd_and_bwd_forms(L, dev, D, film):
    """smd_layernorm_fwd / _fwd_ex / _bwd / _bwd_ex / _bwd_film; dgamma / dbeta start as NaN: they are written, not accumulated"""
    rows, rps = 128, 32
    ns = rows // rps
    g = torch.Generator().manual_seed(D + 3 * film)
    x = torch.randn(rows, D, generator=g) * 1.7 + 0.3
    gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    ss = torch.cat([1 + 0.3 * torch.randn(ns, D, generator=g), 0.2 * torch.randn(ns, D, generator=g)], dim=1)
    dout = bf(torch.randn(rows, D, generator=g))
    xr, gr, br, ssr = (t.double().requires_grad_(True) for t in (x, gamma, beta, ss))
    y = O.layer_norm(xr, {"n.scale": gr, "n.bias": br}, "n")
    y_plain = y
    if film:
        y = O.swish(ssr[:, :D].repeat_interleave(rps, 0) * y + ssr[:, D:].repeat_interleave(rps, 0))
    y.backward(dout.double(), retain_graph=True)
    dx_ref, dg_ref, db_ref = xr.grad.clone(), gr.grad.clone(), br.grad.clone()
    dss_ref = ssr.grad.clone() if film else None
    for t in (xr, gr, br):
        t.grad = None
    y_plain.backward(dout.double())
    npart = ln_partial_min(rows, D, rps if film else 32)

    def body(r):
        xd, gd, bd, sd, dd = r.inp(x), r.inp(gamma), r.inp(beta), r.inp(ss), r.inp(dout)
        fs, fsh = (P(sd), P(sd) + 4 * D) if film else (None, None)
        sw = int(film)
        ck(L.smd_layernorm_fwd(P(xd), rows, D, P(gd), P(bd), fs, fsh, 2 * D, rps, sw, P(r.out("fwd", (rows, D), torch.bfloat16)), st()))
        ck(L.smd_layernorm_fwd_ex(P(xd), None, rows, D, P(gd), P(bd), fs, fsh, 2 * D, rps, sw,
                                  P(r.out("fwd_ex", (rows, D), torch.bfloat16)), st()))
        dx, dg, db = r.out("dx", (rows, D)), r.out("dgamma", (D,)), r.out("dbeta", (D,))
        dss = r.out("dfilm", (ns, 2 * D)) if film else None
        part = r.out("partial", (npart,))
        ck(L.smd_layernorm_bwd(P(xd), rows, D, P(gd), P(bd), fs, fsh, 2 * D, rps, sw, P(dd), P(dx), P(dg), P(db),
                               P(dss), P(dss) + 4 * D if film else None, P(part), npart, st()))
        dx2, dxb2 = r.out("dx_film", (rows, D)), r.out("dxb_film", (rows, D), torch.bfloat16)
        dg2, db2 = r.out("dgamma_film", (D,)), r.out("dbeta_film", (D,))
        dss2 = r.out("dfilm_film", (ns, 2 * D)) if film else None
        part2 = r.out("partial_film", (npart,))
        ck(L.smd_layernorm_bwd_film(P(xd), None, rows, D, P(gd), P(bd), fs, fsh, 2 * D, rps, sw, P(dd), None, None, P(dx2), P(dxb2),
                                    P(dg2), P(db2), P(dss2), P(dss2) + 4 * D if film else None, 0, P(part2), npart, st()))
        dx3, dxb3 = r.out("dx_ex", (rows, D)), r.out("dxb_ex", (rows, D), torch.bfloat16)
        dg3, db3, part3 = r.out("dgamma_ex", (D,)), r.out("dbeta_ex", (D,)), r.out("partial_ex", (npart,))
        ck(L.smd_layernorm_bwd_ex(P(xd), None, rows, D, P(gd), P(bd), P(dd), None, P(dx3), P(dxb3), P(dg3), P(db3), P(part3), npart, st()))

    got, _ = both(dev, body, unwritten=("partial", "partial_film", "partial_ex"))
    assert rel(got["fwd"].float(), y) < 4e-3 and torch.equal(got["fwd"], got["fwd_ex"])          # test_layernorm_fwd_bwd
    for sfx in ("", "_film"):
        assert rel(got["dx" + sfx], dx_ref) < 1e-4 and rel(got["dgamma" + sfx], dg_ref) < 1e-4 and rel(got["dbeta" + sfx], db_ref) < 1e-4
        if film:
            assert rel(got["dfilm" + sfx], dss_ref) < 1e-4
    assert rel(got["dxb_film"].float(), dx_ref) < 4e-3                                            # test_layernorm_bwd_film_forms
    assert rel(got["dx_ex"], xr.grad) < 1e-4 and rel(got["dgamma_ex"], gr.grad) < 1e-4 and rel(got["dbeta_ex"], br.grad) < 1e-4
    assert rel(got["dxb_ex"].float(), xr.grad) < 4e-3


@pytest.mark.parametrize("H", [8, 4, 16])
def test_attention_fwd_bwd(L, dev, H):
    B, S, E = 3, 32, 128
    d = E // H
    g = torch.Generator().manual_seed(H)
    qkv, dout = bf(torch.randn(B * S, 3 * E, generator=g) * 1.5), bf(torch.randn(B * S, E, generator=g))
    qr = qkv.double().requires_grad_(True)
    q, k, v = qr.view(B, S, 3 * E).split(E, dim=-1)
    w = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q.reshape(B, S, H, d) / math.sqrt(d), k.reshape(B, S, H, d)), dim=-1)
    o = torch.einsum("bhqk,bkhd->bqhd", w, v.reshape(B, S, H, d)).reshape(B * S, E)
    o.backward(dout.double())

    def body(r):
        qd, dd = r.inp(qkv), r.inp(dout)
        ck(L.smd_attention_fwd(P(qd), P(r.out("out", (B * S, E), torch.bfloat16)), B, S, E, H, st()))
        ck(L.smd_attention_bwd(P(qd), P(dd), P(r.out("dqkv", (B * S, 3 * E), torch.bfloat16)), B, S, E, H, st()))

    got, _ = both(dev, body)
    assert rel(got["out"].float(), o) < 4e-3 and rel(got["dqkv"].float(), qr.grad) < 4e-3         # test_attention_fwd_bwd


@pytest.mark.parametrize("rows", [32, 96])
def test_ln128_parts_and_bwd_parts_with_poisoned_gaps(L, dev, rows):
    """the consumers of four partial tiles at part_stride = rows * 128 + 2 (two poisoned floats between the tiles)"""
    E, stride = 128, rows * 128 + 2
    g = torch.Generator().manual_seed(rows)
    parts, dparts = torch.randn(4, rows * E, generator=g) * 0.7, torch.randn(4, rows * E, generator=g) * 0.02
    x, dres = torch.randn(rows, E, generator=g) * 1.3 + 0.2, 0.05 * torch.randn(rows, E, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(E, generator=g), 0.1 * torch.randn(E, generator=g)
    s = ((parts[0] + parts[1]) + (parts[2] + parts[3])).view(rows, E)
    xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), torch.zeros(E, dtype=torch.float64, requires_grad=True)
    O.layer_norm(xr, {"n.scale": gr, "n.bias": br}, "n").backward(dparts.double().sum(0).view(rows, E))

    def body(r):
        pd, dpd = r.inp(parts, ld=stride), r.inp(dparts, ld=stride)
        xd, gd, bd = r.inp(x), r.inp(gamma), r.inp(beta)
        xo, lo = r.out("x_out", (rows, E)), r.out("ln_out", (rows, E), torch.bfloat16)
        ck(L.smd_ln128_parts(P(pd), stride, rows, P(gd), P(bd), P(xo), P(lo), st()))
        dx = r.out("dx", (rows, E), init=dres)                                        # dx aliases dres: in place
        dxb, partial = r.out("dx_bf16", (rows, E), torch.bfloat16), r.out("partial", (rows // 32, 2, E))
        ck(L.smd_ln128_bwd_parts(P(xd), P(dpd), stride, rows, P(gd), P(dx), P(dx), P(dxb), P(partial), st()))

    got, _ = both(dev, body)
    assert torch.equal(got["x_out"], s) and rel(got["ln_out"].float(), ln64(s.double(), gamma, beta)) < 4e-3
    dx_ref = xr.grad + dres.double()
    assert rel(got["dx"], dx_ref) < 2e-5 and rel(got["dx_bf16"].float(), dx_ref) < 4e-3          # test_mlp_block_bwd_hidden_split
    assert rel(got["partial"][:, 0].sum(0), gr.grad) < 2e-5 and rel(got["partial"][:, 1].sum(0), br.grad) < 2e-5


# ================================================================================================ e4m3
def test_quantize_rows_e4m3_ragged(L, dev):
    """rows % 4 != 0 and K % 512 != 0, ld > K: out8 is [rows][K] and scale [rows], nothing else"""
    rows, K, ld = 5, 520, 528
    x = bf(torch.randn(rows, K, generator=torch.Generator().manual_seed(3)) * torch.tensor([0.01, 1.0, 30.0, 300.0, 0.3]).view(rows, 1))

    def body(r):
        xd = r.inp(x, ld=ld)
        q, s = r.out("q", (rows, K), torch.uint8), r.out("scale", (rows,), torch.int32)
        ck(L.smd_quantize_rows_e4m3(P(xd), ld, rows, K, P(q), P(s), st()))

    got, _ = both(dev, body)
    # test_quantize_rows_e4m3: the row exponent, the bytes of torch's float8_e4m3fn cast, the dequantised rows
    e = (got["scale"].to(torch.int64) & 0xFF) - 127
    amax = x.float().abs().amax(1)
    assert torch.equal(e, torch.ceil(torch.log2(amax.double() / 448.0)).to(torch.int64))
    want = (x.float() * torch.pow(2.0, -e.float()).unsqueeze(1)).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert float((want.view(torch.uint8) == got["q"]).float().mean()) > 0.999
    deq = got["q"].view(torch.float8_e4m3fn).float().double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double()).unsqueeze(1)
    assert bool(torch.isfinite(deq).all()) and rel(deq, x.double()) < 4e-2


# ================================================================================================ fused encoder half-layers
def mlp_weights(g, M):
    W1, b1 = bf(torch.randn(128, M, generator=g) * 0.09), 0.1 * torch.randn(M, generator=g)          # kernels (in, out)
    W2, b2 = bf(torch.randn(M, 128, generator=g) * (1.0 / math.sqrt(M))), 0.1 * torch.randn(128, generator=g)
    return W1, b1, W2, b2


@pytest.mark.parametrize("rows,M", [(32, 128), (96, 256)])
def test_mlp_block_fwd(L, dev, rows, M):
    g = torch.Generator().manual_seed(rows + M)
    h = torch.randn(rows, 128, generator=g) * 1.5 + 0.3
    gamma, beta = 1 + 0.2 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    W1, b1, W2, b2 = mlp_weights(g, M)
    hd = h.double()
    a2 = bf(ln64(hd, gamma, beta).float())
    z = a2.double() @ W1.double() + b1.double()
    u = bf(O.gelu(z).float())
    ref = hd + u.double() @ W2.double() + b2.double()

    def body(r):
        hD, gD, bD = r.inp(h), r.inp(gamma), r.inp(beta)
        W1t, W2t, b1D, b2D = r.inp(W1.t().contiguous()), r.inp(W2.t().contiguous()), r.inp(b1), r.inp(b2)
        out = r.out("out", (rows, 128))
        sa, sz, su = (r.out(n, (rows, w), torch.bfloat16) for n, w in (("a2", 128), ("z1", M), ("u", M)))
        ck(L.smd_mlp_block_fwd(P(hD), P(out), rows, P(gD), P(bD), P(W1t), P(b1D), P(W2t), P(b2D), M, P(sa), P(sz), P(su), st()))
        inpl = r.out("inplace", (rows, 128), init=h)
        ck(L.smd_mlp_block_fwd(P(inpl), P(inpl), rows, P(gD), P(bD), P(W1t), P(b1D), P(W2t), P(b2D), M, None, None, None, st()))

    got, _ = both(dev, body)
    assert rel(got["out"].double() - hd, ref - hd) < 3e-3                                     # test_mlp_block_fwd_fused
    assert rel(got["a2"].float(), a2.float()) < 2e-3 and rel(got["z1"].float(), z) < 4e-3 and rel(got["u"].float(), u.float()) < 4e-3
    assert torch.equal(got["inplace"], got["out"])


@pytest.mark.parametrize("rows", [32, 192])
def test_mlp_block_fwd_hs_writes_exactly_four_tiles(L, dev, rows):
    M = 512
    g = torch.Generator().manual_seed(rows + M + 1)
    h, a2 = torch.randn(rows, 128, generator=g) * 1.5 + 0.3, bf(torch.randn(rows, 128, generator=g))
    W1, b1, W2, b2 = mlp_weights(g, M)
    u = bf(O.gelu(a2.double() @ W1.double() + b1.double()).float())
    ref = h.double() + u.double() @ W2.double() + b2.double()

    def body(r):
        hD, aD = r.inp(h), r.inp(a2)
        W1t, W2t, b1D, b2D = r.inp(W1.t().contiguous()), r.inp(W2.t().contiguous()), r.inp(b1), r.inp(b2)
        ck(L.smd_mlp_block_fwd_hs(P(aD), P(hD), rows, P(W1t), P(b1D), P(W2t), P(b2D), M, P(r.out("part", (4, rows * 128))), st()))

    p = both(dev, body)[0]["part"]
    x = ((p[0] + p[1]) + (p[2] + p[3])).view(rows, 128)
    assert rel(x.double() - h.double(), ref - h.double()) < 3e-3                              # test_mlp_block_fwd_hidden_split


def test_mlp_block_bwd_hs_writes_exactly_four_tiles(L, dev):
    rows, M = 128, 512
    g = torch.Generator().manual_seed(rows + M + 3)
    a2, dh = bf(torch.randn(rows, 128, generator=g)), bf(torch.randn(rows, 128, generator=g) * 0.05)
    W1, b1, W2, _ = mlp_weights(g, M)
    z = (a2.double() @ W1.double() + b1.double()).requires_grad_(True)
    u_ref = O.gelu(z)
    (gz,) = torch.autograd.grad(u_ref.sum(), z)
    dz_ref = (dh.double() @ W2.double().t()) * gz
    da2_ref = bf(dz_ref.float()).double() @ W1.double().t()

    def body(r):
        aD, dD, b1D = r.inp(a2), r.inp(dh), r.inp(b1)
        W1t, W2p, W1p = r.inp(W1.t().contiguous()), r.inp(W2.contiguous()), r.inp(W1.contiguous())
        u, dz = r.out("u", (rows, M), torch.bfloat16), r.out("dz", (rows, M), torch.bfloat16)
        ck(L.smd_mlp_block_bwd_hs(P(aD), P(dD), rows, P(W1t), P(W2p), P(W1p), P(b1D), M, P(u), P(dz), P(r.out("part", (4, rows * 128))), st()))

    got, _ = both(dev, body)
    p = got["part"]
    da2 = ((p[0] + p[1]) + (p[2] + p[3])).view(rows, 128)
    assert rel(got["u"].float(), u_ref.detach()) < 4e-3 and rel(got["dz"].float(), dz_ref.detach()) < 6e-3   # test_mlp_block_bwd_hidden_split
    assert rel(da2, da2_ref.detach()) < 4e-3


def attn_weights(g, E=128):
    Wqkv, bqkv = bf(torch.randn(E, 3 * E, generator=g) * 0.12), 0.1 * torch.randn(3 * E, generator=g)
    Wo, bo = bf(torch.randn(E, E, generator=g) * 0.09), 0.1 * torch.randn(E, generator=g)
    return Wqkv, bqkv, Wo, bo


@pytest.mark.parametrize("rows,H", [(32, 8), (96, 16), (32, 4), (96, 8)])
def test_attn_block_fwd_and_fwd_ex(L, dev, rows, H):
    """smd_attn_block_fwd with every save_* buffer, and smd_attn_block_fwd_ex on four partial tiles two poisoned floats apart
    with h_comb, a2_out and every save_* buffer"""
    g = torch.Generator().manual_seed(rows + H)
    E, d, B, stride = 128, 128 // H, rows // 32, rows * 128 + 2
    parts = torch.randn(4, rows * E, generator=g) * 0.6
    h = ((parts[0] + parts[1]) + (parts[2] + parts[3])).view(rows, E)
    gamma, beta = 1 + 0.2 * torch.randn(E, generator=g), 0.1 * torch.randn(E, generator=g)
    gamma2, beta2 = 1 + 0.2 * torch.randn(E, generator=g), 0.1 * torch.randn(E, generator=g)
    Wqkv, bqkv, Wo, bo = attn_weights(g)
    hd = h.double()
    a1 = bf(ln64(hd, gamma, beta).float())
    qkv = bf((a1.double() @ Wqkv.double() + bqkv.double()).float())
    q, k, v = [t.double().view(B, 32, H, d).transpose(1, 2) for t in qkv.split(E, dim=-1)]
    p = torch.softmax(bf((q / math.sqrt(d)).float()).double() @ k.transpose(-1, -2), dim=-1)
    o = bf((p @ v).transpose(1, 2).reshape(rows, E).float())
    ref = hd + o.double() @ Wo.double() + bo.double()

    def body(r):
        hD, pD, gD, bD, g2D, b2D = r.inp(h), r.inp(parts, ld=stride), r.inp(gamma), r.inp(beta), r.inp(gamma2), r.inp(beta2)
        WqD, bqD, WoD, boD = r.inp(Wqkv.t().contiguous()), r.inp(bqkv), r.inp(Wo.t().contiguous()), r.inp(bo)
        out = r.out("out", (rows, E))
        sa, sq, so = (r.out(n, (rows, w), torch.bfloat16) for n, w in (("a1", E), ("qkv", 3 * E), ("o", E)))
        ck(L.smd_attn_block_fwd(P(hD), P(out), rows, P(gD), P(bD), P(WqD), P(bqD), P(WoD), P(boD), H, P(sa), P(sq), P(so), st()))
        out2, comb, a2 = r.out("out_ex", (rows, E)), r.out("comb", (rows, E)), r.out("a2", (rows, E), torch.bfloat16)
        sa2, sq2, so2 = (r.out(n, (rows, w), torch.bfloat16) for n, w in (("a1_ex", E), ("qkv_ex", 3 * E), ("o_ex", E)))
        ck(L.smd_attn_block_fwd_ex(None, P(pD), stride, P(comb), P(out2), rows, P(gD), P(bD), P(WqD), P(bqD), P(WoD), P(boD), H,
                                   P(g2D), P(b2D), P(a2), P(sa2), P(sq2), P(so2), st()))

    got, _ = both(dev, body)
    assert rel(got["a1"].float(), a1.float()) < 2e-3 and rel(got["qkv"].float(), qkv.float()) < 2e-3       # test_attn_block_fwd_fused
    assert rel(got["o"].float(), o.float()) < 6e-3 and rel(got["out"].double() - hd, ref - hd) < 6e-3
    assert torch.equal(got["comb"], h) and torch.equal(got["out_ex"], got["out"])            # test_attn_block_fwd_partial_sum_input_and_ln2
    assert all(torch.equal(got[n], got[n + "_ex"]) for n in ("a1", "qkv", "o"))
    assert rel(got["a2"].float(), ln64(got["out"].double(), gamma2, beta2)) < 4e-3


@pytest.mark.parametrize("rows,H", [(32, 8), (96, 16), (32, 4), (96, 8)])
def test_attn_block_bwd_and_bwd_ln(L, dev, rows, H):
    g = torch.Generator().manual_seed(11 * rows + H)
    E, d, B, stride = 128, 128 // H, rows // 32, rows * 128 + 2
    h_mid, h = torch.randn(rows, E, generator=g) * 1.3 + 0.2, torch.randn(rows, E, generator=g) * 0.9 - 0.1
    parts, dh = torch.randn(4, rows * E, generator=g) * 0.02, torch.randn(rows, E, generator=g) * 0.05
    g2, g1 = 1 + 0.2 * torch.randn(E, generator=g), 1 + 0.2 * torch.randn(E, generator=g)
    qkv = bf(torch.randn(rows, 3 * E, generator=g) * 0.8)
    Wo, Wqkv = bf(torch.randn(E, E, generator=g) * 0.09), bf(torch.randn(E, 3 * E, generator=g) * 0.09)
    dmid = bf(torch.randn(rows, E, generator=g) * 0.05)

    def body(r):
        qD, WoD, WqD, dmD = r.inp(qkv), r.inp(Wo), r.inp(Wqkv), r.inp(dmid)
        dq0, da0 = r.out("dqkv_plain", (rows, 3 * E), torch.bfloat16), r.out("da1_plain", (rows, E), torch.bfloat16)
        ck(L.smd_attn_block_bwd(P(dmD), P(qD), P(WoD), P(WqD), P(dq0), P(da0), rows, H, st()))
        hmD, hD, pD, g2D, g1D = r.inp(h_mid), r.inp(h), r.inp(parts, ld=stride), r.inp(g2), r.inp(g1)
        dq, da1 = r.out("dqkv", (rows, 3 * E), torch.bfloat16), r.out("da1", (rows, E), torch.bfloat16)
        dhD = r.out("dh", (rows, E), init=dh)
        mid, dho = r.out("dh_mid", (rows, E), torch.bfloat16), r.out("dh_out", (rows, E), torch.bfloat16)
        p2, p1 = r.out("partial2", (rows // 32, 2, E)), r.out("partial1", (rows // 32, 2, E))
        ck(L.smd_attn_block_bwd_ln(P(qD), P(WoD), P(WqD), P(dq), P(da1), P(hmD), P(pD), stride, P(g2D), P(dhD), P(mid), P(p2),
                                   P(hD), P(g1D), P(dho), P(p1), rows, H, st()))

    got, _ = both(dev, body)

    def attn_bwd64(do):
        leaf = qkv.double().clone().requires_grad_(True)
        q, k, v = [t.view(B, 32, H, d).transpose(1, 2) for t in leaf.split(E, dim=-1)]
        pr = torch.softmax((q / math.sqrt(d)) @ k.transpose(-1, -2), dim=-1)
        ((pr @ v).transpose(1, 2).reshape(rows, E) * do.double()).sum().backward()
        return leaf.grad

    def ln_bwd64(x, gamma, dout):
        xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), torch.zeros(E, dtype=torch.float64, requires_grad=True)
        O.layer_norm(xr, {"n.scale": gr, "n.bias": br}, "n").backward(dout.double())
        return xr.grad, gr.grad, br.grad

    # ---- smd_attn_block_bwd (test_attn_block_bwd_fused)
    ref = attn_bwd64(bf((dmid.double() @ Wo.double().t()).float()))
    assert max(rel(got["dqkv_plain"][:, i * E:(i + 1) * E].float(), ref[:, i * E:(i + 1) * E]) for i in range(3)) < 1e-2
    assert rel(got["da1_plain"].float(), got["dqkv_plain"].double() @ Wqkv.double().t()) < 4e-3
    # ---- smd_attn_block_bwd_ln, stage by stage (test_attn_block_bwd_with_both_layernorm_backwards)
    dx2, dg2, db2 = ln_bwd64(h_mid, g2, parts.double().sum(0).view(rows, E))
    dh_mid_ref = dx2 + dh.double()
    assert rel(got["dh_mid"].float(), dh_mid_ref) < 4e-3
    assert rel(got["dqkv"].float(), attn_bwd64(bf((got["dh_mid"].double() @ Wo.double().t()).float()))) < 1e-2
    assert rel(got["da1"].float(), bf((got["dqkv"].double() @ Wqkv.double().t()).float()).float()) < 4e-3
    dx1, dg1, db1 = ln_bwd64(h, g1, got["da1"].double())
    assert rel(got["dh"].double() - dh_mid_ref, dx1) < 1e-4 and rel(got["dh"], dx1 + dh_mid_ref) < 1e-5
    assert rel(got["dh_out"].float(), dx1 + dh_mid_ref) < 4e-3
    p2, p1 = got["partial2"], got["partial1"]
    assert max(rel(p2[:, 0].sum(0), dg2), rel(p2[:, 1].sum(0), db2), rel(p1[:, 0].sum(0), dg1), rel(p1[:, 1].sum(0), db1)) < 1e-4


# ================================================================================================ e4m3 GEMM and LayerNorm
def dequant(q8, scale):
    e = (scale.to(torch.int64) & 0xFF) - 127
    return q8.view(torch.float8_e4m3fn).float().double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double()).unsqueeze(1)


def test_gemm_e4m3_nt(L, dev):
    """(256, 256, 256) with lda = ldb = K + 16 and ld_out = N + 8, both output forms (bias -> bf16; bias + residual -> fp32)"""
    M = N = K = 256
    g = torch.Generator().manual_seed(M + N + K)
    a, b = bf(torch.randn(M, K, generator=g)), bf(torch.randn(N, K, generator=g) * 0.05)
    bias, res = 0.1 * torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    qs = {}

    def quant(r):
        aD, bD = r.inp(a), r.inp(b)
        ck(L.smd_quantize_rows_e4m3(P(aD), K, M, K, P(r.out("qa", (M, K), torch.uint8)), P(r.out("sa", (M,), torch.int32)), st()))
        ck(L.smd_quantize_rows_e4m3(P(bD), K, N, K, P(r.out("qb", (N, K), torch.uint8)), P(r.out("sb", (N,), torch.int32)), st()))

    qs = both(dev, quant)[0]
    ref = dequant(qs["qa"], qs["sa"]) @ dequant(qs["qb"], qs["sb"]).t() + bias.double()

    def body(r):
        qa, qb = r.inp(qs["qa"], ld=K + 16, gemm=True), r.inp(qs["qb"], ld=K + 16, gemm=True)
        sa, sb, bd, rd = r.inp(qs["sa"]), r.inp(qs["sb"]), r.inp(bias), r.inp(res, ld=N + 8, gemm=True)
        ob = r.out("bf16", (M, N), torch.bfloat16, ld=N + 8, gemm=True)
        ck(L.smd_gemm_e4m3_nt(P(qa), K + 16, P(sa), P(qb), K + 16, P(sb), M, N, K, P(bd), None, 0, None, 0, P(ob), N + 8, st()))
        of = r.out("f32", (M, N), ld=N + 8, gemm=True)
        ck(L.smd_gemm_e4m3_nt(P(qa), K + 16, P(sa), P(qb), K + 16, P(sb), M, N, K, P(bd), P(rd), N + 8, P(of), N + 8, None, 0, st()))

    got, _ = both(dev, body)
    assert rel(got["bf16"].float(), ref) < 4e-3 and rel(got["f32"], ref + res.double()) < 2e-4             # test_gemm_e4m3_nt


# ================================================================================================ engine level
@pytest.mark.parametrize("arch", ["TransformerDDPM", "DenseDDPM"])
def test_engine_stays_inside_its_buffers(L, dev, arch):
    """One handle with EVERY caller-supplied buffer in an arena -- a workspace of exactly smd_engine_workspace_bytes(), params,
    wpack, grads, m, v, ema, the FiLM tables, the step counter and the metrics -- through a forward, one loss_backward +
    optimizer_step (and forward_train + backward_from), prepare_sampler, forward_level,
    init_state / load_state, two sample_steps and one more as its two parts: no red zone is touched, and the inference-only calls leave params and
    wpack bitwise unchanged."""
    import smd_amd.lib as lib
    import smd_amd.schedule as S
    from smd_amd.engine import Engine, NetConfig
    B, C = 3, 42
    cfg = NetConfig(architecture=arch, data_channels=C, seq_len=32, num_layers=2, num_heads=8, num_mlp_layers=1, mlp_dims=2048,
                    num_timesteps=T)
    eng = Engine(cfg, "cuda:0")
    eng.init_params(0)
    torch.cuda.synchronize()
    h, Sq, n = eng.h, eng.S, eng.n_params
    shape = (B, C) if arch == "DenseDDPM" else (B, Sq, C)
    r = Run(dev, F.PATTERNS[0])
    g = torch.Generator().manual_seed(3)
    params = r.out("params", (n,), init=eng.params.cpu())
    nw = int(L.smd_engine_wpack_elems(h))
    wpack = r.out("wpack", (nw,), torch.int16, init=torch.zeros(nw, dtype=torch.int16))      # zero padding of the operands: the caller's
    grads, m, v = (r.out(k, (n,), init=torch.zeros(n)) for k in ("grads", "m", "v"))
    ema = r.out("ema", (n,), init=eng.params.cpu())
    step = r.out("step", (1,), torch.int32, init=torch.zeros(1, dtype=torch.int32))
    metrics = r.out("metrics", (4,))
    film = r.out("film", (int(L.smd_engine_film_table_floats(h)),))
    coef_np = S.reverse_coefficient_table(BETAS)
    coef, sqrt_ap = r.inp(torch.from_numpy(coef_np)), r.inp(torch.from_numpy(np.ascontiguousarray(coef_np[:, 6])))
    ape, slot = r.inp(torch.from_numpy(APE)), r.inp(torch.from_numpy(S.collection_slot_table(T)))
    x0 = r.inp(torch.clamp(0.25 * torch.randn(*shape, generator=g), -1, 1))
    level, labels = r.inp(0.1 + 0.9 * torch.rand(B, generator=g)), r.inp(torch.randint(1, T + 1, (B,), generator=g).int())
    eps = r.inp(torch.randn(*shape, generator=g))
    ws_inf_bytes, ws_tr_bytes = (int(L.smd_engine_workspace_bytes(h, B, tr)) for tr in (0, 1))
    ws_inf, ws_tr = r.out("workspace_inference", (ws_inf_bytes,), torch.uint8), r.out("workspace_training", (ws_tr_bytes,), torch.uint8)
    ck(L.smd_engine_bind_params(h, P(params), P(wpack)), "bind_params")
    ck(L.smd_engine_refresh_weights(h, st()), "refresh_weights")
    ck(L.smd_engine_bind_train(h, P(grads), P(m), P(v), P(ema), P(step), P(metrics)), "bind_train")
    ck(L.smd_engine_bind_schedule(h, P(coef), P(sqrt_ap), P(ape), P(film)), "bind_schedule")
    # ---- forward
    ck(L.smd_engine_bind_workspace(h, P(ws_inf), ws_inf_bytes, B, 0, st()), "bind_workspace")
    out = r.out("eps_hat", shape)
    ck(L.smd_engine_forward(h, P(x0), P(level), P(out), st()), "forward")
    # ---- one training step
    ck(L.smd_engine_bind_workspace(h, P(ws_tr), ws_tr_bytes, B, 1, st()), "bind_workspace")
    ck(L.smd_engine_loss_backward(h, P(x0), P(labels), P(eps), 0, 0, 0, 1.0 / (B * Sq * C), 0, st()), "loss_backward")
    hy = lib.TrainHyper(1e-3, 0.98, 10000, 0.9, 0.999, 1e-8, 1.0, 0.999, 1.0)
    ck(L.smd_engine_optimizer_step(h, ctypes.byref(hy), st()), "optimizer_step")
    # ... and value_and_grad over an arbitrary objective on the same workspace (the gradients are written again)
    out_tr = r.out("eps_hat_train", shape)
    ck(L.smd_engine_forward_train(h, P(x0), P(level), P(out_tr), st()), "forward_train")
    ck(L.smd_engine_backward_from(h, P(eps), 0, st()), "backward_from")
    ck(L.smd_engine_join_update(h, st()), "join_update")
    torch.cuda.synchronize()
    after_step = {k: r.outs[k].snapshot() for k in ("params", "wpack")}
    assert int(step) == 1 and bool(torch.isfinite(grads).all()) and bool(torch.isfinite(params).all())
    assert float((params - eng.params).abs().max()) > 0                     # the step moved the weights in the arena, not elsewhere
    # ---- sampler: FiLM tables, then two reverse steps
    ck(L.smd_engine_bind_workspace(h, P(ws_inf), ws_inf_bytes, B, 0, st()), "bind_workspace")
    ck(L.smd_engine_prepare_sampler(h, st()), "prepare_sampler")
    lvl = r.inp(torch.tensor([T // 2], dtype=torch.int32))
    out_lvl = r.out("eps_hat_level", shape)
    ck(L.smd_engine_forward_level(h, P(x0), P(lvl), P(out_lvl), st()), "forward_level")
    x = r.out("x", shape)
    ck(L.smd_engine_init_state(h, P(x), 7, 0, 0, st()), "init_state")
    t_ptr = r.out("t", (1,), torch.int32, init=torch.tensor([T - 1], dtype=torch.int32))
    mp, coll = r.out("metrics_partial", (T, B, 3)), r.out("collection", (41,) + shape)
    io = lib.SampleIO()
    io.x, io.t_ptr, io.seed_lo, io.seed_hi = P(x), P(t_ptr), 5, 0
    io.metrics_partial, io.collection, io.slot_table = P(mp), P(coll), P(slot)
    ck(L.smd_engine_load_state(h, P(x), st()), "load_state")
    for _ in range(2):
        ck(L.smd_engine_sample_step(h, ctypes.byref(io), st()), "sample_step")
    for part in (1, 2):                                                     # a third iteration as its two halves
        ck(L.smd_engine_sample_step_part(h, ctypes.byref(io), part, st()), "sample_step_part")
    got = r.finish()                                                        # every red zone, every input
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("eps_hat_train", "eps_hat_level", "grads"))
    assert int(got["t"]) == T - 4 and bool(torch.isfinite(got["x"]).all()) and bool(torch.isfinite(got["eps_hat"]).all())
    # the FiLM buffer is the tables, every element written, then bf16 scratch of the generator GEMMs (T * 9 * 128 bf16) + 64 floats
    n_tables = got["film"].numel() - (T * 9 * 128 // 2 + 64)
    assert n_tables > 0 and n_tables % (T * 2 * cfg.mlp_dims) == 0 and bool(torch.isfinite(got["film"][:n_tables]).all())
    for k, snap in after_step.items():
        r.outs[k].assert_same(snap, f"{k} after the inference-only calls")
    del eng


@pytest.mark.parametrize("rows", [1, 33])
def test_layernorm_fwd_e4m3(L, dev, rows):
    """D = 1024, one row and a ragged count (33: a second row group with one row): out8 [rows][D], one scale per row, bf16 copy"""
    D = 1024
    g = torch.Generator().manual_seed(11 + rows)
    x = torch.randn(rows, D, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    y = ln64(x.double(), gamma, beta)

    def body(r):
        xD, gD, bD = r.inp(x), r.inp(gamma), r.inp(beta)
        q, s, ob = r.out("q", (rows, D), torch.uint8), r.out("scale", (rows,), torch.int32), r.out("bf16", (rows, D), torch.bfloat16)
        ck(L.smd_layernorm_fwd_e4m3(P(xD), rows, D, P(gD), P(bD), None, None, D, 32, 0, P(q), P(s), P(ob), st()))

    got, _ = both(dev, body)
    assert rel(dequant(got["q"], got["scale"]), y) < 4e-2 and rel(got["bf16"].float(), y) < 4e-3          # test_layernorm_fwd_e4m3
    e_ref = torch.ceil(torch.log2(y.abs().amax(1) / 448.0)).to(torch.int64)
    assert bool(((((got["scale"].to(torch.int64) & 0xFF) - 127) - e_ref).abs() <= 1).all())


@pytest.mark.parametrize("D,t", [(1024, 2), (512, 9)])
def test_layernorm_fwd_lab_table_row(L, dev, D, t):
    """The sampler's FiLM path (include/smd_hip_lab.h): 33 rows (a second row group with one row; no multiple of rows_per_sample,
    which this path ignores), the FiLM row read through a device timestep, in range and clamped to the last table row; bf16 output,
    e4m3 copy with one scale per row (D = 1024, the wide kernel) and the saved statistics; D = 512 is the row kernel."""
    rows, T = 33, 4
    g = torch.Generator().manual_seed(17 + D)
    x = torch.randn(rows, D, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    table = torch.cat([1 + 0.3 * torch.randn(T, D, generator=g), 0.2 * torch.randn(T, D, generator=g)], 1)
    row = min(max(t, 0), T - 1)
    y = O.swish(table[row, :D].double() * ln64(x.double(), gamma, beta) + table[row, D:].double())
    f8 = D == 1024

    def body(r):
        xD, gD, bD, tab = r.inp(x), r.inp(gamma), r.inp(beta), r.inp(table)
        tD = r.inp(torch.tensor([t], dtype=torch.int32))
        ob, stt = r.out("bf16", (rows, D), torch.bfloat16), r.out("stats", (rows, 2))
        q = r.out("q", (rows, D), torch.uint8) if f8 else None
        s = r.out("scale", (rows,), torch.int32) if f8 else None
        ck(L.smd_layernorm_fwd_lab(P(xD), None, rows, D, P(gD), P(bD), P(tab), P(tab[:, D:]), 2 * D, 32, 1, P(ob), P(q), P(s), P(stt),
                                   P(tD), T, st()))

    got, _ = both(dev, body)
    assert rel(got["bf16"].float(), y) < 4e-3                                      # test_layernorm_fwd_bwd
    assert bool(torch.isfinite(got["stats"]).all())
    if f8:
        assert rel(dequant(got["q"], got["scale"]), y) < 4e-2                      # test_layernorm_fwd_e4m3


# ================================================================================================ Langevin update
def langevin_reference(x, grad, z, alpha, coef):
    """fp64 of next = x + alpha grad + coef z and the per-sample sums behind grad_norm / step_norm / noise_norm
    (utils/ebm_utils.py:157-161: the norm over the sequence axis of every column, summed over the columns)"""
    xd, gd, zd = x.double(), grad.double(), z.double()
    norms = lambda t: torch.sqrt((t * t).sum(1) + 1e-10).sum(1)
    return xd + alpha * gd + coef * zd, torch.stack([norms(gd), norms(alpha * gd), norms(coef * zd)], dim=1)


# Tolerances of the two Langevin cases, from the fp32 format: the update is three roundings per element (two products, two adds,
# one of them fused away or not): rel-L2 <= 4 x 2^-24 of terms no larger than the result here -> 1e-6.  A metric is a sum of 32
# squares, a square root, and a sum of 42 of those in fp32: (32 + 42 + 2) x 2^-24 = 4.5e-6 -> 1e-5.
LANGEVIN_X_TOL, LANGEVIN_M_TOL = 1e-6, 1e-5


def test_langevin_step_direct(L, dev):
    import smd_amd.lib as lib
    B, Sq, C, alpha, coef = 5, 32, 42, 0.0123, 0.456
    g = torch.Generator().manual_seed(21)
    x, grad, z = (torch.randn(B, Sq, C, generator=g) for _ in range(3))
    want, wm = langevin_reference(x, grad, z, np.float32(alpha).item(), np.float32(coef).item())

    def body(r):
        gd, zd = r.inp(grad), r.inp(z)
        io = lib.LangevinIO()
        io.x, io.grad, io.z_in = P(r.out("x", (B, Sq, C), init=x)), P(gd), P(zd)
        io.alpha, io.noise_coef = alpha, coef
        io.metrics_partial, io.collect_out = P(r.out("metrics", (B, 3))), P(r.out("collect", (B, Sq, C)))
        ck(L.smd_langevin_step(ctypes.byref(io), B, Sq, C, st()), "smd_langevin_step")

    got, _ = both(dev, body)
    assert rel(got["x"], want) < LANGEVIN_X_TOL and torch.equal(got["collect"], got["x"])
    assert rel(got["metrics"], wm) < LANGEVIN_M_TOL


@pytest.mark.parametrize("k", [1, -1, 4])
def test_langevin_step_table_mode(L, dev, k):
    """row k of metrics_partial, the slot slot_table[k] of the collection, B floats of sigma_out, one word each of level_out and
    k_ptr; k outside [0, n_steps) changes nothing, k_ptr and arrive included"""
    import smd_amd.lib as lib
    B, Sq, C, n_steps = 5, 32, 42, 4
    g = torch.Generator().manual_seed(22)
    x, grad, z = (torch.randn(B, Sq, C, generator=g) for _ in range(3))
    table = torch.tensor([[0.01, 0.1, 0.0, 0.9], [0.02, 0.2, 0.0, 0.8], [0.03, 0.3, 0.0, 0.7], [0.04, 0.4, 0.0, 0.6]])
    slots = torch.tensor([0, 2, -1, 1], dtype=torch.int32)

    def body(r):
        gd, zd, td, sd = r.inp(grad), r.inp(z), r.inp(table), r.inp(slots)
        io = lib.LangevinIO()
        io.x, io.grad, io.z_in = P(r.out("x", (B, Sq, C), init=x)), P(gd), P(zd)
        io.step_table, io.slot_table, io.n_steps = P(td), P(sd), n_steps
        io.k_ptr = P(r.out("k", (1,), torch.int32, init=torch.tensor([k], dtype=torch.int32)))
        io.arrive = P(r.out("arrive", (1,), torch.int32, init=torch.zeros(1, dtype=torch.int32)))
        io.metrics_partial, io.collection = P(r.out("metrics", (n_steps, B, 3))), P(r.out("collection", (3, B, Sq, C)))
        io.sigma_out, io.level_out = P(r.out("sigma", (B,))), P(r.out("level", (1,), torch.int32))
        io.steps_per_level, io.n_levels = 2, 2
        ck(L.smd_langevin_step(ctypes.byref(io), B, Sq, C, st()), "smd_langevin_step")

    valid = 0 <= k < n_steps
    got, got2 = both(dev, body, unwritten=("metrics", "collection") + (() if valid else ("sigma", "level")))
    for res, fill in ((got, F.PATTERNS[0]), (got2, F.PATTERNS[1])):
        poisoned = lambda v: is_poison(v, fill)
        assert int(res["arrive"]) == 0
        if not valid:
            assert torch.equal(res["x"], x) and int(res["k"]) == k
            assert all(poisoned(res[n]) for n in ("metrics", "collection", "sigma", "level"))
            continue
        want, wm = langevin_reference(x, grad, z, float(table[k, 0]), float(table[k, 1]))
        assert rel(res["x"], want) < LANGEVIN_X_TOL and rel(res["metrics"][k], wm) < LANGEVIN_M_TOL
        assert all(poisoned(res["metrics"][j]) for j in range(n_steps) if j != k)
        slot = int(slots[k])
        assert torch.equal(res["collection"][slot], res["x"]) and all(poisoned(res["collection"][j]) for j in range(3) if j != slot)
        assert torch.equal(res["sigma"], torch.full((B,), float(table[k, 3]))) and int(res["level"]) == min((k + 1) // 2, 1)
        assert int(res["k"]) == k + 1
