"""smd_gemm_f32 (csrc/gemm_f32.hip) judged per element through the C ABI, with the criterion of tests/_gemm_f32_ref.py (derivations
there; tests/test_gemm_f32_ref_host.py shows on the CPU that it has room and that every planted fault fails it).

  exact      integer lattices, act = none: the output equals the int64 result bit for bit (tolerance zero; the buffer starts as
             NaN) over M x N x K = 8 x 11 x 12 = 1056 shapes that cross the 32-row and 128-row tile, the 128-column tile, the form
             switch at N = 512 / 513, the stage of 16, the k pair and the group of four of both vector loaders, each with bias and one
             residual mode; on the reduced list again with 4-byte-only alignment (both scalar loaders, both forms), with every leading
             dimension larger than the row (NaN behind the inputs' rows, a sentinel behind the output's) and with out aliasing
             res, which is how the engine updates its residual streams (run_network_f32: g.res = h; g.out = h).
  bitwise    random N(0, 1) data without zeros: a column gives the same bits in the 128 x 128 and in the 32 x 128 form (N = 640 / 128
             and 513 / 512 on the same W with ldw = 640 / 513), K = 47 equals K = 48 with a zero column / row appended, a row gives the
             same bits at M = 1, 33 and 257.
  regimes    selector W, M = 64, K = 128, N = 128 and 640, both activations, with and without a residual: every element within the
             derived bound, equal to z / 0 / fl(v + res) in the exact places, finite everywhere.
  dense      (96, 146, 128) and (160, 128, 640), |z| up to 8: the Higham bound on z carried through the activation.
  noise      smd_noise_embed_f32 at odd channel counts (the trailing zero column) with ld_out > channels.

Measured on the MI355X: all 1128 lattice problems exact, the 1056-launch sweep in 0.4 s of wall time; worst |err| / bound outside the
exact places (where that figure is 1 / SECOND by construction) and without a residual: GELU 0.490, swish 0.575 through the
selector, 0.147 and 0.281 with dense W ("Per-element criterion of the Dense GEMM").
"""
import time

import pytest
import torch

import _gemm_f32_ref as R
import ddpm_oracle as O

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENTINEL = -777.25


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def launch(L, A, W, M, N, K, bias, act, res, row_mod, out):
    """A, W, res, out are 2-d views (their stride(0) is the leading dimension)"""
    import smd_amd.lib as lib
    lib.check(L.smd_gemm_f32(P(A), A.stride(0), P(W), W.stride(0), M, N, K, P(bias), R.ACT[act], P(res),
                             0 if res is None else res.stride(0), row_mod, P(out), out.stride(0), st()), "smd_gemm_f32")


def padded(t, ld, dev, fill=NAN, offset=0, guard_rows=0):
    """a copy of the 2-d tensor t with leading dimension ld, `offset` elements behind a 16-byte boundary, `fill` in the padding"""
    rows, cols = t.shape
    buf = torch.full((offset + (rows + guard_rows) * ld,), fill, device=dev, dtype=torch.float32)
    v = buf[offset:].view(rows + guard_rows, ld)
    v[:rows, :cols] = t.to(dev)
    return buf, v[:rows, :cols]


def bits(t):
    return t.contiguous().view(torch.int32)


def mode_args(lat, M, mode, dev):
    if mode == "none":
        return None, 0
    return (lat["r"][:M] if mode == "full" else lat["r"][:mode]).float().to(dev), 0 if mode == "full" else mode


def test_lattice_sweep_is_exact_bit_for_bit(L, dev):
    cases = R.sweep_cases()
    groups = {}
    for M, N, K, mode in cases:
        groups.setdefault((N, K), []).append((M, mode))
    bad = torch.zeros(len(cases), dtype=torch.int64, device=dev)
    order = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for (N, K), grp in groups.items():
        lat = R.lattice(N, K)                                # operands once per (N, K); M slices the rows
        A, W, b = lat["A"].float().to(dev), lat["W"].float().to(dev), lat["b"].float().to(dev)
        for M, mode in grp:
            res, row_mod = mode_args(lat, M, mode, dev)
            out = torch.full((M, N), NAN, device=dev)
            launch(L, A[:M], W, M, N, K, b, "none", res, row_mod, out)
            want = R.lattice_want(lat, M, mode).float().to(dev)                  # int64 on the host; exact in fp32
            bad[len(order)] = (bits(out) != bits(want)).sum()
            order.append((M, N, K, mode))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    bad = bad.cpu()
    wrong = [(c, int(n)) for c, n in zip(order, bad) if n]
    print(f"exact sweep: {len(order)} lattice problems, {len(wrong)} with a wrong element, {wall:.2f} s wall time")
    assert len(order) == 1056 and not wrong, wrong[:20]


def test_lattice_is_exact_with_scalar_loaders_padded_leading_dimensions_and_out_aliasing_res(L, dev):
    n = 0
    for i, (M, N, K) in enumerate(R.reduced_cases()):
        lat = R.lattice(N, K)
        A, W, b = lat["A"][:M].float(), lat["W"].float(), lat["b"].float().to(dev)
        modes = [m for m in R.MODES if R.mode_ok(M, m)]
        # (a) A and W one element behind a 16-byte boundary: both scalar loaders, in the form that N selects
        mode = modes[i % len(modes)]
        _, Am = padded(A, K, dev, offset=1)
        _, Wm = padded(W, N, dev, offset=1)
        assert Am.data_ptr() % 16 == 4 and Wm.data_ptr() % 16 == 4
        res, row_mod = mode_args(lat, M, mode, dev)
        out = torch.full((M, N), NAN, device=dev)
        launch(L, Am, Wm, M, N, K, b, "none", res, row_mod, out)
        assert torch.equal(bits(out), bits(R.lattice_want(lat, M, mode).float().to(dev))), ("unaligned", M, N, K, mode)
        # (b) every leading dimension larger than the row: NaN behind the rows of A, W and res, a sentinel behind those of out and
        #     in one row past the last.  lda and ldw grow by 4, so the 16-byte loaders stay in use where K / N allow them.
        mode = [m for m in modes if m != "none"][i % (len(modes) - 1)]
        _, Ap = padded(A, K + 4, dev)
        _, Wp = padded(W, N + 4, dev)
        r = lat["r"][:M].float() if mode == "full" else lat["r"][:mode].float()
        _, rp = padded(r, N + 5, dev)
        obuf, op = padded(torch.full((M, N), NAN), N + 3, dev, fill=SENTINEL, guard_rows=1)
        launch(L, Ap, Wp, M, N, K, b, "none", rp, 0 if mode == "full" else mode, op)
        assert torch.equal(bits(op), bits(R.lattice_want(lat, M, mode).float().to(dev))), ("padded", M, N, K, mode)
        full = obuf.view(M + 1, N + 3)
        assert bool((full[:M, N:] == SENTINEL).all()) and bool((full[M] == SENTINEL).all()), ("padding written", M, N, K)
        # (c) out aliases res, as in the engine's residual updates (row_mod = 0, ld_res = ld_out)
        io = lat["r"][:M].float().to(dev).contiguous()
        launch(L, Ap, Wp, M, N, K, b, "none", io, 0, io)
        assert torch.equal(bits(io), bits(R.lattice_want(lat, M, "full").float().to(dev))), ("aliased", M, N, K)
        n += 3
    torch.cuda.synchronize()
    print(f"reduced list: {n} lattice problems exact (unaligned, padded, aliased)")


def _randn_nonzero(g, *shape):
    x = torch.randn(*shape, generator=g)
    return torch.where(x == 0, torch.ones_like(x), x)


def test_a_column_a_row_and_a_zero_k_tail_give_the_same_bits_in_either_form(L, dev):
    g = torch.Generator().manual_seed(5)
    run = lambda A, W, b, act, out: launch(L, A, W, A.shape[0], W.shape[1], A.shape[1], b, act, None, 0, out)
    for big, small, K in ((640, 128, 146), (513, 512, 47)):
        A, W, b = _randn_nonzero(g, 160, K).to(dev), (_randn_nonzero(g, K, big) / K ** 0.5).to(dev), _randn_nonzero(g, big).to(dev)
        for act in ("none", "gelu", "swish"):
            o_big, o_small = torch.full((160, big), NAN, device=dev), torch.full((160, small), NAN, device=dev)
            run(A, W, b, act, o_big)                          # 128 x 128 form
            run(A, W[:, :small], b, act, o_small)             # 32 x 128 form on the same memory: ldw = big
            assert W[:, :small].stride(0) == big and R.form_rows(big) == 128 and R.form_rows(small) == 32
            assert torch.equal(bits(o_big[:, :small]), bits(o_small)), (big, small, act)
    # K = 47 against K = 48 with an explicit zero column of A and zero row of W
    A, W, b = _randn_nonzero(g, 129, 47), _randn_nonzero(g, 47, 640), _randn_nonzero(g, 640)
    A48, W48 = torch.cat([A, torch.zeros(129, 1)], 1).to(dev), torch.cat([W, torch.zeros(1, 640)], 0).to(dev)
    A, W, b = A.to(dev), W.to(dev), b.to(dev)
    for N in (640, 131):
        o47, o48 = torch.full((129, N), NAN, device=dev), torch.full((129, N), NAN, device=dev)
        run(A, W[:, :N], b[:N], "gelu", o47)
        run(A48, W48[:, :N], b[:N], "gelu", o48)
        assert torch.equal(bits(o47), bits(o48)), N
    # a row at M = 1, 33 and 257
    A = _randn_nonzero(g, 257, 47).to(dev)
    for N in (640, 131):
        outs = {}
        for M in (1, 33, 257):
            outs[M] = torch.full((M, N), NAN, device=dev)
            run(A[:M], W[:, :N], b[:N], "swish", outs[M])
        assert torch.equal(bits(outs[1]), bits(outs[257][:1])) and torch.equal(bits(outs[33]), bits(outs[257][:33])), N
    torch.cuda.synchronize()


WORST = {}


@pytest.mark.parametrize("act", ["gelu", "swish"])
def test_activation_regimes_through_the_selector(L, dev, act):
    worst = {}
    for name, N, part in R.selector_list():
        for with_res in (False, True):
            pr = R.selector_problem(name, N, part, with_res)
            A, W, b = pr["A"].to(dev), pr["W"].to(dev), pr["b"].to(dev)
            res = None if pr["res"] is None else pr["res"].to(dev)
            out = torch.full((R.SEL_M, N), NAN, device=dev)
            launch(L, A, W, R.SEL_M, N, R.SEL_K, b, act, res, 0, out)
            r, inner, finite, exact = R.judge(out, pr["z"], act, pr["res"])
            worst[(name, with_res)] = max(worst.get((name, with_res), 0.0), inner)
            assert finite, (name, N, part, with_res)
            assert exact, (name, N, part, with_res, "not z / 0 / fl(v + res) in an exact place")
            assert r <= 1.0, (name, N, part, with_res, r)
    # without a residual the figure measures the activation's arithmetic; with one the final addition's own rounding leads, and a
    # correctly rounded sum just above a power of two sits at 1 - 2^-23 of its bound U |result| whatever the kernel does
    for with_res in (False, True):
        w = {k[0]: v for k, v in worst.items() if k[1] == with_res}
        print(f"{act}, selector W, {'with' if with_res else 'no'} residual: worst |err| / bound outside the exact places {max(w.values()):.3f} ("
              + ", ".join(f"{k} {v:.3f}" for k, v in w.items()) + ")")


@pytest.mark.parametrize("act", ["gelu", "swish"])
@pytest.mark.parametrize("M,K,N", R.DENSE_SHAPES)
def test_dense_w_with_an_activation_per_element(L, dev, M, K, N, act):
    pr = R.dense_problem(M, K, N)
    out = torch.full((M, N), NAN, device=dev)
    launch(L, pr["A"].to(dev), pr["W"].to(dev), M, N, K, pr["b"].to(dev), act, None, 0, out)
    r, _, finite, _ = R.judge(out, pr["z"], act, None, R.z_err(pr["A"], pr["W"], pr["b"], K))
    print(f"{act}, dense {M}x{K}x{N} ({R.form_rows(N)}-row form), |z| up to {float(pr['z'].abs().max()):.2f}: worst |err| / bound {r:.3f}")
    assert finite and r <= 1.0


@pytest.mark.parametrize("F", [5, 129])
def test_noise_embed_f32_at_odd_channel_counts(L, dev, F):
    """The path that writes the trailing zero column.  Tolerance: the formula of test_noise_embed_f32 (tests/test_gpu_fp32_kernels.py),
    2.74 ulp of the largest argument 5000 s plus 1e-6; the zero column is exactly 0 and the padding behind a row is untouched."""
    import smd_amd.lib as lib
    s = torch.tensor([1.0, 0.9999995, 0.6, 0.0814, 0.3, 1e-3], device=dev)
    n, ld = s.numel(), F + 3
    out = torch.full((n + 1, ld), SENTINEL, device=dev)
    lib.check(L.smd_noise_embed_f32(P(s), n, F, P(out), ld, st()), "smd_noise_embed_f32")
    torch.cuda.synchronize()
    sc = s.double().cpu()
    want = O.noise_encoding(sc[:, None], F)
    got = out.double().cpu()
    err = (got[:n, :F] - want).abs().max(dim=1).values
    tol = 2.74 * 2.0 ** (torch.floor(torch.log2(5000.0 * sc)) - 23) + 1e-6
    print(f"noise_embed_f32 channels {F}: max abs error / tolerance  " + "  ".join(f"{float(a):.4g}: {float(e):.2e} / {float(t):.2e}" for a, e, t in zip(sc, err, tol)))
    assert bool((err <= tol).all())
    assert bool((got[:n, F - 1] == 0).all()) and bool((got[:n, F:] == SENTINEL).all()) and bool((got[n] == SENTINEL).all())
