"""The encoder MLP half-layer kernels, element by element, across GELU regimes (tests/_mlp_ref.py holds the reference, the derivation
of the bound, the regimes, the selector weights and the planted faults; tests/test_mlp_ref_host.py shows on the CPU that the bound has
room and that each planted fault leaves it).  Every assertion is |err| <= bound at every output element, or bitwise equality;
nothing is fitted to GPU output.

Each stage is judged from the kernel's OWN previous observable stage: the fused kernel's a2 from h, its z1 and u from its a2, its
h_out from its u; the backward's u and dz from a2 and dh, each da2 tile from its dz; the hidden-split forward's four tiles, one by
one, from a2 (u is not observable there: the selector W2 phases give the per-unit view).  Shapes are the smallest that reach each
form: 1 / 2 / 4 samples per group, a group that is not the first, 1 / 3 / 4 / 16 chunks per quarter (12 / 16 / 64 in the backward),
hidden width 8192 once, the four-wave fused kernel, the eight-wave hidden-split forward and the fragment re-reading backward.
The last test prints the table of worst |err| / bound per kernel and regime that DESIGN.md quotes.
"""
import time

import pytest
import torch

import _mlp_ref as R

pytestmark = pytest.mark.gpu

ELAPSED = [0.0]
WORST = {}                  # (kernel, regime) -> worst |err| / bound
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


@pytest.fixture(autouse=True)
def _timed():
    t = time.perf_counter()
    yield
    for p in R._PROBLEMS.values():           # the float64 intermediates of the shared problems: rebuilt on demand
        p["_base"].clear()
    ELAPSED[0] += time.perf_counter() - t


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def ck(rc):
    import smd_amd.lib as lib
    lib.check(rc)


class variant:
    """mlp_variant for the duration of a block, 0 again afterwards"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        import smd_amd.lib as lib
        lib.set_tuning("mlp_variant", self.v)

    def __exit__(self, *exc):
        import smd_amd.lib as lib
        lib.set_tuning("mlp_variant", 0)


def judge(kernel, regime, got, ref, bound, what=""):
    r = R.worst_ratio(got, ref, bound)
    WORST[(kernel, regime)] = max(WORST.get((kernel, regime), 0.0), r)
    print(f"{kernel} {regime} {what}: worst |err| / bound {r:.3f}")
    assert r <= 1.0, f"{kernel} {regime} {what}: an element is at {r:.3g} of its bound"
    return r


def nan_bf16(dev, *shape):
    return torch.full(shape, NAN, dtype=torch.bfloat16, device=dev)


# ------------------------------------------------------------------------------------------------ 1. hidden-split forward + ln128_parts
def run_hs_fwd(L, dev, pr):
    rows, M = pr["a2"].shape[0], pr["W1"].shape[1]
    a2, h, W1t, b1 = pr["a2"].to(dev), pr["h"].to(dev), pr["W1"].t().contiguous().to(dev), pr["b1"].to(dev)
    W2t, b2 = pr["W2"].t().contiguous().to(dev), pr["b2"].to(dev)
    part = torch.full((4, rows, 128), NAN, device=dev)
    ck(L.smd_mlp_block_fwd_hs(P(a2), P(h), rows, P(W1t), P(b1), P(W2t), P(b2), M, P(part), st()))
    torch.cuda.synchronize()
    return part


def hs_fwd_case(L, dev, kernel, name, rows, M, phases):
    base = R.problem(name, rows, M)
    for ph in phases:
        pr = base if ph is None else R.with_selector_w2(base, ph)
        part = run_hs_fwd(L, dev, pr).cpu()
        val, bnd = R.fwd_tiles(pr)
        w = "dense W2" if ph is None else f"selector W2 phase {ph}"
        assert bool(torch.isfinite(part).all()), f"{kernel} {name} rows={rows} M={M} {w}: not finite"
        for q in range(4):
            judge(f"{kernel}: tile q", name, part[q], val[q], bnd[q], f"rows={rows} M={M} {w} q={q}")
        if ph is not None and name in ("neg_sat", "pos_sat"):
            # one live unit per element: exactly +-2^j * (-0) in quarters 1 .. 3 of neg_sat, exactly +-2^j bf16(z) of pos_sat
            S = pr["W2"].double()
            z = R.base_quantities(pr)["z"]
            for q in range(1, 4):
                sl = R.quarter(M, q)
                want = (torch.zeros_like(z[:, sl]) if name == "neg_sat" else R.bf(z[:, sl]).double()) @ S[sl]
                assert torch.equal(part[q].double(), want), f"{kernel} {name} rows={rows} M={M} {w} q={q}: not exact"
    return base


HS_ROWS, HS_M = (32, 64, 96, 128, 384), (512, 1024, 1536, 2048)


@pytest.mark.parametrize("M", HS_M)
@pytest.mark.parametrize("rows", HS_ROWS)
def test_hs_fwd_every_tile_in_every_regime(L, dev, rows, M):
    for name in R.Z_REGIMES:
        hs_fwd_case(L, dev, "mlp_block_fwd_hs", name, rows, M, list(range(R.n_phases(M))) + ([None] if name == "mixed" else []))
    hs_fwd_case(L, dev, "mlp_block_fwd_hs", "random", rows, M, [None, 0])


def test_hs_fwd_hidden_8192(L, dev):
    hs_fwd_case(L, dev, "mlp_block_fwd_hs", "mixed", 128, 8192, list(range(R.n_phases(8192))))
    hs_fwd_case(L, dev, "mlp_block_fwd_hs", "random", 128, 8192, [None])


@pytest.mark.parametrize("M", (1536, 2048))
@pytest.mark.parametrize("rows", (128, 384))
def test_hs_fwd_eight_wave_form_and_a_second_launch_are_bitwise_equal(L, dev, rows, M):
    for name in ("mixed", "random", "core"):
        base = R.problem(name, rows, M)
        for pr in (base, R.with_selector_w2(base, R.n_phases(M) - 1)):
            a, b = run_hs_fwd(L, dev, pr), run_hs_fwd(L, dev, pr)
            with variant(5):
                c = run_hs_fwd(L, dev, pr)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name} rows={rows} M={M}: two launches differ"
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), f"{name} rows={rows} M={M}: the eight-wave form differs"
            val, bnd = R.fwd_tiles(pr)
            for q in range(4):
                judge("mlp_block_fwd_hs (eight waves): tile q", name, c[q].cpu(), val[q], bnd[q], f"rows={rows} M={M} q={q}")


@pytest.mark.parametrize("rows", (32, 64, 384))
def test_hs_fwd_second_launch_bitwise_for_smaller_groups(L, dev, rows):
    pr = R.problem("random", rows, 1024)
    assert torch.equal(run_hs_fwd(L, dev, pr).view(torch.int32), run_hs_fwd(L, dev, pr).view(torch.int32))


@pytest.mark.parametrize("regime", R.LN_REGIMES)
@pytest.mark.parametrize("rows", (32, 96, 384))
def test_ln128_parts_sum_and_layernorm(L, dev, rows, regime):
    """x_out bitwise (p0 + p1) + (p2 + p3); ln_out inside ln_fwd_bound of the kernel's own x_out; the null-x_out and null-ln_out
    forms; a padded part_stride (the gap NaN: never read)"""
    x = R.ln_rows(regime, rows)
    g = torch.Generator().manual_seed(rows)
    gamma, beta = 1 + 0.2 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    noise = torch.randn(3, rows, 128, generator=g) * 0.3
    parts = torch.stack([x * 0.5, x * 0.25, x * 0.125, x * 0.125]) if regime == "const" else torch.stack([x - noise.sum(0), noise[0], noise[1], noise[2]])
    for pad in (0, 64):
        stride = rows * 128 + pad
        buf = torch.full((4 * stride,), NAN)
        for k in range(4):
            buf[k * stride:k * stride + rows * 128] = parts[k].reshape(-1)
        pD, gD, bD = buf.to(dev), gamma.to(dev), beta.to(dev)
        xo, xo2 = torch.full((rows, 128), NAN, device=dev), torch.full((rows, 128), NAN, device=dev)
        lo, lo2 = nan_bf16(dev, rows, 128), nan_bf16(dev, rows, 128)
        ck(L.smd_ln128_parts(P(pD), stride, rows, P(gD), P(bD), P(xo), P(lo), st()))
        ck(L.smd_ln128_parts(P(pD), stride, rows, P(gD), P(bD), P(xo2), None, st()))
        ck(L.smd_ln128_parts(P(pD), stride, rows, P(gD), P(bD), None, P(lo2), st()))
        torch.cuda.synchronize()
        want_x = (parts[0] + parts[1]) + (parts[2] + parts[3])
        assert torch.equal(xo.cpu().view(torch.int32), want_x.view(torch.int32)) and torch.equal(xo2.view(torch.int32), xo.view(torch.int32))
        assert torch.equal(lo.view(torch.int16), lo2.view(torch.int16))
        want, e = R.ln_fwd_bound(xo.cpu(), gamma, beta)
        judge("ln128_parts: ln_out from its x_out", "LN " + regime, lo.cpu(), want, e, f"rows={rows} pad={pad}")
        if regime == "const":
            assert torch.equal(xo.cpu()[0::4], x[0::4]) and torch.equal(lo.cpu()[0::4], R.bf(beta).expand(rows // 4, 128))      # variance 0: beta, exactly


def test_hs_fwd_then_ln128_parts_with_a_padded_stride(L, dev):
    rows, M, pad = 96, 1536, 128
    pr = R.problem("random", rows, M)
    part = run_hs_fwd(L, dev, pr)
    stride = rows * 128 + pad
    buf = torch.full((4, stride), NAN, device=dev)
    buf[:, :rows * 128] = part.view(4, -1)
    g = torch.Generator().manual_seed(5)
    gamma, beta = 1 + 0.2 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    gD, bD = gamma.to(dev), beta.to(dev)
    xo, lo = torch.full((rows, 128), NAN, device=dev), nan_bf16(dev, rows, 128)
    ck(L.smd_ln128_parts(P(buf), stride, rows, P(gD), P(bD), P(xo), P(lo), st()))
    torch.cuda.synchronize()
    assert torch.equal(xo, (part[0] + part[1]) + (part[2] + part[3]))
    want, e = R.ln_fwd_bound(xo.cpu(), gamma, beta)
    judge("ln128_parts: ln_out from its x_out", "random", lo.cpu(), want, e, f"rows={rows} after mlp_block_fwd_hs")


# ------------------------------------------------------------------------------------------------ 2. recompute backward
def run_hs_bwd(L, dev, pr):
    rows, M = pr["a2"].shape[0], pr["W1"].shape[1]
    a2, dh, W1t = pr["a2"].to(dev), pr["dh"].to(dev), pr["W1"].t().contiguous().to(dev)
    W2p, W1p, b1 = pr["W2b"].contiguous().to(dev), pr["W1d"].t().contiguous().to(dev), pr["b1"].to(dev)      # [M][128], [128][M]
    u, dz, part = nan_bf16(dev, rows, M), nan_bf16(dev, rows, M), torch.full((4, rows, 128), NAN, device=dev)
    ck(L.smd_mlp_block_bwd_hs(P(a2), P(dh), rows, P(W1t), P(W2p), P(W1p), P(b1), M, P(u), P(dz), P(part), st()))
    torch.cuda.synchronize()
    return u, dz, part


def hs_bwd_case(L, dev, name, rows, M, ph):
    base = R.problem(name, rows, M)
    pr = base if ph is None else R.with_selector_w2(base, ph)
    u, dz, part = run_hs_bwd(L, dev, pr)
    with variant(9):
        u9, dz9, part9 = run_hs_bwd(L, dev, pr)
    what = f"rows={rows} M={M} " + ("dense" if ph is None else f"selector phase {ph}")
    assert torch.equal(u.view(torch.int16), u9.view(torch.int16)) and torch.equal(dz.view(torch.int16), dz9.view(torch.int16)) \
        and torch.equal(part.view(torch.int32), part9.view(torch.int32)), f"{name} {what}: the fragment re-reading form differs"
    u, dz, part = u.cpu(), dz.cpu(), part.cpu()
    assert bool(torch.isfinite(u.float()).all()) and bool(torch.isfinite(dz.float()).all()) and bool(torch.isfinite(part).all()), f"{name} {what}: not finite"
    ur, ub, dzr, dzb, du, z = R.bwd_u_dz(pr)
    judge("mlp_block_bwd_hs: u", name, u, ur, ub, what)
    judge("mlp_block_bwd_hs: dz", name, dz, dzr, dzb, what)
    val, bnd = R.da2_tiles_from_dz(dz, pr["W1d"], M)
    for q in range(4):
        judge("mlp_block_bwd_hs: da2 tile q from its dz", name, part[q], val[q], bnd[q], f"{what} q={q}")
    if name != "random":
        lo, hi = z <= -20.0, z >= 30.0
        uf, df = u.float(), dz.float()
        assert bool((uf[lo] == 0).all()) and bool(torch.signbit(uf[lo]).all()) and bool((df[lo] == 0).all()), f"{name} {what}: z <= -20 must give -0 and 0"
        assert torch.equal(u[hi], R.bf(z)[hi]), f"{name} {what}: z >= 30 must give u = bf16(z)"
        if ph is not None:                                  # du = +-2^j dh exactly: gelu' exactly 1
            assert torch.equal(dz[hi], R.bf(du)[hi]), f"{name} {what}: z >= 30 must give gelu' = 1"
        if name == "dcross":                                # the sign of dz wherever the reference is further from 0 than the bound
            sure = dzr.abs() > dzb
            assert bool((torch.sign(df.double()[sure]) == torch.sign(dzr[sure])).all())
            print(f"   dcross: sign of dz determined at {float(sure.double().mean()):.2f} of the elements, gelu' in [{float(R.gelu_grad(z).min()):.2e}, {float(R.gelu_grad(z).max()):.2e}]")


@pytest.mark.parametrize("M", (512, 1536, 2048))
@pytest.mark.parametrize("rows", (128, 384))
def test_hs_bwd_u_dz_and_every_da2_tile_in_every_regime(L, dev, rows, M):
    for i, name in enumerate(R.Z_REGIMES):
        for ph in (range(R.n_phases(M)) if name == "mixed" else [i % R.n_phases(M)]):
            hs_bwd_case(L, dev, name, rows, M, ph)
    hs_bwd_case(L, dev, "random", rows, M, None)
    hs_bwd_case(L, dev, "mixed", rows, M, None)


def test_hs_bwd_hidden_8192(L, dev):
    hs_bwd_case(L, dev, "mixed", 128, 8192, 15)
    hs_bwd_case(L, dev, "random", 128, 8192, None)


# ------------------------------------------------------------------------------------------------ 3. the fused kernel
FUSED = (("unit", "random"), ("unit", "sel0"), ("unit", "sel6"), ("offset", "random"), ("offset", "sel0"), ("const", "sel0"), ("const", "sel6"))


def fused_problem(ln, wk, rows, M):
    g = torch.Generator().manual_seed(13 * rows + M + len(ln) + 7 * len(wk))
    h = R.ln_rows(ln, rows)
    gamma, beta = 1 + 0.2 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    W2, b2 = R.bf(torch.randn(M, 128, generator=g) / M ** 0.5), 0.1 * torch.randn(128, generator=g)
    if wk == "random":
        W1, b1 = R.bf(torch.randn(128, M, generator=g) * 0.09), 0.1 * torch.randn(M, generator=g)
    else:                                                   # z = 2^k a2[PI(h)] + b1 exactly: |z| <~ 4 (sel0), up to ~250 of both signs (sel6)
        hid = torch.arange(M)
        k = torch.full((M,), 0 if wk == "sel0" else 6, dtype=torch.int64)
        b1v = torch.tensor([0.0, 2.0 ** -9, -2.0 ** -7, 3 * 2.0 ** -12], dtype=R.F64)[hid % 4] if wk == "sel0" else torch.zeros(M, dtype=R.F64)
        W1, b1 = R.selector_w1(M, k, b1v)
        if ln == "const":
            beta = torch.zeros(128)                         # the constant rows give a2 = 0 exactly: z = b1
    return dict(h=h, gamma=gamma, beta=beta, W1=W1, b1=b1, W2=W2, b2=b2)


def run_fused(L, dev, pr, saves, inplace=False):
    rows, M = pr["h"].shape[0], pr["W1"].shape[1]
    hD, gD, bD = pr["h"].to(dev), pr["gamma"].to(dev), pr["beta"].to(dev)
    W1t, b1D, W2t, b2D = pr["W1"].t().contiguous().to(dev), pr["b1"].to(dev), pr["W2"].t().contiguous().to(dev), pr["b2"].to(dev)
    out = hD.clone() if inplace else torch.full((rows, 128), NAN, device=dev)
    src = out if inplace else hD
    sa, sz, su = (nan_bf16(dev, rows, 128), nan_bf16(dev, rows, M), nan_bf16(dev, rows, M)) if saves else (None, None, None)
    ck(L.smd_mlp_block_fwd(P(src), P(out), rows, P(gD), P(bD), P(W1t), P(b1D), P(W2t), P(b2D), M, P(sa), P(sz), P(su), st()))
    torch.cuda.synchronize()
    return out, sa, sz, su


def fused_case(L, dev, kernel, ln, wk, rows, M):
    pr = fused_problem(ln, wk, rows, M)
    name = f"LN {ln}, W1 {wk}"
    what = f"rows={rows} M={M}"
    out, sa, sz, su = run_fused(L, dev, pr, True)
    bare, _, _, _ = run_fused(L, dev, pr, False)
    inpl, _, _, _ = run_fused(L, dev, pr, False, inplace=True)
    assert torch.equal(out.view(torch.int32), bare.view(torch.int32)), f"{kernel} {name} {what}: h_out differs between the saving and the plain form"
    assert torch.equal(out.view(torch.int32), inpl.view(torch.int32)), f"{kernel} {name} {what}: h_out differs in place"
    out, sa, sz, su = out.cpu(), sa.cpu(), sz.cpu(), su.cpu()
    for t in (out, sa.float(), sz.float(), su.float()):
        assert bool(torch.isfinite(t).all()), f"{kernel} {name} {what}: not finite"
    a2, e = R.ln_fwd_bound(pr["h"], pr["gamma"], pr["beta"])
    judge(f"{kernel}: a2 from h", name, sa, a2, e, what)
    val, e = R.fused_z1_from_a2(sa, pr["W1"], pr["b1"])
    judge(f"{kernel}: z1 from its a2", name, sz, val, e, what)
    val, e = R.fused_u_from_a2(sa, pr["W1"], pr["b1"])
    judge(f"{kernel}: u from its a2", name, su, val, e, what)
    val, e = R.fused_hout_from_u(su, pr["W2"], pr["b2"], pr["h"])
    judge(f"{kernel}: h_out from its u", name, out, val, e, what)
    if wk != "random":
        z = sa.double() @ pr["W1"].double() + pr["b1"].double()                # exact in the kernel: one product, representable
        assert torch.equal(sz, R.bf(z)), f"{kernel} {name} {what}: z1 is not bf16 of the exact z"
        lo, hi = z <= -20.0, z >= 30.0
        uf = su.float()
        assert bool((uf[lo] == 0).all()) and bool(torch.signbit(uf[lo]).all()) and torch.equal(su[hi], R.bf(z)[hi]), f"{kernel} {name} {what}: saturated u"
        print(f"   z in [{float(z.min()):.4g}, {float(z.max()):.4g}], {int(lo.sum())} at or below -20, {int(hi.sum())} at or above 30, {int((z == 0).sum())} zeros")
        if ln == "const":
            assert bool((sa[0::4].float() == 0).all()) and bool((z[0::4] == pr["b1"].double()).all())
        if wk == "sel6":
            assert int(lo.sum()) > 0 and int(hi.sum()) > 0


@pytest.mark.parametrize("M", (128, 384, 2048))
@pytest.mark.parametrize("rows", (32, 96, 160))
def test_fused_forward_stage_by_stage(L, dev, rows, M):
    for ln, wk in FUSED:
        fused_case(L, dev, "mlp_block_fwd", ln, wk, rows, M)


@pytest.mark.parametrize("M", (128, 384, 2048))
@pytest.mark.parametrize("rows", (32, 160))
def test_fused_forward_four_wave_form(L, dev, rows, M):
    with variant(4):
        for ln, wk in FUSED:
            fused_case(L, dev, "mlp_block_fwd (four waves)", ln, wk, rows, M)


def test_fused_forward_hidden_8192(L, dev):
    fused_case(L, dev, "mlp_block_fwd", "unit", "random", 32, 8192)
    fused_case(L, dev, "mlp_block_fwd", "unit", "sel6", 32, 8192)
    with variant(4):
        fused_case(L, dev, "mlp_block_fwd (four waves)", "unit", "sel0", 32, 8192)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_unsupported_shapes_are_refused_and_nothing_is_written(L, dev):
    rows_max, M_max = 128, 8320
    f = torch.zeros(rows_max * 128, device=dev)
    v = torch.zeros(M_max, device=dev)
    b = torch.zeros(M_max * 128, dtype=torch.bfloat16, device=dev)
    act = torch.zeros(rows_max * 128, dtype=torch.bfloat16, device=dev)
    out = torch.full((rows_max * 128,), NAN, device=dev)
    part = torch.full((4 * rows_max * 128,), NAN, device=dev)
    su, sz, sa = nan_bf16(dev, rows_max * M_max), nan_bf16(dev, rows_max * M_max), nan_bf16(dev, rows_max * 128)
    fused = lambda rows, M: L.smd_mlp_block_fwd(P(f), P(out), rows, P(v), P(v), P(b), P(v), P(b), P(v), M, P(sa), P(sz), P(su), st())
    fwd = lambda rows, M: L.smd_mlp_block_fwd_hs(P(act), P(f), rows, P(b), P(v), P(b), P(v), M, P(part), st())
    bwd = lambda rows, M: L.smd_mlp_block_bwd_hs(P(act), P(act), rows, P(b), P(b), P(b), P(v), M, P(su), P(sz), P(part), st())
    for what, rc in (("fused rows 48", fused(48, 512)), ("fwd_hs rows 48", fwd(48, 512)), ("bwd_hs rows 48", bwd(48, 512)),
                     ("bwd_hs rows 64", bwd(64, 512)), ("fwd_hs M 640", fwd(128, 640)), ("bwd_hs M 640", bwd(128, 640)),
                     ("fused M 8320", fused(32, 8320)), ("fwd_hs M 8320", fwd(128, 8320)), ("bwd_hs M 8320", bwd(128, 8320))):
        assert rc < 0, f"{what}: accepted"
    with pytest.raises(ValueError):
        ck(fwd(48, 512))
    torch.cuda.synchronize()
    for t in (out, part, su.float(), sz.float(), sa.float()):
        assert bool(torch.isnan(t).all())


# ------------------------------------------------------------------------------------------------ the record
def test_zz_print_the_table_of_worst_ratios():
    """A record, not a check of its own: every ratio was asserted where it was measured.  It prints what the tests that ran before it
    in this process left in WORST (nothing when it is selected alone)."""
    cols = sorted({r for _, r in WORST}, key=lambda r: (R.REGIMES.index(r) if r in R.REGIMES else 100, r))
    print("\nworst |err| / bound per kernel and regime:")
    print("| kernel | " + " | ".join(cols) + " |")
    print("|---|" + "---|" * len(cols))
    for k in sorted({k for k, _ in WORST}):
        print(f"| {k} | " + " | ".join("" if (k, r) not in WORST else f"{WORST[(k, r)]:.2f}" for r in cols) + " |")
    print(f"sum of this file's test times: {ELAPSED[0]:.1f} s")
    assert all(v <= 1.0 for v in WORST.values())
