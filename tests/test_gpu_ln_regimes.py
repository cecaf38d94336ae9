"""The LayerNorm kernels of csrc/norm.hip, element by element, across row-statistic regimes (tests/_ln_ref.py holds the float64 model,
the derivation of the bounds, the regimes and the planted faults; tests/test_ln_ref_host.py shows on the CPU that the bounds have
room and that each planted fault leaves them).  Every assertion is |err| <= bound at every element of every output (the saved rstd:
inside its interval), an admissible e4m3 row exponent, an untouched guard byte, or bitwise equality; nothing is fitted to GPU output.

Every row group of every shape holds several regimes (unit, offset, edge, tiny, zero, three constants that are no power of two, a
nearly constant row, an outlier, 2^40), every FiLM sample one of near 1 / exactly 0 / negative / saturating swish at +-30 / +-100, the
dout rows one of unit / zero / 2^20 / one term per column.  Outputs start as NaN inside guarded arenas (tests/_footprint.py): an
element that is not written fails its bound, a write past the last row fails the guard.

Forms: the row kernel at every D; the row-group forward ln_fwd_wide 1 / 2 / 3 at D = 1024 / 2048 with fp32 / bf16 input, plain /
FiLM + swish, with / without the e4m3 copy, the bf16 output and the statistics; FiLM without swish and swish without FiLM (row kernel);
rows_per_sample = 1; the table-driven FiLM row through smd_layernorm_fwd_lab (t in range, at both ends, clamped on both sides, rows no
multiple of rows_per_sample); the narrow backward's nine instantiations and the generic D = 128 backward; ln_bwd_wide 0 / 1 / 2 at
D = 1024 / 2048 with every (input type, residual, FiLM + swish or plain, outputs) the launcher accepts; the register kernel at D = 256 /
512 / 4096; dfilm_accumulate 0 / 1; saved against recomputed statistics; dres aliasing dx; the 128-wide parts kernels; the fp32 kernel
smd_layernorm_f32, which forms its variance the same way (one pass) and gets the constant, edge and tiny rows.
No entry point of the C ABI reaches launch_ln_bwd_reduce_batched on its own (only the engine's step does): it is left to the engine tests.

Before smd_ln_rstd clamped its argument at eps the constant rows came out NaN in these tests' CPU emulation of the 64-lane order
(tests/test_ln_ref_host.py); with the clamp every row is finite and inside its bound.

Worst |err| / bound against the float64 reference, measured on MI355X (the last test prints this table):
    bwd generic 128                dgamma 0.528   dx bf16 1.000   dx fp32 0.568
    bwd narrow128                  dbeta 0.015   dgamma 0.528   dx bf16 1.000   dx fp32 0.974
    bwd register                   dbeta 0.223   dgamma 0.476   dscale|dshift 0.474   dx bf16 1.000   dx fp32 0.900
    bwd wide4                      dbeta 0.102   dgamma 0.297   dscale|dshift 0.325   dx bf16 1.000   dx fp32 0.521
    bwd wide8                      dbeta 0.099   dgamma 0.242   dscale|dshift 0.450   dx bf16 1.000   dx fp32 0.398
    bwd wide8 (saved statistics)   dbeta 0.028   dgamma 0.023   dscale|dshift 0.206   dx bf16 1.000   dx fp32 0.242
    fwd row                        mean 0.019   out 1.000   rstd 1.000
    fwd t_ptr                      e4m3 1.000   mean 0.002   out 1.000   rstd 1.000
    fwd t_ptr (row kernel)         e4m3 1.000   mean 0.003   out 1.000   rstd 1.000
    fwd wide1                      mean 0.002   out 1.000   rstd 1.000
    fwd wide1 +e4m3                e4m3 1.000   out 1.000
    fwd wide1 e4m3 only            e4m3 1.000   mean 0.002   rstd 1.000
    fwd wide2                      mean 0.002   out 1.000   rstd 1.000
    fwd wide2 +e4m3                e4m3 1.000   out 1.000
    fwd wide2 e4m3 only            e4m3 1.000   mean 0.002   rstd 1.000
    fwd wide3                      e4m3 1.000   mean 0.003   out 1.000   rstd 1.000
    fwd wide3 +e4m3                e4m3 1.000   out 1.000
    fwd wide3 e4m3 only            e4m3 1.000   mean 0.002   rstd 1.000
    layernorm_f32                  out 0.542
    ln128_bwd_parts                dbeta 0.004   dgamma 0.212   dx bf16 1.000   dx fp32 0.516
    ln128_parts                    ln_out 0.998
(1.000 is a ratio that rounds to it from below: a bf16 or e4m3 store next to a tie, an rstd of a clamped row next to rsqrt(eps).)
"""
import pytest
import torch

import _ln_ref as R
from _footprint import guarded

pytestmark = pytest.mark.gpu

NAN = float("nan")
DEFAULTS = {"ln_fwd_wide": 3, "ln_bwd_wide": 2, "ln_bwd_narrow": 1}      # csrc/tuning.hip
WORST = {}                  # (kernel, output) -> worst |err| / bound
_REF = {}


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def ck(rc):
    import smd_amd.lib as lib
    lib.check(rc)


class knob:
    """a process-wide tuning knob for the duration of a block, its default (csrc/tuning.hip) again afterwards"""

    def __init__(self, key, v):
        self.key, self.v = key, v

    def __enter__(self):
        import smd_amd.lib as lib
        lib.set_tuning(self.key, self.v)

    def __exit__(self, *exc):
        import smd_amd.lib as lib
        lib.set_tuning(self.key, DEFAULTS[self.key])


def ref_of(pr):
    if id(pr) not in _REF:
        ref = R.model(pr)
        _REF[id(pr)] = (pr, ref, R.bounds(pr, ref))
    return _REF[id(pr)][1:]


def note(kernel, what, r, where):
    WORST[(kernel, what)] = max(WORST.get((kernel, what), 0.0), r)
    print(f"{kernel} {what} {where}: worst |err| / bound {r:.3f}")
    assert r <= 1.0, f"{kernel} {what} {where}: an element is at {r:.3g} of its bound"


def judge(kernel, what, got, ref, bound, where):
    note(kernel, what, R.worst_ratio(got, ref, bound), where)


def film_ptrs(pr, dev):
    if not pr["film"]:
        return None, None, None
    ssd = pr["ss"].contiguous().to(dev)
    return ssd, P(ssd), P(ssd[:, pr["D"]:])


def x_dev(pr, dev):
    return (R.bf(pr["x"]) if pr["xbf"] else pr["x"]).to(dev)


# ------------------------------------------------------------------------------------------------ forward
def run_fwd(L, dev, pr, out=True, f8=False, stats=True, lab=False):
    rows, D = pr["rows"], pr["D"]
    xd, gd, bd = x_dev(pr, dev), pr["gamma"].to(dev), pr["beta"].to(dev)
    ssd, fsc, fsh = film_ptrs(pr, dev)
    arenas = {}

    def arena(name, shape, dtype):
        v, h = guarded(shape, dtype, dev)
        arenas[name] = (v, h)
        return v

    o = arena("out", (rows, D), torch.bfloat16) if out else None
    q = arena("q", (rows, D), torch.uint8) if f8 else None
    s = arena("scale", (rows,), torch.int32) if f8 else None
    stt = arena("stats", (rows, 2), torch.float32) if stats else None
    xa = (None, P(xd)) if pr["xbf"] else (P(xd), None)
    if lab or pr["t"] is not None:
        td = torch.tensor([pr["t"]], dtype=torch.int32, device=dev) if pr["t"] is not None else None
        ck(L.smd_layernorm_fwd_lab(xa[0], xa[1], rows, D, P(gd), P(bd), fsc, fsh, 2 * D, pr["rps"], int(pr["swish"]), P(o), P(q), P(s), P(stt),
                                   P(td), pr["ss"].shape[0] if pr["t"] is not None else 0, st()))
    else:
        ck(L.smd_layernorm_fwd_stats(xa[0], xa[1], rows, D, P(gd), P(bd), fsc, fsh, 2 * D, pr["rps"], int(pr["swish"]), P(o), P(q), P(s), P(stt), st()))
    torch.cuda.synchronize()
    for name, (_, h) in arenas.items():
        h.assert_untouched(name)
    return {k: v.clone() for k, (v, _) in arenas.items()}


def judge_fwd(kernel, pr, got, where):
    ref, B = ref_of(pr)
    if "out" in got:
        judge(kernel, "out", got["out"].float().cpu(), ref["out"], B["out"], where)
        if not pr["film"] and not pr["swish"]:
            z = R.rows_of(pr, "zero")
            assert torch.equal(got["out"].cpu()[z], R.bf(pr["beta"]).expand(len(z), -1)), f"{kernel} {where}: a zero row is not beta exactly"
    if "stats" in got:
        stt = got["stats"].cpu()
        assert bool(torch.isfinite(stt).all()), f"{kernel} {where}: saved statistics not finite"
        judge(kernel, "mean", stt[:, 0], ref["m"], B["mean"], where)
        note(kernel, "rstd", R.rstd_ratio(stt[:, 1], B, ref), where)
    if "q" in got:
        ratio, bad = R.f8_check(got["q"], got["scale"], ref, B)
        assert bad == 0, f"{kernel} {where}: {bad} rows with an inadmissible e4m3 exponent"
        note(kernel, "e4m3", ratio, where)


FWD_FORMS = ((False, False), (True, True), (True, False), (False, True))      # (FiLM, swish)


@pytest.mark.parametrize("D", (128, 256, 512, 1024, 2048, 4096))
def test_forward_row_kernel(L, dev, D):
    with knob("ln_fwd_wide", 0):
        for film, sw in FWD_FORMS:
            for xbf in (False, True):
                for rows, rps, rot in ((72, 8, 0), (6, 1, 0), (6, 1, 5), (64, 32, 2)):
                    pr = R.problem(D, rows, rps, film=film, swish=sw, xbf=xbf, rot=rot)
                    judge_fwd("fwd row", pr, run_fwd(L, dev, pr), f"D={D} film={film} swish={sw} xbf={xbf} rows={rows}/{rps}")


@pytest.mark.parametrize("wide", (1, 2, 3))
@pytest.mark.parametrize("D", (1024, 2048))
def test_forward_row_group_kernels(L, dev, D, wide):
    with knob("ln_fwd_wide", wide):
        for fs in (False, True):
            for xbf in (False, True):
                for rows, rps, rot in ((72, 8, 0), (64, 32, 3), (8, 8, 1)):
                    pr = R.problem(D, rows, rps, film=fs, swish=fs, xbf=xbf, rot=rot)
                    where = f"D={D} wide={wide} fs={fs} xbf={xbf} rows={rows}/{rps}"
                    a = run_fwd(L, dev, pr, out=True, f8=False, stats=True)
                    b = run_fwd(L, dev, pr, out=True, f8=True, stats=False)
                    c = run_fwd(L, dev, pr, out=False, f8=True, stats=True)
                    judge_fwd(f"fwd wide{wide}", pr, a, where)
                    judge_fwd(f"fwd wide{wide} +e4m3", pr, b, where)
                    judge_fwd(f"fwd wide{wide} e4m3 only", pr, c, where)
                    assert torch.equal(b["q"], c["q"]) and torch.equal(b["scale"], c["scale"])          # one instantiation, with and without the bf16 output


@pytest.mark.parametrize("D", (512, 1024, 2048))
def test_forward_table_row_through_the_lab_entry(L, dev, D):
    """every row reads FiLM row clamp(*t_ptr): t = 0, a middle row, film_rows - 1, -1 and film_rows + 5; 70 rows with rows_per_sample
    32 (ignored); at D = 1024 also on the row kernel"""
    for wide in ((3, 0) if D == 1024 else (3,)):
        with knob("ln_fwd_wide", wide):
            for t in (0, 3, 6, -1, 12):
                for xbf in (False, True):
                    pr = R.problem(D, 70, 32, film=True, swish=True, xbf=xbf, t=t, film_rows=7)
                    got = run_fwd(L, dev, pr, f8=D >= 1024)
                    judge_fwd("fwd t_ptr" + (" (row kernel)" if wide == 0 or D == 512 else ""), pr, got, f"D={D} t={t} xbf={xbf}")
    pr = R.problem(D, 70, 32, film=True, swish=True, t=3, film_rows=7)
    xd, gd, bd = x_dev(pr, dev), pr["gamma"].to(dev), pr["beta"].to(dev)
    ssd, fsc, fsh = film_ptrs(pr, dev)
    o = torch.zeros(70, D, dtype=torch.bfloat16, device=dev)
    td = torch.tensor([3], dtype=torch.int32, device=dev)
    bad = [dict(film_rows=0), dict(fsc=None, fsh=None)]                          # a table without rows; t_ptr without a table
    for b in bad:
        rc = L.smd_layernorm_fwd_lab(P(xd), None, 70, D, P(gd), P(bd), b.get("fsc", fsc), b.get("fsh", fsh), 2 * D, 32, 1, P(o), None, None, None,
                                     P(td), b.get("film_rows", 7), st())
        assert rc < 0, f"smd_layernorm_fwd_lab accepted {b}"
    rc = L.smd_layernorm_fwd_lab(P(xd), None, 70, D, P(gd), P(bd), fsc, fsh, 2 * D, 32, 1, P(o), None, None, None, None, 0, st())
    assert rc < 0, "70 rows with rows_per_sample 32 and no t_ptr must be refused as by smd_layernorm_fwd_stats"
    torch.cuda.synchronize()
    assert bool((o == 0).all())


# ------------------------------------------------------------------------------------------------ backward
def run_bwd(L, dev, pr, om, stats=None):
    """om: 1 fp32 dx, 2 bf16, 3 both; an fp32 residual gradient is passed IN the fp32 dx buffer when there is one (dres aliases dx)"""
    rows, D, res = pr["rows"], pr["D"], pr["res"]
    xd, gd, bd, dyd = x_dev(pr, dev), pr["gamma"].to(dev), pr["beta"].to(dev), pr["dout"].to(dev)
    ssd, fsc, fsh = film_ptrs(pr, dev)
    hs = {}
    dx32 = dxb = dres32 = None
    if om & 1:
        dx32, hs["dx32"] = guarded((rows, D), torch.float32, dev)
        if res == "f32":
            dx32.copy_(pr["dres"])
            dres32 = dx32
    elif res == "f32":
        dres32 = pr["dres"].to(dev)
    if om & 2:
        dxb, hs["dxb"] = guarded((rows, D), torch.bfloat16, dev)
    dresb = R.bf(pr["dres"]).to(dev) if res == "bf16" else None
    dg, db = torch.full((D,), NAN, device=dev), torch.full((D,), NAN, device=dev)
    dss = None
    if pr["film"]:
        dss = pr["dss0"].to(dev).clone() if pr["accumulate"] else torch.full(pr["dss0"].shape, NAN, device=dev)
    partial = torch.zeros(rows * 2 * D, device=dev)
    xa = (None, P(xd)) if pr["xbf"] else (P(xd), None)
    ck(L.smd_layernorm_bwd_stats(xa[0], xa[1], rows, D, P(gd), P(bd), fsc, fsh, 2 * D, pr["rps"], int(pr["swish"]), P(dyd), P(dres32), P(dresb),
                                 P(dx32), P(dxb), P(dg), P(db), P(dss), P(dss[:, D:]) if dss is not None else None, pr["accumulate"],
                                 P(partial), partial.numel(), P(stats), st()))
    torch.cuda.synchronize()
    for name, h in hs.items():
        h.assert_untouched(name)
    return dict(dx32=None if dx32 is None else dx32.clone(), dxb=None if dxb is None else dxb.clone(), dgamma=dg, dbeta=db, dss=dss)


def judge_bwd(kernel, pr, got, where):
    ref, B = ref_of(pr)
    if got["dx32"] is not None:
        judge(kernel, "dx fp32", got["dx32"].cpu(), ref["dx"], B["dx_f32"], where)
    if got["dxb"] is not None:
        judge(kernel, "dx bf16", got["dxb"].float().cpu(), ref["dx"], B["dx_bf16"], where)
    judge(kernel, "dgamma", got["dgamma"].cpu(), ref["dgamma"], B["dgamma"], where)
    judge(kernel, "dbeta", got["dbeta"].cpu(), ref["dbeta"], B["dbeta"], where)
    if got["dss"] is not None:
        judge(kernel, "dscale|dshift", got["dss"].cpu(), ref["dss"], B["dss"], where)


@pytest.mark.parametrize("narrow", (1, 0))
def test_backward_128_wide_every_instantiation(L, dev, narrow):
    """the nine keyed instantiations of the launcher's switch (fp32 x: six (residual, outputs) pairs; bf16 x: three) and one key outside
    it, which the generic kernel takes; 72 rows: groups of 32 + 32 + 8, the last one ragged"""
    keys = [(False, "f32", 3), (False, None, 3), (False, None, 2), (False, "f32", 1), (False, None, 1), (False, "f32", 2),
            (True, "f32", 3), (True, None, 3), (True, None, 2), (True, None, 1)]
    with knob("ln_bwd_narrow", narrow):
        for xbf, res, om in keys:
            for dout in ("mix", "comb"):
                pr = R.problem(128, 72, 8, xbf=xbf, res=res, dout=dout)
                judge_bwd("bwd narrow128" if narrow else "bwd generic 128", pr, run_bwd(L, dev, pr, om), f"xbf={xbf} res={res} om={om} dout={dout}")


@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("D", (1024, 2048))
def test_backward_wide_forms(L, dev, D, mode):
    name = {0: "bwd register", 1: "bwd wide4", 2: "bwd wide8" if D == 2048 else "bwd wide4"}[mode]
    with knob("ln_bwd_wide", mode):
        for fs in (True, False):
            for xbf in (False, True):
                for res in (None, "f32") + (("bf16",) if D == 2048 else ()):
                    for om in (1, 2, 3):
                        acc = 1 if (fs and om == 3) else 0
                        pr = R.problem(D, 72, 8, film=fs, swish=fs, xbf=xbf, res=res, accumulate=acc, rot=om)
                        kernel = "bwd wide8" if res == "bf16" else name
                        judge_bwd(kernel, pr, run_bwd(L, dev, pr, om), f"D={D} mode={mode} fs={fs} xbf={xbf} res={res} om={om} acc={acc}")
        if mode < 2:                                          # FiLM without swish, swish without FiLM: the register and the 4-wave kernel take them
            for film, sw in ((True, False), (False, True)):
                pr = R.problem(D, 64, 32, film=film, swish=sw, res="f32", rot=4)
                judge_bwd(name, pr, run_bwd(L, dev, pr, 3), f"D={D} mode={mode} film={film} swish={sw}")


@pytest.mark.parametrize("D", (256, 512, 4096))
def test_backward_register_kernel(L, dev, D):
    for film, sw in FWD_FORMS:
        for rows, rps, rot in ((72, 8, 0), (6, 1, 2)):
            for acc in ((0, 1) if film else (0,)):
                pr = R.problem(D, rows, rps, film=film, swish=sw, res="f32", accumulate=acc, rot=rot)
                judge_bwd("bwd register", pr, run_bwd(L, dev, pr, 3), f"D={D} film={film} swish={sw} rows={rows}/{rps} acc={acc}")


@pytest.mark.parametrize("fs,xbf,res,om", [(False, True, None, 2), (True, True, "bf16", 2), (True, False, "f32", 3)])
def test_backward_with_saved_and_with_recomputed_statistics(L, dev, fs, xbf, res, om):
    """the 8-wave kernel with the statistics the forward saved and with a NULL pointer: both inside the bound, on regime rows"""
    for rows, rps in ((72, 8), (64, 32)):
        pr = R.problem(2048, rows, rps, film=fs, swish=fs, xbf=xbf, res=res, rot=1)
        f = run_fwd(L, dev, pr)
        judge_fwd("fwd wide3", pr, f, f"saved-statistics case fs={fs} rows={rows}/{rps}")
        saved, again = run_bwd(L, dev, pr, om, f["stats"]), run_bwd(L, dev, pr, om, f["stats"])
        recomputed = run_bwd(L, dev, pr, om, None)
        judge_bwd("bwd wide8 (saved statistics)", pr, saved, f"fs={fs} rows={rows}/{rps}")
        judge_bwd("bwd wide8", pr, recomputed, f"recomputed fs={fs} rows={rows}/{rps}")
        for k in saved:
            if saved[k] is not None:
                assert torch.equal(saved[k].view(torch.uint8), again[k].view(torch.uint8)), f"{k}: two runs differ"


def test_outlier_in_every_lane_chunk_and_row_end(L, dev):
    for D in (1024, 2048):
        pr = R.problem(D, 66, 66, kinds=["outlier"], dout="unit")
        judge_fwd("fwd wide3", pr, run_fwd(L, dev, pr, f8=True), f"outlier sweep D={D}")
        judge_bwd("bwd wide8" if D == 2048 else "bwd wide4", pr, run_bwd(L, dev, pr, 3), f"outlier sweep D={D}")
    pr = R.problem(128, 66, 66, kinds=["outlier"], dout="unit")
    judge_bwd("bwd narrow128", pr, run_bwd(L, dev, pr, 3), "outlier sweep D=128")


def test_one_term_per_column_of_every_column_gradient(L, dev):
    """dout with one non-zero per column, from row c % rows: a wrong column or a wrong row of dgamma / dbeta / dscale / dshift stands alone"""
    for D, rows, rps in ((2048, 64, 32), (2048, 72, 8), (1024, 72, 8)):
        for acc in (0, 1):
            pr = R.problem(D, rows, rps, film=True, swish=True, xbf=True, dout="comb", accumulate=acc)
            judge_bwd("bwd wide8" if D == 2048 else "bwd wide4", pr, run_bwd(L, dev, pr, 2), f"comb D={D} rows={rows}/{rps} acc={acc}")


# ------------------------------------------------------------------------------------------------ 128-wide parts kernels, fp32 kernel
def test_ln128_parts_kernels_on_the_regime_rows(L, dev):
    """four tiles whose fixed-order sum (p0 + p1) + (p2 + p3) is the regime row exactly: p0 = bf16(x), p2 = x - p0, p1 = p3 = 0"""
    rows = 96
    pr = R.problem(128, rows, 32, res="f32")
    x = pr["x"]
    hi = R.bf(x).float()
    parts = torch.stack([hi, torch.zeros_like(x), x - hi, torch.zeros_like(x)])
    assert torch.equal((parts[0] + parts[1]) + (parts[2] + parts[3]), x)
    pD, gD, bD = parts.contiguous().to(dev), pr["gamma"].to(dev), pr["beta"].to(dev)
    xo = torch.full((rows, 128), NAN, device=dev)
    lo = torch.full((rows, 128), NAN, dtype=torch.bfloat16, device=dev)
    ck(L.smd_ln128_parts(P(pD), rows * 128, rows, P(gD), P(bD), P(xo), P(lo), st()))
    torch.cuda.synchronize()
    assert torch.equal(xo.cpu().view(torch.int32), x.view(torch.int32))
    ref, B = ref_of(pr)
    judge("ln128_parts", "ln_out", lo.float().cpu(), ref["out"], B["out"], "regime rows")
    g = torch.Generator().manual_seed(9)
    dparts = torch.randn(4, rows, 128, generator=g) * 0.5
    da = (dparts[0] + dparts[1]) + (dparts[2] + dparts[3])
    prb = dict(pr, dout=da, dout_err=3 * R.U * dparts.double().abs().sum(0))
    refb = R.model(prb)
    Bb = R.bounds(prb, refb)
    dx32, h32 = guarded((rows, 128), torch.float32, dev)
    dxb, hb = guarded((rows, 128), torch.bfloat16, dev)
    partial = torch.full((rows // 32, 2, 128), NAN, device=dev)
    dres, xD, dpD = pr["dres"].to(dev), x.to(dev), dparts.contiguous().to(dev)
    ck(L.smd_ln128_bwd_parts(P(xD), P(dpD), rows * 128, rows, P(gD), P(dres), P(dx32), P(dxb), P(partial), st()))
    torch.cuda.synchronize()
    h32.assert_untouched("dx32")
    hb.assert_untouched("dxb")
    judge("ln128_bwd_parts", "dx fp32", dx32.cpu(), refb["dx"], Bb["dx_f32"], "regime rows")
    judge("ln128_bwd_parts", "dx bf16", dxb.float().cpu(), refb["dx"], Bb["dx_bf16"], "regime rows")
    judge("ln128_bwd_parts", "dgamma", partial[:, 0].double().sum(0).cpu(), refb["dgamma"], Bb["dgamma"], "regime rows")
    judge("ln128_bwd_parts", "dbeta", partial[:, 1].double().sum(0).cpu(), refb["dbeta"], Bb["dbeta"], "regime rows")


@pytest.mark.parametrize("D", (98, 128, 2048))
def test_layernorm_f32_forms_its_variance_in_one_pass_too(L, dev, D):
    """smd_layernorm_f32 (net_f32.hip) computes E[x^2] - mean^2 like the bf16 kernels: constant, nearly constant, edge and tiny rows;
    fp32 output, no store rounding.  D = 98 takes its scalar path."""
    if D == 98:
        g = torch.Generator().manual_seed(3)
        x = torch.stack([torch.full((D,), v) for v in (3.3, 10.1, 100.3)] + [1e-4 * torch.randn(D, generator=g), 10.1 + 1e-3 * torch.randn(D, generator=g)])
        pr = dict(D=D, rows=5, rps=5, film=False, swish=False, xbf=False, x=x, gamma=1 + 0.2 * torch.randn(D, generator=g),
                  beta=0.1 * torch.randn(D, generator=g), t=None, accumulate=0, res=None, kinds=["const3", "const10", "const100", "tiny", "nearconst"])
        cases = [pr]
    else:
        kinds = ["const3", "const10", "const100", "edge", "tiny", "nearconst", "zero"]
        cases = [R.problem(D, 14, 7, kinds=kinds), R.problem(D, 14, 7, film=True, swish=True, kinds=kinds)]
    for pr in cases:
        ref = R.model(pr, backward=False)
        B = R.bounds(pr, ref)
        rows = pr["rows"]
        xd, gd, bd = pr["x"].to(dev), pr["gamma"].to(dev), pr["beta"].to(dev)
        ssd, fsc, fsh = film_ptrs(pr, dev)
        o, h = guarded((rows, D), torch.float32, dev)
        ck(L.smd_layernorm_f32(P(xd), rows, D, P(gd), P(bd), fsc, fsh, 2 * D, pr["rps"], None, 0, int(pr["swish"]), P(o), st()))
        torch.cuda.synchronize()
        h.assert_untouched("out")
        assert bool(torch.isfinite(o).all()), f"layernorm_f32 D={D}: not finite"
        judge("layernorm_f32", "out", o.cpu(), ref["out"], B["y"], f"D={D} film={pr['film']}")


def test_zz_print_the_table_of_worst_ratios():
    """prints what the module docstring quotes"""
    if not WORST:
        return
    for (kernel, what), r in sorted(WORST.items()):
        print(f"    {kernel:32s} {what:14s} {r:.3f}")
    assert max(WORST.values()) <= 1.0
