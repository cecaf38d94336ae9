"""The element-wise criterion of the LayerNorm kernels (tests/_ln_ref.py) is right, has room and is sharp: CPU only.

  * the float64 model equals oracle/ddpm_oracle.py's layer_norm / swish and their float64 autograd gradients; max |swish''| and
    max |swish'''| are below the S2 and S3 the bound uses;
  * the regimes are what they say, exactly: zero rows are zero, constant rows constant, the outlier visits every lane, every
    256-column chunk and both ends, the FiLM rows reach +-30 and +-100, `edge` sits at the largest mean for which the derived
    bound still gives dvar <= (var + eps) / 8;
  * an fp32 emulation of the kernels' arithmetic (three summation orders: the 64-lane layout of the row and wide kernels, the
    16-lane layout of the narrow kernel, one sequential accumulator; the unfolded order of the row / register kernels and the
    folded constants of the wide ones; rsqrt argument clamped at eps) stays inside the bound at EVERY element of every output in
    every regime and every D: nothing is excluded, reference, emulation and bounds are finite everywhere.  The median and the
    maximum of |err| / bound are printed per regime.  The maximum over a regime's outputs is above 1e-3 everywhere: the bf16
    outputs sit at a large share of their half-spacing.  For the fp32 outputs alone the ratio is small by construction (printed):
    the bound allows n U for a sum of n terms in any order, a real order accumulates about sqrt(n) U; it cannot be tightened
    without naming one kernel's layout, which would make it wrong for the others (module docstring of _ln_ref.py);
  * the same emulation WITHOUT the clamp has a negative rsqrt argument on constant rows (the finding that put the clamp into
    smd_ln_rstd);
  * every planted fault leaves the bound where CAUGHT says; for each it is printed whether the whole-tensor thresholds of
    tests/test_gpu_kernels.py on the `unit` draw would have caught it, and how many would.
"""
import pytest
import torch

import _ln_ref as R
import ddpm_oracle as O

DS = (128, 256, 512, 1024, 2048, 4096)


def row_ratio(got, ref, bound):
    """per-row worst |err| / bound (inf where not finite)"""
    got, ref, bound = (torch.as_tensor(t).double() for t in (got, ref, bound))
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r.reshape(r.shape[0], -1).max(1).values


def test_model_agrees_with_the_oracle_and_its_autograd():
    for film, sw in ((False, False), (True, True), (True, False), (False, True)):
        pr = R.problem(256, 16, 8, film=film, swish=sw, kinds=["unit", "offset", "outlier"], res="f32", accumulate=0)
        x = pr["x"].double().requires_grad_(True)
        g, b = pr["gamma"].double().requires_grad_(True), pr["beta"].double().requires_grad_(True)
        y = O.layer_norm(x, {"n.scale": g, "n.bias": b}, "n")
        ss = None
        if film:
            ss = pr["ss"].double().requires_grad_(True)
            y = ss[:, :256].repeat_interleave(8, 0) * y + ss[:, 256:].repeat_interleave(8, 0)
        if sw:
            y = O.swish(y)
        y.backward(pr["dout"].double())
        ref = R.model(pr)
        close = lambda a, w: float((a - w).abs().max()) <= 1e-9 * (1 + float(w.abs().max()))
        assert close(ref["out"], y.detach()) and close(ref["dx"], x.grad + pr["dres"].double())
        assert close(ref["dgamma"], g.grad) and close(ref["dbeta"], b.grad)
        if film:
            assert close(ref["dss"], ss.grad)
    z = torch.linspace(-40, 40, 800001, dtype=R.F64).requires_grad_(True)
    (g1,) = torch.autograd.grad(O.swish(z).sum(), z, create_graph=True)
    (g2,) = torch.autograd.grad(g1.sum(), z, create_graph=True)
    (g3,) = torch.autograd.grad(g2.sum(), z)
    zd = z.detach()
    assert float((R.swish_grad(zd) - g1.detach()).abs().max()) < 1e-13 and float((R.swish_grad2(zd) - g2.detach()).abs().max()) < 1e-13
    print(f"max |swish''| = {float(g2.abs().max()):.4f} (S2 = {R.S2}), max |swish'''| = {float(g3.abs().max()):.4f} (S3 = {R.S3})")
    assert float(g2.abs().max()) <= R.S2 and float(g3.abs().max()) <= R.S3


def test_the_regimes_are_exact():
    for D in DS:
        for xbf in (False, True):
            pr = R.problem(D, 72, 8, film=True, swish=True, xbf=xbf)
            x = pr["x"]
            assert set(pr["kinds"]) == set(R.ROW_KINDS)
            for r0 in range(0, 72, 8):
                assert len(set(pr["kinds"][r0:r0 + 8])) == 8                    # every group of eight rows holds eight regimes
            if xbf:
                assert torch.equal(R.bf(x).float(), x)
            assert bool((x[R.rows_of(pr, "zero")] == 0).all())
            for k, v in R.CONST.items():
                rows = x[R.rows_of(pr, k)]
                assert bool((rows == rows[:, :1]).all()) and abs(float(rows[0, 0]) - v) < 0.01 * v
                m, e = torch.frexp(rows[0, 0].double())
                assert float(m) != 0.5                                           # not a power of two
            mu = R.edge_mean(D, xbf)
            st = R.stats(x[R.rows_of(pr, "edge")])
            assert bool((st["dvar"] <= (st["var"] + R.EPS) / 8).all())
            g = torch.Generator().manual_seed(1)
            worse = R.make_rows(["edge"], D, xbf, g).double() - mu + 1.05 * mu
            worse = R.bf(worse).double() if xbf else worse.float().double()
            sw = R.stats(worse)
            assert bool((sw["dvar"] > (sw["var"] + R.EPS) / 8).all()), "edge is not at the edge"
            print(f"D={D} xbf={xbf}: edge mean / spread = {mu:.2f}")
            st = R.stats(x[R.rows_of(pr, "tiny")])
            assert float(st["var"].max()) < 0.1 * R.EPS
            assert float(x.abs().max()) == float(x[R.rows_of(pr, "huge")].abs().max()) <= 2.0 ** 43
            ref = R.model(pr, backward=False)
            pre = ref["pre"]
            kinds = pr["film_kinds"]
            for s, k in enumerate(kinds):
                p = pre[8 * s:8 * s + 8]
                if k == "sat30":
                    assert float(p.max()) >= 30 and float(p.min()) <= -30
                if k == "sat100":
                    assert float(p.max()) >= 100 and float(p.min()) <= -100
                if k == "zero":
                    assert bool((pr["ss"][s, :D] == 0).all())
                if k == "neg":
                    assert bool((pr["ss"][s, :D] < 0).all())
            assert set(kinds) == set(R.FILM_KINDS)
        cols = R.outlier_cols(D)
        lanes = {(c % 256) // 4 if D > 128 else c // 2 for c in cols}
        assert lanes == set(range(64)) and {c // 256 for c in cols} == set(range(max(D // 256, 1))) and 0 in cols and D - 1 in cols
        pr = R.problem(D, 66, 66, kinds=["outlier"])
        hit = (pr["x"] == 1024.0)
        assert bool((hit.sum(1) == 1).all()) and sorted(hit.float().argmax(1).tolist()) == sorted(cols)
    pr = R.problem(1024, 64, 32, dout="comb")
    nz = (pr["dout"] != 0)
    assert bool((nz.sum(0) == 1).all()) and torch.equal(nz.float().argmax(0), torch.arange(1024) % 64)      # one term per column, from row c % rows


HOST = {}       # (regime, kind of output: "bf16" / "f32") -> list of per-row ratios


def _collect(pr, tag, got, ref, bound, store):
    r = row_ratio(got, ref, bound)
    for row, k in enumerate(pr["kinds"]):
        HOST.setdefault((k, store), []).append(float(r[row]))
    w = float(r.max())
    assert w <= 1.0, f"{tag}: the emulation is at {w:.3g} of its bound in row {int(r.argmax())} ({pr['kinds'][int(r.argmax())]})"
    return w


def _all_finite(*ts):
    return all(bool(torch.isfinite(torch.as_tensor(t).double()).all()) for t in ts)


@pytest.mark.parametrize("D", DS)
def test_emulation_stays_inside_the_bound_in_every_regime(D):
    _emulate(D)


def _emulate(D):
    orders = ("wave", "seq") + (("narrow",) if D == 128 else ())
    worst = 0.0
    for film, sw, xbf, res in ((False, False, False, None), (True, True, True, "bf16"), (True, False, False, "f32"), (False, True, True, None)):
        for acc in ((0, 1) if film and sw else (0,)):
            pr = R.problem(D, 24, 8, film=film, swish=sw, xbf=xbf, res=res, accumulate=acc, rot=D % 7)
            ref = R.model(pr)
            B = R.bounds(pr, ref)
            assert _all_finite(ref["out"], ref["dx"], ref["dgamma"], ref["dbeta"], ref["m"], ref["rs"], B["out"], B["dx_f32"], B["dgamma"], B["dbeta"],
                               B["rs_lo"], B["rs_hi"])
            assert float(B["out"].min()) > 0 and float(B["dx_f32"].min()) > 0 and float(B["rs_lo"].min()) > 0
            for order in orders:
                for folded in (False, True):
                    tag = f"D={D} film={film} swish={sw} xbf={xbf} {order} folded={folded}"
                    f = R.emu_forward(pr, order, folded)
                    assert _all_finite(f["out"].float(), f["rstd"])
                    worst = max(worst, _collect(pr, tag + " out", f["out"].float(), ref["out"], B["out"], "bf16"))
                    _collect(pr, tag + " mean", f["mean"][:, None], ref["m"][:, None], B["mean"][:, None], "f32")
                    assert R.rstd_ratio(f["rstd"], B, ref) <= 1.0, tag + " rstd"
                    ex = R.e4m3_row_exponent(f["y"].abs().max(1).values.double())          # the copy, from the emulation's own fp32 row
                    deq = torch.ldexp(R.e4m3_round(torch.ldexp(f["y"].double(), -ex[:, None])), ex[:, None])
                    ratio, bad = R.f8_check_values(deq, ex, ref, B)
                    assert ratio <= 1.0 and bad == 0, tag + f" e4m3 copy: {ratio:.3g}, {bad} inadmissible exponents"
                    for saved in (None, (f["mean"], f["rstd"])):
                        b = R.emu_backward(pr, order, folded, saved)
                        assert _all_finite(b["dx"], b["dgamma"], b["dbeta"])
                        _collect(pr, tag + " dx fp32", b["dx"], ref["dx"], B["dx_f32"], "f32")
                        _collect(pr, tag + " dx bf16", R.bf(b["dx"]).float(), ref["dx"], B["dx_bf16"], "bf16")
                        for k in ("dgamma", "dbeta") + (("dss",) if film else ()):
                            w = R.worst_ratio(b[k], ref[k], B[k])
                            HOST.setdefault(("columns", "f32"), []).append(w)
                            assert w <= 1.0, f"{tag} {k}: {w:.3g}"
    print(f"D={D}: worst emulation |err| / bound of the forward output {worst:.3f}")


def test_the_bound_is_not_vacuous_in_any_regime():
    """per regime the median and the maximum of the per-row worst ratio, over what the emulation test collected (run alone: over
    D = 128 and 2048)"""
    if not HOST:
        for D in (128, 2048):
            _emulate(D)
    for kind in R.ROW_KINDS + ("columns",):
        line = []
        both = []
        for store in ("bf16", "f32"):
            v = torch.tensor(HOST.get((kind, store), [0.0]), dtype=R.F64)
            both.append(float(v.max()))
            line.append(f"{store}: median {float(v.median()):.2e} max {float(v.max()):.2e}")
        print(f"{kind:10s} " + "   ".join(line))
        assert max(both) <= 1.0
        assert max(both) >= 1e-3, f"{kind}: the bound is too loose to test anything"


def test_without_the_clamp_constant_rows_have_a_negative_rsqrt_argument():
    found = []
    for D in (128, 2048):
        for xbf in (False, True):
            pr = R.problem(D, 22, 22, xbf=xbf)
            for order in ("wave", "seq") + (("narrow",) if D == 128 else ()):
                _, rstd, arg = R.emu_stats(pr["x"], order, clamp=False)
                _, rstd_c, _ = R.emu_stats(pr["x"], order, clamp=True)
                assert bool(torch.isfinite(rstd_c).all()) and float(rstd_c.max()) <= 1000.0 * (1 + 1e-6)
                for r in R.rows_of(pr, "constant") + R.rows_of(pr, "nearconst"):
                    a = float(arg[r])
                    print(f"D={D} xbf={xbf} {order} {pr['kinds'][r]}: rsqrt argument {a:.3e}")
                    if a < 0:
                        found.append((D, xbf, order, pr["kinds"][r]))
                        assert bool(torch.isnan(rstd[r]).all())
                ok = [r for r in range(22) if pr["kinds"][r] not in R.CONST and pr["kinds"][r] != "nearconst"]
                assert torch.equal(rstd[ok], rstd_c[ok])                        # elsewhere the clamp changes no bit
    print(f"negative arguments without the clamp: {found}")
    assert any(f[0] == 2048 and f[2] == "wave" for f in found), "the 64-lane order at D = 2048 no longer emulates to a negative variance"


# fault -> (problem arguments, output that catches it, regime of the row (or None for a column output) where it is caught)
_FS = dict(film=True, swish=True)
CAUGHT = {
    "no-eps": (dict(D=128, rows=22, rps=22), "out", "zero"),
    "unbiased-variance": (dict(D=128, rows=22, rps=22), "rs", "unit"),
    "rsqrt-unclamped": (dict(D=2048, rows=22, rps=22), "out", "constant"),
    "film-neighbour-sample": (dict(D=1024, rows=72, rps=8, **_FS), "out", "unit"),
    "C-beta-plus-shift": (dict(D=1024, rows=72, rps=8, **_FS), "out", "unit"),
    "t-unclamped": (dict(D=1024, rows=22, rps=8, t=-1, **_FS), "out", "unit"),
    "ragged-last-row-dropped": (dict(D=2048, rows=72, rps=8), "out", None),
    "columns-swapped": (dict(D=2048, rows=22, rps=22), "out", "unit"),
    "e4m3-exponent-off-by-one": (dict(D=1024, rows=22, rps=22), "deq", "unit"),
    "dx-missing-mean-term": (dict(D=2048, rows=24, rps=8, **_FS), "dx", "unit"),
    "dres-twice": (dict(D=2048, rows=24, rps=8, res="f32", **_FS), "dx", "unit"),
    "dgamma-missing-last-group": (dict(D=2048, rows=72, rps=8, dout="comb"), "dgamma", None),
    "dscale-overwritten": (dict(D=2048, rows=24, rps=8, accumulate=1, **_FS), "dss", None),
    "rstd-of-previous-row": (dict(D=2048, rows=24, rps=8, **_FS), "dx", "unit"),
}
OLD = dict(out=R.OLD_BF16_REL, deq=R.OLD_E4M3_REL, dx=R.OLD_F32_REL, dgamma=R.OLD_F32_REL, dss=R.OLD_F32_REL, rs=R.OLD_F32_REL)


def test_every_planted_fault_leaves_the_bound_and_most_pass_the_old_thresholds():
    assert set(CAUGHT) == set(R.FAULTS)
    old_caught = []
    for fault, (args, what, regime) in CAUGHT.items():
        pr = R.problem(**args)
        ref, bad = R.model(pr), R.model(pr, fault)
        B = R.bounds(pr, ref)
        if what == "rs":
            rows = R.rows_of(pr, regime)
            sub = dict(rs_lo=B["rs_lo"][rows], rs_hi=B["rs_hi"][rows])
            ratio = R.rstd_ratio(bad["rs"][rows], sub, dict(rs=ref["rs"][rows]))
        elif what == "deq":
            ratio, nbad = R.f8_check_values(bad["deq"], bad["ex"], ref, B)
            ratio = max(ratio, float("inf") if nbad else 0.0)
        else:
            bound = B[{"dx": "dx_f32"}.get(what, what)]
            rr = row_ratio(bad[what], ref[what], bound) if regime else None
            ratio = float(rr[R.rows_of(pr, regime)].max()) if regime else R.worst_ratio(bad[what], ref[what], bound)
        # the same fault on the `unit` draw against the old whole-tensor threshold
        ua = dict(args, kinds=["unit"], film_kinds=["near1"])
        if ua.get("dout") is None:
            ua["dout"] = "unit"
        pu = R.problem(**ua)
        ru, bu = R.model(pu), R.model(pu, fault)
        old = R.rel(torch.nan_to_num(bu[what], nan=1e30), ru[what])
        hit = old >= OLD[what]
        old_caught.append(fault) if hit else None
        print(f"{fault:30s} caught on {what:6s} in {regime or 'columns / last row'}: |err| / bound {ratio:.3g};  "
              f"old threshold on the unit draw: rel {old:.2e} vs {OLD[what]:.0e} -> {'caught' if hit else 'MISSED'}")
        assert ratio > 1.0, f"{fault}: not caught ({ratio:.3g})"
    print(f"the old whole-tensor thresholds on the unit draw catch {len(old_caught)} of {len(CAUGHT)} planted faults: {old_caught}")
