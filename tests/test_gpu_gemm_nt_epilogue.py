"""launch_gemm_nt, every tile form with every epilogue stage, element by element (smd_gemm_nt_lab, include/smd_hip_lab.h).

The cases (tests/_nt_ref.CASES) put every one of the nine gemm_nt_kernel<BM, NS, KG> instantiations and both epilogues of the
256 x 256 kernel under the epilogue list of tests/_nt_ref.EPILOGUES; each asserts from the plan the launcher hands out that the
intended kernel ran.  Every launch:
  * operands and epilogue tensors hold finite garbage (about +-50 .. 70) in their padding columns, outputs start as NaN (an
    accumulating launch: as known data), a residual table read with res_row_mod has exactly `mod` rows and NaN behind them;
  * |got - ref| <= bound at every logical element of every output (float64 reference and derived bound of tests/_nt_ref.py, with
    the KG the plan reports), the padding of every output keeps its bits, a second launch is bitwise equal, and the older
    whole-matrix criteria still hold; the worst |err| / bound per form and stage is printed.
The activation sweep sends every finite bf16 through gelu / swish / gelu' / swish' with an exact accumulator; the refusals check
that smd_gemm_nt_lab launches nothing it should not.
"""
import ctypes

import pytest
import torch

import _nt_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def knob(L, key, value):
    import smd_amd.lib as lib
    lib.check(L.smd_set_tuning(key.encode(), value))


class knobs:
    """sets the knobs of a case, restores the defaults on the way out"""

    def __init__(self, L, pairs):
        self.L, self.pairs = L, dict(pairs)

    def __enter__(self):
        for k, v in self.pairs.items():
            knob(self.L, k, v)

    def __exit__(self, *exc):
        for k in self.pairs:
            knob(self.L, k, R.KNOB_DEFAULTS[k])


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


_PROBLEMS, _REFS = {}, {}


def problem(case, dev):
    key = (case.M, case.N, case.K, case.ld)
    if key not in _PROBLEMS:
        p = R.make_problem(case)
        p["dev"] = {k: p[k].to(dev) for k in ("A", "Bt", "bias", "aux", "res", "resb")}
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


def reference(case, p, ep, KG):
    key = (case.M, case.N, case.K, case.ld, ep.name, KG)
    if key not in _REFS:
        _REFS[key] = R.reference(p, ep, KG)
    return _REFS[key]


def launch(L, dev, p, ep, over=None):
    """one launch on fresh output buffers -> (rc, plan or None, {output: (buffer, initial contents)})"""
    import smd_amd.lib as lib
    c, ld, d = p["case"], p["ld"], p["dev"]
    M, N, K = c.M, c.N, c.K
    e = lib.GemmEpilogue()
    e.alpha, e.act, e.aux_mode, e.accumulate, e.res_row_mod = ep.alpha, ep.act, ep.aux, int(ep.acc), ep.mod
    keep, outs = [], {}
    if ep.bias:
        e.bias = d["bias"].data_ptr()
    if ep.aux:
        e.aux, e.ld_aux = d["aux"].data_ptr(), ld["aux"]
    if ep.resb:
        e.res_bf16, e.ld_resb = d["resb"].data_ptr(), ld["resb"]
    if ep.res and not ep.inplace:
        res = d["res"][:M]
        if ep.mod:                                                  # exactly `mod` rows, NaN behind them
            res = torch.full((ep.mod + 8, ld["res"]), NAN, device=dev)
            res[:ep.mod] = d["res"][:ep.mod]
            keep.append(res)
        e.res_f32, e.ld_res = res.data_ptr(), ld["res"]
    if ep.pre:
        buf = torch.full((M, ld["pre"]), NAN, dtype=torch.bfloat16, device=dev)
        outs["pre"] = (buf, buf.clone())
        e.pre_bf16, e.ld_pre = buf.data_ptr(), ld["pre"]
    if ep.b16:
        buf = torch.full((M, ld["outb"]), NAN, dtype=torch.bfloat16, device=dev)
        outs["b16"] = (buf, buf.clone())
        e.out_bf16, e.ld_outb = buf.data_ptr(), ld["outb"]
    if ep.f32:
        if ep.inplace:                                              # the residual stream updated in place: out_f32 == res_f32
            buf, ldo = d["res"][:M].clone(), ld["res"]
            e.res_f32, e.ld_res = buf.data_ptr(), ldo
        elif ep.acc:
            buf, ldo = p["old"].to(dev), ld["out"]
        else:
            buf, ldo = torch.full((M, ld["out"]), NAN, device=dev), ld["out"]
        outs["f32"] = (buf, buf.clone())
        e.out_f32, e.ld_out = buf.data_ptr(), ldo
    for k, v in (over or {}).items():
        setattr(e, k, v)
    plan = (ctypes.c_int32 * 8)(*([-1] * 8))
    rc = L.smd_gemm_nt_lab(d["A"].data_ptr(), (over or {}).get("lda", ld["a"]), d["Bt"].data_ptr(), ld["b"], M, N,
                           (over or {}).get("K", K), ctypes.byref(e), 0, plan, st())
    torch.cuda.synchronize()
    del keep
    return rc, (tuple(plan) if plan[0] != -1 else None), outs


_WORST = {}          # (form, epilogue, output) -> worst |err| / bound


def run(L, dev, case, ep, expect, pk=None):
    """two launches of `ep` on `case` and every check of the module docstring -> (plan, outputs)"""
    import smd_amd.lib as lib
    p = problem(case, dev)
    N = case.N
    what = f"{case.id} {ep.name}"
    rc, plan, outs = launch(L, dev, p, ep)
    lib.check(rc, what)
    rc2, plan2, outs2 = launch(L, dev, p, ep)
    lib.check(rc2, what)
    assert plan is not None and plan == plan2, what
    assert plan[:4] == expect, f"{what}: the plan is {plan}, the case is meant for {expect}"
    kernel, BM, NS, KG, grid, block, pk_epi, vec = plan
    if kernel == 128:
        assert grid == -(-case.M // BM) * -(-N // 128) and block == 256 * KG and vec == (0 if case.ld == "odd" else 1), (what, plan)
    else:
        assert grid == (case.M // 256) * (N // 256) and block == 512, (what, plan)
        if pk is not None:
            assert pk_epi == pk, (what, plan)
    ref = reference(case, p, ep, KG)
    got = {}
    for k, (buf, init) in outs.items():
        assert torch.equal(bits(buf), bits(outs2[k][0])), f"{what}: {k} differs between two launches"
        assert torch.equal(bits(buf[:, N:]), bits(init[:, N:])), f"{what}: the padding columns of {k} were written"
        got[k] = buf[:, :N].double().cpu()
        assert bool(torch.isfinite(got[k]).all()), f"{what}: {k} holds NaN / inf in its logical columns"
    ratios = {k: R.worst_ratio(got[k], v, b) for k, (v, b, _) in ref.items()}
    form = "<256%s>" % (",pk" if pk_epi else "") if kernel == 256 else f"<{BM},{NS},{KG}>"
    for k, r in ratios.items():
        _WORST[(form, ep.name, k)] = max(_WORST.get((form, ep.name, k), 0.0), r)
    print(f"{what}: plan {plan}, worst |err| / bound " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items())
          + "; rel L2 " + ", ".join(f"{k} {R.rel(got[k], v):.1e}" for k, (v, _, _) in ref.items()))
    for k, r in ratios.items():
        assert r <= 1.0, f"{what}: {k} leaves the element-wise bound, worst |err| / bound = {r:.3g}"
    assert R.old_criteria_hold(got, ref, ep), f"{what}: the whole-matrix criteria fail"
    return plan, outs


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_form_with_every_epilogue(L, dev, case):
    with knobs(L, case.knobs):
        for ep in R.epilogues_for(case):
            run(L, dev, case, ep, case.expect, pk=(1 if ep.name == "bias->bf16" else 0) if case.expect[0] == 256 else None)
        if case.expect[0] == 256:
            # the packed epilogue switched off: the staged one writes the same bits
            _, on = run(L, dev, case, R.EP["bias->bf16"], case.expect, pk=1)
            knob(L, "gemm_nt256_pk", 0)
            try:
                _, off = run(L, dev, case, R.EP["bias->bf16"], case.expect, pk=0)
            finally:
                knob(L, "gemm_nt256_pk", 1)
            assert torch.equal(bits(on["b16"][0]), bits(off["b16"][0]))
            # alpha != 1 and accumulate are not in the 8-column epilogue (oct_ok): the plan leaves the 256 x 256 kernel, forced or
            # not, for the 128-wide default of the shape, and the result is right
            for name in ("alpha", "accumulate", "everything"):
                run(L, dev, case, R.EP[name], (128, 32, 2, 1))


def test_every_form_is_reached_and_the_worst_ratios(L, dev):
    """Reach test: the nine 128-wide instantiations and both epilogues of the 256 x 256 kernel, from the plans the launcher handed out.
    (A case that left its form has already failed; this one fails when a form has no case left.)"""
    if not _WORST:                      # run alone: the parametrised test fills the table
        for case in R.CASES:
            with knobs(L, case.knobs):
                run(L, dev, case, R.EP["bias->bf16"], case.expect)
    forms = {k[0] for k in _WORST}
    want = {f"<{bm},{ns},{kg}>" for bm, ns, kg in [(32, 2, 1), (32, 4, 1), (32, 3, 2)] + list(R.FORMS.values())} | {"<256>", "<256,pk>"}
    assert want <= forms, f"no case reaches {sorted(want - forms)}"
    for form in sorted(forms):
        per = {}
        for (f, epn, k), r in _WORST.items():
            if f == form:
                per[epn] = max(per.get(epn, 0.0), r)
        print(f"{form}: worst |err| / bound " + ", ".join(f"{e} {r:.3f}" for e, r in per.items()))
    print(f"worst |err| / bound over all forms and stages: {max(_WORST.values()):.3f}")
    assert max(_WORST.values()) <= 1.0


# ------------------------------------------------------------------------------------------------ activation sweep
def _sweep_launch(L, dev, which, M, N, ld_out, nt256):
    """every bf16 bit pattern through one activation with an exact accumulator -> (x [M][N] float64, out [M][N] float64, plan)
    act: A = identity (K = M), Bt[n][m] = x[m][n], so acc[m][n] = x[m][n] exactly;  aux: A[:, 0] = 1, Bt[:, 0] = 1, acc = 1 exactly"""
    import smd_amd.lib as lib
    x = R.all_bf16().view(M, N)
    K = M
    e = lib.GemmEpilogue()
    e.alpha = 1.0
    if which in ("gelu", "swish"):
        A = torch.eye(M, K).to(torch.bfloat16)
        Bt = x.t().contiguous()
        e.act = 1 if which == "gelu" else 2
        aux = None
    else:
        A = torch.zeros(M, K, dtype=torch.bfloat16)
        A[:, 0] = 1.0
        Bt = torch.zeros(N, K, dtype=torch.bfloat16)
        Bt[:, 0] = 1.0
        aux = x.to(dev)
        e.aux, e.ld_aux, e.aux_mode = aux.data_ptr(), N, 1 if which == "gelu'" else 2
    Ad, Bd = A.to(dev), Bt.to(dev)
    out = torch.full((M, ld_out), NAN, device=dev)
    e.out_f32, e.ld_out = out.data_ptr(), ld_out
    plan = (ctypes.c_int32 * 8)(*([-1] * 8))
    with knobs(L, {"gemm_nt256": 2} if nt256 else {}):
        lib.check(L.smd_gemm_nt_lab(Ad.data_ptr(), K, Bd.data_ptr(), K, M, N, K, ctypes.byref(e), 0, plan, st()), f"sweep {which}")
        torch.cuda.synchronize()
    return x.double(), out[:, :N].double().cpu(), tuple(plan)


@pytest.mark.parametrize("path", ["vector", "scalar", "nt256"])
@pytest.mark.parametrize("which", list(R.SWEEP))
def test_activation_over_every_bf16(L, dev, which, path):
    M, N = (256, 256) if path == "nt256" else (64, 1024)
    x, got, plan = _sweep_launch(L, dev, which, M, N, N + (1 if path == "scalar" else 0), path == "nt256")
    assert plan[0] == (256 if path == "nt256" else 128) and (path == "nt256" or plan[7] == (0 if path == "scalar" else 1)), plan
    f, err, _ = R.SWEEP[which]
    inside = x.abs() <= R.SWEEP_RANGE
    xi = x[inside]
    # the accumulator is exact up to a flushed denormal; the fp32 store adds nothing
    bound = err(xi) + (f(xi + R.FLOOR) - f(xi - R.FLOOR)).abs() + R.FLOOR
    r = R.worst_ratio(got[inside], f(xi), bound)
    i = int(((got[inside] - f(xi)).abs() / bound).nan_to_num(posinf=1e300).argmax())
    # outside the range: only where the function stops being finite
    xo, go = x[~inside], got[~inside]
    bad = xo[~torch.isfinite(go)].abs()
    print(f"{which} on the {path} path, plan {plan}: {int(inside.sum())} bf16 arguments up to |x| = 65536, worst |err| / bound {r:.3f} "
          f"at x = {float(xi[i]):.6g}; beyond: " + (f"not finite from |x| = {float(bad.min()):.3g}" if bad.numel() else "finite for every bf16"))
    assert r <= 1.0, f"{which} ({path}): leaves its bound, worst |err| / bound {r:.3g} at x = {float(xi[i])!r}"


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_and_nothing_is_written(L, dev):
    import smd_amd.lib as lib
    case = next(c for c in R.CASES if c.ld == "pad" and c.M == 200 and not c.knobs)
    p = problem(case, dev)
    ep = R.EP["everything"]

    def refused(over, match, ep=ep):
        rc, plan, outs = launch(L, dev, p, ep, over)
        with pytest.raises(ValueError, match=match):
            lib.check(rc)
        assert plan is None, plan
        for k, (buf, init) in outs.items():
            assert torch.equal(bits(buf), bits(init)), f"{over}: {k} was written by a refused launch"

    refused({"act": 3}, "0..2")
    refused({"act": -1}, "0..2")
    refused({"aux_mode": 3}, "0..2")
    refused({"aux": None}, "aux_mode without aux")
    for field in ("ld_pre", "ld_aux", "ld_res", "ld_resb", "ld_out", "ld_outb"):
        refused({field: case.N - 1}, "leading dimension")
    refused({"res_row_mod": -1}, "res_row_mod")
    refused({"lda": case.K + 4}, "multiples of 8")           # the launcher's own rules
    refused({"lda": case.K - 8}, "multiples of 8")
    refused({"K": case.K + 32}, "multiple of 64")
    refused({"out_f32": None, "out_bf16": None, "pre_bf16": None}, "no output")
    rc, plan, outs = launch(L, dev, p, ep)                   # and the same arguments unchanged are accepted
    lib.check(rc)
    assert plan is not None
