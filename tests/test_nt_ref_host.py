"""The element-wise NT GEMM + epilogue criterion (tests/_nt_ref.py) is sharp and has room: CPU only.

  * the reference's GELU is the oracle's, written without the cancellation of 1 + tanh;
  * an fp32 emulation of the kernels' expressions (one fp32 addition per 16-wide K step, K-groups added afterwards, exp2 / rcp /
    division correctly rounded) is inside the bound at every element of every output of every case of
    tests/test_gpu_gemm_nt_epilogue.py, and its ACCUMULATOR is inside half of the accumulator's bound: worst 0.008.
    The issue asked for half of the WHOLE bound at every output.  That cannot hold for a bound that is not widened, and the
    figures are kept here as found: u |v| per fp32 operation and 2^-8 |v| per bf16 store are not estimates but the half-spacing
    of the format at the bottom of a binade, so ONE correctly rounded operation reaches them wherever it dominates --
    0.97 for the bf16 store of the plain bias epilogue, 0.65 .. 0.97 for the fp32 output of "everything" / "everything8" (behind
    gelu / swish the carried error is scaled by act' ~ 0 for negative arguments and the residual additions are all that is left),
    0.49 / 0.56 / 0.77 / 0.53 for gelu / swish / gelu' / swish' over every bf16 argument (chains of three to eight roundings).
    Half the bound is asserted where the hardware is NOT specified to round correctly and the derivation therefore leaves it
    room: the matrix core's summation (factor 2).  exp2 / rcp carry 1 ulp where the emulation's are correctly rounded (0.5 ulp);
  * each of the eight planted faults leaves the bound on a case where it applies;
  * whether the older whole-matrix criteria (relative L2 < 2e-5 fp32, 4e-3 bf16, 1e-4 behind an activation) see the same fault is
    recorded as found (OLD_CRITERIA_SEE): at these shapes (200 x 136, 512 x 512) they see all eight.  The least visible are a
    32 x 32 sub-tile without its second K-group (0.12 of the norm) and two stale columns of 134 (0.15).  What none of the older
    tests did is run the stage on the form.
"""
import pytest
import torch

import _nt_ref as R
import ddpm_oracle as O


def case_where(**kw):
    for c in R.CASES:
        if all((getattr(c, k) == v) if k != "KG" else (c.expect[3] == v) for k, v in kw.items()):
            return c
    raise KeyError(kw)


_PROBLEMS = {}


def problem(case):
    key = (case.M, case.N, case.K, case.ld, case.seed)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = R.make_problem(case)
    return _PROBLEMS[key]


def test_the_reference_gelu_is_the_oracles_tanh_form():
    x = torch.linspace(-12.0, 12.0, 4801, dtype=torch.float64)
    # the oracle loses |x| / 2 * eps(1) where 1 + tanh cancels; nothing else separates the two
    assert float(((R.gelu(x) - O.gelu(x)).abs() - 2.0 ** -52 * (1.0 + x.abs())).max()) <= 0.0
    assert float((R.swish(x) - O.swish(x)).abs().max()) < 1e-15
    # the derivatives are those of the values (central differences in float64)
    h = 1e-6
    for f, df in ((R.gelu, R.gelu_grad), (R.swish, R.swish_grad)):
        assert float((((f(x + h) - f(x - h)) / (2 * h)) - df(x)).abs().max()) < 1e-8


def _host_cases():
    seen, out = set(), []
    for c in R.CASES:                  # the schedule variants of the 256 x 256 kernel are one case to the emulation
        key = (c.M, c.N, c.K, c.ld, c.expect[3])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


_EMU_WORST = {}


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: c.id)
def test_fp32_emulation_stays_inside_the_bound_and_its_accumulator_inside_half(case):
    p = problem(case)
    KG = case.expect[3]
    acc = R.emulate_acc(p, KG)
    r_acc = R.worst_ratio(torch.from_numpy(acc).double(), p["acc"], 2.0 * (case.K + KG) * R.U * p["absacc"])
    assert r_acc <= 0.5, f"{case.id}: the emulated accumulator is at {r_acc:.3g} of its bound: the derivation is wrong"
    worst = 0.0
    for ep in R.epilogues_for(case):
        ref = R.reference(p, ep, KG)
        emu = R.emulate(p, ep, KG, acc=acc)
        R.check(emu, ref, what=f"{case.id} {ep.name}")                       # the stores: inside the whole bound
        for k, (v, _, e) in ref.items():                                     # the fp32 values in front of them: inside theirs
            r = R.worst_ratio(emu[k if k == "f32" else k + ":f32"], v, e)
            assert r <= 1.0, f"{case.id} {ep.name}: the emulation's {k} is at {r:.3g} of the bound: the derivation is wrong"
            worst = max(worst, r)
            _EMU_WORST[ep.name] = max(_EMU_WORST.get(ep.name, 0.0), r)
        # and a correctly rounded result is inside it as well
        assert not R.flagged(R.rounded(ref), ref)
    print(f"{case.id}: fp32 emulation, worst |err| / bound: accumulator {r_acc:.3f}, over {len(R.epilogues_for(case))} epilogues {worst:.3f}")


def test_emulation_summary():
    if _EMU_WORST:
        print("fp32 emulation, worst |err| / bound per epilogue: " + ", ".join(f"{k} {v:.3f}" for k, v in _EMU_WORST.items()))
        assert max(_EMU_WORST.values()) <= 1.0


@pytest.mark.parametrize("name", list(R.SWEEP))
def test_emulated_activation_stays_inside_its_bound_over_every_bf16(name):
    f, err, femu = R.SWEEP[name]
    x = R.all_bf16()
    x = x[x.float().abs() <= R.SWEEP_RANGE]
    xd = x.double()
    got = torch.from_numpy(femu(x.float().numpy())).double()
    r = R.worst_ratio(got, f(xd), err(xd))
    print(f"{name}: fp32 emulation over {x.numel()} bf16 arguments, worst |err| / bound {r:.3f}")
    assert r <= 1.0


# fault -> the whole-matrix criteria of the older tests see it too (as found; asserted so that the record stays true)
OLD_CRITERIA_SEE = {
    "bias-one-right": True,
    "row-not-reduced": True,
    "aux-ld-out": True,
    "pre-after-act": True,
    "kgroup-dropped": True,
    "accumulate-overwrites": True,
    "ragged-columns-stale": True,
    "second-tile-first-residual": True,
}
FAULT_CASE = {
    "bias-one-right": dict(N=136, K=64, ld="tight"),
    "row-not-reduced": dict(M=200, N=136, K=192, ld="pad", KG=1),
    "aux-ld-out": dict(M=200, N=136, K=192, ld="pad", KG=1),
    "pre-after-act": dict(N=136, K=64, ld="tight"),
    "kgroup-dropped": dict(M=200, N=136, K=384, KG=2),
    "accumulate-overwrites": dict(N=134, K=64, ld="odd", M=200),
    "ragged-columns-stale": dict(N=134, K=64, ld="odd", M=200),
    "second-tile-first-residual": dict(M=512),
}


@pytest.mark.parametrize("fault", list(R.FAULTS))
def test_every_planted_fault_leaves_the_bound(fault):
    case = case_where(**FAULT_CASE[fault])
    p = problem(case)
    KG = case.expect[3]
    got, ref, ep = R.plant(p, fault, KG)
    worst = max(R.worst_ratio(got[k], v, b) for k, (v, b, _) in ref.items())
    old = {k: R.rel(got[k], v) for k, (v, _, _) in ref.items()}
    seen = not R.old_criteria_hold(got, ref, ep)
    print(f"{fault} on {case.id} ({ep.name}): |err| / bound {worst:.3g}; whole-matrix rel "
          + ", ".join(f"{k} {v:.2e}" for k, v in old.items()) + f": the old criteria {'see' if seen else 'MISS'} it")
    assert not R.flagged(R.rounded(ref), ref)          # the unplanted result passes
    assert R.flagged(got, ref) and worst > 2.0
    assert seen == OLD_CRITERIA_SEE[fault]


def test_a_stale_column_of_nans_is_flagged_too():
    case = case_where(**FAULT_CASE["ragged-columns-stale"])
    got, ref, ep = R.plant(problem(case), "ragged-columns-stale", stale=R.NAN)
    assert R.flagged(got, ref)
