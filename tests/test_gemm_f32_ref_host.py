"""The element-wise criterion of the fp32 Dense GEMM (tests/_gemm_f32_ref.py) is right, has room and is sharp: CPU only.

  * the closed forms equal the oracle's gelu / swish, max |swish''| is below the S2 the bound uses, and the exact places of the
    derivation begin where the regimes say (5.06, 17.33, -10.07, -88.72);
  * the lattice condition holds for every (N, K) of the sweep, every residual mode meets every M, N and K, and the reduced list
    holds every value;
  * the selector regimes put z where they say, exactly, and the sweep visits every multiple of 2^-10 in [-12, 12);
  * a correctly rounded fp32 evaluation of the same expressions (emulate) stays inside the bound at every regime point, gives z
    and 0 exactly where the derivation says so, and equals the int64 lattice result bit for bit with both loaders, with NaN behind
    the rows of A, at every shape of the reduced list;
  * every planted fault is caught by the new criterion on cases that tests/test_gpu_gemm_f32_regimes.py runs (CAUGHT);
  * the table this work rests on: which planted faults the old criterion (rel-L2 <= 1e-5 on the inputs and shapes of
    tests/test_gpu_fp32_kernels.py) misses (OLD_MISSES).  The old threshold is tight: it sees every gross fault that its shapes
    trigger, swapped activation codes included.  It misses the faults its shapes never trigger (no odd K, no N = 512 with more
    than 32 rows, a power-of-two row_mod, no NaN behind a row, no activation together with a residual) and the 1-ulp constant.
"""
import pytest
import torch

import _gemm_f32_ref as R
import ddpm_oracle as O
import test_gpu_fp32_kernels as OLD


def test_closed_forms_agree_with_the_oracle_and_the_exact_places_begin_where_the_regimes_say():
    z = torch.cat([torch.linspace(-12, 12, 48001, dtype=R.F64), torch.tensor([-200.0, -90.0, -30.0, 30.0, 200.0], dtype=R.F64)])
    assert float((R.act_ref(z, "gelu") - O.gelu(z)).abs().max()) <= 1e-14 * 200
    assert float((R.act_ref(z, "swish") - O.swish(z)).abs().max()) <= 1e-14 * 200
    assert torch.equal(R.act_ref(z, "none"), z)
    s2 = float(R.LN.swish_grad2(z).abs().max())
    print(f"max |swish''| = {s2:.4f} (S2 = {R.S2})")
    assert s2 <= R.S2 + 1e-12                               # 1/2 exactly, at 0: the float64 evaluation of it lands one ulp above
    near = z[(z > -3) & (z < 0)]
    assert abs(float(near[R.swish_grad(near).abs().argmin()]) - R.SWISH_MIN) < 1e-3
    assert abs(float(near[R.gelu_grad(near).abs().argmin()]) - R.MLP.DCROSS) < 1e-3
    fine = torch.linspace(-100.0, 30.0, 1300001, dtype=R.F64)
    g1, g0 = R.gelu_zones(fine)
    s1, s0 = R.swish_zones(fine)
    edge = dict(one_gelu=float(fine[g1].min()), exp2_ovf=float(fine[g0].max()), one_swish=float(fine[s1].min()), expf_ovf=float(fine[s0].max()))
    print("the exact places begin at", edge)
    for k, want in dict(one_gelu=R.ONE_GELU, exp2_ovf=R.EXP2_OVF, one_swish=R.ONE_SWISH, expf_ovf=R.EXPF_OVF).items():
        assert abs(edge[k] - want) < 0.01, (k, edge[k])
    s, ds = R.MLP.s_err(fine)                               # the zone restated here is the one s_err switches on
    assert torch.equal(g1, ds == torch.sigmoid(-R.MLP._t(fine)))


def test_the_lattice_condition_holds_for_every_shape_and_the_lists_cover_every_value():
    worst = 0
    for N in R.SWEEP_N:
        for K in R.SWEEP_K:
            lat = R.lattice(N, K)                           # asserts the magnitude condition
            worst = max(worst, lat["mag"])
            assert torch.equal((lat["A"].double() @ lat["W"].double() + lat["b"].double()).long(), lat["z"])
            assert bool((lat["A"] != 0).all()) and bool((lat["W"] != 0).all())
    print(f"largest sum |a||w| + |b| + |r| over the sweep: {worst} = {worst / R.EXACT:.3f} of 2^24")
    cases = R.sweep_cases()
    assert len(cases) == len(R.SWEEP_M) * len(R.SWEEP_N) * len(R.SWEEP_K) == 1056 and len(set(cases)) == 1056
    for M, N, K, mode in cases:
        assert R.mode_ok(M, mode)
    for mode in R.MODES:                                    # every mode meets every N and K, and every M it is valid for
        assert {c[1] for c in cases if c[3] == mode} == set(R.SWEEP_N) and {c[2] for c in cases if c[3] == mode} == set(R.SWEEP_K)
        assert {c[0] for c in cases if c[3] == mode} == {M for M in R.SWEEP_M if R.mode_ok(M, mode)}
    red = R.reduced_cases()
    assert {c[0] for c in red} == set(R.SWEEP_M) and {c[1] for c in red} == set(R.SWEEP_N) and {c[2] for c in red} == set(R.SWEEP_K)
    assert len(set(red)) == len(red) == 24
    assert any(N > 512 and N % 4 for _, N, _ in red) and any(N <= 512 and N % 4 for _, N, _ in red)      # ragged N in both forms


def test_the_selector_regimes_are_exact_and_lie_where_they_say():
    span = dict(zero=(0, 0), tiny=(-2.0 ** -37, 2.0 ** -37), gelu_min=(-0.77, 0.77), swish_min=(-1.3, 1.3), sweep=(-12.2, 12.2),
                one_gelu=(-5.26, 5.26), one_swish=(-17.76, 17.76), exp2_ovf=(-10.26, 10.26), neg_tail=(-64.1, 64.1), expf_ovf=(-89.6, 89.6), big=(-R.ZMAX, R.ZMAX))
    seen = {}
    for name, N, part in R.selector_list():
        pr = R.selector_problem(name, N, part)              # asserts that A, b and z are representable and free of denormals
        W = pr["W"].double()
        assert bool(((W != 0).sum(0) == 1).all()) and torch.equal(pr["A"].double() @ W + pr["b"].double(), pr["z"])
        z = pr["z"]
        assert span[name][0] <= float(z.min()) and float(z.max()) <= span[name][1]
        seen.setdefault((name, N), []).append(z.flatten())
    for (name, N), zs in seen.items():
        z = torch.cat(zs)
        print(f"{name} N {N}: {len(zs)} part(s), z in [{float(z.min()):.6g}, {float(z.max()):.6g}], {int(torch.unique(z).numel())} distinct values")
        if name == "sweep":
            grid = torch.arange(-12 * 1024, 12 * 1024, dtype=R.F64) / 1024
            assert bool(torch.isin(grid, z).all())
        for act, regime, side in (("gelu", "one_gelu", 0), ("swish", "one_swish", 0), ("gelu", "exp2_ovf", 1), ("swish", "expf_ovf", 1)):
            if name == regime:                              # both sides of the edge of the exact place
                zone = R.zones(z, act)[side]
                assert bool(zone.any()) and bool((~zone & (z * (1 if side == 0 else -1) > 0)).any())
        if name == "expf_ovf":                              # and both sides of the end of the normal sigmoids
            s = torch.sigmoid(z[z < 0])
            assert bool((s < 2.0 ** -126).any()) and bool((s > 2.0 ** -126).any())
        if name == "gelu_min":
            gz = R.gelu_grad(z[z < 0])
            assert float(gz.min()) < 0 < float(gz.max())
        if name == "swish_min":
            gz = R.swish_grad(z[z < 0])
            assert float(gz.min()) < 0 < float(gz.max())
        if name == "zero":
            assert bool((z == 0).all())


def judge_selector(out, pr, act):
    return R.judge(out, pr["z"], act, pr["res"])


def selector_passes(out, pr, act):
    r, _, finite, exact = judge_selector(out, pr, act)
    return r <= 1.0 and finite and exact


@pytest.mark.parametrize("act", ["gelu", "swish"])
def test_a_correctly_rounded_fp32_evaluation_stays_inside_the_bound_at_every_regime_point(act):
    worst = {}
    for name, N, part in R.selector_list():
        for res in (False, True):
            pr = R.selector_problem(name, N, part, res)
            r, inner, finite, exact = judge_selector(R.emulate(pr, act), pr, act)
            if not res:
                worst[name] = max(worst.get(name, 0.0), inner)
            assert finite and exact and r <= 1.0, (name, N, part, res, r, finite, exact)
    print(f"{act}, selector W, no residual: worst |err| / bound of the emulation outside the exact places, per regime: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for M, K, N in R.DENSE_SHAPES:
        pr = R.dense_problem(M, K, N)
        ref, bound = R.out_ref_bound(pr["z"], act, R.z_err(pr["A"], pr["W"], pr["b"], K))
        r = R.worst_ratio(R.emulate(pr, act), ref, bound)
        print(f"{act}, dense {M}x{K}x{N}: |z| up to {float(pr['z'].abs().max()):.2f}, worst |err| / bound of the emulation {r:.3f}")
        assert r <= 1.0 and float(pr["z"].max()) > 5.0 and float(pr["z"].min()) < -5.0


def test_the_emulation_equals_the_int64_result_bit_for_bit_on_the_reduced_list():
    for i, (M, N, K) in enumerate(R.reduced_cases()):
        mode = [m for m in R.MODES if R.mode_ok(M, m)][i % 3]
        pr = R.lattice_problem(M, N, K, mode)
        want = R.lattice_want(R.lattice(N, K), M, mode).float()
        for vec, pad in ((True, None), (False, None), (True, float("nan"))):
            assert R.bits_equal(R.emulate(pr, vec=vec, a_pad=pad), want), (M, N, K, mode, vec, pad)


# ------------------------------------------------------------------------------------------------ planted faults
def exact_subset():
    """the slice of the GPU test's exact sweep that the host emulates for the fault table"""
    return [c for c in R.sweep_cases() if c[0] in (33, 129) and c[1] in (129, 512)]


def new_criterion_sees(fault):
    """kinds of GPU test cases on which the planted fault fails the new criterion (the unplanted emulation passes all of them)"""
    seen = set()
    for M, N, K, mode in exact_subset():
        pr, want = R.lattice_problem(M, N, K, mode), R.lattice_want(R.lattice(N, K), M, mode).float()
        assert R.bits_equal(R.emulate(pr), want)
        if not R.bits_equal(R.emulate(pr, fault=fault), want):
            seen.add("exact")
    for M, N, K in R.reduced_cases()[:12]:
        pr, want = R.lattice_problem(M, N, K, "none"), R.lattice_want(R.lattice(N, K), M, "none").float()
        if not R.bits_equal(R.emulate(pr, fault=fault, a_pad=float("nan")), want):
            seen.add("padded")
    for name, act, res in (("sweep", "gelu", False), ("sweep", "swish", True), ("neg_tail", "swish", False)):
        pr = R.selector_problem(name, 128, 0, res)
        assert selector_passes(R.emulate(pr, act), pr, act)
        if not selector_passes(R.emulate(pr, act, fault=fault), pr, act):
            seen.add("selector")
    return seen


_OLD_REF = {}


def old_criterion_sees(fault):
    """old cases (index into OLD.CASES) on which the fault moves the rel-L2 above 1e-5 or leaves a NaN: float64 arithmetic, so the
    figure is the fault's own effect (the rounding of a correct kernel adds 1e-7)"""
    seen = []
    for i, (M, K, N, epi) in enumerate(OLD.CASES):
        pr = R.old_problem(M, K, N, epi)
        if i not in _OLD_REF:
            _OLD_REF[i] = R.emulate(pr, pr["act"], fast=True)
        bad = R.emulate(pr, pr["act"], fault=fault, fast=True)
        e = R.rel(bad, _OLD_REF[i])
        if not e <= R.OLD_REL:
            seen.append(i)
    return seen


CAUGHT = {                                      # fault -> kinds of new cases that must catch it
    "odd-k-last-pair-dropped": {"exact"}, "k-tail-of-partial-stage-dropped": {"exact"}, "group-of-four-on-ragged-k-dropped": {"exact"},
    "group-of-four-on-ragged-k-read": {"padded"}, "last-row-dropped": {"exact"}, "last-row-duplicated": {"exact"},
    "last-col-dropped": {"exact"}, "last-col-duplicated": {"exact"}, "form-switch-at-512": {"exact"},
    "row-and-instead-of-mod": {"exact"}, "residual-before-activation": {"selector"}, "act-codes-swapped": {"selector"},
    "sigmoid-arg-1ulp": {"selector"}, "cd-row-permuted": {"exact"},
}
# the faults that rel-L2 <= 1e-5 on the old inputs and shapes lets through
OLD_MISSES = {"odd-k-last-pair-dropped", "group-of-four-on-ragged-k-read", "form-switch-at-512", "row-and-instead-of-mod",
              "residual-before-activation", "sigmoid-arg-1ulp"}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_is_caught_by_the_new_criterion_and_what_the_old_threshold_sees(fault):
    assert set(CAUGHT) == set(R.FAULTS) and OLD_MISSES <= set(R.FAULTS)
    new, old = new_criterion_sees(fault), old_criterion_sees(fault)
    print(f"{fault}: new criterion fails on {sorted(new)}; old rel-L2 <= 1e-5 " +
          ("MISSES it" if not old else "sees it on " + ", ".join("x".join(map(str, OLD.CASES[i][:3])) + " " + OLD.CASES[i][3] for i in old)))
    assert CAUGHT[fault] <= new, (fault, new)
    assert (not old) == (fault in OLD_MISSES), (fault, old)


def test_the_gelu_constant_one_ulp_off_is_inside_the_allowance_of_the_derivation():
    """The limit of the criterion, stated: 8 U |t| is granted to the folded constants, and a constant that is one ulp off uses 2 U."""
    for fault in R.BEYOND:
        for name in ("sweep", "exp2_ovf"):
            pr = R.selector_problem(name, 128, 0)
            r, _, finite, exact = judge_selector(R.emulate(pr, "gelu", fault=fault), pr, "gelu")
            print(f"{fault} on {name}: worst |err| / bound {r:.3f}")
            assert r <= 1.0 and finite and exact
        assert not old_criterion_sees(fault)
