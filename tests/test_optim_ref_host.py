"""tests/_optim_ref.py on the CPU: the fp32 emulation of the optimiser kernels stays inside the derived bounds in every regime, both
summation orders and both contraction forms; every planted fault leaves the bound in its named regime; which of them the old
whole-tensor thresholds miss; the exact-norm rows are exact in fp32; the work-table model owns every parameter exactly once."""
import math

import numpy as np
import pytest

import _optim_ref as R

N, HEAD = 4099, 1029            # a flat size that is no multiple of 4; a slice boundary that leaves three head scalars and a tail


def _inside(s, hp, exact, n=N):
    ref = R.model(s, hp)
    worst = {}
    for order, ho in (("flat", 0), ("slots", HEAD)):
        B = R.bounds(s, hp, ref, R.sum_depth(n, order), exact)
        for fma in (False, True):
            e = R.emu(s, hp, order, ho, fma)
            for k, r in R.ratios(e, ref, B).items():
                worst[k] = max(worst.get(k, 0.0), r)
            assert e["step"] == ref["step"]
            assert e["metrics"][3] == R.f32(s["step"])
            n_ref, n_emu = ref["metrics"][0], e["metrics"][0]
            assert n_emu == n_ref or abs(n_emu - n_ref) <= B["en"] * n_ref, (order, n_emu, n_ref)
            assert abs(e["metrics"][2] - ref["lr"]) <= (B["elr"] + R.U) * ref["lr"]
    return ref, worst


@pytest.mark.parametrize("group", R.GROUPS)
def test_emulation_stays_inside_the_bound(group):
    for name, s, hp, exact in R.regimes(N, group):
        ref, worst = _inside(s, hp, exact)
        print(f"{group}: {name}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, (name, worst)
        assert np.isfinite(ref["p"]).all()


def test_inf_and_nan_gradients_follow_fp32_semantics():
    name, s, hp, _ = R.regimes(N, "norm")[-1]
    assert "1e20" in name
    for order in ("flat", "slots"):
        e = R.emu(s, hp, order, HEAD)
        assert e["gmul"] == 0.0 and math.isinf(e["metrics"][0]) and e["metrics"][1] == hp.clip and np.isfinite(e["p"]).all()
    ref = R.model(s, hp)
    assert ref["gmul"] == 0.0 and math.isinf(ref["norm"]) and ref["metrics"][1] == hp.clip
    s = R.nan_state(N)
    ref, e = R.model(s, R.Hyper()), R.emu(s, R.Hyper())
    assert math.isnan(ref["metrics"][0]) and math.isnan(e["metrics"][0]) and np.isnan(e["p"]).all() and np.isnan(ref["p"]).all()


def test_exact_norm_rows_are_exact_in_fp32():
    for n in (5, 1027, N):
        s, norm = R.exact_norm_state(n)
        r = math.isqrt(n)
        for order, ho in (("flat", 0), ("slots", n // 4 + 1)):
            assert float(R.emu_sumsq(s["g"], order, ho)) == r * r * 2.0 ** -24
        up, dn = float(np.nextafter(np.float32(norm), np.float32(np.inf))), float(np.nextafter(np.float32(norm), np.float32(0)))
        for clip, clipped in ((norm, True), (up, False), (dn, True)):
            hp = R.Hyper(clip=clip)
            assert hp.clip == clip                                           # representable
            e, ref = R.emu(s, hp), R.model(s, hp)
            assert e["metrics"][0] == norm == ref["norm"] and ref["unclipped"] == (not clipped)
            assert e["metrics"][1] == min(norm, clip)
            assert (e["gmul"] == 1.0) == (not clipped or clip == norm)
    # `<=` for `<` at norm == clip: the same function (clip / norm is exactly 1)
    s, hp, exact, _ = R.fault_case("clip-le")
    a, b = R.model(s, hp), R.model(s, hp, "clip-le")
    assert a["unclipped"] != b["unclipped"] and a["gmul"] == b["gmul"] and np.array_equal(a["p"], b["p"]) and a["metrics"] == b["metrics"]


# what the old thresholds (1e-6 of |w| on parameters and EMA; 1e-4 of the update as one ratio) see on their own N(0, 0.01) draw
OLD_NOTICES = {
    "eps-inside-sqrt": (True, True), "eps-before-bias-correction": (True, True), "lr-index-off-by-one": (False, False),
    "bias-correction-from-step": (True, True), "grad-scale-once": (False, False), "norm-without-grad-scale": (False, False),
    "sumsq-head-dropped": (False, False), "sumsq-tail-twice": (False, False), "tile-updated-twice": (True, True),
    "pack-transposed-pre-update": (False, False), "ema-mixes-old-parameter": (True, False), "ema-never-moves": (True, False),
    "v-from-unclipped-gradient": (True, True), "clip-always": (False, False), "metrics-step-after-increment": (False, False),
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_leaves_the_bound(fault):
    s, hp, exact, kw = R.fault_case(fault)
    ref, worst = _inside(s, hp, exact)
    assert max(worst.values()) <= 1.0                                        # the regime itself has room
    B = R.bounds(s, hp, ref, R.sum_depth(N, "slots"), exact)
    bad = R.model(s, hp, fault, **kw)
    if fault == "pack-transposed-pre-update":
        lay = R.layout(*R.MODELS["dense42"])
        st = R.base_state(lay["n_params"], 3)
        new = R.emu(st, hp)["p"]
        before = np.full(lay["n_wpack"], 0x7FC1, dtype=np.uint16)
        good, wrong = R.pack_model(new, lay["dense"], before), R.pack_model(new, lay["dense"], before, fault, st["p"])
        left = int((good != wrong).sum())
        print(f"{fault}: {left} pack elements differ")
        assert left > 0
        return
    if fault == "metrics-step-after-increment":
        assert bad["metrics"][3] != ref["metrics"][3]
        return
    r = R.ratios(bad, ref, B)
    print(f"{fault}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) > 1.0, r


def test_old_thresholds_table():
    got = {f: R.old_thresholds_notice(f) for f in R.FAULTS}
    for f, (a, b) in got.items():
        print(f"{f:32s} params/ema 1e-6 of |w|: {'notices' if a else 'misses'}   update 1e-4: {'notices' if b else 'misses'}")
    assert got == OLD_NOTICES
    missed = [f for f, (a, b) in got.items() if not a and not b]
    assert len(missed) >= 8


@pytest.mark.parametrize("key", sorted(R.MODELS))
def test_work_tables_own_every_parameter_once(key):
    lay = R.layout(*R.MODELS[key])
    t = R.opt_tables(lay)
    assert t["fused"] and t["count"].min() == 1 and t["count"].max() == 1 and (t["form"] >= 0).all()
    sizes = [int(np.prod(sh)) for _, _, sh in lay["tensor_table"]]
    offs = [o for _, o, _ in lay["tensor_table"]]
    assert offs == list(np.cumsum([0] + sizes[:-1])) and offs[-1] + sizes[-1] == lay["n_params"]
    forms = set(int(f) for f in np.unique(t["form"]))
    assert R.FAST in forms and R.FLAT in forms
    if key != "dense64":
        assert R.EDGE in forms and len(t["parts"][1]["tail"]) == 2
    else:
        assert max(b - a for p in t["parts"] for a, b in p["flats"]) > 1024
    # head_off is a multiple of 128 in every configuration the engine accepts (embed = film = 128, mlp_dims % 256 == 0), and the
    # buffers are 256-byte aligned: the engine never gives grad_sumsq_slots_kernel head scalars; the emulation above does (HEAD)
    assert lay["head_off"] % 128 == 0 and all(len(p["head"]) == 0 for p in t["parts"])


def test_a_deep_dense_model_overflows_the_tables():
    lay = R.layout("DenseDDPM", 42, 12, 1, 256)               # 12 blocks x 5 kernels + out_proj = 61 > 60 in the output-stage slice
    assert not R.opt_tables(lay)["fused"]
