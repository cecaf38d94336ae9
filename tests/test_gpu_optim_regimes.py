"""The optimiser kernels of csrc/optim.hip, element by element, across gradient, norm, step, grad_scale and EMA regimes
(tests/_optim_ref.py holds the float64 model, the derivation of the bounds, the regimes, the fp32 emulation, the planted faults and the
work-table model; tests/test_optim_ref_host.py shows on the CPU that the bounds have room and that each planted fault leaves them).
Every assertion is |err| <= bound at every element of p, m, v, ema, an exact metric or step counter where the model says it is exact,
an untouched guard byte, or bitwise equality; nothing is fitted to GPU output.

Forms: the stand-alone smd_adam_clip_ema (grad_sumsq_kernel, adam_clip_ema_kernel) at n = 1, 3, 4, 5, 1023, 1027 and once above
2048 * 1024 + 3; the engine's fused sweep (grad_sumsq_slots_kernel, opt_prepare_kernel, adam_recast_kernel) on the four smallest models
that reach the vector tiles, the element-by-element tiles of ragged or unaligned kernels, flat runs up to and above 1024 elements and a
tail behind the last float4 of a norm slice; option "opt_fused" = 0 (the three-pass fallback) and "opt_side_blocks" (the throttled
grid-stride walk) against the fused sweep (the latter bitwise); recast_all (through refresh_weights) at K and N of 1, 63, 64, 65, 130.
Every buffer lies in a guarded arena (tests/_footprint.py); the operand pack starts as the sentinel, so its pad columns must keep it.

Not reachable through the C ABI or the engine, so not run here: launch_recast_weight (no entry point calls it), leading dimensions
other than the engine's own round_up(., 64), and head scalars in grad_sumsq_slots_kernel (the slices begin at multiples of 128 elements
of 256-byte-aligned buffers); the host test runs the emulation of the latter.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import ddpm_oracle as O
import _optim_ref as R
from _footprint import guarded

pytestmark = pytest.mark.gpu

BETAS = O.create_noise_schedule(1e-6, 0.01, 1000, "linear")
SENTINEL = np.uint16(0x7FC1)
WORST = {}                  # (form, output) -> worst |err| / bound
_ENG = {}
BIG_N = 2048 * 1024 + 1031
KEYS = sorted(R.MODELS)


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


def engine(key, train=True):
    """an engine of R.MODELS[key] (or of the tuple `key`) whose every optimiser buffer is a guarded arena"""
    if (key, train) in _ENG:
        return _ENG[(key, train)]
    import smd_amd.lib as lib
    from smd_amd.engine import Engine, NetConfig
    arch, C, Ln, K, M = R.MODELS[key] if isinstance(key, str) else key
    eng = Engine(NetConfig(architecture=arch, data_channels=C, seq_len=32, num_layers=Ln, num_heads=8, num_mlp_layers=K, mlp_dims=M,
                           num_timesteps=1000))
    lay = R.layout(arch, C, Ln, K, M)
    assert [(n, o, tuple(s)) for n, o, s in eng.tensor_table] == lay["tensor_table"]
    assert eng.head_offset == lay["head_off"] and eng.n_params == lay["n_params"] and eng.wpack.numel() == lay["n_wpack"]
    dev, n = eng.device, eng.n_params
    ar = {}
    for name in ("params", "grads", "m", "v", "ema"):
        view, ar[name] = guarded((n,), torch.float32, dev)
        view.zero_()
    wp, ar["wpack"] = guarded((lay["n_wpack"],), torch.int16, dev)
    eng.params, eng.wpack = ar["params"].view, wp
    lib.check(eng.L.smd_engine_bind_params(eng.h, P(eng.params), P(eng.wpack)), "bind_params")
    eng.lay, eng.arenas = lay, ar
    if train:
        eng.grads, eng.m, eng.v, eng.ema = (ar[k].view for k in ("grads", "m", "v", "ema"))
        eng.step_counter = torch.zeros(1, dtype=torch.int32, device=dev)
        eng.metrics = torch.zeros(4, dtype=torch.float32, device=dev)
        set_ema(eng, True)
        eng.set_option("side_wgrad", 1)
        eng.set_schedule(BETAS, with_sampler=False)
        eng.bind(4, training=True)
    _ENG[(key, train)] = eng
    return eng


def set_ema(eng, on):
    import smd_amd.lib as lib
    eng.ema = eng.arenas["ema"].view if on else None
    lib.check(eng.L.smd_engine_bind_train(eng.h, P(eng.grads), P(eng.m), P(eng.v), P(eng.ema), P(eng.step_counter), P(eng.metrics)), "bind_train")


def plant(eng, s):
    for k, name in (("p", "params"), ("g", "grads"), ("m", "m"), ("v", "v")):
        eng.arenas[name].view.copy_(torch.from_numpy(s[k]))
    if s["ema"] is not None:
        eng.arenas["ema"].view.copy_(torch.from_numpy(s["ema"]))
    eng.step_counter.fill_(int(s["step"]))
    eng.metrics.fill_(-1.0)


def read(eng, has_ema=True):
    out = {k: getattr(eng, name).cpu().numpy() for k, name in (("p", "params"), ("m", "m"), ("v", "v"))}       # params first: it joins a deferred update
    out["ema"] = eng.arenas["ema"].view.cpu().numpy() if has_ema else None
    out["wpack"] = eng.arenas["wpack"].view.cpu().numpy().view(np.uint16)
    out["step"] = int(eng.step_counter.item())
    out["metrics"] = eng.metrics.cpu().numpy().astype(np.float64)
    return out


def step(eng, s, hp):
    plant(eng, s)
    eng.optimizer_step(*hp.args())
    got = read(eng, s["ema"] is not None)
    torch.cuda.synchronize()
    return got


def judge(form, name, got, s, hp, exact, depth):
    """every element of p, m, v, ema against its bound; the metrics and the step counter exactly where the model says so"""
    ref = R.model(s, hp)
    B = R.bounds(s, hp, ref, depth, exact)
    r = R.ratios(got, ref, B)
    for k, v in r.items():
        WORST[(form, k)] = max(WORST.get((form, k), 0.0), v)
    mt = got["metrics"]
    print(f"{form}: {name}: " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"  metrics {mt.tolist()}")
    assert max(r.values()) <= 1.0, (form, name, r)
    assert got["step"] == ref["step"] and mt[3] == R.f32(s["step"])
    if math.isinf(ref["norm"]):
        assert math.isinf(mt[0]) and mt[1] == hp.clip and np.isfinite(got["p"]).all()          # fp32 semantics: gmul == 0
        assert np.array_equal(got["m"], (np.float32(hp.beta1) * s["m"]).astype(np.float32))
    elif exact or ref["S"] == 0.0:
        assert mt[0] == ref["norm"] and mt[1] == min(ref["norm"], hp.clip)
    else:
        assert abs(mt[0] - ref["norm"]) <= B["en"] * ref["norm"]
        assert mt[1] == (mt[0] if mt[0] < hp.clip else hp.clip)
    if ref["idx"] == 0:
        assert mt[2] == hp.lr0
    else:
        assert abs(mt[2] - ref["lr"]) <= (B["elr"] + R.U) * ref["lr"]
    return ref


# ------------------------------------------------------------------------------------------------ stand-alone smd_adam_clip_ema
def flat_call(L, s, hp, n):
    import smd_amd.lib as lib
    dev = torch.device("cuda:0")
    ar = {}
    for k in ("p", "g", "m", "v", "ema"):
        if s[k] is not None:
            view, ar[k] = guarded((n,), torch.float32, dev)
            view.copy_(torch.from_numpy(s[k]))
    scratch, ar["scratch"] = guarded((1024,), torch.float32, dev)
    scratch.zero_()
    stp = torch.full((1,), int(s["step"]), dtype=torch.int32, device=dev)
    metrics = torch.full((4,), -1.0, device=dev)
    h = lib.TrainHyper(hp.lr0, hp.gamma, hp.interval, hp.beta1, hp.beta2, hp.eps, hp.clip, hp.mu, hp.gs)
    ptr = lambda k: ar[k].ptr if k in ar else None
    rc = L.smd_adam_clip_ema(ptr("p"), ptr("g"), ptr("m"), ptr("v"), ptr("ema"), n, ctypes.byref(h), P(stp), ptr("scratch"), P(metrics), st())
    torch.cuda.synchronize()
    for k, a in ar.items():
        a.assert_untouched(k)
    got = {k: ar[k].view.cpu().numpy() if k in ar else None for k in ("p", "g", "m", "v", "ema")}
    got.update(step=int(stp.item()), metrics=metrics.cpu().numpy().astype(np.float64), rc=rc)
    return got


@pytest.mark.parametrize("with_ema", [True, False])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1027])
def test_flat_kernels_every_regime(L, n, with_ema):
    depth = R.sum_depth(n, "flat")
    for group in R.GROUPS:
        for name, s, hp, exact in R.regimes(n, group):
            if s["ema"] is None and with_ema:
                continue
            s = dict(s, ema=s["ema"] if with_ema else None)
            got = flat_call(L, s, hp, n)
            assert got["rc"] == 0 and np.array_equal(got["g"].view(np.uint32), s["g"].view(np.uint32))
            judge("flat", f"n={n} {name}", got, s, hp, exact, depth)


def test_flat_kernels_walk_both_grid_stride_loops(L):
    """n above 2048 * 1024 + 3: the update's 2048 workgroups and the norm's 1024 take a second trip, the 1024-slot cap holds"""
    assert BIG_N // 4 > 2048 * 256 and R.norm_blocks_for(BIG_N) == 1024
    name, s, hp, exact = R.regimes(BIG_N, "scale")[1]
    got = flat_call(L, s, hp, BIG_N)
    assert got["rc"] == 0
    judge("flat", f"n={BIG_N} {name}", got, s, hp, exact, R.sum_depth(BIG_N, "flat"))


def test_nan_gradient_is_not_hidden(L):
    s = R.nan_state(1027)
    got = flat_call(L, s, R.Hyper(), 1027)
    assert math.isnan(got["metrics"][0])
    eng = engine("dense42")
    s = R.nan_state(eng.n_params)
    got = step(eng, s, R.Hyper())
    print(f"NaN gradient: metrics {got['metrics'].tolist()}, NaN parameters {int(np.isnan(got['p']).sum())} of {got['p'].size}")
    assert math.isnan(got["metrics"][0])


# ------------------------------------------------------------------------------------------------ the engine's fused sweep
@pytest.mark.parametrize("group", R.GROUPS)
@pytest.mark.parametrize("key", KEYS)
def test_fused_sweep_every_regime(key, group):
    eng = engine(key)
    n = eng.n_params
    depth = R.sum_depth(n, "slots")
    try:
        for name, s, hp, exact in R.regimes(n, group):
            set_ema(eng, s["ema"] is not None)
            got = step(eng, s, hp)
            ref = judge(f"fused {key}", name, got, s, hp, exact, depth)
            forms = R.opt_tables(eng.lay)["form"] if name.startswith("mu 0.999") else None
            if forms is not None:                                            # the worst ratio per code form, once per model
                B = R.bounds(s, hp, ref, depth, exact)
                for f, fname in ((R.FAST, "vector tiles"), (R.EDGE, "scalar tiles"), (R.FLAT, "flat runs")):
                    sel = forms == f
                    if sel.any():
                        for k in ("p", "m", "v", "ema"):
                            WORST[(fname, k)] = max(WORST.get((fname, k), 0.0), R.worst_ratio(got[k][sel], ref[k][sel], B[k][sel]))
    finally:
        set_ema(eng, True)


@pytest.mark.parametrize("key", KEYS)
def test_fused_sweep_structure_and_pack(key):
    """a state that differs at every index: every element is updated exactly once (a second update decays m twice and leaves its
    bound), both layouts of the pack are the bf16 of the GPU's own updated fp32 parameters bit for bit, the pad columns of the pack
    keep the sentinel, nothing outside the buffers is written; and refresh_weights (recast_all) gives the same pack"""
    eng = engine(key)
    t = R.opt_tables(eng.lay)
    assert t["fused"] and t["count"].min() == 1 and t["count"].max() == 1
    forms = set(int(f) for f in np.unique(t["form"]))
    assert {R.FAST, R.FLAT} <= forms and (R.EDGE in forms or key == "dense64")
    if key == "dense64":
        assert max(b - a for p in t["parts"] for a, b in p["flats"]) > 1024 and any(kind == R.FAST for kind, _ in t["parts"][1]["blocks"])
    else:
        assert len(t["parts"][1]["tail"]) > 0
    n = eng.n_params
    s, hp = R.base_state(n, 5), R.Hyper(clip=0.5)
    eng.arenas["wpack"].view.fill_(int(SENTINEL.view(np.int16)))
    before = np.full(eng.lay["n_wpack"], SENTINEL, dtype=np.uint16)
    got = step(eng, s, hp)
    judge(f"fused {key}", "structure", got, s, hp, False, R.sum_depth(n, "slots"))
    want = R.pack_model(got["p"], eng.lay["dense"], before)
    assert (want == SENTINEL).sum() > 0 or key == "dense64"                  # there are pad columns to keep
    bad = np.nonzero(got["wpack"] != want)[0]
    assert bad.size == 0, f"{bad.size} pack elements differ from bf16(p), first at {int(bad[0])}"
    for name, a in eng.arenas.items():
        a.assert_untouched(f"{key} {name}")
    eng.arenas["wpack"].view.fill_(int(SENTINEL.view(np.int16)))
    eng.refresh_weights()
    torch.cuda.synchronize()
    assert np.array_equal(eng.arenas["wpack"].view.cpu().numpy().view(np.uint16), want)
    eng.arenas["wpack"].assert_untouched(f"{key} wpack (recast_all)")


@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
def test_recast_all_per_element(C):
    """recast_all through refresh_weights: in_proj is (C, 256) and out_proj (256, C), so K and N take the value C; leading dimensions are
    the engine's round_up(., 64), above the minimum except at C = 64"""
    eng = engine(("DenseDDPM", C, 1, 1, 256), train=False)
    lay = eng.lay
    d = {x["name"]: x for x in lay["dense"]}
    assert (d["in_proj"]["K"], d["out_proj"]["N"]) == (C, C) and d["out_proj"]["ldw"] == -(-C // 64) * 64 == d["in_proj"]["ldwt"]
    p = R.base_state(lay["n_params"])["p"]
    eng.arenas["params"].view.copy_(torch.from_numpy(p))
    eng.arenas["wpack"].view.fill_(int(SENTINEL.view(np.int16)))
    eng.refresh_weights()
    torch.cuda.synchronize()
    want = R.pack_model(p, lay["dense"], np.full(lay["n_wpack"], SENTINEL, dtype=np.uint16))
    got = eng.arenas["wpack"].view.cpu().numpy().view(np.uint16)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"C={C}: {bad.size} pack elements differ, first at {int(bad[0])}"
    assert np.array_equal(eng.arenas["params"].view.cpu().numpy().view(np.uint32), p.view(np.uint32))
    eng.arenas["wpack"].assert_untouched("wpack")
    eng.arenas["params"].assert_untouched("params")


# ------------------------------------------------------------------------------------------------ equivalences
def _same(a, b, keys):
    return {k: int((a[k].view(np.uint32 if a[k].dtype == np.float32 else a[k].dtype) != b[k].view(np.uint32 if b[k].dtype == np.float32 else b[k].dtype)).sum())
            for k in keys}


@pytest.mark.parametrize("key", ["tr42", "dense64"])
def test_three_pass_fallback_against_the_fused_sweep(key):
    """option "opt_fused" = 0 (what a DenseDDPM too deep for the tables takes by itself).  The two paths sum the norm in different
    orders, and adam_clip_ema_kernel and adam_recast_kernel are separate kernels whose a b + c the compiler contracts into fma
    independently, so the source guarantees no bitwise equality -- not even on the unclipped side, where gmul is grad_scale exactly:
    measured on MI355X, m differs in the last place at a third of the elements (tr42: p 1308, m 296401, v 4785, ema 226424 of 906538),
    the pack at none.  Asserted, what IS guaranteed: both paths inside the element bounds on the clipped and the unclipped side, the
    same step counter, LR and step metric bitwise, the fallback's pack (recast_all) the bf16 of its OWN parameters bit for bit, pad
    columns untouched, and on the unclipped side gmul-independent metrics[1] == metrics[0] on both."""
    eng = engine(key)
    n = eng.n_params
    s = R.base_state(n, 10001)
    raw = math.sqrt(float(np.sum(s["g"].astype(np.float64) ** 2)))
    keys = ("p", "m", "v", "ema", "wpack")
    before = np.full(eng.lay["n_wpack"], SENTINEL, dtype=np.uint16)
    try:
        for name, hp, clipped in (("unclipped, grad_scale 3", R.Hyper(clip=8 * raw, gs=3.0), False), ("clipped", R.Hyper(clip=raw / 4), True)):
            eng.set_option("opt_fused", 1)
            eng.arenas["wpack"].view.fill_(int(SENTINEL.view(np.int16)))
            a = step(eng, s, hp)
            eng.set_option("opt_fused", 0)
            eng.arenas["wpack"].view.fill_(int(SENTINEL.view(np.int16)))
            b = step(eng, s, hp)
            ref = judge(f"fused {key}", name, a, s, hp, False, R.sum_depth(n, "slots"))
            judge(f"three-pass {key}", name, b, s, hp, False, max(R.sum_depth(n, "slots"), R.sum_depth(n, "flat")))
            diff = _same(a, b, keys)
            print(f"{key} {name}: elements that differ between the paths {diff}; norms {a['metrics'][0]!r} {b['metrics'][0]!r}")
            assert a["step"] == b["step"] and np.array_equal(a["metrics"][2:], b["metrics"][2:])
            assert np.array_equal(b["wpack"], R.pack_model(b["p"], eng.lay["dense"], before))
            assert np.array_equal(a["wpack"], R.pack_model(a["p"], eng.lay["dense"], before))
            if not clipped:
                assert ref["unclipped"] and a["metrics"][1] == a["metrics"][0] and b["metrics"][1] == b["metrics"][0]
    finally:
        eng.set_option("opt_fused", 1)


@pytest.mark.parametrize("key", ["tr42", "dense64"])
def test_throttled_walk_is_bitwise_the_full_grid(key):
    """option "opt_side_blocks" in {1, 7, more than there are workgroups} against 0, in the opt_overlap mode that consults it (the
    output-stage slice on the side stream as a grid-stride walk) and on the caller's stream (where it is not consulted)"""
    eng = engine(key)
    n = eng.n_params
    s, hp = R.base_state(n, 4), R.Hyper(clip=0.5, interval=4, gamma=0.5)
    blocks = len(R.opt_tables(eng.lay)["parts"][1]["blocks"])
    assert blocks > 7
    keys = ("p", "m", "v", "ema", "wpack")
    try:
        ref = step(eng, s, hp)
        judge(f"fused {key}", "throttle reference", ref, s, hp, False, R.sum_depth(n, "slots"))
        for mode in (1, 0):
            eng.set_option("opt_overlap", mode)
            eng._opt_overlap = mode
            for sb in (0, 1, 7, blocks + 1000):
                eng.set_option("opt_side_blocks", sb)
                got = step(eng, s, hp)
                diff = _same(ref, got, keys)
                assert not any(diff.values()) and got["step"] == ref["step"] and np.array_equal(got["metrics"], ref["metrics"]), (mode, sb, diff)
    finally:
        eng.set_option("opt_side_blocks", 0)
        eng.set_option("opt_overlap", 0)
        eng._opt_overlap = 0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(L):
    import smd_amd.lib as lib
    from smd_amd.engine import Engine, NetConfig
    eng = engine("dense42")
    s = R.base_state(eng.n_params, 3)
    plant(eng, s)
    eng.arenas["wpack"].view.fill_(int(SENTINEL.view(np.int16)))
    for interval in (0, -3):
        with pytest.raises((ValueError, RuntimeError), match="lr_interval"):
            eng.optimizer_step(*R.Hyper(interval=interval).args())
    torch.cuda.synchronize()
    got = read(eng)
    for k, name in (("p", "p"), ("m", "m"), ("v", "v"), ("ema", "ema")):
        assert np.array_equal(got[k].view(np.uint32), s[name].view(np.uint32)), k
    assert got["step"] == 3 and (got["wpack"] == SENTINEL).all() and (got["metrics"] == -1.0).all()
    # the stand-alone entry: interval <= 0 and null pointers
    n = 1027
    s = R.base_state(n, 3)
    for hp, drop in ((R.Hyper(interval=0), None), (R.Hyper(), "p"), (R.Hyper(), "g"), (R.Hyper(), "m"), (R.Hyper(), "v")):
        got = flat_call(L, dict(s, **({drop: None} if drop else {})), hp, n)
        assert got["rc"] != 0 and got["step"] == 3 and (got["metrics"] == -1.0).all()
        for k in ("p", "m", "v", "ema"):
            if k != drop:
                assert np.array_equal(got[k].view(np.uint32), s[k].view(np.uint32)), (drop, k)
    h = lib.TrainHyper(1e-3, 0.98, 10000, 0.9, 0.999, 1e-8, 1.0, 0.999, 1.0)
    buf = torch.zeros(8, device="cuda")
    stp = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.smd_adam_clip_ema(P(buf), P(buf), P(buf), P(buf), None, 0, ctypes.byref(h), P(stp), P(buf), None, st()) != 0
    assert L.smd_adam_clip_ema(P(buf), P(buf), P(buf), P(buf), None, 8, None, P(stp), P(buf), None, st()) != 0
    assert L.smd_adam_clip_ema(P(buf), P(buf), P(buf), P(buf), None, 8, ctypes.byref(h), None, P(buf), None, st()) != 0
    torch.cuda.synchronize()
    assert int(stp.item()) == 0 and float(buf.abs().sum()) == 0.0
    # an engine without training buffers, and an fp32 engine
    cfg = dict(architecture="DenseDDPM", data_channels=42, num_layers=1, num_mlp_layers=1, mlp_dims=256)
    fresh = Engine(NetConfig(**cfg))
    with pytest.raises((ValueError, RuntimeError), match="not bound"):
        fresh.optimizer_step(1e-3)
    f32e = Engine(NetConfig(dtype="fp32", **cfg))
    before = f32e.params.clone()
    with pytest.raises((ValueError, RuntimeError), match="fp32"):
        f32e.optimizer_step(1e-3)
    torch.cuda.synchronize()
    assert torch.equal(f32e.params, before)


def test_worst_ratios_table():
    """prints the measured worst |err| / bound per form (the table of DESIGN.md section 22); runs last"""
    forms = sorted({f for f, _ in WORST})
    for f in forms:
        print(f"    {f:28s} " + "   ".join(f"{k} {WORST[(f, k)]:.3f}" for k in ("p", "m", "v", "ema") if (f, k) in WORST))
    assert all(v <= 1.0 for v in WORST.values())
