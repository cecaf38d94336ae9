"""The engine's multi-problem weight-gradient launchers, element by element, on problem lists of the test's choosing.

smd_wgrad_lab_launch (include/smd_hip_lab.h) runs launch_gemm_tn_grouped (kind 0: the 128 x 128-tile kernel, up to 8 problems
per launch, one split-K factor, slabs carved from one workspace, one reduce_slabs_kernel) or launch_gemm_tn256_multi (kind 1:
1..4 problems of the 256 x 256-tile kernel, direct write when unsplit) and reports the (tiles, nsplit, ktiles_per_split) each
kernel launch really used.  Every case:
  * X ~ N(0, 1), dY ~ 0.1 N(0, 1) + 0.01 as bf16, the padding columns finite garbage (tests/_wgrad_ref.make_problem);
  * out, bias_out and the slab start as NaN; a written NaN, an unwritten element or a read of the slab's stale part shows;
  * runs twice, bitwise equal;
  * dW and db against float64 of the same operands (computed on the device) under the element-wise bound of
    tests/_wgrad_ref.py, with the nsplit the launch reported; the worst |err| / bound is printed;
  * the slab behind the launch's nsplit * sum(stride) floats is still NaN.
test_the_cases_reach_every_path asserts over the reported plans that the cases are on the paths they are meant for.
"""
import ctypes

import pytest
import torch

import _wgrad_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


@pytest.fixture(scope="module")
def ws(L, dev):
    """(zero page, slab of the engine's size): shared, the slab is refilled with NaN by every run"""
    return torch.zeros(128, dtype=torch.bfloat16, device=dev), torch.empty(int(L.smd_gemm_tn_slab_elems()), device=dev)


def st():
    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def launch(L, kind, probs, zero, slab, slab_elems):
    """probs: [(X, ldx, dY, ldy, Mrows, Kd, N, out, ldo, bias)] device tensors -> (rc, [(tiles, nsplit, per)] per kernel launch)"""
    import smd_amd.lib as lib
    arr = (lib.WgradProblem * max(1, len(probs)))()
    for a, (X, ldx, dY, ldy, Mrows, Kd, N, out, ldo, bias) in zip(arr, probs):
        a.X, a.dY, a.out, a.bias_out = X.data_ptr(), dY.data_ptr(), out.data_ptr(), None if bias is None else bias.data_ptr()
        a.ldx, a.ldy, a.ldo, a.Mrows, a.Kd, a.N = ldx, ldy, ldo, Mrows, Kd, N
    plan = (ctypes.c_int32 * 30)(*([-1] * 30))
    count = ctypes.c_int32(-1)
    rc = L.smd_wgrad_lab_launch(arr, len(probs), kind, zero.data_ptr(), slab.data_ptr(), slab_elems, plan, 30, ctypes.byref(count), st())
    return rc, [tuple(plan[3 * j:3 * j + 3]) for j in range(max(0, count.value))]


def stride128(Kd, N):
    return (Kd * N + N + 3) // 4 * 4


_RATIOS = {0: [0.0, 0.0], 1: [0.0, 0.0]}         # kind -> worst |err| / bound seen (dW, db)


def run_group(L, dev, ws, kind, specs, Mrows, seed, slab_elems=None, ldo_pad=0, what=""):
    """specs: [(Kd, N, ldx, ldy, with_bias)].  Runs the list twice and checks everything the module docstring lists.
    -> the reported plans [(tiles, nsplit, ktiles_per_split)]"""
    import smd_amd.lib as lib
    zero, slab = ws
    slab_elems = slab.numel() if slab_elems is None else slab_elems
    ops, refs = [], []
    for i, (Kd, N, ldx, ldy, with_bias) in enumerate(specs):
        X, dY = R.small_problem(Mrows) if (Kd, N, ldx, ldy) == (128, 128, 128, 128) and len(specs) == 1 else R.make_problem(seed + i, Mrows, Kd, N, ldx, ldy)
        Xd, Yd = X.to(dev), dY.to(dev)
        ops.append((Xd, Yd))
        refs.append(R.reference(Xd[:, :Kd], Yd[:, :N]))
    runs = []
    for _ in range(2):
        slab.fill_(NAN)
        outs = [(torch.full((Kd, N + ldo_pad), NAN, device=dev), torch.full((N,), NAN, device=dev) if wb else None)
                for Kd, N, ldx, ldy, wb in specs]
        probs = [(Xd, ldx, Yd, ldy, Mrows, Kd, N, o, N + ldo_pad, b) for (Xd, Yd), (Kd, N, ldx, ldy, wb), (o, b) in zip(ops, specs, outs)]
        rc, plans = launch(L, kind, probs, zero, slab, slab_elems)
        lib.check(rc, what)
        torch.cuda.synchronize()
        runs.append((outs, plans))
    (outs, plans), (outs2, plans2) = runs
    assert plans == plans2 and len(plans) == ((len(specs) + 7) // 8 if kind == 0 else 1), plans
    worst = [0.0, 0.0]
    for i, ((Kd, N, ldx, ldy, wb), (o, b), (o2, b2), ref) in enumerate(zip(specs, outs, outs2, refs)):
        assert same_bits(o, o2) and (b is None or same_bits(b, b2)), f"{what}: problem {i} differs between two runs"
        tiles, nsplit, per = plans[i // 8 if kind == 0 else 0]
        if ldo_pad:
            assert bool(torch.isnan(o[:, N:]).all()), f"{what}: problem {i}: columns N .. ldo were written"
        rW, rb = R.check(o[:, :N], b, ref, Mrows, nsplit, Kd // 256 if kind == 1 else 1, what=f"{what}: problem {i} ({Kd} x {N})")
        worst = [max(worst[0], rW), max(worst[1], rb)]
    # the slab: nothing behind what the launch's partials take (kind 0: every launch starts again at the beginning)
    if kind == 0:
        used = 0
        for j, (tiles, nsplit, per) in enumerate(plans):
            group = specs[8 * j:8 * j + 8]
            assert tiles == sum(-(-Kd // 128) * -(-N // 128) for Kd, N, *_ in group)
            used = max(used, nsplit * sum(stride128(Kd, N) for Kd, N, *_ in group) if nsplit > 1 else 0)
        assert used <= slab_elems
    else:
        tiles, nsplit, per = plans[0]
        assert tiles == sum((Kd // 256) * (N // 256) for Kd, N, *_ in specs)
        used = sum(((nsplit * Kd * N if nsplit > 1 else 0) + (nsplit * (Kd // 256) * N) + 3) // 4 * 4 for Kd, N, *_ in specs)
    assert bool(torch.isnan(slab[used:]).all()), f"{what}: the slab was written behind its first {used} floats"
    total_kt = -(-Mrows // 64)
    assert (nsplit - 1) * per < total_kt <= nsplit * per
    for k in (0, 1):
        _RATIOS[kind][k] = max(_RATIOS[kind][k], worst[k])
    print(f"{what}: Mrows {Mrows}, {len(specs)} problems, launches (tiles, nsplit, K-tiles per split) {plans}: worst |err| / bound dW {worst[0]:.2e} db {worst[1]:.2e}")
    return [dict(kind=kind, tiles=t, nsplit=n, per=p, total_kt=total_kt, launches=len(plans)) for t, n, p in plans]


def knob(L, key, value):
    import smd_amd.lib as lib
    lib.check(L.smd_set_tuning(key, value))


# ------------------------------------------------------------------------------------------------ the cases
def P(Kd, N, ldx=None, ldy=None, bias=True):
    r8 = lambda v: (v + 7) // 8 * 8
    return (Kd, N, ldx or r8(Kd), ldy or r8(N), bias)


E, M, C = 128, 2048, 512
ENC_LAYER = [P(E, 3 * E), P(E, E), P(E, M), P(M, E)]                      # attn.qkv, attn.out, mlp.fc1, mlp.fc2
FILM = [P(128, 512), P(512, 512), P(512, 2 * M)] * 2                      # film.k.fc1, .fc2, .ss of two DenseResBlocks
ELEVEN = [P(128, 128), P(128, 384), P(256, 128), P(42, 128, ldx=64), P(128, 146, ldy=192), P(384, 128, bias=False), P(128, 256), P(64, 64),
          P(128, 128), P(200, 136), P(128, 512, bias=False)]


def small_case(Mrows, cap, model, plan):
    def f(L, dev, ws):
        slab_elems = None if cap is None else cap * stride128(128, 128) + stride128(128, 128) - 1
        knob(L, b"tn_split_model", model)
        try:
            got = run_group(L, dev, ws, 0, [P(128, 128)], Mrows, 0, slab_elems, what=f"128x128 Mrows={Mrows} cap={cap} model={model}")
        finally:
            knob(L, b"tn_split_model", 1)
        assert [(g["tiles"], g["nsplit"], g["per"]) for g in got] == [(1, *plan)]        # what tests/test_wgrad_ref_host.py emulated
        for g in got:
            g["cap"] = cap
        return got
    return f


def group_case(kind, specs, Mrows, seed, **kw):
    def f(L, dev, ws):
        if kind == 1:
            knob(L, b"gemm_tn256", 2)
        try:
            return run_group(L, dev, ws, kind, specs, Mrows, seed, **kw)
        finally:
            knob(L, b"gemm_tn256", 1)
    return f


CASES = {f"one128-M{Mrows}-cap{cap}-model{model}": small_case(Mrows, cap, model, plan) for Mrows, cap, model, plan in R.SMALL_CASES}
CASES.update({
    # the four grouped launches of a C = 512 train step (SmdEngine::flush_grouped_wgrads), with the engine's layer shapes
    "c512-film-B64": group_case(0, FILM, 64, 100, what="FiLM generators, B = 64"),
    "c512-film-B8": group_case(0, FILM, 8, 110, what="FiLM generators, B = 8"),
    "c512-out_proj+up": group_case(0, [P(M, C), P(E, M)], 1024, 120, what="out_proj + up"),
    "c512-encoder-layer": group_case(0, ENC_LAYER, 1024, 130, what="encoder layer"),
    "c512-layer0+in_proj": group_case(0, ENC_LAYER + [P(C, E)], 1024, 140, what="layer 0 + in_proj"),
    # ragged data widths next to a 128-wide peer
    "c42-ragged": group_case(0, [P(42, E, ldx=64), P(M, 42, ldy=64), P(E, E)], 96, 150, what="in_proj / out_proj of C = 42"),
    "c146-ragged": group_case(0, [P(146, E, ldx=192), P(M, 146, ldy=192), P(E, E)], 96, 160, what="in_proj / out_proj of C = 146"),
    "eleven": group_case(0, ELEVEN, 200, 170, what="11 problems, two launches"),
    "some-without-bias": group_case(0, [P(E, E), P(E, 3 * E, bias=False), P(256, E), P(E, 256, bias=False)], 300, 190, what="bias on problems 0 and 2 only"),
    # Kd * N no multiple of 4: the last float4 of dW in reduce_slabs_kernel straddles the dW / db boundary (with a bias) or the end
    "straddle": group_case(0, [P(3, 146, ldx=8, ldy=192), P(E, E), P(3, 146, ldx=8, ldy=192, bias=False)], 200, 200, what="Kd * N % 4 != 0"),
    "256-one": group_case(1, [P(M, M)], 512, 300, what="256-wide: one 2048^2"),
    "256-four-direct": group_case(1, [P(M, M)] * 4, 512, 310, ldo_pad=4, what="256-wide: four 2048^2, direct write, ldo = N + 4"),
    "256-three-ragged": group_case(1, [P(256, 512, ldx=264, ldy=520), P(512, 256), P(256, 256)], 1000, 320, what="256-wide: three problems, ragged Mrows"),
    "256-two-short-last-split": group_case(1, [P(256, 256), P(512, 512)], 640, 330, what="256-wide: 10 K-tiles in splits of 6"),
    "256-without-bias": group_case(1, [P(256, 256, bias=False), P(256, 512)], 512, 340, what="256-wide: problem 0 without bias"),
})
_DONE = {}


def run_case(name, L, dev, ws):
    if name not in _DONE:
        _DONE[name] = CASES[name](L, dev, ws)
    return _DONE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_case(L, dev, ws, name):
    run_case(name, L, dev, ws)


def test_the_cases_reach_every_path(L, dev, ws):
    """If the planner's defaults move so that a case leaves the path it is here for, this fails: the cases do not quietly test less."""
    plans = {name: run_case(name, L, dev, ws) for name in CASES}
    flat = [dict(p, case=name) for name, ps in plans.items() for p in ps]
    k0, k1 = [p for p in flat if p["kind"] == 0], [p for p in flat if p["kind"] == 1]
    reached = {
        "unsplit, direct write": [p for p in k0 if p["nsplit"] == 1 and p["total_kt"] > 1],
        "less than one K-tile": [p for p in k0 if p["total_kt"] == 1],
        "one K-tile per split, nsplit == total_kt": [p for p in k0 if p["nsplit"] == p["total_kt"] > 1],
        "the cap of 32 splits": [p for p in k0 if p["nsplit"] == 32],
        "capacity-bound split": [p for p in k0 if p.get("cap") and p["nsplit"] == p["cap"]
                                 and any(q["nsplit"] > p["cap"] for q in k0 if q.get("cap", 0) is None and q["total_kt"] == p["total_kt"] and q["tiles"] == p["tiles"])],
        "no capacity: unsplit": [p for p in k0 if p.get("cap") == 0 and p["nsplit"] == 1],
        "short last split": [p for p in k0 if p["per"] * p["nsplit"] > p["total_kt"]],
        "two launches for one call": [p for p in k0 if p["launches"] == 2],
        "several problems, split": [p for p in k0 if p["tiles"] > 1 and p["nsplit"] > 1],
        "256-wide nsplit 1": [p for p in k1 if p["nsplit"] == 1],
        "256-wide nsplit 2": [p for p in k1 if p["nsplit"] == 2],
        "256-wide nsplit 4": [p for p in k1 if p["nsplit"] == 4],
        "256-wide short last split": [p for p in k1 if p["per"] * p["nsplit"] > p["total_kt"]],
    }
    for what, ps in reached.items():
        print(f"{what}: {sorted({p['case'] for p in ps})}")
    missing = [what for what, ps in reached.items() if not ps]
    assert not missing, f"no case reaches: {missing}"
    print(f"worst |err| / bound over all cases: 128-wide grouped dW {_RATIOS[0][0]:.2e} db {_RATIOS[0][1]:.2e}; "
          f"256-wide multi dW {_RATIOS[1][0]:.2e} db {_RATIOS[1][1]:.2e}")


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_argument_lists_are_refused_before_any_launch(L, dev, ws):
    import smd_amd.lib as lib
    zero, slab = ws

    def prob(Kd, N, Mrows, ldo=None):
        X, dY = R.make_problem(Kd + N + Mrows, Mrows, Kd, N)
        return [X.to(dev), Kd, dY.to(dev), N, Mrows, Kd, N, torch.full((Kd, ldo or N), NAN, device=dev), ldo or N, torch.full((N,), NAN, device=dev)]

    def refused(kind, probs, n=None, slab_elems=None, match=""):
        slab.fill_(NAN)
        rc, plans = launch(L, kind, [tuple(p) for p in probs][:len(probs) if n is None else n], zero, slab, slab.numel() if slab_elems is None else slab_elems)
        with pytest.raises(ValueError, match=match):
            lib.check(rc)
        torch.cuda.synchronize()
        assert plans == []
        for p in probs:
            assert bool(torch.isnan(p[7]).all()) and bool(torch.isnan(p[9]).all())
        assert bool(torch.isnan(slab).all())

    refused(0, [prob(128, 128, 96)], n=0, match="problems")                                           # n < 1
    # nine good problems and a tenth with another Mrows: the first launch of eight must not happen either
    refused(0, [prob(128, 128, 96) for _ in range(9)] + [prob(128, 128, 160)], match="contraction length")
    refused(1, [prob(256, 256, 512), prob(256, 256, 576)], match="contraction length")
    refused(0, [prob(128, 128, 96), prob(128, 128, 96, ldo=132)], match="ldo == N")
    knob(L, b"gemm_tn256", 2)
    try:
        refused(1, [prob(256, 256, 512), prob(128, 128, 512)], match="not eligible")                   # no multiple of 256
        refused(1, [prob(256, 256, 448)], match="not eligible")                                        # 7 K-tiles
        refused(1, [prob(256, 256, 512) for _ in range(5)], match="problems")                          # n > 4
        # every problem alone fits 600 000 floats (the largest takes 4 x 512 x 256 + 4 x 2 x 256), the three together do not
        refused(1, [prob(256, 512, 1000), prob(512, 256, 1000), prob(256, 256, 1000)], slab_elems=600000, match="slab workspace too small")
    finally:
        knob(L, b"gemm_tn256", 1)
    knob(L, b"gemm_tn256", 1)
    refused(1, [prob(256, 256, 512)], match="not eligible")                                            # small grid without the test knob
