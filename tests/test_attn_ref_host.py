"""The element-wise attention criterion (tests/_attn_ref.py) is right, has room and is sharp: CPU only.

  * the closed-form forward / backward equal float64 autograd of softmax(q k^T / sqrt(d)) v and the oracle's self_attention;
  * every regime has the property it claims, as a number;
  * the kernels' rounding points, restated in float64 (qs, p, dS and the outputs in bf16), stay inside the bound against the exact
    reference in every regime at head widths 8, 16 and 32 -- and a bound of 2^-9 |x| per bf16 store would not hold for ONE
    correctly rounded store (test_half_spacing_of_bf16...), which is why the bound counts the half-spacing hulp(x) instead;
  * each planted fault leaves the bound in at least one regime; PLANTED records, per fault and regime, whether the element-wise
    criterion and / or the whole-matrix rel() < 6e-3 (o) / 1e-2 (dqkv) of tests/test_gpu_kernels.py see it, as found.
    What only the element-wise criterion sees: a dS row dot product over half the keys and a dk without its scale wherever the
    softmax is sharp (sharp30, routing: dq and dk are then ~1e-5 of dv in norm, and the whole-matrix ratio is taken over
    [dq | dk | dv]), the same dot product with two tied keys, and a key swap confined to one head of the mixed sample.
"""
import math

import pytest
import torch

import _attn_ref as R
import ddpm_oracle as O

GEOM = [(16, 8), (8, 16), (4, 32)]          # (heads, head width) at stream width 128


@pytest.mark.parametrize("H,d", GEOM + [(2, 32), (6, 16)])
def test_closed_form_equals_autograd_and_the_oracle(H, d):
    qkv, dO = R.make_rows("mixed", H, d, 3)
    E, rows = H * d, 96
    leaf = qkv.double().clone().requires_grad_(True)
    q, k, v = [t.view(3, 32, H, d).transpose(1, 2) for t in leaf.split(E, dim=-1)]
    p = torch.softmax((q / math.sqrt(d)) @ k.transpose(-1, -2), dim=-1)
    o = (p @ v).transpose(1, 2).reshape(rows, E)
    (o * dO.double()).sum().backward()
    r = R.backward(qkv, dO, H)
    assert float((R.forward(qkv, H)["out"] - o.detach()).abs().max()) <= 1e-12 * float(o.detach().abs().max())
    assert float((r["out"] - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max())
    # the oracle's self_attention (its qkv projection in front, an identity out projection behind)
    g = torch.Generator().manual_seed(H)
    x = torch.randn(3, 32, E, generator=g, dtype=torch.float64)
    params = {"a.qkv.kernel": 0.4 * torch.randn(E, 3 * E, generator=g, dtype=torch.float64), "a.qkv.bias": torch.zeros(3 * E, dtype=torch.float64),
              "a.out.kernel": torch.eye(E, dtype=torch.float64), "a.out.bias": torch.zeros(E, dtype=torch.float64)}
    want = O.self_attention(x, params, "a", H).reshape(rows, E)
    mine = R.forward((x @ params["a.qkv.kernel"]).reshape(rows, 3 * E), H)["out"]
    assert float((mine - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_half_spacing_of_bf16_is_the_store_bound_and_2_to_minus_9_is_not():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.9921875 + 2.0 ** -8, 3.0 + 2.0 ** -7 * 0.999], dtype=torch.float64)
    err = (R.bf(x).double() - x).abs()
    assert bool((err <= R.hulp(x)).all())
    assert float(err[0]) > 2.0 ** -9 * float(x[0])             # a correct store of 1 + 2^-8 misses 2^-9 |x| by a factor 2
    every = torch.arange(0x0080, 0x7F80, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).double()     # every positive normal bf16
    mid = (every[:-1] + every[1:]) / 2
    assert bool(((R.bf(mid).double() - mid).abs() <= R.hulp(mid)).all())
    assert bool((R.hulp(every) <= 2.0 ** -8 * every).all()) and bool((R.hulp(every) > 2.0 ** -9 * every * (1 - 2.0 ** -7)).all())


@pytest.mark.parametrize("H,d", GEOM)
def test_every_regime_has_the_property_it_claims(H, d):
    out = []
    for name in R.HEAD_REGIMES:
        qkv, _ = R.make_rows(name, H, d, 5)
        fw = R.forward(qkv, H)
        s, p = fw["s"], fw["p"]
        spread = s.max(-1).values - s.min(-1).values
        if name == "uniform":
            out.append(f"uniform: median spread {float(spread.median()):.2f}, max p {float(p.max()):.2f}")
            assert float(spread.median()) < 4.0
        elif name in ("sharp8", "sharp30"):
            share99, share50 = float((p.max(-1).values > 0.99).double().mean()), float((p.max(-1).values > 0.5).double().mean())
            out.append(f"{name}: median spread {float(spread.median()):.1f}, rows with max p > 0.99: {share99:.2f}, > 0.5: {share50:.2f}")
            want = 8.0 if name == "sharp8" else 30.0
            assert abs(float(spread.median()) - want) < 0.1 * want
            # logits of rank <= d over 32 keys of equal norm are symmetric about 0: the gap to the runner-up is about half the
            # spread, so a spread of 8 gives max p ~ 0.5 (peaked, not saturated) and 30 saturates every row
            if name == "sharp30":
                assert share99 >= 0.9
            else:
                assert share50 >= 0.3 and float((s.argmax(-1) == torch.tensor(R.PI)).double().mean()) == 1.0
        elif name in ("offset", "offset100"):
            L = 80.0 if name == "offset" else 100.0
            out.append(f"{name}: min |logit| {float(s.abs().min()):.1f}, max {float(s.abs().max()):.1f}, median spread {float(spread.median()):.2f}")
            assert float(s.abs().min()) > L - 3 and float(s.abs().max()) < L + 3 and 0.5 < float(spread.median()) < 2.0
            assert bool((s[0::2] > 0).all()) and bool((s[1::2] < 0).all())         # the sign goes with the sample
        elif name == "ties2":
            out.append(f"ties2: p of the tied keys {float(p[..., 0].min())!r} .. {float(p[..., 1].max())!r}, the rest <= {float(p[..., 2:].max()):.1e}")
            assert torch.equal(p[..., 0], p[..., 1]) and float((p[..., 0] - 0.5).abs().max()) <= 2.0 ** -53
        elif name == "ties32":
            out.append(f"ties32: p in [{float(p.min())!r}, {float(p.max())!r}]")
            assert bool((p == 1.0 / 32).all())
        elif name == "routing":
            hit = float((s.argmax(-1) == torch.tensor(R.PI)).double().mean())
            v = fw["v"]
            o_is_v = torch.equal(R.bf(fw["o"]), R.bf(v[:, :, R.PI]))
            distinct = min(int(torch.unique(v[b, h], dim=0).shape[0]) for b in range(v.shape[0]) for h in range(H))
            out.append(f"routing: argmax == pi on {hit:.2f} of the rows, 1 - max p <= {float(1 - p.max(-1).values.min()):.1e}, bf16(o_i) == v_pi(i): {o_is_v}")
            assert hit == 1.0 and o_is_v and distinct == 32 and torch.equal(R.bf(v).double(), v)
    names = {n for b in range(5) for n in R.head_names("mixed", H, b)}
    assert names == set(R.HEAD_REGIMES) and len(set(R.head_names("mixed", 4, 0))) == 4
    print(f"H={H} d={d}: " + "; ".join(out))


_HOST_WORST = {}


@pytest.mark.parametrize("name", R.REGIMES)
@pytest.mark.parametrize("H,d", GEOM)
def test_the_restated_rounding_points_stay_inside_the_bound(H, d, name):
    qkv, dO = R.make_rows(name, H, d, 5)
    fq = R.forward(qkv, H, qs_bf16=True)
    rf = R.worst_ratio(R.forward_rounded(qkv, H), fq["out"], R.forward_bound(fq, "fused"))
    bw = R.backward(qkv, dO, H)
    rb = R.worst_ratio(R.backward_rounded(qkv, dO, H), bw["out"], R.backward_bound(bw, "fused"))
    # the plain kernels round only their outputs, the fp32 kernel nothing: the exact result, stored, is inside their bounds
    fw = R.forward(qkv, H)
    rp = R.worst_ratio(R.bf(fw["out"]), fw["out"], R.forward_bound(fw, "plain"))
    r32 = R.worst_ratio(fw["out"].float(), fw["out"], R.forward_bound(fw, "f32") + R.U * fw["out"].abs())
    nflag = int((fq["qstep"] > 0).sum())
    print(f"{name} d={d}: restated rounding points, worst |err| / bound: fwd {rf:.3f} bwd {rb:.3f} (plain store {rp:.3f}); "
          f"{nflag} of {fq['qstep'].numel()} qs within {R.QS_ULPS} fp32 ulps of a bf16 boundary; "
          f"max |p(fwd) - p(bwd)| {R.delta_p_fwd_bwd(qkv, H):.2e}")
    assert rf <= 1.0 and rb <= 1.0 and rp <= 1.0 and r32 <= 1.0
    assert (d != 16) or R.delta_p_fwd_bwd(qkv, H) == 0.0
    _HOST_WORST[(name, d)] = (rf, rb)


# fault -> one letter per regime of R.REGIMES: B both criteria see it, E only the element-wise one, - neither (the fault changes
# nothing there), e the element-wise one sees it (asserted) and the whole-matrix ratio is within a factor 2 of its threshold (0.0118
# against 6e-3: printed, its side not asserted).  As found at 8 heads, 5 samples.
#                                 uniform sharp8 sharp30 offset offset100 ties2 ties32 routing mixed
PLANTED = {
    "no-max-subtraction":         "----B---B",
    "pv-keys-swapped":            "BBBeB--BE",
    "neighbour-head-v":           "BBBBBBB-B",
    "sum-over-one-half":          "BBBBBBBBB",
    "fwd-last-sample-from-first": "BBBBBBB-B",
    "dot-over-one-half":          "BBEBBEBEB",
    "dk-scale-dropped":           "BBEBBBBEB",
    "bwd-last-sample-from-first": "BBBBBBBBB",
}


@pytest.mark.parametrize("fault", list(PLANTED))
def test_every_planted_fault_leaves_the_bound(fault):
    H, B = 8, 5
    fwd = fault in R.FWD_FAULTS
    f = (R.FWD_FAULTS if fwd else R.BWD_FAULTS)[fault]
    row, line = "", []
    for name in R.REGIMES:
        qkv, dO = R.make_rows(name, H, 16, B)
        r = R.forward(qkv, H, qs_bf16=True) if fwd else R.backward(qkv, dO, H)
        bound = R.forward_bound(r, "fused") if fwd else R.backward_bound(r, "fused")
        assert R.worst_ratio(R.bf(r["out"]), r["out"], bound) <= 1.0          # the unplanted result passes
        got = R.bf(f(r))
        ratio, whole = R.worst_ratio(got, r["out"], bound), R.rel(got, r["out"])
        el, old = ratio > 1.0, not (whole < (R.OLD_FWD_REL if fwd else R.OLD_BWD_REL))
        row += "B" if el and old else "E" if el else "O" if old else "-"
        line.append(f"{name} {ratio:.3g} / {whole:.1e}")
    print(f"{fault}: |err| / bound and whole-matrix rel per regime: " + ", ".join(line) + f" -> {row}")
    assert "B" in row or "E" in row
    assert all(a == b or (b == "e" and a in "BE") for a, b in zip(row, PLANTED[fault])), (row, PLANTED[fault])


def test_at_least_seven_faults_and_the_selector_weights_select():
    assert len(R.FWD_FAULTS) + len(R.BWD_FAULTS) >= 7
    for paired in (False, True):
        Wqkv, Wo = R.selector_weights(3, sq=4.0, sk=0.5, paired=paired)
        W = Wqkv.double()
        for blk, s in ((W[:, :128], 4.0), (W[:, 128:256], 0.5), (W[:, 256:], 1.0), (Wo.double(), 1.0)):
            assert bool(((blk != 0).sum(0) == 1).all()) and bool(((blk != 0).sum(1) == 1).all()) and bool((blk.abs().sum(0) == s).all())
    x = R.bf(torch.randn(32, 128, generator=torch.Generator().manual_seed(0))).double()
    assert torch.equal(((x @ Wo.double()) @ Wo.double().t()), x)          # dO is an exact permutation of dh_mid and back
    # fused_targets: LayerNorm of h_in gives heads 0 .. H/2-1 q = A, k = B and the other heads the transposed problem
    for H in (4, 8, 16):
        h_in, sq = R.fused_targets("routing", H, 1)
        a1 = R.bf(O.layer_norm(h_in.double(), {"n.scale": torch.ones(128, dtype=torch.float64), "n.bias": torch.zeros(128, dtype=torch.float64)}, "n"))
        Wqkv, _ = R.selector_weights(5, sq=sq, paired=True)
        qkv = R.bf(a1.double() @ Wqkv.double())
        s = R.forward(qkv, H)["s"][0]
        pi = torch.tensor(R.PI)
        inv = torch.empty_like(pi)
        inv[pi] = torch.arange(32)
        assert bool((s[:H // 2].argmax(-1) == pi).all()) and bool((s[H // 2:].argmax(-1) == inv).all())
        assert float(R.forward(qkv, H)["p"].max(-1).values.min()) > 0.99
        # ties32: identical keys (p = 1/32 exactly in heads 0 .. H/2-1) from tokens that differ, so that v has 32 distinct rows
        h_in, sq = R.fused_targets("ties32", H, 1)
        a1 = R.bf(O.layer_norm(h_in.double(), {"n.scale": torch.ones(128, dtype=torch.float64), "n.bias": torch.zeros(128, dtype=torch.float64)}, "n"))
        Wqkv, _ = R.selector_weights(5, sq=sq, paired=True)
        qkv = R.bf(a1.double() @ Wqkv.double())
        assert bool((R.forward(qkv, H)["p"][0, :H // 2] == 1.0 / 32).all()) and int(torch.unique(qkv[:, 256:].float(), dim=0).shape[0]) == 32
