"""The e4m3 criterion of tests/_e4m3_ref.py checked on the host: the from-scratch encoder against torch's float8_e4m3fn cast on
every value, every tie and one fp32 ulp to either side; the row exponent against ceil(log2(amax / 448)); the exactness premises
of the GEMM operands; and every planted fault seen by the cases tests/test_gpu_e4m3_regimes.py runs.  No GPU."""
import math

import pytest
import torch

import _e4m3_ref as R

F64 = torch.float64


def torch_cast(v):
    """the CPU cast tests/test_gpu_fp8.py relies on: float32 -> float8_e4m3fn bytes"""
    return v.float().to(torch.float8_e4m3fn).view(torch.uint8)


def test_decode_table_is_the_format():
    codes = torch.tensor(R.FINITE_CODES, dtype=torch.uint8)
    assert len(R.FINITE_CODES) == 254
    assert torch.equal(R.decode(codes), codes.view(torch.float8_e4m3fn).double())
    assert math.isnan(float(R.DECODE[0x7F])) and math.isnan(float(R.DECODE[0xFF]))
    assert float(R.DECODE[0x7E]) == 448.0 and float(R.DECODE[0x01]) == 2.0 ** -9 and float(R.DECODE[0x08]) == 2.0 ** -6
    assert float(R.DECODE[R.ONE]) == 1.0 and math.copysign(1.0, float(R.DECODE[0x80])) == -1.0


def test_encode_round_trips_all_254_finite_codes():
    codes = torch.tensor(R.FINITE_CODES, dtype=torch.uint8)
    assert torch.equal(R.encode(R.decode(codes)), codes)                       # -0.0 -> 0x80 included


def test_encode_agrees_with_torch_on_values_ties_and_their_neighbours():
    pos = R.decode(torch.arange(0, 0x7F, dtype=torch.uint8))                   # 0 .. 448 ascending
    mid = (pos[:-1] + pos[1:]) / 2
    assert torch.equal(mid, torch.tensor(sorted(R.tie_values()), dtype=F64))   # the regime's ties ARE the midpoints
    assert torch.equal(mid.float().double(), mid)
    m32 = mid.float()
    below, above = torch.nextafter(m32, torch.zeros_like(m32)), torch.nextafter(m32, torch.full_like(m32, 1e9))
    v = torch.cat([pos, mid, below.double(), above.double()])
    v = torch.cat([v, -v])
    assert torch.equal(R.encode(v), torch_cast(v))
    # ties go to the even code, the neighbours to their side
    assert torch.equal(R.encode(mid) % 2, torch.zeros(len(mid), dtype=torch.uint8))
    lo = torch.arange(0, 0x7E, dtype=torch.uint8)
    assert torch.equal(R.encode(below.double()), lo) and torch.equal(R.encode(above.double()), lo + 1)
    away = R.encode(mid, ties="away")
    assert torch.equal(away, lo + 1) and not torch.equal(away, R.encode(mid))


def test_same_value_is_blind_to_the_sign_of_zero_only():
    a = torch.arange(256, dtype=torch.uint8)
    eq = R.same_value(a[:, None], a[None, :])
    want = torch.eye(256, dtype=torch.bool)
    want[0x00, 0x80] = want[0x80, 0x00] = True
    assert torch.equal(eq, want)
    assert R.zero_sign_diffs(torch.tensor([0, 0x80, 0x80, 1]), torch.tensor([0x80, 0, 0x80, 0x81])) == 2


def test_row_exponent_against_the_closed_form():
    bits = torch.arange(0x0080, 0x7F80, dtype=torch.int32)                     # every positive normal bf16
    amax = (bits << 16).view(torch.float32)
    e = R.row_exponent(amax)
    want = torch.ceil(torch.log2(amax.double() / 448.0)).long().clamp_min(-126)
    # log2 in float64 is exact enough at 8 significant bits except AT the boundary 1.75 2^k, where the ratio is a power of two
    assert torch.equal(e, want)
    scaled = torch.ldexp(amax.double(), -e)
    ok = e > -126
    assert bool((scaled[ok] <= 448).all()) and bool((scaled[ok] > 224).all())    # the smallest e that fits
    for p in (-20, -1, 0, 1, 7, 100):
        at, nxt = torch.tensor([1.75 * 2.0 ** p]), torch.tensor([(1.75 + 2.0 ** -7) * 2.0 ** p])
        assert int(R.row_exponent(at)) == p - 8 and int(R.row_exponent(nxt)) == p - 7
        assert int(R.row_exponent(nxt, bump=False)) == p - 8
    assert int(R.row_exponent(torch.tensor([0.0]))) == 0 and int(R.row_exponent(torch.tensor([1.0]))) == -8
    assert int(R.row_exponent(torch.tensor([R.BF16_MAX]))) == 120


def test_row_exponent_clamps_on_denormals_and_tiny_rows():
    den = (torch.arange(1, 0x80, dtype=torch.int32) << 16).view(torch.float32)           # every bf16 denormal
    assert bool((R.row_exponent(den) == -126).all())
    assert int(R.row_exponent(torch.tensor([2.0 ** -126]))) == -126 and int(R.row_exponent(torch.tensor([2.0 ** -118]))) == -126
    assert int(R.row_exponent(torch.tensor([2.0 ** -117]))) == -125
    x = R.regime_row("denormal", 520, 0).unsqueeze(0)
    q, e = R.quantize_rows(x)
    y = torch.ldexp(x.double(), torch.tensor(126))                                       # k 2^-7, k = 1 .. 127: all of them survive
    assert int(e) == -126 and bool(((q & 0x7F) != 0).all()) and bool(((R.decode(q) - y).abs() <= y.abs() * 2.0 ** -4).all())


@pytest.mark.parametrize("rows,K,ld", R.QUANT_SHAPES)
def test_quantiser_cases_hold_what_they_name(rows, K, ld):
    seen = set()
    for call in R.quant_calls(rows):
        c = R.quant_case(rows, K, ld, call)
        x, q, e = c["x"][:, :K].double(), c["q"], c["e"]
        assert bool(torch.isfinite(c["x"]).all()) and (ld == K or bool((c["x"][:, K:].double() > 1e38).all()))
        amax = x.abs().amax(1)
        for r, name in enumerate(c["names"]):
            seen.add(name)
            if name == "zero":
                assert int(e[r]) == 0 and bool(R.same_value(q[r], torch.zeros(K, dtype=torch.uint8)).all())
                continue
            top = float(amax[r]) * 2.0 ** -int(e[r])
            assert (224 < top <= 448) or name == "denormal"
            assert int(q[r].long().bitwise_and(0x7F).max()) <= 0x7E
            if name == "m175":
                assert top == 448 and int(q[r].long().bitwise_and(0x7F).max()) == 0x7E
            if name == "m175_next":
                assert top == 225
            if name == "neg_amax":
                assert float(x[r].min()) == -float(amax[r])
            if name.startswith("slot"):
                assert int(x[r].abs().argmax()) % 8 == int(name[4:])
            if name == "last_col":
                assert int(x[r].abs().argmax()) == K - 1
            if name == "sub_mid":
                assert bool((q[r, :K - 1].long() & 0x7F == 0).all()) and int((q[r] == 0x80).sum()) > 0 or K == 8
        # the dequantised values sit within one spacing of the input (its binade, or the subnormal spacing 2^-9 2^e)
        d = torch.ldexp(R.decode(q), e.unsqueeze(1).expand(-1, K))
        spacing = torch.ldexp(torch.ones_like(d), (torch.frexp(d.abs().clamp_min(2.0 ** -7 * torch.exp2(e.double()).unsqueeze(1)))[1] - 4))
        assert bool(((d - x).abs() <= spacing).all())
    assert seen == set(R.REGIMES)                                              # every regime meets every shape


@pytest.mark.parametrize("fault", R.QUANT_FAULTS)
def test_quantiser_faults_are_seen(fault):
    hits = {}
    for rows, K, ld in R.QUANT_SHAPES:
        for call in R.quant_calls(rows):
            c = R.quant_case(rows, K, ld, call)
            q, e = R.quantize_rows(c["x"][:, :K].contiguous(), fault=fault)
            bad = (~R.same_value(q, c["q"])).any(1) | (e != c["e"])
            for r in torch.nonzero(bad).flatten().tolist():
                hits.setdefault(c["names"][r], set()).add((rows, K))
    print(f"{fault}: seen by {sorted(hits)}")
    if fault == "exponent-without-bump":
        assert "m175_next" in hits and "m175" not in hits and "bf16_max" in hits
        assert len(hits["m175_next"]) == len(R.QUANT_SHAPES)                   # at every shape
    elif fault == "round-half-away":
        assert "ties" in hits and len(hits["ties"]) == len(R.QUANT_SHAPES)
    else:
        assert "last_col" in hits and {k for _, k in hits["last_col"]} == {520, 1024, 2048}     # every K with a second pass
        assert all(k > 512 for v in hits.values() for _, k in v)


def _gemm_cases():
    out = [R.gemm_case(*s) for s in R.GEMM_SHAPES]
    out += [R.gemm_case(*R.ONEHOT_SHAPE, kind=k) for k in ("onehot_a", "onehot_b")]
    return out


def test_gemm_operands_meet_the_exactness_condition():
    for c in _gemm_cases():
        K = c["K"]
        mag = R.exact_condition(c["A8"][:, :K], c["sa"], c["B8"][:, :K], c["sb"])
        assert mag <= 16 * K <= 2 ** 15
        want = c["want"]
        assert torch.equal(want.float().double(), want)                        # fp32 holds the result
        # ... and every partial sum: an integer below 2^24 times one power of two inside the normal range
        sh = c["sa"][:, None] + c["sb"][None, :]
        assert int(sh.min()) >= -16 and int(sh.max()) <= 16 and mag < 2 ** 24
        for e, n in ((c["sa"], c["M"]), (c["sb"], c["N"])):
            i = torch.arange(n)
            assert bool((e != e[i ^ 1]).all()) and bool((e[32:] != e[:-32]).all())
        if c["lda"] > K:
            assert bool((c["A8"][:, K:] == R.PAD_BYTE).all()) and bool((c["B8"][:, K:] == R.PAD_BYTE).all())
        for t in (c["bias"], c["res"]):
            assert torch.equal(t.double() * 64, (t.double() * 64).round())


def test_onehot_output_names_the_k_index():
    M, N, K = R.ONEHOT_SHAPE
    c = R.gemm_case(M, N, K, kind="onehot_a")
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    k = (37 * m + 11) % K
    assert torch.equal(c["want"], torch.ldexp(((n + 3 * k) % 9 - 4).double(), c["sa"][:, None] + c["sb"][None, :]))
    c = R.gemm_case(M, N, K, kind="onehot_b")
    k = (37 * n + 11) % K
    assert torch.equal(c["want"], torch.ldexp(((m + 3 * k) % 9 - 4).double(), c["sa"][:, None] + c["sb"][None, :]))


@pytest.mark.parametrize("fault", sorted(R.GEMM_FAULTS))
def test_gemm_faults_are_seen_by_every_case(fault):
    for c in _gemm_cases():
        got = R.GEMM_FAULTS[fault](c)
        n = int((got != c["want"]).sum())
        assert n > 0, (fault, c["M"], c["N"], c["K"])
        # ... and by the bf16-output bound as well as by bit equality
        ref, bound = R.epilogue_ref(c["want"], bf16_out=True)
        assert R.worst_ratio(got, ref, bound) > 1.0


def test_random_operands_span_twenty_binades_and_the_bound_is_relative():
    a, b = R.random_operands()
    qa, ea = R.quantize_rows(a)
    qb, eb = R.quantize_rows(b)
    assert int(ea.max()) - int(ea.min()) >= 18 and int(eb.max()) - int(eb.min()) >= 18
    ref, bound = R.random_ref(qa, ea, qb, eb)
    assert bool((bound > 0).all()) and bool(torch.isfinite(ref).all())
    # the bound is 2.4e-4 of sum |a b| at K = 2048, an average product 4.9e-4 of it: a dropped large product is outside
    d = R.dequant(qa, ea)[3] * R.dequant(qb, eb)[5]
    assert float(d.abs().max()) > 4 * float(bound[3, 5])
