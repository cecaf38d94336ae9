"""The fused exponential Adams update (adams_step_kernel) alone, through smd_adams_step: no network, the
caller supplies the state, eps_hat, the ring, the tables and t.

Bound of the state, per element, against float64 on the float32 tables the kernel read:
  |err| <= 5 * 2^-23 * (|A0 x0| + |A1 h1| + |A2 h2| + |A3 h3| + |b x| + |y|)
the multistep kernel's four units plus one for each extra fma of the chain (h2, h3: two at most, so five covers every pattern).
Worst ratio observed on an MI355X: see DESIGN.md section 29.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import _adams_ref as A
from test_gpu_full_walk import BETAS
from test_gpu_strided import find_bf16_input, partials64, transformer_model

pytestmark = pytest.mark.gpu
T = 1000
K = 20
DEV = "cuda:0"
# (B, S, C): VEC 1 / RG 4; VEC 4 / RG 4; RG 1; ragged rows (5 rows on 4 row groups) with a second column block of one live thread
SHAPES = [(3, 32, 42), (2, 32, 512), (3, 1, 512), (2, 5, 516)]


def taus20():
    return A.logsnr_timesteps(T, K, BETAS)


def tables(corrector=True, clip=1.0):
    import smd_amd.schedule as S
    return S.adams_coefficient_table(BETAS, taus20(), corrector, clip)


def padded(C):
    return -(-C // 8) * 8


class Launch:
    """one smd_adams_step call on fresh device buffers"""

    def __init__(self, shape, coef, plan, t, x, eh, hist, infill=None, hist_ptr=None, T_arg=T):
        import smd_amd.lib as lib
        B, S, C = shape
        self.lib = lib
        d = lambda v: v.to(DEV).contiguous()
        self.coef, self.plan = d(torch.from_numpy(coef)), d(torch.from_numpy(plan))
        self.x, self.eh, self.hist = d(x.clone()), d(eh), d(hist.clone())
        self.t_ptr = torch.tensor([t], dtype=torch.int32, device=DEV)
        self.arrive = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.mp = torch.zeros((T, B, 3), device=DEV)
        self.coll = torch.full((41, *shape), 7.0, device=DEV)
        self.Cp = padded(C)
        self.xb = torch.full((B * S, self.Cp), 3.0, dtype=torch.bfloat16, device=DEV)
        a = lib.AdamsStepArgs()
        a.x, a.hist, a.eps_hat = self.x.data_ptr(), (self.hist.data_ptr() if hist_ptr is None else hist_ptr(self.hist)), self.eh.data_ptr()
        a.B, a.S, a.C, a.Cp, a.T = B, S, C, self.Cp, T_arg
        a.coef, a.plan, a.t_ptr = self.coef.data_ptr(), self.plan.data_ptr(), self.t_ptr.data_ptr()
        a.t_advance, a.arrive = self.t_ptr.data_ptr(), self.arrive.data_ptr()
        a.x_bf16, a.metrics_partial, a.collection = self.xb.data_ptr(), self.mp.data_ptr(), self.coll.data_ptr()
        if infill is not None:
            self.inf = [d(v) for v in infill]
            a.infill_samples, a.infill_masks, a.infill_z_in = (v.data_ptr() for v in self.inf)
        self.args = a

    def run(self):
        rc = self.lib.get_lib().smd_adams_step(ctypes.byref(self.args), torch.cuda.current_stream().cuda_stream)
        self.lib.check(rc, "adams_step")
        torch.cuda.synchronize()
        return self


def inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x, eh, iz = (torch.randn(*shape, generator=g) for _ in range(3))
    hist = torch.clamp(0.5 * torch.randn(3, *shape, generator=g), -1, 1)
    samples = torch.clamp(0.25 * torch.randn(*shape, generator=g), -1, 1)
    masks = (torch.rand(*shape, generator=g) < 0.5).float()
    return x, eh, hist, (samples, masks, iz)


def round32(fr):
    """the float32 nearest to the exact rational ``fr``, ties to even"""
    best = np.float32(float(fr))
    for n in (np.nextafter(best, np.float32(-np.inf)), np.nextafter(best, np.float32(np.inf))):
        d0, d1 = abs(Fraction(float(best)) - fr), abs(Fraction(float(n)) - fr)
        if d1 < d0 or (d1 == d0 and (int(n.view(np.uint32)) & 1) == 0):
            best = n
    return best


def x0_bits(sr, sm1, clip, x, eh):
    """the kernel's clamped x0 in exact arithmetic, rounded where the kernel rounds: p = rn(sm1 eh), perr = sm1 eh - p (exact),
    x0 = clamp(rn(rn(sr x - p) - perr))"""
    out = np.empty(len(x), dtype=np.float32)
    F = lambda v: Fraction(float(v))
    for i in range(len(x)):
        p = round32(F(sm1) * F(eh[i]))
        perr = round32(F(sm1) * F(eh[i]) - F(p))
        r = round32(F(round32(F(sr) * F(x[i]) - F(p))) - F(perr))
        out[i] = min(max(r, np.float32(-clip)), np.float32(clip))
    return out


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("corrector", [False, True])
def test_update_against_float64_ring_and_outputs(shape, corrector):
    B, S, C = shape
    coef, plan = tables(corrector)
    taus = taus20()
    rows = A.table_rows(coef, plan, taus, BETAS)
    x, eh, hist, infill = inputs(shape, 100 + C + S)
    d = lambda v: v.double().cpu()
    worst = 0.0
    for j in range(5):
        t = int(taus[j])
        Acoef = [float(coef[t, c]) for c in (2, 8, 9, 10)]
        assert [a != 0 for a in Acoef] == [True, j >= 1, j >= 2, corrector and j >= 3]
        hs = [hist[(j - i) % 3] for i in (1, 2, 3)]
        for use_infill in (False, True):
            L = Launch(shape, coef, plan, t, x, eh, hist, infill if use_infill else None).run()
            row = {k: (v[j] if k == "A" else (int(v[j]) if k in ("t", "next_t") else float(v[j]))) for k, v in rows.items()}
            ref, x0, y = A.update(d(x), d(eh), [d(h) for h in hs], row, T, *(d(v) for v in (infill[1], infill[0], infill[2])) if use_infill else ())
            mag = (Acoef[0] * x0).abs() + sum((Acoef[i] * d(hs[i - 1])).abs() for i in (1, 2, 3)) + (float(coef[t, 3]) * d(x)).abs()
            if use_infill:
                mag = mag + y.abs()
            ratio = float(((d(L.x) - ref).abs() / (5 * 2.0 ** -23 * mag)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (shape, j, use_infill, ratio)
            # the ring: slot j mod 3 holds the clamped x0 (before the blend), the other two are untouched bitwise
            own = j % 3
            for k in range(3):
                if k != own:
                    assert torch.equal(L.hist[k].view(torch.int32).cpu(), hist[k].view(torch.int32)), (j, k)
            mag_h = (float(coef[t, 0]) * d(x)).abs() + (float(coef[t, 1]) * d(eh)).abs()
            assert float(((d(L.hist[own]) - x0).abs() / (4 * 2.0 ** -23 * mag_h)).max()) <= 1.0
            assert float(L.hist[own].abs().max()) <= 1.0
            if C == 42:                                                # exactly: the first row of every sample
                got = L.hist[own][:, 0].reshape(-1).cpu().numpy()
                want = x0_bits(coef[t, 0], coef[t, 1], coef[t, 5], x[:, 0].reshape(-1).numpy(), eh[:, 0].reshape(-1).numpy())
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (j, use_infill)
            # t, collection row, bf16 re-cast (padding untouched), metrics row
            assert int(L.t_ptr.item()) == int(plan[t, 0]) and int(L.arrive.item()) == 0
            slot = int(plan[t, 2])
            for k in range(41):
                assert torch.equal(L.coll[k], L.x) if k == slot else bool((L.coll[k] == 7.0).all()), (k, slot)
            assert torch.equal(L.xb[:, :C], L.x.reshape(-1, C).to(torch.bfloat16)) and bool((L.xb[:, C:] == 3.0).all())
            pm = lambda v: partials64(v.reshape(B, C) if S == 1 else v, S)          # one row: the norm runs over the channels
            want = torch.stack([pm(d(eh)), pm(d(x) - ref), pm(torch.zeros_like(ref))], dim=1)
            got = L.mp[t].double().cpu()
            assert float(((got - want).abs() / want.abs()).max()) <= 1e-5
            L.mp[t] = 0
            assert not bool(L.mp.any())
    print(f"[adams update {shape} corrector={corrector}] worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_a_ring_of_nans_reaches_only_the_live_terms(shape):
    coef, plan = tables(True)
    taus = taus20()
    x, eh, hist, _ = inputs(shape, 7)
    nan = torch.full_like(hist, float("nan"))
    # j = 0: nothing of the ring is read
    t = int(taus[0])
    a, b = Launch(shape, coef, plan, t, x, eh, nan).run(), Launch(shape, coef, plan, t, x, eh, torch.zeros_like(hist)).run()
    assert bool(torch.isfinite(a.x).all()) and torch.equal(a.x.view(torch.int32), b.x.view(torch.int32))
    assert bool(torch.isfinite(a.hist[0]).all()) and bool(torch.isnan(a.hist[1:]).all())
    # j = 1: only h1 (slot 0) is read
    t = int(taus[1])
    ring = nan.clone()
    ring[0] = hist[0]
    a, b = Launch(shape, coef, plan, t, x, eh, ring).run(), Launch(shape, coef, plan, t, x, eh, hist).run()
    assert bool(torch.isfinite(a.x).all()) and torch.equal(a.x.view(torch.int32), b.x.view(torch.int32))
    ring = hist.clone()
    ring[0] = float("nan")
    assert bool(torch.isnan(Launch(shape, coef, plan, t, x, eh, ring).run().x).all())       # ... and it is read


@pytest.mark.parametrize("C", [42, 512])
@pytest.mark.parametrize("infill", [False, True])
def test_with_a2_a3_zero_it_is_the_multistep_kernel_bit_for_bit(C, infill):
    """an order-2 multistep table (a1 in column 8, columns 9 and 10 zero) through smd_engine_multistep_step and through
    smd_engine_adams_step from the same state: state, collection row, bf16 re-cast and metrics are the same bits.  (The engine
    runs its network in front of both, on the same input: the same eps_hat.)"""
    import smd_amd.lib as lib
    import smd_amd.schedule as S
    model = transformer_model(C)
    eng = model.engine
    B, shape = 3, (3, 32, C)
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(B, training=False)
    eng.prepare_sampler()
    taus = taus20()
    coef, plan = S.multistep_coefficient_table(BETAS, taus, 2)
    assert not coef[:, 9:].any()
    coef_d, plan_d = torch.from_numpy(coef).to(DEV), torch.from_numpy(plan).to(DEV)
    sp = lib.MultistepPlan()
    sp.coef, sp.plan, sp.T = coef_d.data_ptr(), plan_d.data_ptr(), T
    x_in, _, hist_in, (samples, masks, iz) = inputs(shape, 11)
    samples, masks, iz = (v.to(DEV) for v in (samples, masks, iz))
    located = None
    for j in (0, 1, 2, len(taus) - 1):
        t = int(taus[j])
        assert (coef[t, 8] != 0) == (j in (1, 2))
        out = []
        for kind in ("multistep", "adams"):
            x = x_in.to(DEV).clone()
            ring = hist_in.to(DEV).clone()
            t_ptr = torch.tensor([t], dtype=torch.int32, device=DEV)
            mp = torch.zeros((T, B, 3), device=DEV)
            coll = torch.full((41, *shape), 7.0, device=DEV)
            io = lib.SampleIO()
            io.x, io.t_ptr, io.metrics_partial, io.collection = x.data_ptr(), t_ptr.data_ptr(), mp.data_ptr(), coll.data_ptr()
            if infill:
                io.infill_samples, io.infill_masks, io.infill_z_in = samples.data_ptr(), masks.data_ptr(), iz.data_ptr()
            eng.load_state(x)
            if located is None:
                torch.cuda.synchronize()
                located = find_bf16_input(eng, x)
            if kind == "multistep":
                prev = ring[(j - 1) % 3].clone()
                eng.multistep_step(io, sp, prev)
                new_hist = prev
            else:
                eng.adams_step(io, sp, ring)
                new_hist = ring[j % 3]
            torch.cuda.synchronize()
            off, nbytes, _ = located
            out.append([v.clone() for v in (x, coll, mp, eng.workspace[off:off + nbytes], new_hist, t_ptr)])
        for u, v in zip(*out):
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), j
        assert bool(torch.isfinite(out[0][0]).all())


def test_off_the_walk_is_a_no_op_for_the_ring_too():
    shape = SHAPES[0]
    coef, plan = tables(True)
    taus = taus20()
    x, eh, hist, infill = inputs(shape, 9)
    for t in (-1, T, T + 5, int(taus[0]) - 1):
        L = Launch(shape, coef, plan, t, x, eh, hist, infill)
        before = [v.clone() for v in (L.x, L.hist, L.mp, L.coll, L.xb, L.arrive)]
        L.run()
        for u, v in zip(before, (L.x, L.hist, L.mp, L.coll, L.xb, L.arrive)):
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), t
        assert int(L.t_ptr.item()) == t


def test_argument_refusals_launch_nothing():
    coef, plan = tables(True)
    t = int(taus20()[0])
    for shape in (SHAPES[1], SHAPES[0]):
        x, eh, hist, _ = inputs(shape, 3)
        cases = [(dict(hist_ptr=lambda h: None), "null history"), (dict(T_arg=0), "T=0")]
        if shape[2] % 4 == 0:
            cases.append((dict(hist_ptr=lambda h: h.data_ptr() + 4), "16-byte aligned"))
        cases.append((dict(hist_ptr=lambda h: h.data_ptr() + 2), "not aligned to its element"))
        for kw, match in cases:
            L = Launch(shape, coef, plan, t, x, eh, hist, **kw)
            with pytest.raises(ValueError, match=match):
                L.run()
            torch.cuda.synchronize()
            assert torch.equal(L.x.cpu(), x) and torch.equal(L.hist.cpu(), hist) and int(L.t_ptr.item()) == t
    # the engine's own checks: a plan of another T, a null ring, a ring that is not the state's triple
    import smd_amd.lib as lib
    model = transformer_model(42)
    eng = model.engine
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(3, training=False)
    eng.prepare_sampler()
    coef_d, plan_d = torch.from_numpy(coef).to(DEV), torch.from_numpy(plan).to(DEV)
    sp = lib.MultistepPlan()
    sp.coef, sp.plan, sp.T = coef_d.data_ptr(), plan_d.data_ptr(), T - 1
    xs = torch.randn(3, 32, 42, device=DEV)
    ring = torch.zeros(3, 3, 32, 42, device=DEV)
    t_ptr = torch.tensor([t], dtype=torch.int32, device=DEV)
    io = lib.SampleIO()
    io.x, io.t_ptr = xs.data_ptr(), t_ptr.data_ptr()
    before = xs.clone()
    with pytest.raises(ValueError, match="timesteps"):
        eng.adams_step(io, sp, ring)
    sp.T = T
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(ValueError, match="null history"):
        lib.check(eng.L.smd_engine_adams_step(eng.h, ctypes.byref(io), ctypes.byref(sp), None, 0, st), "adams_step")
    with pytest.raises(ValueError, match="part"):
        lib.check(eng.L.smd_engine_adams_step(eng.h, ctypes.byref(io), ctypes.byref(sp), ring.data_ptr(), 3, st), "adams_step")
    for bad in (torch.zeros(3, 32, 42, device=DEV), torch.zeros(3, 3, 32, 42, dtype=torch.bfloat16, device=DEV), torch.zeros(3, 3, 32, 42)):
        with pytest.raises(ValueError, match="hist must be"):
            eng.adams_step(io, sp, bad)
    torch.cuda.synchronize()
    assert torch.equal(xs, before) and int(t_ptr.item()) == t
