"""The two kernels of the analytic reverse variance (csrc/analytic.hip) alone on the GPU.

smd_score_moments against float64 on the same float32 inputs and table rows.  Bound per element, derived: eps_hat is one FMA of
two products (relative 2^-24 each), its square and the running sum one FMA per row, B rows and at most B / 8 + 1 chunk adds:
|err| <= 2^-23 (B + 8) sum_b (|A x_t| + |B out|)^2 + 1e-30.
smd_engine_analytic_step against float64 from the network's own eps_hat, bound of tests/test_gpu_strided.py:
|err| <= 4 * 2^-23 (|a x0| + |b x| + |sig z| + |y|) + 1e-12; a constant table against smd_engine_strided_step, bitwise.
"""
import numpy as np
import pytest
import torch

import _strided_ref as R
from test_gpu_full_walk import BETAS
from test_gpu_strided import dense_model, find_bf16_input, partials64, transformer_model

pytestmark = pytest.mark.gpu
T = 1000
K = 20
DEV = "cuda:0"


def _chunk():
    import smd_amd.lib as lib
    return lib.MOMENT_CHUNK


def run_moments(x_t, out, table_d, t, sums=None, next_t=None):
    """one smd_score_moments call on device tensors: (sums [T][...], t after the call)"""
    import smd_amd.lib as lib
    L = lib.get_lib()
    B = x_t.shape[0]
    S, C = (x_t.shape[1], x_t.shape[2]) if x_t.dim() == 3 else (1, x_t.shape[1])
    chunks = (B + _chunk() - 1) // _chunk()
    partial = torch.full((chunks, S, C), float("nan"), device=DEV)
    if sums is None:
        sums = torch.full((T, S, C), -7.0, device=DEV)
    t_ptr = torch.tensor([t], dtype=torch.int32, device=DEV)
    arrive = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(L.smd_score_moments(x_t.data_ptr(), out.data_ptr(), B, S, C, table_d.data_ptr(), T, t_ptr.data_ptr(),
                                  None if next_t is None else next_t.data_ptr(), arrive.data_ptr(), partial.data_ptr(), sums.data_ptr(),
                                  None), "score_moments")
    torch.cuda.synchronize()
    assert int(arrive.item()) == 0
    run_moments.partial = partial
    return sums, int(t_ptr.item())


# (3,32,42): VEC = 1, the last element block masked; (3,32,512): VEC = 4; (3,32,146): VEC = 1, odd row length; DenseDDPM rows;
# two full batch chunks plus 3 rows at C = 42: the cross-chunk combine and a partial chunk
SHAPES = [(3, 32, 42), (3, 32, 512), (3, 32, 146), (5, 42), (5, 512), (2 * 8 + 3, 32, 42)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_score_moments_against_float64(shape):
    import smd_amd.schedule as S
    assert _chunk() == 8
    g = torch.Generator().manual_seed(sum(shape))
    x_t = torch.randn(*shape, generator=g).to(DEV)
    out = torch.randn(*shape, generator=g).to(DEV)
    B = shape[0]
    worst = 0.0
    for kind in ("eps", "x0", "v"):
        table, next_t = S.analytic_moment_tables(BETAS, np.arange(T), kind)
        table_d, next_d = torch.from_numpy(table).to(DEV), torch.from_numpy(next_t).to(DEV)
        for t in (0, 1, 500, 999):
            sums, t_after = run_moments(x_t, out, table_d, t, next_t=next_d)
            assert t_after == (t + 1 if t < T - 1 else -1)
            A, Bc = float(table[t, 0]), float(table[t, 1])
            ax, bo = A * x_t.double().cpu(), Bc * out.double().cpu()
            want = ((ax + bo) ** 2).sum(dim=0)
            bound = 2.0 ** -23 * (B + 8) * ((ax.abs() + bo.abs()) ** 2).sum(dim=0) + 1e-30
            got = sums[t].double().cpu().reshape(want.shape)
            ratio = float(((got - want).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (kind, t, ratio)
            rest = torch.cat([sums[:t], sums[t + 1:]])
            assert bool((rest == -7.0).all())                            # only row t is written
            again, _ = run_moments(x_t, out, table_d, t, next_t=next_d)
            assert torch.equal(again[t].view(torch.int32), sums[t].view(torch.int32))     # two calls: the same bits
        # the terminators write nothing -- neither launch: the canaries of sums and of the partials stand -- and advance nothing
        for t_end in (-1, T):
            sums, t_after = run_moments(x_t, out, table_d, t_end, next_t=next_d)
            assert bool((sums == -7.0).all()) and t_after == t_end
            assert bool(torch.isnan(run_moments.partial).all())
    print(f"[score_moments {shape}] worst |err| / bound = {worst:.3f}")


def test_score_moments_refuses_misaligned_vector_inputs():
    import smd_amd.lib as lib
    import smd_amd.schedule as S
    table_d = torch.from_numpy(S.analytic_moment_tables(BETAS, np.arange(T), "eps")[0]).to(DEV)
    x = torch.randn(3 * 32 * 512 + 4, device=DEV)
    ok = x[:3 * 32 * 512].view(3, 32, 512)
    off = x[1:1 + 3 * 32 * 512].view(3, 32, 512)
    assert off.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="16-byte aligned"):
        run_moments(off, ok, table_d, 5)
    with pytest.raises(ValueError, match="null pointer"):
        L = lib.get_lib()
        lib.check(L.smd_score_moments(ok.data_ptr(), ok.data_ptr(), 3, 32, 512, table_d.data_ptr(), T, None, None, None, None, None,
                                      None), "score_moments")


# ------------------------------------------------------------------ the step with a per-element noise scale
def _setup(arch, B, C, dtype=None):
    model = transformer_model(C) if arch == "transformer" else dense_model(C)
    eng = model.engine
    shape = (B, eng.S, C) if eng.S > 1 else (B, C)
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(B, training=False)
    eng.prepare_sampler()
    return model, eng, shape


def _plan(coef, plan):
    import smd_amd.lib as lib
    coef_d, plan_d = torch.from_numpy(coef).to(DEV), torch.from_numpy(plan).to(DEV)
    sp = lib.StridePlan()
    sp.coef, sp.plan, sp.T = coef_d.data_ptr(), plan_d.data_ptr(), T
    return sp, (coef_d, plan_d)


def _sigma(table_d):
    import smd_amd.lib as lib
    st = lib.SigmaTable()
    st.sig, st.K = table_d.data_ptr(), table_d.shape[0]
    return st


@pytest.mark.parametrize("arch,B,C", [("transformer", 3, 42), ("transformer", 3, 512), ("transformer", 3, 146), ("dense", 5, 42),
                                      ("dense", 5, 512), ("transformer", 19, 42)])
def test_analytic_step_alone_against_float64(arch, B, C):
    import smd_amd.lib as lib
    import smd_amd.schedule as S
    model, eng, shape = _setup(arch, B, C)
    Sq = eng.S
    taus = S.stride_timesteps(T, K)
    g = torch.Generator().manual_seed(13)
    samples = torch.clamp(0.25 * torch.randn(*shape, generator=g), -1, 1).to(DEV)
    masks = (torch.rand(*shape, generator=g) < 0.5).float().to(DEV)
    sig = (0.05 + torch.rand(K, *shape[1:], generator=g)).to(DEV)                 # random positive, O(1)
    st = _sigma(sig)
    located = None
    worst = 0.0
    for eta, clip in ((0.0, 1.0), (0.7, float("inf"))):
        coef, plan = S.strided_coefficient_table(BETAS, taus, eta, clip)
        coef[taus, 4] = 1.0
        sp, keep = _plan(coef, plan)
        for j in (0, K // 2, K - 1):
            t = int(taus[j])
            for infill in (False, True):
                x = (torch.randn(*shape, generator=g) * (1.0 if j < K - 1 else 0.5)).to(DEV)
                z, iz = torch.randn(*shape, generator=g).to(DEV), torch.randn(*shape, generator=g).to(DEV)
                x_in = x.clone()
                t_ptr = torch.tensor([t], dtype=torch.int32, device=DEV)
                mp = torch.zeros((T, B, 3), device=DEV)
                coll = torch.full((41, *shape), 7.0, device=DEV)
                io = lib.SampleIO()
                io.x, io.t_ptr, io.z_in = x.data_ptr(), t_ptr.data_ptr(), z.data_ptr()
                io.metrics_partial, io.collection = mp.data_ptr(), coll.data_ptr()
                if infill:
                    io.infill_samples, io.infill_masks, io.infill_z_in = samples.data_ptr(), masks.data_ptr(), iz.data_ptr()
                eng.load_state(x)
                if located is None:
                    torch.cuda.synchronize()
                    located = find_bf16_input(eng, x)
                eng.analytic_step(io, sp, st)
                torch.cuda.synchronize()
                eh = eng.last_pred().clone()
                d = lambda v: v.double().cpu()
                row = dict(zip(("sqrt_recip", "sqrt_m1", "a", "b", "sigma", "clip", "sqrt_as", "sqrt_1m_as"), (float(v) for v in coef[t])))
                row.update(t=t, next_t=int(plan[t, 0]), sigma=0.0)
                base, x0, y = R.update(d(x_in), d(eh), d(z), row, T, None, d(samples), d(iz))
                sz = d(sig[j]) * d(z)
                ref = base + sz
                if infill:
                    y = row["sqrt_as"] * d(samples) + row["sqrt_1m_as"] * d(iz) if 0 <= row["next_t"] < T else d(samples)
                    ref = ref * (1 - d(masks)) + y * d(masks)
                mag = (row["a"] * x0).abs() + (row["b"] * d(x_in)).abs() + sz.abs() + (y.abs() if infill else 0)
                ratio = float(((d(x) - ref).abs() / (4 * 2.0 ** -23 * mag + 1e-12)).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (eta, clip, t, infill, ratio)
                off, nbytes, (rows, Cp) = located
                xb = eng.workspace[off:off + nbytes].view(torch.bfloat16).view(rows, Cp)
                assert torch.equal(xb[:, :C], x.reshape(rows, C).to(torch.bfloat16)) and not bool(xb[:, C:].any())
                assert int(t_ptr.item()) == int(plan[t, 0])
                want = torch.stack([partials64(d(eh), Sq), partials64(d(x_in) - ref, Sq), partials64(sz, Sq)], dim=1)
                got = mp[t].double().cpu()
                assert float(((got - want).abs() / want.abs()).max()) <= 1e-5
                mp[t] = 0
                assert not bool(mp.any())
                slot = int(plan[t, 2])
                for k in range(41):
                    assert torch.equal(coll[k], x) if k == slot else bool((coll[k] == 7.0).all()), (k, slot)
        # the terminators, a timestep off the walk, and an iteration past the table's rows: nothing changes, bit for bit
        short = _sigma(sig[:K // 2])
        for t_end, tab in ((-1, st), (T, st), (int(taus[0]) - 1, st), (int(taus[K - 1]), short)):
            t_ptr.fill_(t_end)
            mp.zero_()
            before = [v.clone() for v in (x, mp, coll, eng.workspace[off:off + nbytes])]
            eng.analytic_step(io, sp, tab)
            torch.cuda.synchronize()
            for u, v in zip(before, (x, mp, coll, eng.workspace[off:off + nbytes])):
                assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
            assert int(t_ptr.item()) == t_end
    print(f"[{arch} B={B} C={C}] analytic update: worst |err| / bound = {worst:.3f}")
    if C % 4 == 0:
        bad = _sigma(sig)
        bad.sig = sig.data_ptr() + 4
        t_ptr.fill_(int(taus[0]))
        with pytest.raises(ValueError, match="16-byte aligned"):
            eng.analytic_step(io, sp, bad)


def _one_step(eng, shape, step, j, taus, rng_mode, infill_t, bf16=True):
    """state, bf16 input bytes, collection, metrics and t after one launch of ``step`` from a fixed state"""
    import smd_amd.lib as lib
    g = torch.Generator().manual_seed(17)
    x = torch.randn(*shape, generator=g).to(DEV)
    t = int(taus[j])
    B = shape[0]
    t_ptr = torch.tensor([t], dtype=torch.int32, device=DEV)
    mp = torch.zeros((T, B, 3), device=DEV)
    coll = torch.zeros((41, *shape), device=DEV)
    io = lib.SampleIO()
    io.x, io.t_ptr = x.data_ptr(), t_ptr.data_ptr()
    io.metrics_partial, io.collection = mp.data_ptr(), coll.data_ptr()
    io.seed_lo, io.seed_hi, io.sample_offset = 1234, 99, 3
    keep = [infill_t]
    if infill_t is not None:
        io.infill_samples, io.infill_masks = infill_t[0].data_ptr(), infill_t[1].data_ptr()
    if rng_mode == "threefry":
        keys = torch.arange(4 * len(taus), dtype=torch.int32, device=DEV).reshape(2, len(taus), 2) * 7919 + 5
        io.tf_noise_keys, io.tf_infill_keys = keys[0].data_ptr(), keys[1].data_ptr()
        io.tf_n_total = (B + 3) * int(np.prod(shape[1:]))
        keep.append(keys)
    eng.load_state(x)
    torch.cuda.synchronize()
    off, nbytes, _ = find_bf16_input(eng, x) if bf16 else (0, 0, None)
    step(io)
    torch.cuda.synchronize()
    return x, eng.workspace[off:off + nbytes].clone(), coll, mp, int(t_ptr.item())


@pytest.mark.parametrize("arch,B,C", [("transformer", 3, 42), ("transformer", 3, 512), ("dense", 5, 42)])
@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("rng_mode", ["philox", "threefry"])
def test_constant_table_is_the_strided_step_bitwise(arch, B, C, sigma, rng_mode):
    import smd_amd.schedule as S
    model, eng, shape = _setup(arch, B, C)
    taus = S.stride_timesteps(T, K)
    coef, plan = S.strided_coefficient_table(BETAS, taus, 0.0)
    g = torch.Generator().manual_seed(19)
    infill_t = (torch.clamp(0.25 * torch.randn(*shape, generator=g), -1, 1).to(DEV), (torch.rand(*shape, generator=g) < 0.5).float().to(DEV))
    c_str = coef.copy()
    c_str[taus, 4] = sigma
    c_ana = coef.copy()
    c_ana[taus, 4] = 1.0
    sp_s, k1 = _plan(c_str, plan)
    sp_a, k2 = _plan(c_ana, plan)
    sig = torch.full((K, *shape[1:]), sigma, device=DEV)
    st = _sigma(sig)
    for j in (0, K - 1):
        for inf in (None, infill_t):
            a = _one_step(eng, shape, lambda io: eng.strided_step(io, sp_s), j, taus, rng_mode, inf)
            b = _one_step(eng, shape, lambda io: eng.analytic_step(io, sp_a, st), j, taus, rng_mode, inf)
            for name, u, v in zip(("state", "bf16 input", "collection", "metrics"), a[:4], b[:4]):
                assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), (name, j, inf is not None)
            assert a[4] == b[4] == int(plan[taus[j], 0])


def test_parts_one_then_two_equal_part_zero_and_fp32_refuses_them():
    import smd_amd.ncsn as N
    import smd_amd.schedule as S
    from smd_amd.engine import NetConfig
    model, eng, shape = _setup("transformer", 3, 42)
    taus = S.stride_timesteps(T, K)
    coef, plan = S.strided_coefficient_table(BETAS, taus, 1.0)
    coef[taus, 4] = 1.0
    sp, keep = _plan(coef, plan)
    sig = (0.05 + torch.rand(K, *shape[1:], generator=torch.Generator().manual_seed(23))).to(DEV)
    st = _sigma(sig)
    whole = _one_step(eng, shape, lambda io: eng.analytic_step(io, sp, st, 0), 3, taus, "philox", None)
    halves = _one_step(eng, shape, lambda io: (eng.analytic_step(io, sp, st, 1), eng.analytic_step(io, sp, st, 2)), 3, taus, "philox", None)
    for u, v in zip(whole[:4], halves[:4]):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    assert whole[4] == halves[4]
    m32 = N.Model(NetConfig(data_channels=42, num_layers=2, num_heads=8, num_mlp_layers=1, num_timesteps=T, dtype="fp32"), DEV, seed=0)
    e32 = m32.engine
    e32.set_schedule(BETAS, with_sampler=True)
    e32.bind(3, training=False)
    e32.prepare_sampler()
    for part in (1, 2):
        with pytest.raises(ValueError, match="not available under fp32"):
            _one_step(e32, shape, lambda io: e32.analytic_step(io, sp, st, part), 3, taus, "philox", None, bf16=False)
    _one_step(e32, shape, lambda io: e32.analytic_step(io, sp, st, 0), 3, taus, "philox", None, bf16=False)
