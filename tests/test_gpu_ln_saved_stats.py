"""The 2048-wide LayerNorm with saved row statistics and folded FiLM constants (csrc/norm.hip: layernorm_fwd_wide_kernel,
layernorm_bwd_wide8_kernel), through the entry points smd_layernorm_fwd_stats / smd_layernorm_bwd_stats.

Every case runs the forward with a statistics buffer and the backward twice, with the saved statistics and with a NULL
pointer (recomputed), on the kernel's own inputs; everything is compared with float64 torch on the CPU at the tolerances
tests/test_gpu_kernels.py applies to these kernels (test_layernorm_fwd_bwd, test_layernorm_bwd_film_forms; the e4m3 copy at
tests/test_gpu_fp8.py::test_layernorm_fwd_e4m3's):
    bf16 outputs (forward, dx) 4e-3      fp32 dx / dgamma / dbeta / dscale+dshift 1e-4      e4m3 copy 4e-2      (rel-L2)

The statistics themselves are checked against float64 to fp32 rounding.  The kernel sums a row's 2048 values as 32 per lane
(sequential) and six xor-shuffle steps: at most 38 roundings on any path, each <= 2^-24 of the partial sum, so
    |mean - mean64| <= 38 * 2^-24 * mean(|x|)
and the same for E[x^2] (the squares enter by FMA).  var = E[x^2] - mean^2 then carries at most
    dvar = 2^-24 * (39 * E[x^2] + (2 * 38 + 2) * |mean| * mean(|x|))      (one rounding each for the product and the difference)
and rstd = rsq(var + eps) half of dvar / var relatively, plus v_rsq_f32's 1 ulp (2^-23) and the rounding of its argument.
"""
import pytest
import torch

import ddpm_oracle as O
from _footprint import guarded

pytestmark = pytest.mark.gpu

D = 2048
EPS = 1e-6
U = 2.0 ** -24
TOL_BF16, TOL_F32, TOL_E4M3 = 4e-3, 1e-4, 4e-2

# form -> (FiLM + swish, bf16 x, residual gradient, outputs: 1 fp32 dx, 2 bf16 dx, 3 both, e4m3 forward)
FORMS = {
    "plain": (False, True, None, 2, False),                  # ln_o of the training step
    "film_bf16": (True, True, None, 2, False),               # ResBlock ln2
    "film_bf16_res_bf16": (True, True, "bf16", 2, False),    # ResBlock ln1, the <..., 2, ...> form
    "film_f32_res_f32": (True, False, "f32", 3, False),      # fp32 trunk: fp32 x, fp32 residual gradient in place
    "film_bf16_e4m3": (True, True, None, 2, True),           # the e4m3-out forward (--dtype=fp8)
}
# (rows, rows_per_sample): two samples of 32 rows; nine groups of 8 with FiLM and 32 + 32 + 8 rows without (the r_end clamp
# of the last group); one group with one row per wave.  A FiLM group is a sample's rows and the launch refuses rows that are no
# multiple of rows_per_sample (check_ln), so a ragged LAST group exists only without FiLM: the plain form is where the clamp
# can be reached, and 72 rows reach it there.
SHAPES = [(64, 32), (72, 8), (8, 8)]


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bf(x):
    return x.to(torch.bfloat16)


def dequant(q, s):
    v = q.view(torch.float8_e4m3fn).float().double().cpu()
    e = (s.cpu().to(torch.int64) & 0xFF) - 127
    return v * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double()).unsqueeze(1)


def stat_bounds(xd):
    """float64 (mean, rstd) of the rows of xd and the module docstring's bounds: absolute for the mean, relative for rstd"""
    mean = xd.mean(1)
    ex2 = (xd * xd).mean(1)
    var = ex2 - mean * mean
    absx = xd.abs().mean(1)
    return mean, 1.0 / torch.sqrt(var + EPS), 38 * U * absx, 0.5 * U * (39 * ex2 + 78 * mean.abs() * absx) / var + 4 * U


_CASES = {}


def case(form, rows, rps):
    """inputs and the float64 reference of one (form, shape): computed once, shared by the tests, never modified"""
    key = (form, rows, rps)
    if key in _CASES:
        return _CASES[key]
    fs, xbf, res, om, f8 = FORMS[form]
    g = torch.Generator().manual_seed(1000 * rows + 10 * rps + len(form))
    x = torch.randn(rows, D, generator=g) * 1.3 - 0.2
    if xbf:
        x = bf(x).float()
    gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    ns = rows // rps
    ss = torch.cat([1 + 0.3 * torch.randn(ns, D, generator=g), 0.2 * torch.randn(ns, D, generator=g)], dim=1)
    dout = bf(torch.randn(rows, D, generator=g))
    dres = torch.randn(rows, D, generator=g)
    if res == "bf16":
        dres = bf(dres).float()
    dss0 = torch.randn(ns, 2 * D, generator=g)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ssr = ss.double().requires_grad_(True)
    y = O.layer_norm(xr, {"n.scale": gr, "n.bias": br}, "n")
    if fs:
        y = O.swish(ssr[:, :D].repeat_interleave(rps, 0) * y + ssr[:, D:].repeat_interleave(rps, 0))
    y.backward(dout.double())
    mean, rstd, mean_tol, rstd_rtol = stat_bounds(x.double())
    c = dict(fs=fs, xbf=xbf, res=res, om=om, f8=f8, rows=rows, rps=rps, ns=ns, x=x, gamma=gamma, beta=beta, ss=ss, dout=dout,
             dres=dres, dss0=dss0, y=y.detach(), dx=xr.grad + (dres.double() if res else 0.0), dg=gr.grad, db=br.grad,
             dss=ssr.grad if fs else None, mean=mean, rstd=rstd,
             mean_tol=mean_tol, rstd_rtol=rstd_rtol)
    _CASES[key] = c
    return c


class Run:
    """device copies of a case's inputs + one forward with a guarded, NaN-filled statistics buffer"""

    def __init__(self, L, dev, c):
        self.L, self.c = L, c
        self.xd = (bf(c["x"]) if c["xbf"] else c["x"]).to(dev)
        self.gd, self.bd, self.ssd = c["gamma"].to(dev), c["beta"].to(dev), c["ss"].contiguous().to(dev)
        self.doutd = c["dout"].to(dev)
        self.dev = dev
        self.stats, self.stats_h = guarded((c["rows"], 2), torch.float32, dev)
        assert bool(torch.isnan(self.stats).all())

    def film(self):
        c = self.c
        return (P(self.ssd), P(self.ssd[:, D:])) if c["fs"] else (None, None)

    def forward(self, stats):
        import smd_amd.lib as lib
        c, rows = self.c, self.c["rows"]
        out = torch.zeros(rows, D, dtype=torch.bfloat16, device=self.dev)
        q = torch.zeros(rows, D, dtype=torch.uint8, device=self.dev) if c["f8"] else None
        s = torch.zeros(rows, dtype=torch.int32, device=self.dev) if c["f8"] else None
        fsc, fsh = self.film()
        lib.check(self.L.smd_layernorm_fwd_stats(None if c["xbf"] else P(self.xd), P(self.xd) if c["xbf"] else None, rows, D,
                                                 P(self.gd), P(self.bd), fsc, fsh, 2 * D, c["rps"], int(c["fs"]), P(out), P(q), P(s),
                                                 P(stats), st()))
        torch.cuda.synchronize()
        return out, q, s

    def backward(self, stats, accumulate):
        import smd_amd.lib as lib
        c, rows, res, om = self.c, self.c["rows"], self.c["res"], self.c["om"]
        dx32 = c["dres"].to(self.dev).clone() if res == "f32" else torch.zeros(rows, D, device=self.dev)      # in place when fp32
        dresb = bf(c["dres"]).to(self.dev) if res == "bf16" else None
        dxb = torch.zeros(rows, D, dtype=torch.bfloat16, device=self.dev)
        dg, db = torch.zeros(D, device=self.dev), torch.zeros(D, device=self.dev)
        dss = c["dss0"].to(self.dev).clone()
        partial = torch.zeros(rows * 2 * D, device=self.dev)
        fsc, fsh = self.film()
        lib.check(self.L.smd_layernorm_bwd_stats(None if c["xbf"] else P(self.xd), P(self.xd) if c["xbf"] else None, rows, D,
                                                 P(self.gd), P(self.bd), fsc, fsh, 2 * D, c["rps"], int(c["fs"]), P(self.doutd),
                                                 P(dx32) if res == "f32" else None, P(dresb), P(dx32) if om & 1 else None,
                                                 P(dxb) if om & 2 else None, P(dg), P(db), P(dss) if c["fs"] else None,
                                                 P(dss[:, D:]) if c["fs"] else None, accumulate, P(partial), partial.numel(),
                                                 P(stats), st()))
        torch.cuda.synchronize()
        return dict(dx32=dx32 if om & 1 else None, dxb=dxb if om & 2 else None, dg=dg, db=db, dss=dss if c["fs"] else None)


def check_backward(c, got, accumulate, what):
    if got["dx32"] is not None:
        assert rel(got["dx32"], c["dx"]) < TOL_F32, what
    if got["dxb"] is not None:
        assert rel(got["dxb"].float(), c["dx"]) < TOL_BF16, what              # bf16 output rounding
    assert rel(got["dg"], c["dg"]) < TOL_F32, what
    assert rel(got["db"], c["db"]) < TOL_F32, what
    if c["fs"]:
        want = c["dss"] + (c["dss0"].double() if accumulate else 0.0)
        assert rel(got["dss"], want) < TOL_F32, what


@pytest.mark.parametrize("rows,rps", SHAPES)
@pytest.mark.parametrize("form", list(FORMS))
def test_forward_saves_exactly_the_row_statistics(L, dev, form, rows, rps):
    """Forward output(s) against float64; the NaN-filled statistics buffer holds rows x 2 finite floats afterwards, the float64
    mean and 1 / sqrt(var + eps) to fp32 rounding (module docstring), and not one byte around it changed; a NULL statistics
    pointer writes nothing; two runs agree bitwise."""
    c = case(form, rows, rps)
    r = Run(L, dev, c)
    out0, _q0, _s0 = r.forward(None)
    assert bool(torch.isnan(r.stats).all()), "a forward without a statistics pointer wrote the buffer"
    r.stats_h.assert_untouched("stats (NULL pointer)")
    out, q, s = r.forward(r.stats)
    r.stats_h.assert_untouched("stats")
    got = r.stats.clone()
    assert bool(torch.isfinite(got).all())
    e_out = rel(out.float(), c["y"])
    d_mean = (got[:, 0].double().cpu() - c["mean"]).abs()
    d_rstd = (got[:, 1].double().cpu() / c["rstd"] - 1).abs()
    print(f"ln_saved_stats fwd {form} rows={rows}: out {e_out:.2e}  mean err/bound {float((d_mean / c['mean_tol']).max()):.2f}  "
          f"rstd err/bound {float((d_rstd / c['rstd_rtol']).max()):.2f}")
    assert e_out < TOL_BF16                                                     # bf16 output rounding
    assert torch.equal(out, out0)                                               # saving the statistics changes no output
    assert bool((d_mean <= c["mean_tol"]).all()) and bool((d_rstd <= c["rstd_rtol"]).all())
    if c["f8"]:
        e8 = rel(dequant(q, s), c["y"])
        print(f"ln_saved_stats fwd {form} rows={rows}: e4m3 copy {e8:.2e}")
        assert e8 < TOL_E4M3
    out2, q2, s2 = r.forward(r.stats)
    assert torch.equal(out2, out) and torch.equal(r.stats, got)
    if c["f8"]:
        assert torch.equal(q2, q) and torch.equal(s2, s)


@pytest.mark.parametrize("rows,rps", SHAPES)
@pytest.mark.parametrize("form", [f for f in FORMS if not FORMS[f][4]])
def test_backward_with_saved_statistics(L, dev, form, rows, rps):
    """Backward with the statistics the forward saved and with a NULL pointer, both dfilm_accumulate modes: each against float64
    at test_gpu_kernels.py's tolerances (so the two differ by at most what those allow); their observed difference is
    printed; two runs with saved statistics agree bitwise.  The two paths give the same bits when both are right, so a
    dropped pointer would pass all of that: a third call with every rstd doubled must change dx (dx scales with rstd in its
    leading term, so by far more than the 10 % asserted), which proves that the kernel reads the buffer."""
    c = case(form, rows, rps)
    r = Run(L, dev, c)
    r.forward(r.stats)
    for accumulate in (0, 1):
        saved = r.backward(r.stats, accumulate)
        again = r.backward(r.stats, accumulate)
        recomputed = r.backward(None, accumulate)
        diffs = {k: rel(saved[k].float(), recomputed[k].float()) for k in saved if saved[k] is not None}
        print(f"ln_saved_stats bwd {form} rows={rows} accumulate={accumulate}: saved vs recomputed " +
              "  ".join(f"{k} {v:.2e}" for k, v in diffs.items()))
        check_backward(c, saved, accumulate, "saved statistics")
        check_backward(c, recomputed, accumulate, "recomputed statistics")
        for k in saved:
            if saved[k] is not None:
                assert torch.equal(saved[k], again[k]), f"{k}: two runs differ"
    r.stats_h.assert_untouched("stats (backward)")
    wrong = r.stats.clone()
    wrong[:, 1] *= 2
    perturbed = r.backward(wrong, 0)
    k = "dxb" if saved["dxb"] is not None else "dx32"
    want_dx = c["dx"] - (c["dres"].double() if c["res"] else 0.0)              # the LayerNorm's own share of dx
    moved = float((perturbed[k].double().cpu() - saved[k].double().cpu()).norm() / want_dx.norm())
    print(f"ln_saved_stats bwd {form} rows={rows}: doubled rstd moves dx by {moved:.2f} of the LayerNorm gradient")
    assert moved > 0.1, "the backward ignored the statistics it was given"


def test_engine_saves_statistics_only_when_training_and_asked(dev):
    """Training workspace: forward_train fills the five [rows][2] buffers (ln1 / ln2 of both ResBlocks, ln_o) with the statistics
    of exactly the rows those LayerNorms read, and the gradient with saved statistics is the recomputed one to 1e-4 (both
    are fp32 evaluations of one formula); with option ln_saved_stats = 0 the forward leaves the NaN-filled buffers alone."""
    import smd_amd.ncsn as N
    from smd_amd.engine import NetConfig
    B, K = 4, 2
    model = N.Model(NetConfig(data_channels=64, num_layers=1, num_heads=8, num_mlp_layers=K), "cuda:0", seed=3)
    eng = model.train_engine(ema=False)
    g = torch.Generator().manual_seed(5)
    x = torch.clamp(0.25 * torch.randn(B, 32, 64, generator=g), -1, 1)
    s = 0.05 + 0.95 * torch.rand(B, generator=g)
    dpred = torch.randn(B, 32, 64, generator=g)
    eng.bind(B, training=True)
    grads = {}
    for opt in (1, 0):
        eng.set_option("ln_saved_stats", opt)
        for i in range(2 * K + 1):
            eng.debug_tensor("ln_stats", i).fill_(float("nan"))
        eng.forward_train(x, s)
        torch.cuda.synchronize()
        for i in range(2 * K + 1):
            got = eng.debug_tensor("ln_stats", i)
            if not opt:
                assert bool(torch.isnan(got).all()), f"ln_saved_stats = 0: buffer {i} was written"
                continue
            src = eng.debug_tensor("y", K) if i == 2 * K else eng.debug_tensor("y" if i % 2 == 0 else "o1", i // 2)
            mean, rstd, mean_tol, rstd_rtol = stat_bounds(src.double())
            assert got.shape == (B * 32, 2) and bool(torch.isfinite(got).all())
            assert bool(((got[:, 0].double() - mean).abs() <= mean_tol).all())
            assert bool(((got[:, 1].double() / rstd - 1).abs() <= rstd_rtol).all())
        eng.backward_from(dpred)
        torch.cuda.synchronize()
        grads[opt] = eng.grads.clone()
    e = rel(grads[1], grads[0])
    print(f"ln_saved_stats engine: gradient with saved vs recomputed statistics rel {e:.2e}")
    assert bool(torch.isfinite(grads[1]).all()) and e < 1e-4
    eng.set_option("ln_saved_stats", 1)


def test_inference_workspace_holds_no_statistics_and_stays_inside_its_bytes(dev):
    """An engine bound for inference (what model(x, s) and the sampler run) has no statistics buffers: its workspace, placed
    here in a guarded arena of exactly smd_engine_workspace_bytes(B, training = 0) bytes, is not left by one byte during a
    forward with ln_saved_stats = 1 (the default), the statistics view does not exist, the training workspace is larger by
    at least the five [rows][2] buffers, and eps_hat is bitwise what ln_saved_stats = 0 gives: the option touches nothing."""
    import smd_amd.lib as lib
    import smd_amd.ncsn as N
    from smd_amd.engine import NetConfig
    B, K = 4, 2
    model = N.Model(NetConfig(data_channels=64, num_layers=1, num_heads=8, num_mlp_layers=K), "cuda:0", seed=3)
    eng = model.engine
    Lb = eng.L
    g = torch.Generator().manual_seed(6)
    x = torch.clamp(0.25 * torch.randn(B, 32, 64, generator=g), -1, 1)
    s = 0.05 + 0.95 * torch.rand(B, generator=g)
    nbytes = int(Lb.smd_engine_workspace_bytes(eng.h, B, 0))
    assert int(Lb.smd_engine_workspace_bytes(eng.h, B, 1)) >= nbytes + (2 * K + 1) * B * 32 * 2 * 4
    ws, ws_h = guarded((nbytes,), torch.uint8, dev)
    lib.check(Lb.smd_engine_bind_workspace(eng.h, ws.data_ptr(), nbytes, B, 0, st()), "bind_workspace")
    eng.workspace, eng.batch, eng.training = ws, B, False          # Engine.bind() then keeps this workspace
    eng.generation += 1
    outs = {}
    for opt in (1, 0):
        eng.set_option("ln_saved_stats", opt)
        outs[opt] = eng.forward(x, s).clone()
        torch.cuda.synchronize()
        ws_h.assert_untouched(f"inference workspace (ln_saved_stats = {opt})")
        with pytest.raises(ValueError):
            eng.debug_tensor("ln_stats", 0)
    eng.set_option("ln_saved_stats", 1)
    assert eng.workspace is ws and bool(torch.isfinite(outs[1]).all()) and torch.equal(outs[1], outs[0])
