"""smd_param_mse_fwd_bwd (include/smd_hip.h) element by element against tests/_prediction_ref.py, the
float64 reference evaluated on the stored fp32 noise level.  Every output lies in a guarded arena (tests/_footprint.py): the
padding columns [C, Cp) of dpred and the bytes around every output must come back untouched.

Shapes, the smallest that reach every path of param_mse_loss_grad_kernel:
  (3, 32, 42, 64)    VEC = 1 (C % 4 != 0), 1344 elements: a second trip of the 1024-thread loop
  (2, 32, 132, 192)  VEC = 4, 4224 > 4096 elements: a second trip of the vector loop
  (4, 1, 5, 8)       fewer elements than threads: the DenseDDPM layout
Noise levels: s = 1 (label 1: ap = 1 exactly), s = sqrt(ap_T) of the base schedule and a mid value, rotated so that every sample
meets each.  iw null / given, gamma 0 (no SNR factor) / 5.

Bounds.  weight_per_sample: the 16 fp32 roundings tests/test_gpu_timestep.py allows the weighted kernel (this weight takes
fewer: s s, 1 - s, 1 + s, their product, one quotient or one product, iw).  loss_per_sample: that test's rtol 1e-5 -- the target adds
one FMA and one square root, each below 2^-23 relative on terms of the size of the difference, far inside it, so the 2x
allowance of measured error was not needed.  dpred: the reference rounded to bf16, at most one bf16 ulp away.
Measured over all 72 runs of this file: weight within 2.28 fp32 roundings, loss within 1.81e-7 relative, dpred never more than one
bf16 ulp from the rounded reference.
"""
import numpy as np
import pytest
import torch

import _footprint as F
import _prediction_ref as R
import _timestep_ref as TR

pytestmark = pytest.mark.gpu

GAMMA = 5.0
SHAPES = [(3, 32, 42, 64), (2, 32, 132, 192), (4, 1, 5, 8)]


def _levels():
    import smd_amd.schedule as S
    ap_T = float(S.alphas_cumprod(S.create_noise_schedule(1e-6, 0.01, 1000, "linear"))[-1])
    return np.array([1.0, np.sqrt(ap_T), np.sqrt(0.5)], np.float32)


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def ck(rc, what=""):
    import smd_amd.lib as lib
    lib.check(rc, what)


def bits(t):
    return t.detach().contiguous().view(torch.uint8).cpu()


_CASES = {}


def case(B, S, C):
    """(pred, eps, x0) fp32, made once per shape and never changed"""
    if (B, S, C) not in _CASES:
        g = torch.Generator().manual_seed(26000 + B * 1000 + S * 10 + C)
        _CASES[(B, S, C)] = tuple(torch.randn(B, S, C, generator=g) for _ in range(3))
    return _CASES[(B, S, C)]


def run(L, dev, kind, pred, eps, x0, s, iw, gamma, Cp, inv):
    B, S, C = pred.shape
    loss, hl = F.guarded((B,), torch.float32, dev)
    w, hw = F.guarded((B,), torch.float32, dev)
    dp, hd = F.guarded((B * S, C), torch.bfloat16, dev, ld=Cp)
    ins = [pred.to(dev), eps.to(dev), x0.to(dev), torch.as_tensor(s).to(dev), None if iw is None else torch.as_tensor(iw).to(dev)]
    with F.unchanged(*[t for t in ins if t is not None]):
        ck(L.smd_param_mse_fwd_bwd(P(ins[0]), P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), gamma, kind, B, S, C, Cp, inv, P(loss), P(w),
                                   P(dp), st()), "param_mse")
        torch.cuda.synchronize()
    for h, name in ((hl, "loss"), (hw, "weight"), (hd, "dpred")):
        h.assert_untouched(name)                       # red zones and the canaries in columns C .. Cp of every dpred row
    return loss.clone(), w.clone(), dp.clone()


@pytest.mark.parametrize("kind", [1, 2], ids=["x0", "v"])
@pytest.mark.parametrize("B,S,C,Cp", SHAPES)
def test_param_loss_gradient(L, dev, B, S, C, Cp, kind):
    pred, eps, x0 = case(B, S, C)
    lv = _levels()
    inv = float(np.float32(1.0 / (4 * B * S * C)))              # a global batch of four shards
    iw_given = (0.25 + np.arange(B, dtype=np.float32) * 1.5).astype(np.float32)
    for rot in range(3):                                        # every sample meets every noise level
        s = lv[(np.arange(B) + rot) % 3]
        for iw in (None, iw_given):
            for gamma in (0.0, GAMMA):
                loss, w, dp = run(L, dev, kind, pred, eps, x0, s, iw, gamma, Cp, inv)
                loss2, w2, dp2 = run(L, dev, kind, pred, eps, x0, s, iw, gamma, Cp, inv)
                assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(w), bits(w2)) and torch.equal(bits(dp), bits(dp2)), \
                    "two runs are bitwise equal"
                g64, loss64, w64 = R.param_grad(kind, pred.numpy(), eps.numpy(), x0.numpy(), s, iw, gamma, inv)
                wg = w.cpu().numpy().astype(np.float64)
                lg = loss.cpu().numpy().astype(np.float64)
                w_err = float(np.max(np.abs(wg - w64) / np.maximum(np.abs(w64), 1e-300) * (w64 != 0)))
                l_err = float(np.max(np.abs(lg - loss64) / loss64))
                bad, worst = R.check_dpred(dp.float().cpu().numpy().reshape(B, S, C), g64)
                print(f"kind {kind} {B, S, C, Cp} rot={rot} iw={'null' if iw is None else 'given'} gamma={gamma}: weight rel err "
                      f"{w_err / TR.U:.2f} u, loss rel err {l_err:.2e}, dpred worst {worst:.3f} bf16 ulp")
                assert np.isfinite(wg).all() and (np.abs(wg - w64) <= TR.FP32_ROUNDINGS * TR.U * np.abs(w64)).all(), (wg, w64)
                if gamma == 0.0:                                # no SNR factor: iw alone, exactly (1 when iw is null)
                    assert wg.tolist() == ([1.0] * B if iw is None else iw.astype(np.float64).tolist())
                else:                                           # ap = 1: x0 gives gamma, v gives 0 -- finite, never a NaN
                    at1 = wg[s == 1.0] / (1.0 if iw is None else iw[s == 1.0])
                    assert (at1 == (GAMMA if kind == 1 else 0.0)).all(), at1
                np.testing.assert_allclose(lg, loss64, rtol=1e-5)
                assert bad == 0, (bad, worst)


@pytest.mark.parametrize("B,S,C,Cp", SHAPES)
def test_kind0_is_the_weighted_kernel(L, dev, B, S, C, Cp):
    """kind = 0 through the new entry forwards to smd_weighted_mse_fwd_bwd: the same bits, and x0 is not read (NULL)"""
    pred, eps, x0 = case(B, S, C)
    lv = _levels()
    inv = float(np.float32(1.0 / (B * S * C)))
    s = lv[np.arange(B) % 3]
    iw = (0.5 + np.arange(B, dtype=np.float32)).astype(np.float32)
    pd, ed, sd, iwd = pred.to(dev), eps.to(dev), torch.as_tensor(s).to(dev), torch.as_tensor(iw).to(dev)
    out = []
    for which in ("weighted", "param"):
        loss, hl = F.guarded((B,), torch.float32, dev)
        w, hw = F.guarded((B,), torch.float32, dev)
        dp, hd = F.guarded((B * S, C), torch.bfloat16, dev, ld=Cp)
        if which == "weighted":
            ck(L.smd_weighted_mse_fwd_bwd(P(pd), P(ed), P(sd), P(iwd), GAMMA, B, S, C, Cp, inv, P(loss), P(w), P(dp), st()), which)
        else:
            ck(L.smd_param_mse_fwd_bwd(P(pd), P(ed), None, P(sd), P(iwd), GAMMA, 0, B, S, C, Cp, inv, P(loss), P(w), P(dp), st()), which)
        torch.cuda.synchronize()
        for h in (hl, hw, hd):
            h.assert_untouched(which)
        out.append((bits(loss), bits(w), bits(dp)))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_argument_errors(L, dev):
    """the checks of the launcher, in smd_weighted_mse_fwd_bwd's style: a message, a non-zero return, no launch"""
    err = lambda: L.smd_last_error().decode()
    B, S, C = 2, 1, 8
    z = torch.zeros(B, S, C, device=dev)
    sv = torch.ones(B, device=dev)
    loss, w = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    dp = torch.zeros(B * S, C, dtype=torch.bfloat16, device=dev)
    call = lambda eps, x0, s, kind, gamma=0.0: L.smd_param_mse_fwd_bwd(P(z), P(eps), P(x0), P(s), None, gamma, kind, B, S, C, C,
                                                                     1.0, P(loss), P(w), P(dp), st())
    assert call(z, z, sv, 3) != 0 and "kind" in err()
    assert call(z, None, sv, 1) != 0                       # x0 is needed by kinds 1 and 2
    assert call(None, z, sv, 2) != 0 and "v target" in err()
    assert call(z, z, None, 2) != 0
    assert call(z, z, None, 1, GAMMA) != 0 and "noise levels" in err()
    assert call(None, z, None, 1) == 0                     # x0 without an SNR factor reads neither eps nor the levels
    torch.cuda.synchronize()


def test_param_mse_custom_op_and_its_fake_rule(L, dev):
    """torch.ops.smd_amd.param_mse: the eager path has the C entry's bits; the fake rule gives the same shapes and dtypes"""
    import smd_amd.ops  # noqa: F401  (registers the ops)
    from torch._subclasses.fake_tensor import FakeTensorMode
    B, S, C, Cp = SHAPES[1]
    pred, eps, x0 = case(B, S, C)
    s = _levels()[np.arange(B) % 3]
    iw = (0.5 + np.arange(B, dtype=np.float32)).astype(np.float32)
    inv = float(np.float32(1.0 / (B * S * C)))
    args = [t.to(dev) for t in (pred, eps, x0, torch.as_tensor(s), torch.as_tensor(iw))]
    for kind in (0, 1, 2):
        loss, w, dp = torch.ops.smd_amd.param_mse(*args, GAMMA, kind, inv)
        torch.cuda.synchronize()
        if kind:
            loss0, w0, dp0 = run(L, dev, kind, pred, eps, x0, s, iw, GAMMA, C, inv)
            assert torch.equal(bits(loss), bits(loss0)) and torch.equal(bits(w), bits(w0)) and torch.equal(bits(dp), bits(dp0.reshape(B * S, C)))
        else:
            loss0, w0, dp0 = torch.ops.smd_amd.weighted_mse(args[0], args[1], args[3], args[4], GAMMA, inv)
            assert torch.equal(bits(loss), bits(loss0)) and torch.equal(bits(w), bits(w0)) and torch.equal(bits(dp), bits(dp0))
        with FakeTensorMode(allow_non_fake_inputs=False) as mode:
            fk = [mode.from_tensor(t) for t in args]
            fl, fw, fd = torch.ops.smd_amd.param_mse(*fk, GAMMA, kind, inv)
        for f, r in ((fl, loss), (fw, w), (fd, dp)):
            assert tuple(f.shape) == tuple(r.shape) and f.dtype == r.dtype
    with pytest.raises(ValueError, match="kind"):
        torch.ops.smd_amd.param_mse(*args, GAMMA, 3, inv)
