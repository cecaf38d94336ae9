"""The kernels of weighted training through the C-ABI (include/smd_hip.h), element by element against
tests/_timestep_ref.py: smd_weighted_mse_fwd_bwd, smd_timestep_draw, smd_timestep_update.  Every output lies in a guarded arena
(tests/_footprint.py): padding columns and the bytes around an output must come back untouched."""
import numpy as np
import pytest
import torch

import _footprint as F
import _timestep_ref as R

pytestmark = pytest.mark.gpu

GAMMA = 5.0
INF = float("inf")


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


def arena(shape, dtype, dev, ld=None, init=None):
    view, h = F.guarded(shape, dtype, dev, ld=ld)
    if init is not None:
        view.copy_(torch.as_tensor(init))
    return view, h


# ================================================================================================ weighted loss gradient
# SNR << gamma, SNR >> gamma, SNR = gamma (to fp32), and s = 1 exactly (SNR = inf: the weight must be 0, not NaN)
S_REGIMES = np.array([np.sqrt(0.01 / 1.01), np.sqrt(2000.0 / 2001.0), np.sqrt(GAMMA / (1 + GAMMA)), 1.0], np.float32)
SHAPES = [(3, 32, 512, 512), (2, 32, 42, 64), (2, 1, 512, 512), (1, 32, 6, 64)]
_CASES = {}


def grad_case(B, S, C):
    if (B, S, C) not in _CASES:
        g = torch.Generator().manual_seed(B * 1000 + S * 10 + C)
        _CASES[(B, S, C)] = (torch.randn(B, S, C, generator=g), torch.randn(B, S, C, generator=g))
    return _CASES[(B, S, C)]


def run_weighted(L, dev, pred, eps, s, iw, gamma, Cp, inv):
    B, S, C = pred.shape
    loss, hl = arena((B,), torch.float32, dev)
    w, hw = arena((B,), torch.float32, dev)
    dp, hd = arena((B * S, C), torch.bfloat16, dev, ld=Cp)
    ins = [pred.to(dev), eps.to(dev), None if s is None else torch.as_tensor(s).to(dev), None if iw is None else torch.as_tensor(iw).to(dev)]
    with F.unchanged(*[t for t in ins if t is not None]):
        ck(L.smd_weighted_mse_fwd_bwd(P(ins[0]), P(ins[1]), P(ins[2]), P(ins[3]), gamma, B, S, C, Cp, inv, P(loss), P(w), P(dp), st()),
           "weighted_mse")
        torch.cuda.synchronize()
    for h, name in ((hl, "loss"), (hw, "weight"), (hd, "dpred")):
        h.assert_untouched(name)                       # red zones and the columns C .. Cp of every dpred row
    return loss.clone(), w.clone(), dp.clone()


def run_plain(L, dev, pred, eps, Cp, inv):
    B, S, C = pred.shape
    loss, _ = arena((B,), torch.float32, dev)
    dp, _ = arena((B * S, C), torch.bfloat16, dev, ld=Cp)
    pd, ed = pred.to(dev), eps.to(dev)
    ck(L.smd_mse_fwd_bwd(P(pd), P(ed), B, S, C, Cp, inv, P(loss), P(dp), st()), "mse")
    torch.cuda.synchronize()
    return loss.clone(), dp.clone()


@pytest.mark.parametrize("iw_kind", ["null", "one", "1e3"])
@pytest.mark.parametrize("B,S,C,Cp", SHAPES)
def test_weighted_loss_gradient(L, dev, B, S, C, Cp, iw_kind):
    pred, eps = grad_case(B, S, C)
    inv = float(np.float32(1.0 / (4 * B * S * C)))              # a global batch of four shards
    iw = {"null": None, "one": np.ones(B, np.float32), "1e3": np.full(B, 1e3, np.float32)}[iw_kind]
    loss0, dp0 = run_plain(L, dev, pred, eps, Cp, inv)
    if iw is None:                                              # (iw NULL, gamma = 0) and gamma = inf: the unweighted bits
        for gamma in (0.0, INF):
            loss, w, dp = run_weighted(L, dev, pred, eps, S_REGIMES[np.arange(B) % 4], None, gamma, Cp, inv)
            assert torch.equal(bits(loss), bits(loss0)) and torch.equal(bits(dp), bits(dp0)), gamma
            assert w.cpu().tolist() == [1.0] * B
        loss, w, dp = run_weighted(L, dev, pred, eps, None, None, 0.0, Cp, inv)        # no SNR factor: the levels are not read
        assert torch.equal(bits(dp), bits(dp0))
    for rot in range(4):                                        # every sample meets every regime
        s = S_REGIMES[(np.arange(B) + rot) % 4]
        loss, w, dp = run_weighted(L, dev, pred, eps, s, iw, GAMMA, Cp, inv)
        assert torch.equal(bits(loss), bits(loss0)), "loss_per_sample is the unweighted kernel's, bit for bit"
        g64, loss64, w64 = R.weighted_grad(pred.numpy(), eps.numpy(), s, iw, GAMMA, inv)
        wg = w.cpu().numpy().astype(np.float64)
        assert np.isfinite(wg).all() and (np.abs(wg - w64) <= R.FP32_ROUNDINGS * R.U * np.abs(w64)).all(), (wg, w64)
        assert (wg[s == 1.0] == 0.0).all()                      # ap = 1: a finite weight
        np.testing.assert_allclose(loss.cpu().numpy(), loss64, rtol=1e-5)          # (fp32 sums of S C squares)
        bad, worst = R.check_grad(dp.float().cpu().numpy().reshape(B, S, C), g64)
        print(f"dpred {B, S, C, Cp} iw={iw_kind} rot={rot}: worst error / bound = {worst:.3f}")
        assert bad == 0, (bad, worst)


# ================================================================================================ draw
_TABLES = {}


def table(n):
    """a warmed-up table from a random history: (p fp32, cdf fp32)"""
    if n not in _TABLES:
        rng = np.random.default_rng(n)
        h = (rng.random((n, R.DEPTH)) * (0.05 + rng.random((n, 1))) * 2).astype(np.float32)
        _p, p32, cdf, _w = R.tables(h, np.full(n, R.DEPTH, np.int32))
        _TABLES[n] = (p32, cdf)
    return _TABLES[n]


def run_draw(L, dev, cdf, p, B, base, u=None, key=(7, 9), offset=0, step=0, step_ptr=None):
    n = len(p)
    labels, hl = arena((B,), torch.int32, dev)
    iw, hi = arena((B,), torch.float32, dev)
    ins = [torch.as_tensor(cdf).to(dev), torch.as_tensor(p).to(dev), None if u is None else torch.as_tensor(u).to(dev)]
    with F.unchanged(*[t for t in ins if t is not None]):
        ck(L.smd_timestep_draw(P(ins[0]), P(ins[1]), n, base, B, key[0], key[1], offset, step, P(step_ptr), P(ins[2]), P(labels), P(iw),
                               st()), "timestep_draw")
        torch.cuda.synchronize()
    hl.assert_untouched("labels")
    hi.assert_untouched("iw")
    return labels.cpu().numpy().copy(), iw.cpu().numpy().copy()


@pytest.mark.parametrize("n", [15, 1000])
def test_draw_with_explicit_uniforms(L, dev, n):
    p, cdf = table(n)
    f = np.float32
    below1 = np.nextafter(f(1), f(0))
    u = [f(0), below1]
    for k in (0, 1, n // 2, n - 2, n - 1):                      # exactly on an entry and one ulp to either side
        u += [cdf[k], np.nextafter(cdf[k], f(0)), min(np.nextafter(cdf[k], f(2)), below1)]
    u = np.concatenate([np.array(u, f), np.random.default_rng(n).random(300).astype(f)])
    for base in (0, 1):
        labels, iw = run_draw(L, dev, cdf, p, len(u), base, u)
        assert R.check_draw(labels, iw, cdf, p, u, base) == (0, 0)
        assert labels.min() >= base and labels.max() <= base + n - 1
    assert run_draw(L, dev, cdf, p, 1, 1, u[:1])[0][0] == 1 + int(np.argmax(cdf > 0))       # u = 0: the first timestep with mass
    # a cdf that ends below 1 through rounding: u above its last entry lands on the last timestep
    short = cdf.copy()
    short[-1] = f(1) - f(2.0 ** -24)
    assert short[-2] < short[-1]
    labels, iw = run_draw(L, dev, short, p, 3, 1, np.array([below1, short[-1], np.nextafter(short[-1], f(0))], f))
    assert labels.tolist() == [n, n, n] and R.check_draw(labels, iw, short, p, np.array([below1] * 3, f), 1)[1] == 0
    # one shard and two shards give equal arrays
    cut = 101
    la, ia = run_draw(L, dev, cdf, p, cut, 1, u[:cut], offset=0)
    lb, ib = run_draw(L, dev, cdf, p, len(u) - cut, 1, u[cut:], offset=cut)
    l1, i1 = run_draw(L, dev, cdf, p, len(u), 1, u)
    assert np.array_equal(np.concatenate([la, lb]), l1) and np.array_equal(np.concatenate([ia, ib]).view(np.int32), i1.view(np.int32))


@pytest.mark.parametrize("n", [15, 1000])
def test_draw_from_the_philox_stream(L, dev, n):
    p, cdf = table(n)
    N = 65536
    labels, iw = run_draw(L, dev, cdf, p, N, 1, key=(123, 456), step=3)
    assert labels.min() >= 1 and labels.max() <= n
    np.testing.assert_array_equal(iw.view(np.int32), (1.0 / (n * p[labels - 1].astype(np.float64))).astype(np.float32).view(np.int32))
    stat, q = R.chi2_stat(labels, p, 1, N), R.chi2_quantile(n - 1)
    print(f"n={n}: chi-square {stat:.1f} against the 1 - 1e-6 quantile {q:.1f} ({n - 1} degrees of freedom)")
    assert stat < q
    again, iw2 = run_draw(L, dev, cdf, p, N, 1, key=(123, 456), step=3)
    assert labels.tobytes() == again.tobytes() and iw.tobytes() == iw2.tobytes()          # same key: the same bytes
    assert not np.array_equal(labels, run_draw(L, dev, cdf, p, N, 1, key=(123, 456), step=4)[0])      # another step
    assert not np.array_equal(labels, run_draw(L, dev, cdf, p, N, 1, key=(124, 456), step=3)[0])      # another key
    # the device step counter replaces the host value
    sp = torch.tensor([3], dtype=torch.int32, device=dev)
    assert np.array_equal(labels, run_draw(L, dev, cdf, p, N, 1, key=(123, 456), step=99, step_ptr=sp)[0])
    # keyed by the global sample index: two shards draw what the whole batch draws
    cut = 1000
    la, _ = run_draw(L, dev, cdf, p, cut, 1, key=(123, 456), step=3, offset=0)
    lb, _ = run_draw(L, dev, cdf, p, 3000, 1, key=(123, 456), step=3, offset=cut)
    assert np.array_equal(np.concatenate([la, lb]), labels[:cut + 3000])


# ================================================================================================ update
def update_case(n, Bg, completes, base):
    """state with rows at counts 0, 9 and 10; a batch that touches the first and the last timestep, holds one timestep 23 times
    (a full row wrapped more than twice) and brings the last count to 10 -- or stops one sample short of it"""
    rng = np.random.default_rng(n * 10000 + Bg * 2 + completes)
    hist = (rng.random((n, R.DEPTH)) * 2 + 0.01).astype(np.float32)
    counts = np.full(n, R.DEPTH, np.int32)
    a, z, hot = 3, n - 4, 7
    counts[a] = 9
    if Bg == 1:
        labels = [a if completes else 0]
    else:
        counts[z] = 0
        hist[z] = 0
        labels = [0, n - 1] + [hot] * 23 + ([a] if completes else []) + [z] * (10 if completes else 9)
        free = np.setdiff1d(np.arange(n), [a, z])
        labels += [-1, n][:max(0, min(2, Bg - len(labels)))]             # labels outside the table are dropped
        labels += rng.choice(free, size=Bg - len(labels)).tolist()
        labels = rng.permutation(np.array(labels)).tolist()
    assert len(labels) == Bg
    loss = (rng.random(Bg) * 3 + 0.01).astype(np.float32)
    return hist, counts, (np.array(labels) + base).astype(np.int32), loss


def run_update(L, dev, hist, counts, labels, loss, base):
    n = hist.shape[0]
    h, hh = arena((n, R.DEPTH), torch.float32, dev, init=hist)
    c, hc = arena((n,), torch.int32, dev, init=counts)
    p, hp = arena((n,), torch.float32, dev)
    cdf, hcdf = arena((n,), torch.float32, dev)
    warmed, hw = arena((1,), torch.int32, dev)
    ld, lo = torch.as_tensor(labels).to(dev), torch.as_tensor(loss).to(dev)
    with F.unchanged(ld, lo):
        ck(L.smd_timestep_update(P(ld), P(lo), len(labels), P(h), P(c), n, base, float(R.MIX), P(p), P(cdf), P(warmed), st()),
           "timestep_update")
        torch.cuda.synchronize()
    for hd, name in ((hh, "history"), (hc, "counts"), (hp, "p"), (hcdf, "cdf"), (hw, "warmed")):
        hd.assert_untouched(name)
    return [t.cpu().numpy().copy() for t in (h, c, p, cdf, warmed)]


@pytest.mark.parametrize("completes", [False, True])
@pytest.mark.parametrize("Bg", [1, 37, 4100])
@pytest.mark.parametrize("n", [15, 1000])
def test_update(L, dev, n, Bg, completes):
    base = 1
    hist, counts, labels, loss = update_case(n, Bg, completes, base)
    h, c, p, cdf, warmed = run_update(L, dev, hist, counts, labels, loss, base)
    rh, rc = R.ring_update(hist, counts, labels, loss, base)
    assert h.tobytes() == rh.tobytes() and c.tobytes() == rc.tobytes()                    # history and counts, byte for byte
    _p64, _p32, _cdf, rw = R.tables(rh, rc)
    assert rw == completes and int(warmed[0]) == int(completes)                           # both sides of the last count reaching 10
    assert R.check_tables(p, cdf, rh, rc) == []
    if not completes:
        assert (p == np.float32(1.0 / n)).all()                                           # warm-up: uniform
    else:
        assert p.max() > 1.5 * p.min()
    again = run_update(L, dev, hist, counts, labels, loss, base)
    for x, y in zip((h, c, p, cdf, warmed), again):
        assert x.tobytes() == y.tobytes()                                                 # the same state, the same bytes
    # the tables the update wrote are the ones the draw reads: a draw from them matches the reference draw
    u = np.random.default_rng(Bg).random(64).astype(np.float32)
    labels2, iw2 = run_draw(L, dev, cdf, p, 64, base, u)
    assert R.check_draw(labels2, iw2, cdf, p, u, base) == (0, 0)


# ================================================================================================ torch ops
def test_custom_ops_run_the_same_kernels(L, dev):
    import smd_amd.ops  # noqa: F401  (registers torch.ops.smd_amd.*)
    p, cdf = table(15)
    u = np.random.default_rng(1).random(50).astype(np.float32)
    labels, iw = torch.ops.smd_amd.timestep_draw(torch.as_tensor(cdf).to(dev), torch.as_tensor(p).to(dev), torch.as_tensor(u).to(dev), 1)
    want = run_draw(L, dev, cdf, p, 50, 1, u)
    assert np.array_equal(labels.cpu().numpy(), want[0]) and iw.cpu().numpy().tobytes() == want[1].tobytes()
    B, S, C, Cp = SHAPES[0]
    pred, eps = grad_case(B, S, C)
    s, w_in = S_REGIMES[:B], np.full(B, 0.5, np.float32)
    inv = float(np.float32(1.0 / (B * S * C)))
    loss, w, dp = torch.ops.smd_amd.weighted_mse(pred.to(dev), eps.to(dev), torch.as_tensor(s).to(dev), torch.as_tensor(w_in).to(dev), GAMMA, inv)
    l2, w2, dp2 = run_weighted(L, dev, pred, eps, s, w_in, GAMMA, Cp, inv)
    assert torch.equal(bits(loss), bits(l2)) and torch.equal(bits(w), bits(w2)) and torch.equal(bits(dp), bits(dp2))
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.smd_amd.timestep_draw(torch.as_tensor(cdf), torch.as_tensor(p), torch.as_tensor(u), 1)
