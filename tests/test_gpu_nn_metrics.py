"""The nearest-neighbour metrics (smd_amd.metrics knn_radii / ball_cover / precision_recall / realism_scores, csrc/nn_metrics.hip)
against the float64 brute force of tests/_nn_metrics_ref.py.

Error model (derived, not tuned).  The fp32 d2 = (-2 <x,y> + |x|^2) + |y|^2 of a pair differs from the exact one by at most
m = (d + 4) 2^-24 (|x| + |y|)^2, taken with the largest row norms of the two sets.
  * The k-th smallest of perturbed values is within the largest perturbation of the true k-th smallest: |r2_gpu - r2_f64| <= m.
  * s_q = max_j (r2_j - d2_qj) in float64 decides coverage; with radius and distance each within m the GPU must agree
    wherever |s_q| > 2m.  The other rows are undecidable and may differ; their share -- in the float64 reference alone -- must
    stay within 0.5 % of the queries (a condition on the test's inputs, asserted), and precision / recall must be within
    undecidable / n of float64.
  * Identity case (the set against itself, pair (i, i) excluded): a row q that is exactly the k-th neighbour of j has
    r2_j - d2_qj = 0 by definition, which the rule above would call undecidable for ~8 % of the rows.  The kernels form the d2 of
    a pair with the same bits from either side, so such a row IS covered on the GPU whenever q is j's k-th neighbour there too,
    which is certain when j's k-th distance is more than 2m away from its (k-1)-th and (k+1)-th.  Those rows count as certain.
  * realism2 = max_j r2_j / d2_qj over the kept j: with r2 and d2 within m and one rounding of the division, the GPU value lies
    in [max_j (r2_j - m) / (d2_qj + m), max_j (r2_j + m) / (d2_qj - m)] widened by 2^-22 relative, checked on the rows whose kept
    distances all exceed 2m.  The GPU's own median mask is used where a radius is too close to the median to call: a radius is
    within dr = m / r of float64's, so the masks may differ only on rows within 2 max(dr) of the float64 median."""

import numpy as np
import pytest
import torch

import _nn_metrics_ref as R

pytestmark = pytest.mark.gpu

CAP = 0.005


def sets(nx, ny, d, shift, scale, seed=0):
    """X = clip(0.25 N(0,1), +-1), Y = clip(scale 0.25 N(0,1) + shift, +-1): the normalised latent range"""
    rng = np.random.default_rng(seed)
    x = np.clip(0.25 * rng.standard_normal((nx, d)), -1, 1).astype(np.float32)
    y = np.clip(scale * 0.25 * rng.standard_normal((ny, d)) + shift, -1, 1).astype(np.float32)
    return x, y


d2_bound = R.d2_error_bound


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_radii(x, k, r2_gpu):
    r2 = R.knn_radii2(x, k)
    m = d2_bound(x.shape[1], x, x)
    err = float(np.abs(r2_gpu.astype(np.float64) - r2).max())
    print(f"  radii n={len(x)} d={x.shape[1]} k={k}: max |r2_gpu - r2_f64| = {err:.3e}, bound m = {m:.3e}")
    assert err <= m
    return r2


def check_cover(name, s, certain, covered_gpu):
    """exact agreement on the certain rows, the cap on the undecidable ones, the rate within undecidable / n"""
    n = len(s)
    und = int((~certain).sum())
    ref = s >= 0
    differ = int((covered_gpu.astype(bool) != ref).sum())
    print(f"  {name}: float64 {ref.mean():.4f} gpu {covered_gpu.mean():.4f}, undecidable {und} of {n} ({100.0 * und / n:.3f} %), "
          f"rows that differ {differ}")
    assert und <= CAP * n, "the float64 reference alone exceeds the cap: a bad test input"
    assert np.array_equal(covered_gpu.astype(bool)[certain], ref[certain])
    assert abs(float(covered_gpu.mean()) - float(ref.mean())) <= und / n


def check_keep(r2_f64, keep_gpu, m):
    r = np.sqrt(r2_f64)
    dr = float((m / r).max())
    close = np.abs(r - np.median(r)) <= 2 * dr
    differ = keep_gpu.astype(bool) != R.keep_mask(r2_f64)
    print(f"  median mask: {int(differ.sum())} rows differ, {int(close.sum())} within 2 dr = {2 * dr:.3e} of the median")
    assert not (differ & ~close).any()


def check_realism(dqx, r2_f64, keep, m, realism2_gpu, exclude_diagonal=False):
    keep = np.asarray(keep, bool)
    dk = np.where(keep[None, :], dqx, np.inf)
    if exclude_diagonal:
        np.fill_diagonal(dk, np.inf)
    sure = dk.min(1) > 2 * m
    lo = ((r2_f64[None, :] - m) / (dk + m)).max(1)
    hi = ((r2_f64[None, :] + m) / np.maximum(dk - m, R.FLT_MIN)).max(1)          # only read where every kept dk > 2m
    g = realism2_gpu.astype(np.float64)
    ref = R.realism2(dqx, r2_f64, keep, exclude_diagonal)
    rel = float((np.abs(g - ref) / ref)[sure].max())
    print(f"  realism2: {int(sure.sum())} of {len(sure)} rows checked, max relative difference to float64 {rel:.3e}, "
          f"widest allowed {float(((hi - lo) / ref)[sure].max()):.3e}")
    assert sure.mean() >= 1 - CAP
    assert np.all(np.isfinite(g))
    assert np.all(g[sure] >= lo[sure] * (1 - 2.0 ** -22)) and np.all(g[sure] <= hi[sure] * (1 + 2.0 ** -22))


# the issue's table (n, d, shift, scale) and ragged shapes with nq != nx, each re-checked for the cap on the CPU
CASES = [(4096, 4096, 42, 0.0, 1.0), (4096, 4096, 42, 0.05, 0.9), (4096, 4096, 146, 0.02, 0.95), (2048, 2048, 512, 0.01, 0.97),
         (4096, 4096, 8, 0.1, 0.8), (4001, 1333, 42, 0.05, 0.9), (333, 2500, 146, 0.02, 0.95)]


@pytest.mark.parametrize("nx,ny,d,shift,scale", CASES)
def test_precision_recall_realism_match_float64(nx, ny, d, shift, scale):
    import smd_amd.metrics as M
    k = 3
    x, y = sets(nx, ny, d, shift, scale)
    xt, yt = cuda(x), cuda(y)
    m = d2_bound(d, x, y)
    r2x_g, r2y_g = M.knn_radii(xt, k), M.knn_radii(yt, k)
    r2x = check_radii(x, k, r2x_g.cpu().numpy())
    r2y = check_radii(y, k, r2y_g.cpu().numpy())
    keep_g = M.median_keep_mask(r2x_g)
    check_keep(r2x, keep_g.cpu().numpy(), d2_bound(d, x, x))
    dyx = R.sqdist(y, x)
    cov_p, real2 = M.ball_cover(yt, xt, r2x_g, keep_g)
    cov_r, _ = M.ball_cover(xt, yt, r2y_g)
    sp, sr = R.cover_margin(dyx, r2x), R.cover_margin(dyx.T, r2y)
    check_cover("precision", sp, np.abs(sp) > 2 * m, cov_p.cpu().numpy())
    check_cover("recall", sr, np.abs(sr) > 2 * m, cov_r.cpu().numpy())
    check_realism(dyx, r2x, keep_g.cpu().numpy(), m, real2.cpu().numpy())
    # the public functions are these passes
    p, r = M.precision_recall(x, y, k)
    assert p == float(cov_p.double().mean()) and r == float(cov_r.double().mean())
    assert np.array_equal(M.realism_scores(x, y, k), np.sqrt(real2.cpu().numpy().astype(np.float64)))
    im = M.improved_metrics(M.ReferenceSet(x), y, k)
    assert im["improved_precision"] == p and im["improved_recall"] == r and im["improved_f1"] == M.f1_score(p, r)
    ref = R.metrics(x, y, k)
    assert abs(im["improved_f1"] - ref["improved_f1"]) <= 2 * CAP


@pytest.mark.parametrize("n,d,shift,scale", [(4096, 42, 0.0, 1.0), (4096, 146, 0.02, 0.95), (4001, 8, 0.1, 0.8)])
def test_identity_case_gives_the_leave_one_out_values(n, d, shift, scale):
    import smd_amd.metrics as M
    k = 3
    x, _ = sets(n, n, d, shift, scale)
    m = d2_bound(d, x, x)
    dxx = R.sqdist(x)
    r2 = R.knn_radii2(x, k, dxx)
    s, certain = R.loo_certain(dxx, r2, k, m)              # module docstring: unambiguous k-th neighbours are certainly covered
    print(f"  rows with s_q == 0: {int((s == 0).sum())}, of them certain: {int(((s == 0) & certain).sum())}")
    ref = M.ReferenceSet(x)
    r2_g, keep_g = ref.radii(k)
    check_radii(x, k, r2_g.cpu().numpy())
    check_keep(r2, keep_g.cpu().numpy(), m)
    cov, real2 = M.ball_cover(ref.frames, ref.frames, r2_g, keep_g, exclude_diagonal=True)
    check_cover("leave-one-out coverage", s, certain, cov.cpu().numpy())
    check_realism(dxx, r2, keep_g.cpu().numpy(), m, real2.cpu().numpy(), exclude_diagonal=True)
    # the same object (or the ReferenceSet itself) as the sample set takes this path; a copy does not: every row then lies at
    # distance 0 from its twin and is covered
    for fake in (x, ref):
        im = M.improved_metrics(ref if fake is ref else x, fake, k)
        assert im["improved_precision"] == im["improved_recall"] == float(cov.double().mean())
        assert im["ipr_realism"] == float(np.sqrt(real2.cpu().numpy().astype(np.float64)).mean())
    assert M.precision_recall(x, x.copy(), k) == (1.0, 1.0)
    assert np.all(np.isfinite(M.realism_scores(x, x.copy(), k)))


def test_duplicated_rows():
    """self is excluded by index, not by value: a duplicated row has its twin at distance exactly 0"""
    import smd_amd.metrics as M
    x, _ = sets(700, 1, 42, 0.0, 1.0, seed=3)
    x[100:200] = x[0:100]
    xt = cuda(x)
    r2 = M.knn_radii(xt, 1).cpu().numpy()
    assert np.all(r2[:200] == 0.0) and np.all(r2[200:] > 0.0)
    check_radii(x, 1, r2)
    r3 = M.knn_radii(xt, 3)
    check_radii(x, 3, r3.cpu().numpy())
    assert np.all(r3.cpu().numpy() > 0.0)
    cov, real2 = M.ball_cover(xt, xt, M.knn_radii(xt, 1), exclude_diagonal=True)
    cov = cov.cpu().numpy()
    assert np.all(cov[:200] == 1)                      # the twin's ball of radius 0 holds the row: d2 == 0 <= 0
    assert np.all(np.isfinite(real2.cpu().numpy()))
    cov3, real3 = M.ball_cover(xt, xt, r3, M.median_keep_mask(r3), exclude_diagonal=True)
    assert np.all(cov3.cpu().numpy()[:200] == 1) and np.all(np.isfinite(real3.cpu().numpy()))
    # d2 == 0 under a positive radius: r2 / FLT_MIN, finite
    assert float(real3.max()) > 1e30


def test_every_k():
    import smd_amd.metrics as M
    x, _ = sets(1000, 1, 42, 0.0, 1.0, seed=4)
    xt = cuda(x)
    prev = np.zeros(1000)
    for k in range(1, 9):
        r2 = M.knn_radii(xt, k).cpu().numpy()
        check_radii(x, k, r2)
        assert np.all(r2 >= prev)
        prev = r2
    small = cuda(x[:9])
    check_radii(x[:9], 8, M.knn_radii(small, 8).cpu().numpy())        # n = k + 1: the farthest other row


def test_two_calls_are_bitwise_equal():
    import smd_amd.metrics as M
    x, y = sets(5000, 3000, 146, 0.02, 0.95, seed=5)
    xt, yt = cuda(x), cuda(y)
    a, b = M.knn_radii(xt, 3), M.knn_radii(xt, 3)
    assert torch.equal(a, b)
    keep = M.median_keep_mask(a)
    o1, o2 = M.ball_cover(yt, xt, a, keep), M.ball_cover(yt, xt, a, keep)
    assert torch.equal(o1[0], o2[0]) and torch.equal(o1[1], o2[1])
    assert o1[0].dtype == torch.uint8 and set(o1[0].unique().tolist()) <= {0, 1}


def test_strided_inputs_are_read_as_their_values():
    import smd_amd.metrics as M
    base = cuda(sets(600, 1, 84, 0.0, 1.0, seed=6)[0])
    xs = base[:, ::2]                                   # columns not unit-strided: copied by the wrapper
    rows = cuda(sets(500, 1, 64, 0.0, 1.0, seed=7)[0])[:, :42]      # rows 64 apart: read in place
    assert xs.stride(1) == 2 and rows.stride(0) == 64 and not rows.is_contiguous()
    xc, rc = xs.contiguous(), rows.contiguous()
    assert torch.equal(M.knn_radii(xs, 3), M.knn_radii(xc, 3)) and torch.equal(M.knn_radii(rows, 3), M.knn_radii(rc, 3))
    r2 = M.knn_radii(xc, 3)
    for q, c in ((rows, xs), (rc, xs), (rows, xc)):
        got, want = M.ball_cover(q, c, r2), M.ball_cover(rc, xc, r2)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # an (N, S, C) array is N*S frames of C
    real = sets(20 * 32, 1, 42, 0.0, 1.0, seed=8)[0]
    fake = sets(20 * 32, 1, 42, 0.05, 0.9, seed=9)[0]
    assert M.precision_recall(real.reshape(20, 32, 42), torch.from_numpy(fake.reshape(20, 32, 42))) == M.precision_recall(real, fake)


def test_argument_errors_raise_and_launch_nothing():
    import smd_amd.lib as lib
    import smd_amd.metrics as M
    L = lib.get_lib()
    x = torch.rand(10, 4, device="cuda")
    for k in (0, 9):
        with pytest.raises(ValueError, match=r"k=\d must be in \[1, 8\]"):
            M.knn_radii(x, k)
    with pytest.raises(ValueError, match="other rows"):
        M.knn_radii(x[:3], 3)
    with pytest.raises(ValueError, match="d mismatch"):
        M.ball_cover(torch.rand(5, 3, device="cuda"), x, torch.zeros(10, device="cuda"))
    with pytest.raises(ValueError, match="squared radii"):
        M.ball_cover(x, x, torch.zeros(9, device="cuda"))
    with pytest.raises(ValueError, match="nq == nx"):
        M.ball_cover(x[:5], x, torch.zeros(10, device="cuda"), exclude_diagonal=True)
    need = L.smd_knn_radii_workspace_bytes(10, 3)
    assert need > 0 and L.smd_knn_radii_workspace_bytes(10, 0) == -1 and L.smd_knn_radii_workspace_bytes(3, 3) == -1
    ws = torch.zeros(max(need, L.smd_ball_cover_workspace_bytes(10, 10)), dtype=torch.uint8, device="cuda")
    r2 = torch.full((10,), -7.0, device="cuda")
    cov = torch.full((10,), 9, dtype=torch.uint8, device="cuda")
    re2 = torch.full((10,), -7.0, device="cuda")

    def knn(xp=x.data_ptr(), ld=4, n=10, d=4, k=3, wsp=ws.data_ptr(), wsb=need, out=r2.data_ptr()):
        return L.smd_knn_radii(xp, ld, n, d, k, wsp, wsb, out, None)

    for kw, word in ((dict(k=0), b"k=0"), (dict(k=9), b"k=9"), (dict(xp=x.data_ptr() + 2), b"aligned"), (dict(out=r2.data_ptr() + 1), b"aligned"),
                     (dict(wsp=ws.data_ptr() + 4), b"aligned"), (dict(wsb=need - 8), b"workspace"), (dict(ld=3), b"row stride"),
                     (dict(xp=None), b"null"), (dict(n=3), b"other rows")):
        assert knn(**kw) < 0 and word in L.smd_last_error(), kw
    bneed = L.smd_ball_cover_workspace_bytes(10, 10)

    def cover(qp=x.data_ptr(), xp=x.data_ptr(), rp=r2.data_ptr(), nq=10, excl=0, wsp=ws.data_ptr(), wsb=bneed, rout=re2.data_ptr()):
        return L.smd_ball_cover(qp, 4, nq, xp, 4, 10, 4, rp, None, excl, wsp, wsb, cov.data_ptr(), rout, None)

    for kw, word in ((dict(qp=x.data_ptr() + 2), b"aligned"), (dict(rp=r2.data_ptr() + 2), b"aligned"), (dict(rout=re2.data_ptr() + 2), b"aligned"),
                     (dict(wsb=bneed - 8), b"workspace"), (dict(nq=5, excl=1), b"nq == nx"), (dict(xp=None), b"null")):
        assert cover(**kw) < 0 and word in L.smd_last_error(), kw
    # the launch bound: n = 2,200,000 rows are 17,188 tiles x 1,075 column splits of 256 work-items, past HIP's 2^32 per launch.
    # It is checked before the workspace, so the refusal needs no 9 GB buffer (and a workspace this short is refused anyway).
    big = torch.zeros(2200000, 1, device="cuda")
    br2 = torch.full((2200000,), -7.0, device="cuda")
    bcov = torch.full((2200000,), 9, dtype=torch.uint8, device="cuda")
    assert L.smd_knn_radii(big.data_ptr(), 1, 2200000, 1, 1, ws.data_ptr(), ws.numel(), br2.data_ptr(), None) < 0
    assert b"exceed one launch" in L.smd_last_error()
    assert L.smd_ball_cover(big.data_ptr(), 1, 2200000, big.data_ptr(), 1, 2200000, 1, br2.data_ptr(), None, 0, ws.data_ptr(), ws.numel(),
                            bcov.data_ptr(), br2.data_ptr(), None) < 0
    assert b"exceed one launch" in L.smd_last_error()
    torch.cuda.synchronize()
    # nothing was launched: no output was touched
    assert bool((r2 == -7.0).all()) and bool((re2 == -7.0).all()) and bool((cov == 9).all())
    assert bool((br2 == -7.0).all()) and bool((bcov == 9).all())
