"""The evaluation distances (smd_amd.metrics, csrc/metrics.hip) against the float64 restatement of utils/metrics.py:24-77
and sklearn 0.19's kernels (tests/_metrics_ref.py)."""

import numpy as np
import pytest
import torch

import _metrics_ref as R

pytestmark = pytest.mark.gpu

FLT_MIN = 2.0 ** -126          # kernel values below fp32's normal range are not representable by an fp32 kernel


def data(n, d, seed, lo=-1.0, hi=1.0):
    """the normalised latent range [-1, 1] that evaluate() expects"""
    return np.random.default_rng(seed).uniform(lo, hi, (n, d)).astype(np.float32)


SHAPES = [(1, 1, 1), (37, 53, 3), (129, 257, 42), (1000, 777, 146), (8192, 8000, 512)]


@pytest.mark.parametrize("symmetric", [False, True], ids=["full", "symmetric"])
@pytest.mark.parametrize("nx,ny,d", SHAPES)
def test_pair_kernel_sums_match_float64(nx, ny, d, symmetric):
    import smd_amd.metrics as M
    x = data(nx, d, 1)
    y = x if symmetric else data(ny, d, 2, -0.9, 1.0)
    xt = torch.from_numpy(x).cuda()
    yt = None if symmetric else torch.from_numpy(y).cuda()
    ny_ = nx if symmetric else ny
    # gamma = 1 at d = 512: every off-diagonal exp underflows (also in float64 for the full product's largest terms)
    for gamma, degree, coef0 in ((1.0, 1, 0.0), (1.0 / d, 2, 0.5), (0.1 / d, 3, 1.0)):
        got = M.pair_kernel_sums(xt, yt, gamma, 1.0, coef0, degree).cpu().numpy()
        ref = R.kernel_sums(x, y, symmetric, gamma, 1.0, coef0, degree)
        floor = nx * ny_ * FLT_MIN
        assert abs(got[0] - ref[0]) <= 2e-5 * ref[1] + floor, (gamma, got[0], ref[0])
        assert abs(got[1] - ref[2]) <= 2e-5 * ref[3], (degree, got[1], ref[2])


def test_padded_rows_are_masked():
    """nx = 129, ny = 130 (one and two rows past a 128-row tile): with gamma -> 0 every real pair contributes exp(~0) = 1 and
    (0 + c0)^1 = c0 from each zero-padded pair would show; unmasked padding would count 256 x 256 pairs."""
    import smd_amd.metrics as M
    x, y = torch.from_numpy(data(129, 5, 3)).cuda(), torch.from_numpy(data(130, 5, 4)).cuda()
    got = M.pair_kernel_sums(x, y, 1e-12, 1.0, 1.0, 1).cpu().numpy()
    ref = R.kernel_sums(x.cpu().numpy(), y.cpu().numpy(), False, 1e-12, 1.0, 1.0, 1)
    assert abs(got[0] - 129 * 130) < 1e-3
    assert abs(got[1] - ref[2]) <= 2e-5 * ref[3]
    sym = M.pair_kernel_sums(x, None, 1e-12, 1.0, 1.0, 1).cpu().numpy()
    assert abs(sym[0] - 129 * 129) < 1e-3


def test_duplicates_and_repeatability():
    import smd_amd.metrics as M
    x = data(1000, 146, 5)
    assert abs(M.mmd_rbf(x, x)) <= 1e-7 and abs(M.mmd_polynomial(x, x)) <= 1e-7
    # a copy runs the full (non-symmetric) product: the k-ordered norms cancel the duplicated rows' distances exactly
    assert abs(M.mmd_rbf(x, x.copy())) <= 1e-7 and abs(M.mmd_polynomial(x, x.copy())) <= 1e-7
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(data(777, 146, 6)).cuda()
    for y in (yt, None):
        a = M.pair_kernel_sums(xt, y, 1.0 / 146, 1.0, 0.0, 2).cpu().numpy()
        b = M.pair_kernel_sums(xt, y, 1.0 / 146, 1.0, 0.0, 2).cpu().numpy()
        assert a.tobytes() == b.tobytes()
    m1 = M.moments(xt)
    m2 = M.moments(xt)
    assert all(torch.equal(p, q) for p, q in zip(m1, m2))


@pytest.mark.parametrize("n,d", [(20, 42), (300, 3), (4097, 146), (32000, 512)])
def test_moments_match_np_cov(n, d):
    import smd_amd.metrics as M
    rng = np.random.default_rng(n)
    x = (rng.uniform(-1, 1, (n, d)) * rng.uniform(0.1, 1.0, d) + rng.uniform(-0.5, 0.5, d)).astype(np.float32)
    mu, cov = (t.cpu().numpy() for t in M.moments(torch.from_numpy(x).cuda()))
    x64 = x.astype(np.float64)
    rmu, rcov = x64.mean(0), np.cov(x64, rowvar=False)
    assert np.linalg.norm(mu - rmu) <= 1e-6 * np.linalg.norm(rmu)
    assert np.linalg.norm(cov - rcov) <= 1e-6 * np.linalg.norm(rcov)
    assert np.array_equal(cov, cov.T)


@pytest.mark.parametrize("n1,n2,d", [(2000, 1500, 42), (5000, 4000, 146), (30, 20, 42), (64, 700, 146)])
def test_frechet_distance(n1, n2, d):
    import smd_amd.metrics as M
    x = data(n1, d, 7)
    y = (data(n2, d, 8) * 0.8 + 0.1).astype(np.float32)
    got = M.frechet_distance(x, y)
    ref, unit = R.frechet(x, y)
    assert abs(got - ref) <= 1e-5 * unit, (got, ref, unit)
    assert abs(M.frechet_distance(x, x)) <= 1e-6 * unit


def _anisotropic(n, stds, seed, shift=0.0):
    """n fp32 rows with per-direction standard deviations ``stds`` in a random orthonormal basis"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((len(stds), len(stds))))
    return ((rng.standard_normal((n, len(stds))) * stds + shift) @ q).astype(np.float32)


@pytest.mark.parametrize("n,stds", [(32000, np.geomspace(1.0, 0.01, 42)), (32000, np.r_[np.ones(60), np.full(452, 0.03)]),
                                    (30, np.geomspace(1.0, 0.01, 42))], ids=["42-1e4", "512-collapsed", "42-rank-deficient"])
def test_frechet_distance_with_a_spread_of_eigenvalues(n, stds):
    """Variance spreads of 1e4 (near-collapsed latent dimensions) against scipy's sqrtm (n > d) or the float64 eigen form
    (n <= d); X against itself and against a copy gives 0."""
    import smd_amd.metrics as M
    d = len(stds)
    x = _anisotropic(n, stds, 1)
    y = _anisotropic(max(n * 3 // 4, 20), stds * np.linspace(0.8, 1.2, d), 2, shift=0.01)
    got = M.frechet_distance(x, y)
    ref, unit = R.frechet(x, y)
    assert abs(got - ref) <= 1e-5 * unit, (got, ref, unit)
    _, unit_xx = R.frechet(x, x)
    assert abs(M.frechet_distance(x, x)) <= 1e-6 * unit_xx
    assert abs(M.frechet_distance(x, x.copy())) <= 1e-6 * unit_xx


def test_strided_columns_are_read_as_their_values():
    """pair_kernel_sums / moments on tensors whose columns are not unit-strided give what their contiguous copies give"""
    import smd_amd.metrics as M
    base = torch.from_numpy(data(300, 84, 14)).cuda()
    xs = base[:, ::2]
    assert xs.stride(1) == 2
    xc = xs.contiguous()
    y = torch.from_numpy(data(200, 42, 15)).cuda()
    assert torch.equal(M.pair_kernel_sums(xs, y), M.pair_kernel_sums(xc, y))
    assert torch.equal(M.pair_kernel_sums(y, xs), M.pair_kernel_sums(y, xc))
    assert torch.equal(M.pair_kernel_sums(xs), M.pair_kernel_sums(xc))
    assert all(torch.equal(a, b) for a, b in zip(M.moments(xs), M.moments(xc)))


def test_mmds_match_float64():
    import smd_amd.metrics as M
    x, y = data(3000, 42, 9), (data(2500, 42, 10) * 0.9).astype(np.float32)
    for kw in (dict(gamma_rbf=1.0, degree=2, gamma_poly=1.0, coef0=0.0), dict(gamma_rbf=0.05, degree=3, gamma_poly=0.1, coef0=1.0)):
        got = M.kernel_mmds(x, y, **kw)
        rr, rp, sr, sp = R.mmds(x, y, **kw)
        assert abs(got["mmd_rbf"] - rr) <= 2e-5 * sr and abs(got["mmd_polynomial"] - rp) <= 2e-5 * sp
    assert abs(M.mmd_rbf(x, y) - M.kernel_mmds(x, y)["mmd_rbf"]) == 0
    assert abs(M.mmd_polynomial(x, y, 3, 0.1, 1.0) - M.kernel_mmds(x, y, degree=3, gamma_poly=0.1, coef0=1.0)["mmd_polynomial"]) == 0
    ref = M.ReferenceSet(x)
    assert M.kernel_mmds(ref, y) == M.kernel_mmds(x, y) and M.frechet_distance(ref, y) == M.frechet_distance(x, y)


def test_input_forms_give_the_same_values():
    """numpy, CPU tensor, cuda tensor and a non-contiguous (n, S, C) view are the same frames"""
    import smd_amd.metrics as M
    rng = np.random.default_rng(11)
    base = rng.uniform(-1, 1, (40, 32, 84)).astype(np.float32)
    view = torch.from_numpy(base).cuda()[:, :, ::2]                 # (40, 32, 42), strided
    assert not view.is_contiguous()
    frames = view.reshape(-1, 42).cpu().numpy()
    real = data(900, 42, 12)
    outs = []
    for fake in (frames, torch.from_numpy(frames), torch.from_numpy(frames).cuda(), view, view.cpu().numpy()):
        outs.append((M.frechet_distance(real, fake), M.mmd_rbf(real, fake), M.mmd_polynomial(real, fake)))
    assert all(o == outs[0] for o in outs), outs


def test_argument_errors_raise_through_last_error():
    import smd_amd.lib as lib
    import smd_amd.metrics as M
    x, y = torch.rand(10, 4, device="cuda"), torch.rand(12, 5, device="cuda")
    with pytest.raises(ValueError, match="d mismatch"):
        M.pair_kernel_sums(x, y)
    with pytest.raises(ValueError, match="degree=0 must be >= 1"):
        M.mmd_polynomial(x, x.clone(), degree=0)
    with pytest.raises(ValueError, match="integer degree"):
        M.mmd_polynomial(x, x.clone(), degree=1.5)
    L = lib.get_lib()
    need = L.smd_pair_kernel_sums_workspace_bytes(10, 12, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    y4 = torch.rand(12, 3, device="cuda")
    rc = L.smd_pair_kernel_sums(x.data_ptr(), 4, 10, y4.data_ptr(), 3, 12, 4, 0, 1.0, 1.0, 0.0, 2, ws.data_ptr(), need,
                                out.data_ptr(), None)
    assert rc < 0 and b"row strides" in L.smd_last_error()
    short = L.smd_pair_kernel_sums_workspace_bytes(10, 10, 0) - 8
    rc = L.smd_pair_kernel_sums(x.data_ptr(), 4, 10, x.data_ptr(), 4, 10, 4, 0, 1.0, 1.0, 0.0, 2, ws.data_ptr(), short,
                                out.data_ptr(), None)
    assert rc < 0 and b"workspace" in L.smd_last_error()
    rc = L.smd_pair_kernel_sums(x.data_ptr(), 4, 10, None, 4, 12, 4, 1, 1.0, 1.0, 0.0, 2, ws.data_ptr(), need,
                                out.data_ptr(), None)
    assert rc < 0 and b"symmetric" in L.smd_last_error()
    rc = L.smd_pair_kernel_sums(x.data_ptr() + 2, 4, 10, x.data_ptr(), 4, 10, 4, 0, 1.0, 1.0, 0.0, 2, ws.data_ptr(), need,
                                out.data_ptr(), None)
    assert rc < 0 and b"aligned" in L.smd_last_error()
    # nx = ny = 600,000 in full mode: 4688^2 tiles of 256 work-items pass HIP's 2^32 work-item bound of one launch -> refused
    big = torch.zeros(600000, 1, device="cuda")
    bneed = L.smd_pair_kernel_sums_workspace_bytes(600000, 600000, 0)
    bws = torch.empty(bneed, dtype=torch.uint8, device="cuda")
    rc = L.smd_pair_kernel_sums(big.data_ptr(), 1, 600000, big.data_ptr(), 1, 600000, 1, 0, 1.0, 1.0, 0.0, 2, bws.data_ptr(), bneed,
                                out.data_ptr(), None)
    assert rc < 0 and b"exceed one launch" in L.smd_last_error()
    del bws, big
    mws = L.smd_moments_workspace_bytes(10, 4)
    mw = torch.empty(mws, dtype=torch.uint8, device="cuda")
    cov = torch.empty(16, dtype=torch.float64, device="cuda")
    rc = L.smd_moments(x.data_ptr(), 4, 10, 4, mw.data_ptr(), mws - 8, out.data_ptr(), cov.data_ptr(), None)
    assert rc < 0 and b"workspace" in L.smd_last_error()
    rc = L.smd_moments(x.data_ptr(), 4, 1, 4, mw.data_ptr(), mws, out.data_ptr(), cov.data_ptr(), None)
    assert rc < 0 and b"at least 2" in L.smd_last_error()
    with pytest.raises(ValueError, match="null"):
        lib.check(L.smd_moments(None, 4, 10, 4, mw.data_ptr(), mws, out.data_ptr(), cov.data_ptr(), None))
    torch.cuda.synchronize()


class _Recorder:
    def __init__(self):
        self.rows = []

    def scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass


def test_evaluate_on_a_device_collection_matches_float64():
    """sample_ncsn.evaluate() on a device collection (41, 8, 32, 42) and an eval set (8, 32, 42): every logged value against
    the numpy float64 reference."""
    import sample_ncsn
    rng = np.random.default_rng(13)
    real = rng.uniform(-1, 1, (8, 32, 42)).astype(np.float32)
    coll = np.stack([np.clip(rng.standard_normal((8, 32, 42)) * (1.0 - t / 45.0), -1, 1) for t in range(41)]).astype(np.float32)
    w = _Recorder()
    stats = sample_ncsn.evaluate(w, real, torch.from_numpy(coll).cuda(), None, real, seed=5)
    idx = np.linspace(0, 40, 20).astype(np.uint32)
    rand = np.random.default_rng(5).standard_normal((8, 32, 42)).astype(np.float32)
    fr = real.reshape(-1, 42)
    expect = {("ncsn", i): coll[k].reshape(-1, 42) for i, k in enumerate(idx)}
    expect[("random", 0)] = rand.reshape(-1, 42)
    expect[("real", 0)] = fr
    got = {(t, s): v for t, v, s in w.rows}
    assert len(got) == 3 * len(expect) == len(w.rows)
    for (model, i), y in expect.items():
        yy = fr if model == "real" else y
        fd, unit = R.frechet(fr, yy)
        rr, rp, sr, sp = R.mmds(fr, fr if model == "real" else yy)
        assert abs(got[(f"{model}/frechet_distance", i)] - fd) <= 1e-5 * unit, (model, i)
        assert abs(got[(f"{model}/mmd_rbf", i)] - rr) <= 2e-5 * sr, (model, i)
        assert abs(got[(f"{model}/mmd_polynomial", i)] - rp) <= 2e-5 * sp, (model, i)
    assert got[("real/mmd_rbf", 0)] == 0.0 and got[("real/mmd_polynomial", 0)] == 0.0
    assert stats == {"frechet_dist": got[("ncsn/frechet_distance", 19)], "mmd_rbf": got[("ncsn/mmd_rbf", 19)],
                     "mmd_polynomial": got[("ncsn/mmd_polynomial", 19)]}
