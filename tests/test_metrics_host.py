"""Host-side parts of --compute_metrics (no GPU): evaluate()'s point selection and tag / step layout with the GPU distances
replaced by the float64 numpy restatement, the eigen-form Frechet trace against scipy's sqrtm, and the flag check."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Recorder:
    def __init__(self):
        self.rows = []
        self.flushed = False

    def scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        self.flushed = True


@pytest.fixture
def numpy_metrics(monkeypatch):
    """smd_amd.metrics with the GPU pieces replaced by tests/_metrics_ref.py; records the fake sets it was handed."""
    import smd_amd.metrics as M
    seen = []

    class Ref:
        def __init__(self, data, device=None):
            self.source = data

    def frechet(ref, fake):
        seen.append(fake)
        return float(R.frechet(np.asarray(ref.source).reshape(-1, ref.source.shape[-1]),
                               np.asarray(fake).reshape(-1, ref.source.shape[-1]))[0])

    def mmds(ref, fake):
        x = np.asarray(ref.source).reshape(-1, ref.source.shape[-1])
        y = x if fake is ref.source else np.asarray(fake).reshape(-1, x.shape[-1])
        rr, rp, _, _ = R.mmds(x, y)
        return {"mmd_rbf": rr, "mmd_polynomial": rp}

    monkeypatch.setattr(M, "ReferenceSet", Ref)
    monkeypatch.setattr(M, "frechet_distance", frechet)
    monkeypatch.setattr(M, "kernel_mmds", mmds)
    return seen


def _collection(t=41, n=3, s=4, c=5, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (t, n, s, c)).astype(np.float32), rng.uniform(-1, 1, (n, s, c)).astype(np.float32)


def test_evaluate_points_tags_and_steps(numpy_metrics):
    import sample_ncsn
    coll, real = _collection()
    w = _Recorder()
    stats = sample_ncsn.evaluate(w, real, coll, None, real, seed=3)
    idx = np.linspace(0, 40, 20).astype(np.uint32)
    assert list(idx[:4]) == [0, 2, 4, 6] and idx[-1] == 40
    # ncsn points in order, then the random control (seeded), then the real control (the eval set itself)
    assert len(numpy_metrics) == 22
    for i, k in enumerate(idx):
        assert numpy_metrics[i] is not None and np.array_equal(numpy_metrics[i], coll[k])
    assert np.array_equal(numpy_metrics[20], np.random.default_rng(3).standard_normal(real.shape).astype(np.float32))
    assert numpy_metrics[21] is real
    tags = [(t, s) for t, _, s in w.rows]
    names = ("frechet_distance", "mmd_rbf", "mmd_polynomial")
    assert tags == ([(f"ncsn/{m}", i) for i in range(20) for m in names] + [(f"random/{m}", 0) for m in names]
                    + [(f"real/{m}", 0) for m in names])
    assert not any(t.startswith("baseline/") for t, _ in tags)               # baseline None: skipped
    assert w.flushed
    last = {t: v for t, v, s in w.rows if t.startswith("ncsn/") and s == 19}
    assert stats == {"frechet_dist": last["ncsn/frechet_distance"], "mmd_rbf": last["ncsn/mmd_rbf"],
                     "mmd_polynomial": last["ncsn/mmd_polynomial"]}
    real_vals = {t: v for t, v, s in w.rows if t.startswith("real/")}
    assert real_vals["real/mmd_rbf"] == 0 and real_vals["real/mmd_polynomial"] == 0


def test_evaluate_final_only_and_baseline(numpy_metrics):
    import sample_ncsn
    coll, real = _collection(seed=1)
    w = _Recorder()
    sample_ncsn.evaluate(w, real, coll, coll[7], real, compute_final_only=True)
    tags = [(t, s) for t, _, s in w.rows]
    assert [t for t in tags if t[0].startswith("ncsn/")] == [("ncsn/frechet_distance", 0), ("ncsn/mmd_rbf", 0),
                                                              ("ncsn/mmd_polynomial", 0)]
    assert tags[:3] == [("baseline/frechet_distance", 0), ("baseline/mmd_rbf", 0), ("baseline/mmd_polynomial", 0)]
    assert np.array_equal(numpy_metrics[0], coll[7]) and np.array_equal(numpy_metrics[1], coll[40])
    with pytest.raises(AssertionError):
        sample_ncsn.evaluate(w, real[:2], coll, None, real)                   # collection.shape[1:] != real.shape


def test_eigen_trace_matches_scipy_sqrtm():
    scipy_linalg = pytest.importorskip("scipy.linalg")
    import smd_amd.metrics as M
    rng = np.random.default_rng(0)
    for d in (1, 3, 42, 146):
        for _ in range(3):
            a, b = rng.standard_normal((d, 2 * d + 3)), rng.standard_normal((d, 2 * d + 5)) * 0.5
            s1, s2 = a @ a.T / a.shape[1], b @ b.T / b.shape[1] + 0.1 * np.eye(d)
            ref = np.trace(scipy_linalg.sqrtm(s1 @ s2)).real
            assert abs(M.trace_sqrt_product(s1, s2) - ref) <= 1e-9 * (np.trace(s1) + np.trace(s2))
    # rank-deficient covariances (n < d): real and finite from the eigen form, the eigenvalues past rank n - 1 zeroed
    x = rng.standard_normal((10, 42))
    s = np.cov(x, rowvar=False)
    r = M.cov_rank(*x.shape)
    assert r == 9
    t = M.trace_sqrt_product(s, s, rank1=r, rank2=r)
    assert np.isfinite(t) and abs(t - np.trace(s)) <= 1e-9 * np.trace(s)
    assert abs(M.frechet_from_moments(x.mean(0), s, x.mean(0), s, rank1=r, rank2=r)) <= 1e-9 * np.trace(s)


def _anisotropic(n, stds, seed, shift=0.0, rotate=True):
    """n rows with per-direction standard deviations ``stds`` (optionally in a random orthonormal basis)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, len(stds))) * stds + shift
    if rotate:
        q, _ = np.linalg.qr(rng.standard_normal((len(stds), len(stds))))
        x = x @ q
    return x


@pytest.mark.parametrize("stds", [np.geomspace(1.0, 0.01, 42), np.geomspace(1.0, 0.02, 42),
                                  np.r_[np.ones(60), np.full(452, 0.03)]], ids=["42-1e4", "42-2.5e3", "512-collapsed"])
def test_frechet_keeps_small_eigenvalues_of_full_rank_covariances(stds):
    """Variance spreads of 1e4 and more (near-collapsed latent dimensions): the eigen form with full-rank covariances drops
    nothing, matches scipy's sqrtm and gives 0 for X against itself."""
    scipy_linalg = pytest.importorskip("scipy.linalg")
    import smd_amd.metrics as M
    d = len(stds)
    x = _anisotropic(4 * d + 500, stds, 1)
    y = _anisotropic(3 * d + 400, stds * np.linspace(0.8, 1.2, d), 2, shift=0.01)
    mu1, s1, mu2, s2 = x.mean(0), np.cov(x, rowvar=False), y.mean(0), np.cov(y, rowvar=False)
    r1, r2 = M.cov_rank(*x.shape), M.cov_rank(*y.shape)
    assert r1 == r2 == d
    diff = mu1 - mu2
    ref = diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * np.trace(scipy_linalg.sqrtm(s1 @ s2)).real
    unit = np.trace(s1) + np.trace(s2) + diff.dot(diff)
    got = M.frechet_from_moments(mu1, s1, mu2, s2, rank1=r1, rank2=r2)
    assert abs(got - ref) <= 1e-9 * unit, (got, ref)
    assert abs(M.frechet_from_moments(mu1, s1, mu1, s1, rank1=r1, rank2=r1)) <= 1e-12 * unit


def test_frechet_rank_deficient_drops_only_the_null_space():
    """n <= d: only the eigenvalues beyond rank n - 1 are zeroed.  Against the same eigen form without truncation in float64
    (whose null-space eigenvalues are ~1e-16 round-off), with a 1e4 spread inside the rank."""
    import smd_amd.metrics as M
    d = 42
    x = _anisotropic(30, np.geomspace(1.0, 0.01, d), 3)
    y = _anisotropic(20, np.geomspace(1.0, 0.01, d), 4, shift=0.05)
    s1, s2 = np.cov(x, rowvar=False), np.cov(y, rowvar=False)
    got = M.trace_sqrt_product(s1, s2, rank1=M.cov_rank(*x.shape), rank2=M.cov_rank(*y.shape))
    ref = R.trace_sqrt_product_eig(s1, s2)
    assert abs(got - ref) <= 1e-6 * (np.trace(s1) + np.trace(s2))
    # the truncation is what keeps round-off out: a 1e-9 perturbation of the null space moves the untruncated form by
    # ~sqrt(1e-9) per direction, the truncated one not at all
    e = np.random.default_rng(5).standard_normal((d, d)) * 1e-9
    s1p = s1 + e @ e.T
    assert abs(M.trace_sqrt_product(s1p, s2, rank1=29, rank2=19) - got) <= 1e-7 * np.trace(s1)


def test_compute_metrics_refuses_interpolate():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sample_ncsn.py"), "--sampling=ddpm", "--interpolate=true",
                        "--compute_metrics=true"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--compute_metrics does not apply to --interpolate" in r.stderr, r.stderr[-2000:]
