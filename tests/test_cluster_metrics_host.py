"""Host-side parts of --cluster_metrics (no GPU): the flags and their refusals, the float64 PRD curve, F-beta and NDB test of
smd_amd.metrics on hand-made histograms with closed-form answers (and against tests/_cluster_metrics_ref.py), evaluate()'s tags
with the GPU pieces replaced, and the argument checks of the library entry points, which refuse before anything is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _cluster_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KM = ("precision", "recall", "f1", "ndb")


def test_flags_parse_with_their_defaults():
    import smd_amd.flags as F
    fl = F.make_flags(include_sample=True)
    assert fl.cluster_metrics is False and (fl.prd_clusters, fl.prd_runs, fl.ndb_bins) == (20, 10, 50)
    fl.parse(["--compute_metrics", "--cluster_metrics", "--prd_clusters=16", "--prd_runs=3", "--ndb_bins=100"])
    assert fl.cluster_metrics is True and (fl.prd_clusters, fl.prd_runs, fl.ndb_bins) == (16, 3, 100)
    with pytest.raises(F.FlagError):
        F.make_flags(True).parse(["--ndb_bins=fifty"])
    # the engine's own group: the reference's flag surface is untouched
    names = [d.name for d in F.ENGINE_FLAGS]
    assert names.index("cluster_metrics") == names.index("nn_k") + 1
    assert not {"cluster_metrics", "prd_clusters", "prd_runs", "ndb_bins"} & {d.name for d in F.TRAIN_FLAGS + F.SAMPLE_FLAGS}


def _sample(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, os.path.join(ROOT, "sample_ncsn.py"), "--sampling=ddpm", *flags], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("flags,sentence", [
    (("--cluster_metrics=true",), "--cluster_metrics adds the k-means metrics to the evaluation: it needs --compute_metrics"),
    (("--cluster_metrics=true", "--interpolate=true"), "--cluster_metrics does not apply to --interpolate"),
    (("--cluster_metrics=true", "--compute_metrics=true", "--prd_clusters=1"), "--prd_clusters=1"),
    (("--cluster_metrics=true", "--compute_metrics=true", "--prd_clusters=129"), "--prd_clusters=129"),
    (("--cluster_metrics=true", "--compute_metrics=true", "--prd_runs=0"), "--prd_runs=0"),
    (("--cluster_metrics=true", "--compute_metrics=true", "--prd_runs=101"), "--prd_runs=101"),
    (("--cluster_metrics=true", "--compute_metrics=true", "--ndb_bins=1"), "--ndb_bins=1"),
    (("--cluster_metrics=true", "--compute_metrics=true", "--ndb_bins=129"), "--ndb_bins=129"),
    # 1 example of 32 frames is fewer than the 50 bins; 40 examples of shape (2,) are 40 frames
    (("--cluster_metrics=true", "--compute_metrics=true", "--data_shape=32,512", "--sample_size=1"), "are 32 frames, fewer than the 50 clusters"),
    (("--cluster_metrics=true", "--compute_metrics=true", "--data_shape=2", "--sample_size=40"), "are 40 frames, fewer than the 50 clusters"),
])
def test_refusals_fire_before_the_gpu_is_touched(flags, sentence):
    r = _sample(*flags)
    assert r.returncode != 0 and sentence in r.stderr, r.stderr[-2000:]


def test_prd_curve_closed_forms():
    import smd_amd.metrics as M
    # disjoint supports: nothing of one distribution lies under the other
    p, r = M.prd_curve([0.5, 0.5, 0, 0], [0, 0, 0.25, 0.75])
    assert p.shape == r.shape == (1001,) and (p == 0).all() and (r == 0).all()
    assert M.prd_f_beta_score((p, r)) == (0.0, 0.0)
    # equal histograms: precision = min(slope, 1), recall = min(1, 1 / slope), both 1 at slope 1 (angle 500 of 1001)
    h = np.array([0.1, 0.2, 0.3, 0.4])
    p, r = M.prd_curve(h, h)
    slopes = np.tan(np.linspace(1e-10, np.pi / 2 - 1e-10, 1001))
    assert np.abs(p - np.minimum(slopes, 1.0)).max() <= 1e-15 and np.abs(r - np.minimum(1.0, 1.0 / slopes)).max() <= 1e-12
    assert abs(p[500] - 1.0) <= 1e-12 and abs(r[500] - 1.0) <= 1e-12
    f8, f18 = M.prd_f_beta_score((p, r))
    assert 1 - 1e-9 <= f8 <= 1 and 1 - 1e-9 <= f18 <= 1
    # half of the samples' mass outside the support of the reference: precision tops out at 1/2, recall reaches 1
    p, r = M.prd_curve([0.5, 0.5, 0.0], [0.25, 0.25, 0.5])
    assert abs(p.max() - 0.5) <= 1e-12 and abs(r.max() - 1.0) <= 1e-12
    # F_b = (1 + b^2) p r / (b^2 p + r + 1e-10) on a one-point curve
    f8, f18 = M.prd_f_beta_score((np.array([0.5]), np.array([0.25])))
    assert f8 == pytest.approx(65 * 0.125 / (64 * 0.5 + 0.25), rel=1e-9) and f18 == pytest.approx((1 + 1 / 64) * 0.125 / (0.5 / 64 + 0.25), rel=1e-9)
    # and the reference restatement agrees on random histograms
    rng = np.random.default_rng(0)
    a, b = rng.dirichlet(np.ones(20)), rng.dirichlet(np.ones(20))
    for got, want in zip(M.prd_curve(a, b), R.prd_curve(a, b)):
        assert np.abs(got - want).max() <= 1e-12
    assert np.abs(np.array(M.prd_f_beta_score(M.prd_curve(a, b))) - np.array(R.f_beta(R.prd_curve(a, b)))).max() <= 1e-12
    with pytest.raises(ValueError):
        M.prd_f_beta_score((p, r), beta=0)


def test_ndb_two_bin_z_either_side_of_the_threshold():
    import smd_amd.metrics as M
    # two bins, n_r = n_s = 100, p_r = (1/2, 1/2), p_s = (1/2 + a, 1/2 - a): P = 1/2 +- a/2, z = a / sqrt((1/4 - a^2/4) / 50)
    z = lambda a: a / np.sqrt((0.25 - a * a / 4) / 50)
    assert z(0.13) < R.Z95 < z(0.14)
    for a, want in ((0.13, 0.0), (0.14, 1.0)):
        assert abs(R.ndb_z([0.5, 0.5], [0.5 + a, 0.5 - a], 100, 100)[0][0] - z(a)) <= 1e-12
        assert M.ndb_from_proportions([0.5, 0.5], [0.5 + a, 0.5 - a], 100, 100) == want == R.ndb([0.5, 0.5], [0.5 + a, 0.5 - a], 100, 100)
    # one of three bins differs; a bin empty on both sides has SE = 0 and does not count
    assert M.ndb_from_proportions([0.5, 0.5, 0.0, 0.0], [0.5, 0.0, 0.5, 0.0], 1000, 1000) == 0.5
    assert M.ndb_from_proportions([0.25] * 4, [0.25] * 4, 10, 10 ** 6) == 0.0
    assert M.Z_TWO_SIDED_05 == R.Z95 == 1.959963984540054


def test_constants_of_the_driver_are_unchanged():
    import sample_ncsn
    assert sample_ncsn.METRICS_KMEANS == KM
    assert sample_ncsn.NN_METRICS == ("improved_precision", "improved_recall", "improved_f1", "ipr_realism")
    assert sample_ncsn.METRICS_NOT_UPSTREAM == ("precision", "recall", "f1", "improved_precision", "improved_recall", "improved_f1",
                                                "ipr_realism", "ndb")
    assert sample_ncsn.CLUSTER_METRICS == KM


class _Recorder:
    def __init__(self):
        self.rows = []

    def scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass


def test_evaluate_adds_the_four_tags_per_point(monkeypatch):
    import sample_ncsn
    import smd_amd.metrics as M
    seen = []

    class Ref:
        def __init__(self, data, device=None):
            self.source = data

    def clustered(ref, samples, prd_clusters, prd_runs, ndb_bins, seed):
        seen.append((prd_clusters, prd_runs, ndb_bins, seed))
        same = samples is ref.source
        return {"precision": 1.0 if same else 0.25, "recall": 1.0 if same else 0.5, "f1": 1.0 if same else 1 / 3, "ndb": 0.0 if same else 0.5}

    monkeypatch.setattr(M, "ReferenceSet", Ref)
    monkeypatch.setattr(M, "frechet_distance", lambda ref, fake: 1.0)
    monkeypatch.setattr(M, "kernel_mmds", lambda ref, fake: {"mmd_rbf": 2.0, "mmd_polynomial": 3.0})
    monkeypatch.setattr(M, "cluster_metrics", clustered)
    rng = np.random.default_rng(0)
    coll = rng.uniform(-1, 1, (41, 3, 4, 5)).astype(np.float32)
    real = rng.uniform(-1, 1, (3, 4, 5)).astype(np.float32)
    w = _Recorder()
    stats = sample_ncsn.evaluate(w, real, coll, None, real, seed=3, cluster_metrics=True, prd_clusters=4, prd_runs=2, ndb_bins=6)
    names = ("frechet_distance", "mmd_rbf", "mmd_polynomial") + KM
    assert [(t, s) for t, _, s in w.rows] == ([(f"ncsn/{m}", i) for i in range(20) for m in names]
                                              + [(f"random/{m}", 0) for m in names] + [(f"real/{m}", 0) for m in names])
    assert seen == [(4, 2, 6, 3)] * 22
    got = {(t, s): v for t, v, s in w.rows}
    assert set(stats) == {"frechet_dist", "mmd_rbf", "mmd_polynomial"} | set(KM)
    assert all(stats[n] == got[(f"ncsn/{n}", 19)] for n in KM)
    assert got[("real/precision", 0)] == got[("real/recall", 0)] == 1.0 and got[("real/ndb", 0)] == 0.0
    # without the flag: the three distances alone
    w2 = _Recorder()
    sample_ncsn.evaluate(w2, real, coll, None, real, compute_final_only=True)
    assert len(w2.rows) == 9 and not any(t.split("/")[1] in KM for t, _, _ in w2.rows)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """SMD_ARG_CHECK returns before the first HIP call, so the refusals can be seen without a GPU (the pointers are never read)"""
    import smd_amd.lib as lib
    L = lib.get_lib()
    p = 0x10000
    assert L.smd_kmeans_assign_workspace_bytes(64000, 20) == 64000 * 4 + 128 * 4 + 500 * 16      # norms of rows and centres, 500 slab partials
    assert L.smd_kmeans_assign_workspace_bytes(0, 5) == L.smd_kmeans_assign_workspace_bytes(10, 0) == L.smd_kmeans_assign_workspace_bytes(10, 129) == -1
    assert L.smd_kmeans_update_workspace_bytes(64000, 512, 20) == 250 * 20 * 512 * 8 + 250 * 20 * 4
    assert L.smd_kmeans_update_workspace_bytes(10, 0, 5) == L.smd_kmeans_update_workspace_bytes(10, 4, 129) == -1
    need = L.smd_kmeans_assign_workspace_bytes(10, 3)
    #        x, ld, n, d, centres, k, prev, workspace, bytes, labels, min_d2, inertia, changed
    for args, word in (((p, 4, 10, 4, p, 0, 0, p, need, p, p, p, p), b"k=0 must be in [1, 128]"),
                       ((p, 4, 10, 4, p, 129, 0, p, need, p, p, p, p), b"k=129 must be in [1, 128]"),
                       ((p, 4, 0, 4, p, 3, 0, p, need, p, p, p, p), b"must be >= 1"), ((p, 4, 10, 0, p, 3, 0, p, need, p, p, p, p), b"must be >= 1"),
                       ((p, 3, 10, 4, p, 3, 0, p, need, p, p, p, p), b"row stride"), ((p + 2, 4, 10, 4, p, 3, 0, p, need, p, p, p, p), b"aligned"),
                       ((p, 4, 10, 4, p, 3, 0, p + 4, need, p, p, p, p), b"aligned"), ((p, 4, 10, 4, p, 3, 0, p, need, p, p, p + 4, p), b"aligned"),
                       ((p, 4, 10, 4, p, 3, 0, p, need, p, p, p, p + 4), b"aligned"), ((p, 4, 10, 4, p, 3, 0, p, need - 8, p, p, p, p), b"workspace"),
                       ((None, 4, 10, 4, p, 3, 0, p, need, p, p, p, p), b"null"), ((p, 4, 10, 4, p, 3, 0, p, need, p, None, None, p), b"null")):
        assert L.smd_kmeans_assign(*args, None) < 0 and word in L.smd_last_error(), args
    with pytest.raises(ValueError, match="k=0"):
        lib.check(L.smd_kmeans_assign(p, 4, 10, 4, p, 0, 0, p, need, p, p, p, p, None), "smd_kmeans_assign")
    uneed = L.smd_kmeans_update_workspace_bytes(10, 4, 3)
    #        x, ld, n, d, labels, prev_centres, k, workspace, bytes, centres, counts
    for args, word in (((p, 4, 10, 4, p, p, 0, p, uneed, p, p), b"k=0 must be in [1, 128]"), ((p, 4, 10, 4, p, p, 129, p, uneed, p, p), b"k=129"),
                       ((p, 4, 0, 4, p, p, 3, p, uneed, p, p), b"must be >= 1"), ((p, 3, 10, 4, p, p, 3, p, uneed, p, p), b"row stride"),
                       ((p, 4, 10, 4, p + 2, p, 3, p, uneed, p, p), b"aligned"), ((p, 4, 10, 4, p, p, 3, p, uneed, p, p + 4), b"aligned"),
                       ((p, 4, 10, 4, p, p, 3, p, uneed - 8, p, p), b"workspace"), ((p, 4, 10, 4, None, p, 3, p, uneed, p, p), b"null"),
                       ((p, 1 << 24, 10, 1 << 23, p, p, 3, p, 1 << 40, p, p), b"exceed one launch")):
        assert L.smd_kmeans_update(*args, None) < 0 and word in L.smd_last_error(), args
