"""Host-side parts of --nn_metrics (no GPU): the float64 restatement of the nearest-neighbour metrics (tests/_nn_metrics_ref.py)
on hand-built cases, the flags and their refusals, evaluate()'s tags with the GPU pieces replaced, and the argument checks of the
library entry points, which refuse before anything is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _nn_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NN = ("improved_precision", "improved_recall", "improved_f1", "ipr_realism")


def line(*pos):
    return np.array(pos, np.float64)[:, None]


def test_radii_of_points_on_a_line():
    x = line(0, 1, 3, 6, 10)
    assert np.array_equal(R.knn_radii2(x, 1), np.array([1, 1, 2, 3, 4.0]) ** 2)
    assert np.array_equal(R.knn_radii2(x, 2), np.array([3, 2, 3, 4, 7.0]) ** 2)
    assert np.array_equal(R.knn_radii2(x, 4), np.array([10, 9, 7, 6, 10.0]) ** 2)
    # self is excluded by index, not by value: a duplicated row has a neighbour at distance 0
    assert np.array_equal(R.knn_radii2(line(0, 0, 5), 1), [0.0, 0.0, 25.0])
    assert np.array_equal(R.knn_radii2(line(0, 0, 5), 2), [25.0, 25.0, 25.0])
    with pytest.raises(AssertionError):
        R.knn_radii2(line(0, 1), 2)


def test_fake_sets_inside_and_outside_every_ball():
    real = line(0, 1, 3, 6, 10)                       # k = 1 balls: [-1, 1], [0, 2], [1, 5], [3, 9], [6, 14]
    inside, outside = line(0.5, 2.0, 9.0, 14.0), line(-1.5, 14.5, 100.0, -30.0)
    m_in, m_out = R.metrics(real, inside, k=1), R.metrics(real, outside, k=1)
    assert m_in["improved_precision"] == 1.0 and m_out["improved_precision"] == 0.0
    # recall: the fake balls (k = 1 radii 1.5, 1.5, 5, 5 round 0.5, 2, 9, 14) hold 0, 1, 3 (|3 - 2| <= 1.5), 6 and 10
    assert m_in["improved_recall"] == 1.0
    assert m_out["improved_recall"] == 1.0            # radii 16, 85.5, 85.5, 28.5: huge balls hold everything
    assert m_out["improved_f1"] == 0.0 and m_in["improved_f1"] == 1.0
    assert R.f1_score(0.0, 0.0) == 0.0 and R.f1_score(0.5, 1.0) == pytest.approx(2 / 3)
    # the boundary belongs to the ball
    assert (R.cover_margin(R.sqdist(line(14.0), real), R.knn_radii2(real, 1)) >= 0).all()
    assert (R.cover_margin(R.sqdist(line(14.0 + 1e-9), real), R.knn_radii2(real, 1)) < 0).all()


def test_median_pruning_with_even_and_odd_counts():
    odd = line(0, 1, 3, 6, 10)                        # radii 1, 1, 2, 3, 4: median 2 keeps three
    assert np.array_equal(R.keep_mask(R.knn_radii2(odd, 1)), [True, True, True, False, False])
    even = line(0, 1, 3, 6)                           # radii 1, 1, 2, 3: median 1.5 keeps two
    assert np.array_equal(R.keep_mask(R.knn_radii2(even, 1)), [True, True, False, False])
    # realism of q = 8: kept centres 0, 1, 3 with radii 1, 1, 2 at distances 8, 7, 5 -> 2 / 5 (unpruned: 4 / 2 from the centre 10)
    q = line(8.0)
    r2 = R.knn_radii2(odd, 1)
    assert np.sqrt(R.realism2(R.sqdist(q, odd), r2, R.keep_mask(r2)))[0] == pytest.approx(0.4)
    assert np.sqrt(R.realism2(R.sqdist(q, odd), r2))[0] == pytest.approx(2.0)
    assert R.metrics(odd, line(8.0, 30.0), k=1)["ipr_realism"] == pytest.approx((2 / 5 + 2 / 27) / 2)      # the mean over the fake rows
    # a query on a centre: the squared distance is clamped to FLT_MIN and the score stays finite
    assert np.isfinite(R.realism2(R.sqdist(line(1.0), odd), r2, R.keep_mask(r2)))[0]


def test_identity_case_is_leave_one_out():
    x = line(0, 1, 3, 6, 10)
    m = R.metrics(x, None, k=1)
    # 0 in [0, 2] of 1; 1 in [-1, 1] of 0; 3 in [3, 9] of 6; 6 in [6, 14] of 10; 10 is in no other row's ball
    assert m["improved_precision"] == m["improved_recall"] == 0.8
    # kept centres 0, 1, 3: row 0 scores 1 / 1 from centre 1, row 10 scores 2 / 7 from centre 3 (1 / 9 and 1 / 10 from 1 and 0)
    assert m["realism_scores"][0] == pytest.approx(1.0) and m["realism_scores"][4] == pytest.approx(2 / 7)
    # a copy is not the identity case: every row lies at distance 0 from its twin
    assert R.metrics(x, x.copy(), k=1)["improved_precision"] == 1.0


def test_flags_parse_with_their_defaults():
    import smd_amd.flags as F
    fl = F.make_flags(include_sample=True)
    assert fl.nn_metrics is False and fl.nn_k == 3
    fl.parse(["--compute_metrics", "--nn_metrics", "--nn_k=5"])
    assert fl.nn_metrics is True and fl.nn_k == 5 and fl.compute_metrics is True
    with pytest.raises(F.FlagError):
        F.make_flags(True).parse(["--nn_k=three"])


def _sample(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, os.path.join(ROOT, "sample_ncsn.py"), "--sampling=ddpm", *flags], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=300)


def test_refusals_fire_before_the_gpu_is_touched():
    r = _sample("--nn_metrics=true")
    assert r.returncode != 0 and "--nn_metrics adds the nearest-neighbour metrics to the evaluation: it needs --compute_metrics" in r.stderr
    r = _sample("--nn_metrics=true", "--interpolate=true")
    assert r.returncode != 0 and "--nn_metrics does not apply to --interpolate" in r.stderr, r.stderr[-2000:]
    r = _sample("--nn_metrics=true", "--compute_metrics=true", "--nn_k=9")
    assert r.returncode != 0 and "--nn_k=9" in r.stderr, r.stderr[-2000:]


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

    def improved(ref, fake, k=3):
        seen.append(k)
        x = np.asarray(ref.source).reshape(-1, ref.source.shape[-1])
        m = R.metrics(x, None if fake is ref.source else np.asarray(fake).reshape(-1, x.shape[-1]), k)
        return {n: m[n] for n in NN}

    monkeypatch.setattr(M, "ReferenceSet", Ref)
    monkeypatch.setattr(M, "frechet_distance", lambda ref, fake: 1.0)
    monkeypatch.setattr(M, "kernel_mmds", lambda ref, fake: {"mmd_rbf": 2.0, "mmd_polynomial": 3.0})
    monkeypatch.setattr(M, "improved_metrics", improved)
    rng = np.random.default_rng(0)
    coll = rng.uniform(-1, 1, (41, 3, 4, 5)).astype(np.float32)
    real = rng.uniform(-1, 1, (3, 4, 5)).astype(np.float32)
    w = _Recorder()
    stats = sample_ncsn.evaluate(w, real, coll, None, real, seed=3, nn_metrics=True, nn_k=2)
    names = ("frechet_distance", "mmd_rbf", "mmd_polynomial") + NN
    assert [(t, s) for t, _, s in w.rows] == ([(f"ncsn/{m}", i) for i in range(20) for m in names]
                                              + [(f"random/{m}", 0) for m in names] + [(f"real/{m}", 0) for m in names])
    assert seen == [2] * 22
    got = {(t, s): v for t, v, s in w.rows}
    assert set(stats) == {"frechet_dist", "mmd_rbf", "mmd_polynomial"} | set(NN)
    assert all(stats[n] == got[(f"ncsn/{n}", 19)] for n in NN)
    loo = R.metrics(real.reshape(-1, 5), None, 2)
    assert all(got[(f"real/{n}", 0)] == loo[n] for n in NN)
    # the warning of a run without --nn_metrics still names every metric that is not computed
    assert set(NN) <= set(sample_ncsn.METRICS_NOT_UPSTREAM) and not set(NN) & set(sample_ncsn.METRICS_KMEANS)
    w2 = _Recorder()
    sample_ncsn.evaluate(w2, real, coll, None, real, compute_final_only=True)
    assert len(w2.rows) == 9 and not any(t.split("/")[1] in NN for t, _, _ in w2.rows)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """SMD_ARG_CHECK returns before the first HIP call, so the refusals can be seen without a GPU (the pointers are never read)"""
    import smd_amd.lib as lib
    L = lib.get_lib()
    p = 0x10000
    assert L.smd_knn_radii_workspace_bytes(32000, 3) == 32000 * 4 + 16 * 32000 * 3 * 4        # norms + 16 column splits of 3-lists
    assert L.smd_knn_radii_workspace_bytes(10, 0) == L.smd_knn_radii_workspace_bytes(10, 9) == L.smd_knn_radii_workspace_bytes(3, 3) == -1
    assert L.smd_ball_cover_workspace_bytes(0, 5) == -1 and L.smd_ball_cover_workspace_bytes(100, 5000) == 5100 * 4 + 3 * 100 * 4 + 304
    need = L.smd_knn_radii_workspace_bytes(10, 3)
    for args, word in (((p, 4, 10, 4, 0, p, need, p), b"k=0 must be in [1, 8]"), ((p, 4, 10, 4, 9, p, need, p), b"k=9 must be in [1, 8]"),
                       ((p + 2, 4, 10, 4, 3, p, need, p), b"aligned"), ((p, 4, 10, 4, 3, p + 4, need, p), b"aligned"),
                       ((p, 4, 10, 4, 3, p, need - 8, p), b"workspace"), ((p, 4, 3, 4, 3, p, need, p), b"other rows"),
                       ((p, 3, 10, 4, 3, p, need, p), b"row stride"), ((None, 4, 10, 4, 3, p, need, p), b"null"),
                       ((p, 1, 2200000, 1, 1, p, need, p), b"exceed one launch")):
        assert L.smd_knn_radii(*args, None) < 0 and word in L.smd_last_error(), args
    with pytest.raises(ValueError, match="k=0"):
        lib.check(L.smd_knn_radii(p, 4, 10, 4, 0, p, need, p, None), "smd_knn_radii")
    bneed = L.smd_ball_cover_workspace_bytes(10, 10)
    for args, word in (((p + 2, 4, 10, p, 4, 10, 4, p, None, 0, p, bneed, p, p), b"aligned"), ((p, 4, 10, p, 4, 10, 4, p + 2, None, 0, p, bneed, p, p), b"aligned"),
                       ((p, 4, 10, p, 4, 10, 4, p, None, 0, p, bneed - 8, p, p), b"workspace"), ((p, 4, 5, p, 4, 10, 4, p, None, 1, p, bneed, p, p), b"nq == nx"),
                       ((p, 4, 10, p, 4, 10, 4, None, None, 0, p, bneed, p, p), b"null"), ((p, 4, 10, p, 3, 10, 4, p, None, 0, p, bneed, p, p), b"row strides"),
                       ((p, 1, 2200000, p, 1, 2200000, 1, p, None, 0, p, bneed, p, p), b"exceed one launch")):
        assert L.smd_ball_cover(*args, None) < 0 and word in L.smd_last_error(), args
