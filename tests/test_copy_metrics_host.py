"""Host-side parts of --copy_metrics (no GPU): the float64 restatement of the nearest-neighbour search and the copy metrics
(tests/_nn_search_ref.py) on hand-made cases, the flags, the refusals of sample_ncsn.py before the GPU is touched, and the
argument checks of smd_nn_search, which return before anything is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _nn_search_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def line(*v):
    return np.array(v, np.float64).reshape(-1, 1)


def test_search_orders_by_distance_then_index_and_pads_with_inf():
    x = line(0, 5, 5, 9)
    d2, idx, gap = S.nn_search(line(4), x, 3, x_base=10)
    assert d2.tolist() == [[1.0, 1.0, 16.0]] and idx.tolist() == [[11, 12, 10]] and gap.tolist() == [9.0]
    d2, idx, gap = S.nn_search(line(4, 9), x, 8)
    assert d2[0, :4].tolist() == [1.0, 1.0, 16.0, 25.0] and np.all(np.isinf(d2[:, 4:])) and np.all(idx[:, 4:] == -1)
    assert idx[1, :4].tolist() == [3, 1, 2, 0] and np.all(np.isinf(gap))
    # self is excluded by index, in global numbering: a duplicate of the query stays, at distance 0
    d2, idx, _ = S.nn_search(x, x, 1, q_base=7, x_base=7, exclude_self=True)
    assert idx[:, 0].tolist() == [8, 9, 8, 8] and d2[:, 0].tolist() == [25.0, 0.0, 0.0, 16.0]
    d2, idx, _ = S.nn_search(x[1:3], x, 1, q_base=1, exclude_self=True)
    assert idx[:, 0].tolist() == [2, 1]
    # slabs: the merged lists of two halves are the list of the whole
    whole = S.nn_search(line(4), x, 3)
    a, b = S.nn_search(line(4), x[:2], 3), S.nn_search(line(4), x[2:], 3, x_base=2)
    both = sorted(zip(np.r_[a[0][0], b[0][0]], np.r_[a[1][0], b[1][0]]))[:3]
    assert [v for v, _ in both] == whole[0][0].tolist() and [i for _, i in both] == whole[1][0].tolist()


def test_exact_copies_are_not_authentic_and_are_counted():
    train = np.random.default_rng(0).integers(-8, 9, (50, 6)).astype(np.float64)      # small integers: every d2 is exact
    assert S.r1_sq(train)[0].min() > 0
    fake = train[[3, 3, 17, 40]]
    rep = S.copy_report(train, train[:5] + 0.5, fake)
    assert rep["authenticity"] == 0.0 and rep["exact_copies"] == 4 and rep["nn_idx"][:, 0].tolist() == [3, 3, 17, 40]
    assert rep["median_nn_fake"] == 0.0 and rep["copy_gap"] == 0.0
    assert S.authenticity(train, fake)[0] == 0.0


def test_the_boundary_counts_as_authentic():
    train = line(0, 2, 10)                          # r1 = 2, 2, 8
    assert S.r1_sq(train)[0].tolist() == [4.0, 4.0, 64.0] and S.r1_sq(train)[1].tolist() == [1, 0, 1]
    score, flags, margin = S.authenticity(train, line(-2, -1.5, 3, 18, 17))
    # -2 is 2 from row 0, whose radius is 2: on the boundary; -1.5 is inside; 3 is 1 from row 1 (radius 2); 18 is 8 from row 2
    assert flags.tolist() == [True, False, False, True, False] and margin[0] == 0.0 and margin[3] == 0.0 and score == 0.4


def test_the_training_set_against_itself_is_leave_one_out():
    train = line(0, 1, 3, 6, 10)
    score, flags, margin = S.authenticity(train)
    # row i is one of the OTHER rows of its nearest row i*, so i* is never farther from its own nearest row than from i
    assert score == 1.0 and margin.tolist() == [0.0, 0.0, 3.0, 5.0, 7.0]
    # a copy of the set is not the identity case: every row finds its twin at distance 0
    assert S.authenticity(train, train.copy())[0] == 0.0
    rep = S.copy_report(train, line(20), None, k=2)
    # row 2 (at 3) is 3 away from row 0 and from row 3: the lower index comes first
    assert rep["nn_idx"].tolist() == [[1, 2], [0, 2], [1, 0], [2, 4], [3, 2]] and rep["exact_copies"] == 0
    assert rep["median_nn_fake"] == 2.0 and rep["median_nn_held_out"] == 10.0 and rep["copy_gap"] == 0.2


def test_copy_gap_is_one_when_the_samples_are_the_held_out_set():
    rng = np.random.default_rng(1)
    train, held = rng.standard_normal((80, 5)), rng.standard_normal((30, 5))
    rep = S.copy_report(train, held, held.copy())
    assert rep["copy_gap"] == 1.0 and rep["median_nn_fake"] == rep["median_nn_held_out"] > 0 and rep["exact_copies"] == 0


def test_iid_samples_score_between_copies_and_far_away_points():
    rng = np.random.default_rng(2)
    train, fake = (np.clip(0.25 * rng.standard_normal((400, 8)), -1, 1) for _ in range(2))
    copies = S.authenticity(train, train[:100])[0]
    far = S.authenticity(train, fake + 10.0)[0]
    iid = S.authenticity(train, fake)[0]
    print(f"  authenticity: copies {copies}, iid samples of the training law {iid}, far away {far}")
    assert copies == 0.0 and far == 1.0 and copies < iid < far


def test_pair_bound_is_section_14s():
    q, x = np.array([[3.0, 4.0]]), np.array([[0.0, 0.0], [6.0, 8.0]])
    assert S.pair_bound(2, q, x).tolist() == [[6 * 2.0 ** -24 * 25, 6 * 2.0 ** -24 * 225]]


def test_flags_parse_with_their_defaults():
    import smd_amd.flags as F
    fl = F.make_flags(include_sample=True)
    assert fl.copy_metrics is False and fl.copy_k == 1 and fl.copy_train_examples == 0
    fl.parse(["--copy_metrics", "--copy_k=4", "--copy_train_examples=100"])
    assert fl.copy_metrics is True and fl.copy_k == 4 and fl.copy_train_examples == 100 and fl.compute_metrics is False
    with pytest.raises(F.FlagError):
        F.make_flags(True).parse(["--copy_k=one"])
    assert not {"copy_metrics", "copy_k", "copy_train_examples"} & {d.name for d in F.TRAIN_FLAGS + F.SAMPLE_FLAGS}


def _sample(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, os.path.join(ROOT, "sample_ncsn.py"), "--sampling=ddpm", *flags], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("flags,sentence", [
    (("--copy_metrics=true", "--interpolate=true"), "--copy_metrics does not apply to --interpolate"),
    (("--copy_metrics=true", "--copy_k=0"), "--copy_k=0: --copy_metrics keeps from 1 to 8 training neighbours per row"),
    (("--copy_metrics=true", "--copy_k=9"), "--copy_k=9: --copy_metrics keeps from 1 to 8 training neighbours per row"),
    (("--copy_metrics=true", "--copy_train_examples=-1"), "--copy_train_examples=-1: 0 (every training example)"),
])
def test_refusals_fire_before_the_gpu_is_touched(flags, sentence):
    r = _sample(*flags)
    assert r.returncode != 0 and sentence in r.stderr, r.stderr[-2000:]


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """SMD_ARG_CHECK returns before the first HIP call, so the refusals can be seen without a GPU (the pointers are never read)"""
    import smd_amd.lib as lib
    L = lib.get_lib()
    assert {"smd_nn_search", "smd_nn_search_workspace_bytes"} <= set(lib.declared_symbols(lab=False))
    p = 0x10000
    # norms of both sets + per column split of 2048 candidates one (d2, 32-bit index) list per query
    assert L.smd_nn_search_workspace_bytes(32000, 32000, 3) == 64000 * 4 + 16 * 32000 * 3 * 8
    assert L.smd_nn_search_workspace_bytes(3, 2049, 8) == 2052 * 4 + 2 * 3 * 8 * 8
    assert L.smd_nn_search_workspace_bytes(10, 10, 0) == L.smd_nn_search_workspace_bytes(10, 10, 9) == -1
    assert L.smd_nn_search_workspace_bytes(0, 10, 1) == L.smd_nn_search_workspace_bytes(10, 0, 1) == -1
    need = L.smd_nn_search_workspace_bytes(10, 12, 3)

    def call(q=p, ldq=4, nq=10, qb=0, x=p, ldx=4, nx=12, xb=0, d=4, k=3, ws=p, wsb=need, d2=p, idx=p):
        return L.smd_nn_search(q, ldq, nq, qb, x, ldx, nx, xb, d, k, 0, 0, ws, wsb, d2, idx, None)

    for kw, word in ((dict(k=0), b"k=0 must be in [1, 8]"), (dict(k=9), b"k=9 must be in [1, 8]"), (dict(q=p + 2), b"aligned"),
                     (dict(x=p + 1), b"aligned"), (dict(d2=p + 2), b"aligned"), (dict(idx=p + 4), b"aligned"), (dict(ws=p + 4), b"aligned"),
                     (dict(wsb=need - 8), b"workspace"), (dict(ldq=3), b"row stride"), (dict(ldx=3), b"row stride"), (dict(q=None), b"null"),
                     (dict(idx=None), b"null"), (dict(nq=0), b"must be >= 1"), (dict(d=0), b"must be >= 1"), (dict(xb=-1), b"x_base=-1"),
                     (dict(nq=2200000, nx=2200000, ldq=1, ldx=1, d=1, k=1), b"exceed one launch")):
        assert call(**kw) < 0 and word in L.smd_last_error(), kw
