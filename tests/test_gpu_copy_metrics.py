"""TrainIndex / authenticity / copy_report / copy_metrics (smd_amd.metrics, csrc/nn_search.hip) against the float64 reference of
tests/_nn_search_ref.py at n_train = 600, n_fake = n_held = 200 examples of (S, C) = (4, 42) and (4, 5), at frame level (N*S rows
of C) and sequence level (N rows of S*C).

What fp32 can change (M = (d + 4) 2^-24 (2 max |row|)^2 bounds the error of every d2 involved):
  * a row's nearest training row, where its two nearest float64 distances are within 2M of each other;
  * its authenticity flag, where the float64 margin d2(q, x_i*) - r1_sq[i*] is within 2M of 0 (each side moves by at most M).
Rows with either are undecidable; authenticity must be within undecidable / n of float64.  Planted copies are exact: a copied row
has d2 = 0 on the GPU (the norm is the fmaf chain of the MFMA's dot product) and every other nearest distance is far above its
bound.  Leave-one-out: a row and its nearest row that are each other's nearest are the same pair, on the boundary by index."""
import numpy as np
import pytest
import torch

import _nn_search_ref as S
from _nn_metrics_ref import d2_error_bound

pytestmark = pytest.mark.gpu

N_TRAIN, N_FAKE, SEQ = 600, 200, 4
COPIED = (3, 250, 599, 41, 41, 200, 400)          # training examples the first 7 fake examples copy whole
_CACHE = {}


def latent(shape, seed):
    return np.clip(0.25 * np.random.default_rng(seed).standard_normal(shape), -1, 1).astype(np.float32)


def case(C):
    """(train, held, fake, float64 reports per level), computed once per C and shared"""
    if C not in _CACHE:
        train, held, fake = latent((N_TRAIN, SEQ, C), [C, 0]), latent((N_FAKE, SEQ, C), [C, 1]), latent((N_FAKE, SEQ, C), [C, 2])
        fake[:len(COPIED)] = train[list(COPIED)]
        fake[10, 2] = train[33, 1]                # one lifted frame inside an otherwise new example
        ref = {}
        for seq in (False, True):
            rows = (lambda a: a.reshape(len(a), -1)) if seq else (lambda a: a.reshape(-1, C))
            t, h, f = rows(train), rows(held), rows(fake)
            M = d2_error_bound(t.shape[1], np.concatenate([t, f]), t)
            d2, idx, gap = S.nn_search(f, t, 1)
            r1, _ = S.r1_sq(t)
            margin = d2[:, 0] - r1[idx[:, 0]]
            ref[seq] = dict(rep=S.copy_report(t, h, f, 2), und=(gap <= 2 * M) | (np.abs(margin) <= 2 * M), M=M, r1=r1, t=t, f=f)
        _CACHE[C] = (train, held, fake, ref)
    return _CACHE[C]


def slabs_of(train):
    """three slabs of 200 examples: two on the host, one already on the device"""
    return [train[:200], torch.from_numpy(train[200:400]).cuda(), train[400:]]


@pytest.mark.parametrize("seq", [False, True], ids=["frames", "sequences"])
@pytest.mark.parametrize("C", [42, 5])
def test_index_and_report_match_float64(C, seq):
    import smd_amd.metrics as M
    train, held, fake, ref = case(C)
    r = ref[seq]
    index = M.TrainIndex(slabs_of(train), sequences=seq)
    n, d = r["t"].shape
    assert (index.n, index.d) == (n, d) == ((N_TRAIN, SEQ * C) if seq else (N_TRAIN * SEQ, C))
    err = float(np.abs(index.r1_sq.cpu().numpy().astype(np.float64) - r["r1"]).max())
    print(f"  C={C} {'sequences' if seq else 'frames'}: max |r1_sq - f64| = {err:.3e}, bound M = {r['M']:.3e}")
    assert err <= r["M"]
    assert np.allclose(index.norm.cpu().numpy(), np.sqrt((r["t"].astype(np.float64) ** 2).sum(1)), rtol=1e-12)
    rep, want = M.copy_report(index, held, fake, 2), r["rep"]
    nf = len(r["f"])
    und = int(r["und"].sum())
    print(f"  authenticity gpu {rep['authenticity']:.4f} float64 {want['authenticity']:.4f}, undecidable rows {und} of {nf}; "
          f"exact copies {rep['exact_copies']}; copy_gap gpu {rep['copy_gap']:.6f} float64 {want['copy_gap']:.6f}")
    assert und <= 0.005 * nf, "the float64 reference alone exceeds the cap: a bad test input"
    assert abs(rep["authenticity"] - want["authenticity"]) <= und / nf
    assert abs(M.authenticity(index, fake)["authenticity"] - want["authenticity"]) <= und / nf
    assert rep["exact_copies"] == want["exact_copies"] == (len(COPIED) if seq else len(COPIED) * SEQ + 1)
    # nearest rows: the copies point at their originals (a twice-copied original, twice), values within the bound
    first = rep["nn_idx"][:, 0]
    if seq:
        assert first[:len(COPIED)].tolist() == list(COPIED)
    else:
        assert first[:len(COPIED) * SEQ].tolist() == [e * SEQ + s for e in COPIED for s in range(SEQ)] and first[10 * SEQ + 2] == 33 * SEQ + 1
    assert rep["nn_d2"].shape == rep["nn_idx"].shape == (nf, 2) and np.all(rep["nn_d2"][:, 0] <= rep["nn_d2"][:, 1])
    ok = ~r["und"]
    assert np.array_equal(first[ok], want["nn_idx"][ok, 0])
    assert np.abs(rep["nn_d2"][ok, 0] - want["nn_d2"][ok, 0]).max() <= r["M"]
    # medians of distances: a d2 within M of float64 is a distance within M / (2 sqrt(d2)) to first order; the medians here are far from 0
    mf, mh = want["median_nn_fake"], want["median_nn_held_out"]
    df, dh = r["M"] / mf, r["M"] / mh
    assert abs(rep["median_nn_fake"] - mf) <= df and abs(rep["median_nn_held_out"] - mh) <= dh
    # a quotient of two such values: |a'/b' - a/b| <= (da + (a/b) db) / (b - db)
    assert abs(rep["copy_gap"] - want["copy_gap"]) <= (df + want["copy_gap"] * dh) / (mh - dh)
    assert (rep["k"], rep["n_train"], rep["n_fake"], rep["n_held_out"], rep["version"]) == (2, n, nf, nf, M.COPY_METRICS_VERSION)
    # samples that ARE the held-out set: the gap is exactly 1
    assert M.copy_report(index, held, held.copy(), 1)["copy_gap"] == 1.0


@pytest.mark.parametrize("C", [42, 5])
def test_the_training_set_against_itself_is_leave_one_out(C):
    import smd_amd.metrics as M
    train, held, _, ref = case(C)
    slabs = slabs_of(train)
    index = M.TrainIndex(slabs)
    t, r1, Mb = ref[False]["t"], ref[False]["r1"], ref[False]["M"]
    d2, idx, gap = S.nn_search(t, t, 1, exclude_self=True)
    nearest = idx[:, 0]
    mutual = S.r1_sq(t)[1][nearest] == np.arange(len(t))
    und = ~mutual & ((gap <= 2 * Mb) | (np.abs(d2[:, 0] - r1[nearest]) <= 2 * Mb))
    want = S.authenticity(t)[0]
    print(f"  leave-one-out: float64 {want}, mutual nearest pairs {int(mutual.sum())} rows, undecidable {int(und.sum())} of {len(t)}")
    assert want == 1.0 and und.sum() <= 0.005 * len(t)
    for fake in (index, slabs):                                       # the index itself, or the object it was built from
        got = M.authenticity(index, fake)
        assert got["authentic"].shape == (len(t),) and abs(got["authenticity"] - want) <= und.sum() / len(t)
    rep = M.copy_report(index, held, index, 2)
    assert rep["exact_copies"] == 0 and not np.any(rep["nn_idx"] == np.arange(len(t))[:, None])
    assert np.array_equal(rep["nn_d2"][:, 0].view(np.uint32), index.r1_sq.cpu().numpy().view(np.uint32))
    assert np.array_equal(rep["nn_idx"][:, 0], index.nn1_idx.cpu().numpy())
    # a COPY of the training set is no identity: every row is an exact copy and none is authentic
    twin = M.copy_report(index, held, train.copy(), 1)
    assert twin["authenticity"] == 0.0 and twin["exact_copies"] == len(t) and twin["median_nn_fake"] == 0.0 == twin["copy_gap"]


def test_both_levels_in_one_report_and_one_slab_equals_three():
    import smd_amd.metrics as M
    train, held, fake, ref = case(5)
    rep = M.copy_metrics(slabs_of(train), held, fake, 2)
    one = M.copy_metrics(train, held, fake, 2)
    for s in ("", "_seq"):
        for name in M.COPY_SCALARS:
            assert rep[name + s] == one[name + s], name + s
        assert np.array_equal(rep["nn_idx" + s], one["nn_idx" + s]) and np.array_equal(rep["nn_d2" + s].view(np.uint32), one["nn_d2" + s].view(np.uint32))
    assert rep["exact_copies"] == len(COPIED) * SEQ + 1 and rep["exact_copies_seq"] == len(COPIED)
    assert rep["nn_idx"].shape == (N_FAKE * SEQ, 2) and rep["nn_idx_seq"].shape == (N_FAKE, 2)
    assert (rep["n_train"], rep["n_train_seq"], rep["k"]) == (N_TRAIN * SEQ, N_TRAIN, 2)
    with pytest.raises(ValueError, match="row length"):
        M.TrainIndex([train[:10], train[10:20, :, :3]])
    with pytest.raises(ValueError, match="d mismatch"):
        M.TrainIndex(train).query(np.zeros((3, 7), np.float32))
