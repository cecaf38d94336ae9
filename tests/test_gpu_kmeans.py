"""csrc/kmeans.hip (smd_kmeans_assign, smd_kmeans_update) and the k-means, PRD and NDB functions of smd_amd.metrics on the GPU
against the float64 brute force of tests/_cluster_metrics_ref.py.

Error model.  s_ij = -2 <x_i, c_j> + |c_j|^2 in fp32 differs from the exact value by at most
e_ij = (d + 4) 2^-24 (2 |x_i| |c_j| + |c_j|^2).  A row is CERTAIN when the float64 gap from its best centre to every other one
exceeds e_i,best + e_ij: there the GPU's label must be float64's.  The share of the other rows is a property of the inputs alone
and is asserted to stay below 0.5 %.  min_d2 is within e_i,label + (d + 4) 2^-24 |x_i|^2, the inertia within the sum of those.
A mean is within 2^-24 |c| + n_c 2^-52 max|x| (fp64 accumulation of fp32 values in any order, one division, one rounding)."""
import numpy as np
import pytest
import torch

import _cluster_metrics_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1003, 7, 2), (4099, 42, 20), (4099, 146, 50), (1003, 512, 128), (4099, 512, 50), (77, 42, 1)]
FAMILIES = ("gaussian", "mixture")
CAP = 0.005
_CASES = {}


def case(family, n, d, k):
    """(x fp32, centres fp32, float64 labels, certain, s, e) of one shape and family, computed once"""
    key = (family, n, d, k)
    if key not in _CASES:
        rng = np.random.default_rng([FAMILIES.index(family), n, d, k])
        x = R.gaussian(rng, n, d) if family == "gaussian" else R.mixture(rng, n, d, max(k, 2))
        c = R.make_centres(rng, x, k)
        _CASES[key] = (x, c) + R.labels_certain(x, c)
    return _CASES[key]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_labels(name, lab_gpu, lab, certain):
    und = int((~certain).sum())
    differ = int((lab_gpu != lab).sum())
    print(f"  {name}: uncertain rows {und} of {len(lab)} ({100.0 * und / len(lab):.3f} %), labels that differ from float64: {differ}")
    assert und <= CAP * len(lab), "the float64 reference alone exceeds the cap: a bad test input"
    assert lab_gpu.min() >= 0 and np.array_equal(lab_gpu[certain], lab[certain])


def check_min_d2(name, x, s, e, lab_gpu, m_gpu, inertia_gpu):
    ref, bound = R.min_d2(x, s, lab_gpu), R.min_d2_bound(x, e, lab_gpu)
    err = np.abs(m_gpu.astype(np.float64) - ref)
    print(f"  {name}: max |min_d2 - f64| / bound = {float((err / bound).max()):.3f}, inertia {inertia_gpu:.9g} f64 {ref.sum():.9g} "
          f"(bound {bound.sum():.3e})")
    assert (err <= bound).all()
    assert abs(inertia_gpu - ref.sum()) <= bound.sum()
    # the inertia is the fp64 sum of the fp32 values it returns beside it
    assert abs(inertia_gpu - m_gpu.astype(np.float64).sum()) <= 2 * len(x) * 2.0 ** -53 * float(m_gpu.astype(np.float64).sum())


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_assign_against_float64(n, d, k, family):
    import smd_amd.metrics as M
    x, c, lab, certain, s, e = case(family, n, d, k)
    lab_gpu, m_gpu, inertia, changed = M.kmeans_assign(cuda(x), cuda(c))
    lab_gpu, m_gpu = lab_gpu.cpu().numpy(), m_gpu.cpu().numpy()
    assert lab_gpu.dtype == np.int32 and lab_gpu.max() < k and int(changed) == n
    check_labels(f"{family} {(n, d, k)}", lab_gpu, lab, certain)
    check_min_d2(f"{family} {(n, d, k)}", x, s, e, lab_gpu, m_gpu, float(inertia))


def test_ties_strides_changed_and_repeatability():
    import smd_amd.metrics as M
    x, c, lab, certain, s, e = case("mixture", 4099, 146, 50)
    xg, cg = cuda(x), cuda(c)
    l0, m0, i0, _ = M.kmeans_assign(xg, cg)
    # two calls: the same bits
    l1, m1, i1, _ = M.kmeans_assign(xg, cg)
    assert torch.equal(l0, l1) and torch.equal(m0, m1) and float(i0) == float(i1)
    # a centre with a twin of identical bits at a higher index: the twin is never chosen, and nothing else moves
    twin = np.concatenate([c, c[:7]])
    lt = M.kmeans_assign(xg, cuda(twin))[0]
    assert torch.equal(lt, l0) and int(lt.max()) < 50
    swapped = np.concatenate([c[:7], c])                      # now the ORIGINALS of 0..6 sit at 7..13: rows of those clusters move down
    ls = M.kmeans_assign(xg, cuda(swapped))[0].cpu().numpy()
    want = np.where(l0.cpu().numpy() < 7, l0.cpu().numpy(), l0.cpu().numpy() + 7)
    assert np.array_equal(ls, want)
    # ld > d: a column slice of a wider tensor gives the bits of its contiguous copy
    wide = torch.zeros(4099, 200, device="cuda")
    wide[:, 31:177] = xg
    wide[:, :31] = 7.0
    wide[:, 177:] = -7.0
    sl = wide[:, 31:177]
    assert sl.stride(0) == 200 and not sl.is_contiguous()
    l2, m2, i2, _ = M.kmeans_assign(sl, cg)
    assert torch.equal(l2, l0) and torch.equal(m2, m0) and float(i2) == float(i0)
    u2, n2 = M.kmeans_update(sl, l0, cg)
    u0, n0 = M.kmeans_update(xg, l0, cg)
    assert torch.equal(u2, u0) and torch.equal(n2, n0)
    # changed counts exactly against a perturbed previous labelling, and prev_labels is the buffer that is written
    rng = np.random.default_rng(5)
    prev = l0.cpu().numpy().copy()
    hit = rng.choice(4099, 333, replace=False)
    prev[hit] = (prev[hit] + 1 + rng.integers(0, 49, 333)) % 50
    buf = cuda(prev)
    l3, _, _, ch = M.kmeans_assign(xg, cg, buf)
    assert int(ch) == 333 and l3.data_ptr() == buf.data_ptr() and torch.equal(buf, l0)
    assert int(M.kmeans_assign(xg, cg, buf)[3]) == 0


@pytest.mark.parametrize("n,d,k", [(1003, 7, 2), (4099, 146, 50), (1003, 512, 128), (77, 42, 1), (300, 65, 3)])
def test_update_against_float64(n, d, k):
    import smd_amd.metrics as M
    if (n, d, k) == (300, 65, 3):                              # a strip of one column, slabs of 256 and 44 rows
        rng = np.random.default_rng(9)
        x = R.mixture(rng, n, d, k)
        c = R.make_centres(rng, x, k)
        lab = R.scores(x, c).argmin(1)
    else:
        x, c, lab = case("mixture", n, d, k)[:3]
    far = np.full((1, d), 9.0, np.float32)                     # a centre far outside the data: its cluster is empty
    far[0, ::2] = -9.0
    c2 = np.concatenate([c[:k // 2], far, c[k // 2:]]) if k < 128 else np.concatenate([c[:64], far, c[65:]])
    lab2 = R.scores(x, c2).argmin(1).astype(np.int32)
    empty = np.flatnonzero(np.bincount(lab2, minlength=len(c2)) == 0)
    assert (k // 2 if k < 128 else 64) in empty
    new, counts = M.kmeans_update(cuda(x), cuda(lab2), cuda(c2))
    new2, counts2 = M.kmeans_update(cuda(x), cuda(lab2), cuda(c2))
    assert torch.equal(new, new2) and torch.equal(counts, counts2)
    new, counts = new.cpu().numpy(), counts.cpu().numpy()
    ref, ref_counts = R.means(x, lab2, c2)
    assert counts.dtype == np.int64 and np.array_equal(counts, ref_counts) and counts.sum() == n
    err = np.abs(new.astype(np.float64) - ref)
    bound = R.mean_bound(x, ref, ref_counts)
    print(f"  update {(n, d, len(c2))}: max err {float(err.max()):.3e}, max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, "
          f"empty clusters {len(empty)}")
    assert (err <= bound).all()
    assert np.array_equal(new[empty].view(np.uint32), c2[empty].view(np.uint32))       # kept bit for bit


@pytest.mark.parametrize("n,d,k", [(4099, 42, 20), (4099, 512, 50)])
def test_whole_runs_teacher_forced(n, d, k):
    import smd_amd.metrics as M
    x = case("mixture", n, d, k)[0]
    xg = cuda(x)
    trace = []
    centres, labels, inertia, n_iter = M.kmeans(xg, k, seed=[3, 1], max_iter=100, trace=trace)
    seeds = trace[0]["seeds"]
    steps = trace[1:]
    assert len(set(seeds.tolist())) == k and seeds[0] == min(int(np.random.default_rng([3, 1, 0]).random(k)[0] * n), n - 1)
    assert np.array_equal(steps[0]["centres"].cpu().numpy(), x[seeds])
    assert steps[-1]["changed"] == 0 and n_iter == len(steps) - 1 < 100
    assert steps[0]["changed"] == n
    assert torch.equal(steps[-1]["labels"], labels) and steps[-1]["inertia"] == inertia and torch.equal(steps[-1]["centres"], centres)
    emax = []                                                  # sum_i max_j e_ij of every iteration's centres
    for t, st in enumerate(steps):
        c = st["centres"].cpu().numpy()
        lab, certain, s, e = R.labels_certain(x, c)
        emax.append(float(e.max(1).sum()))
        lab_gpu = st["labels"].cpu().numpy()
        check_labels(f"{(n, d, k)} iteration {t}", lab_gpu, lab, certain)
        assert abs(st["inertia"] - R.min_d2(x, s, lab_gpu).sum()) <= R.min_d2_bound(x, e, lab_gpu).sum()
        if t > 0:
            prev = steps[t - 1]
            prev_lab, prev_c = prev["labels"].cpu().numpy(), prev["centres"].cpu().numpy()
            want, counts = R.means(x, prev_lab, prev_c)
            assert (np.abs(c.astype(np.float64) - want) <= R.mean_bound(x, want, counts)).all()
            assert st["changed"] == int((lab_gpu != prev_lab).sum())
            # Lloyd descent up to round-off (the update and the assignment both lower the exact inertia): 2 sum_i max_j e_ij, each
            # of the two inertias with the e of its own centres
            assert st["inertia"] <= prev["inertia"] + emax[t - 1] + emax[t]
    print(f"  kmeans {(n, d, k)}: {n_iter} updates, inertia {steps[0]['inertia']:.6g} -> {inertia:.6g}")
    # the same seed: the same bits
    c2, l2, i2, n2 = M.kmeans(xg, k, seed=[3, 1], max_iter=100)
    assert torch.equal(c2, centres) and torch.equal(l2, labels) and i2 == inertia and n2 == n_iter
    # max_iter: the labels are those of the returned centres
    c3, l3, i3, n3 = M.kmeans(xg, k, seed=[3, 1], max_iter=2)
    assert n3 == 2 and torch.equal(M.kmeans_assign(xg, c3)[0], l3)
    # n_init: the lowest inertia wins
    assert M.kmeans(xg, k, seed=7, n_init=3)[2] <= M.kmeans(xg, k, seed=7, n_init=1)[2]


def test_seeding_with_fewer_distinct_rows_than_clusters():
    import smd_amd.metrics as M
    rng = np.random.default_rng(2)
    two = rng.uniform(-1, 1, (2, 42)).astype(np.float32)
    x = two[[0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1]]
    xg = cuda(x)
    for seed in range(4):
        u = np.random.default_rng([seed, 0]).random(5)
        idx = M.kmeans_seeds(xg, 5, u).cpu().numpy()
        first = min(int(u[0] * 11), 10)
        assert idx[0] == first and len(set(idx.tolist())) == 5
        assert (x[idx[1]] != x[first]).any()                  # the second centre is the other row: all the mass is there
        # after both rows are centres the mass is zero: the lowest-index rows not yet chosen, in order
        free = [i for i in range(11) if i not in idx[:2]]
        assert idx[2:].tolist() == free[:3], (idx, free)
    centres, labels, inertia, n_iter = M.kmeans(xg, 5, seed=0)
    assert inertia == 0.0 and np.array_equal(x[labels.cpu().numpy() >= 0], x)
    assert np.array_equal(centres.cpu().numpy()[labels.cpu().numpy()], x)


def test_prd_and_ndb_from_gpu_labels():
    import smd_amd.metrics as M
    rng = np.random.default_rng(11)
    real, fake = R.mixture(rng, 2048, 42, 20), R.mixture(rng, 1536, 42, 20)
    rg, fg = cuda(real), cuda(fake)
    # PRD: the host part on the GPU's labels equals the reference's host part on the same labels
    k, runs = 20, 3
    prec, rec = np.zeros(1001), np.zeros(1001)
    for run in range(runs):
        lab = M.kmeans(torch.cat((rg, fg)), k, seed=[4, run])[1].cpu().numpy()
        p, r = R.prd_curve(R.histogram(lab[:2048], k), R.histogram(lab[2048:], k))
        prec += p / runs
        rec += r / runs
    prd = M.precision_recall_distribution(rg, fg, num_clusters=k, num_runs=runs, seed=4)
    assert prd[0].shape == prd[1].shape == (1001,)
    assert np.abs(prd[0] - prec).max() <= 1e-12 and np.abs(prd[1] - rec).max() <= 1e-12
    assert np.abs(np.array(M.prd_f_beta_score(prd)) - np.array(R.f_beta((prec, rec)))).max() <= 1e-12
    # NDB likewise
    ref = M.ReferenceSet(rg)
    centres, p_r = ref.ndb_bins(50, 4)
    assert ref.ndb_bins(50, 4)[0] is centres                   # cached per (k, seed)
    p_s = R.histogram(M.kmeans_assign(fg, centres)[0].cpu().numpy(), 50)
    assert abs(p_r.sum() - 1.0) <= 1e-12 and abs(M.ndb_score(ref, fg, k=50, seed=4) - R.ndb(p_r, p_s, 2048, 1536)) <= 1e-12
    # a set against itself: equal histograms, no different bin -- no identity special case is needed
    f8, f18 = M.prd_f_beta_score(M.precision_recall_distribution(ref, ref, num_runs=2, seed=4))
    assert f8 >= 1 - 1e-6 and f18 >= 1 - 1e-6
    f8, f18 = M.prd_f_beta_score(M.precision_recall_distribution(rg, rg.clone(), num_runs=2, seed=4))
    assert f8 >= 1 - 1e-6 and f18 >= 1 - 1e-6
    assert M.ndb_score(ref, ref, k=50, seed=4) == 0.0 and M.ndb_score(rg, rg.clone(), k=50, seed=4) == 0.0
    km = M.cluster_metrics(ref, fg, prd_clusters=k, prd_runs=runs, ndb_bins=50, seed=4)
    want_r, want_p = R.f_beta((prec, rec))
    assert abs(km["precision"] - want_p) <= 1e-12 and abs(km["recall"] - want_r) <= 1e-12
    assert km["f1"] == M.f1_score(km["precision"], km["recall"]) and 0.0 <= km["ndb"] <= 1.0
    # a shifted copy lands in few bins: most bins differ
    g = R.gaussian(rng, 4099, 42)
    shifted = M.ndb_score(g, g + np.float32(0.5), k=50, seed=0)
    print(f"  ndb of clip(0.25 N) against its copy shifted by 0.5: {shifted:.3f}")
    assert shifted >= 0.5


def test_argument_errors_raise_before_any_launch():
    import smd_amd.metrics as M
    x = torch.zeros(200, 8, device="cuda")
    with pytest.raises(ValueError, match="k=0"):
        M.kmeans(x, 0)
    with pytest.raises(ValueError, match="k=129"):
        M.kmeans(x, 129)
    with pytest.raises(ValueError, match="n=100 rows cannot seed k=128"):
        M.kmeans(x[:100], 128)
    with pytest.raises(ValueError, match="d mismatch"):
        M.kmeans_assign(x, torch.zeros(4, 9, device="cuda"))
    with pytest.raises(ValueError, match="d mismatch"):
        M.kmeans_update(x, torch.zeros(200, dtype=torch.int32, device="cuda"), torch.zeros(4, 9, device="cuda"))
    with pytest.raises(ValueError, match="k=0"):
        M.kmeans_assign(x, torch.zeros(0, 8, device="cuda"))
    with pytest.raises(ValueError, match="k=129"):
        M.kmeans_assign(x, torch.zeros(129, 8, device="cuda"))
    with pytest.raises(ValueError, match="labels"):
        M.kmeans_update(x, torch.zeros(200, dtype=torch.int64, device="cuda"), torch.zeros(4, 8, device="cuda"))
    with pytest.raises(ValueError, match="k=129"):
        M.ndb_score(x, x, k=129)
    with pytest.raises(ValueError, match="d mismatch"):
        M.precision_recall_distribution(x, torch.zeros(200, 9, device="cuda"))
