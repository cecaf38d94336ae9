"""smd_nn_search (csrc/nn_search.hip, smd_amd.metrics.nn_search) against the float64 brute force of tests/_nn_search_ref.py.

Error model (DESIGN.md sections 14 and 24, derived, not tuned).  The fp32 d2 = (-2 <q,x> + |q|^2) + |x|^2 of a pair differs from the
exact one by at most m = (d + 4) 2^-24 (|q| + |x|)^2, taken per pair.
  * Values: every returned d2 is within m of the float64 d2 of the pair (query, returned index).
  * Indices: perturbing every distance of a query by at most M_q = max_i m(q, x_i) cannot move a candidate across a float64 gap
    wider than 2 M_q, so where the gap between the k-th and the (k+1)-th float64 distance exceeds 2 M_q the returned index SET is
    the reference's.  The other queries are undecidable; their share -- in the float64 reference alone -- is capped at 0.5 % of
    the queries (a condition on the test's inputs, asserted).
The shapes are the smallest that cross each boundary of the kernel: the tile is 128 rows, a column split 16 tiles = 2048
candidates."""
import numpy as np
import pytest
import torch

import _nn_search_ref as S
from _nn_metrics_ref import sqdist

pytestmark = pytest.mark.gpu

CAP = 0.005
INF = float("inf")


def latent(n, d, seed):
    return np.clip(0.25 * np.random.default_rng(seed).standard_normal((n, d)), -1, 1).astype(np.float32)


def sets(nq, nx, d, seed=0):
    """candidates: the normalised latent law.  Queries: iid of the same law, except at the sequence-level d, where the order
    statistics of iid distances (spread ~ 23 around 2048) lie closer than 2m ~ 8: there a query sits on the segment between two
    candidates, 0.3 of the way, so its first two neighbours (0.09 D, 0.49 D) and the rest (~0.79 D) are far apart."""
    x = latent(nx, d, [seed, 1])
    if d < 1024:
        return latent(nq, d, [seed, 2]), x
    rng = np.random.default_rng([seed, 3])
    a, b = rng.permutation(nx)[:nq], rng.permutation(nx)[:nq]
    b = np.where(a == b, (b + 1) % nx, b)
    return (x[a] + np.float32(0.3) * (x[b] - x[a])).astype(np.float32), x


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(name, q, x, k, d2_g, idx_g, q_base=0, x_base=0, exclude_self=False):
    """the module docstring's two checks; returns the float64 reference"""
    nq, d = q.shape
    dqx = sqdist(q, x)
    d2_r, idx_r, gap = S.nn_search(q, x, k, q_base, x_base, exclude_self, dqx=dqx)
    m = S.pair_bound(d, q, x)
    assert d2_g.shape == idx_g.shape == (nq, k) and d2_g.dtype == np.float32 and idx_g.dtype == np.int64
    # the (+inf, -1) tail sits exactly where the reference has it
    empty = idx_r < 0
    assert np.array_equal(idx_g < 0, empty) and np.all(idx_g[empty] == -1) and np.all(np.isposinf(d2_g[empty]))
    assert np.all(np.isfinite(d2_g[~empty])) and np.all(idx_g[~empty] >= x_base) and np.all(idx_g[~empty] < x_base + len(x))
    # ascending pairs, no index twice
    a, b = d2_g[:, :-1], d2_g[:, 1:]
    with np.errstate(invalid="ignore"):
        assert np.all((a < b) | ((a == b) & ((idx_g[:, :-1] < idx_g[:, 1:]) | empty[:, 1:])))
    if exclude_self:
        assert not np.any(idx_g == (q_base + np.arange(nq))[:, None])
    rows = np.arange(nq)[:, None].repeat(k, 1)
    loc = np.where(empty, 0, idx_g - x_base)
    err = np.where(empty, 0.0, np.abs(d2_g.astype(np.float64) - dqx[rows, loc]) / m[rows, loc])
    und = gap <= 2 * m.max(1)
    print(f"  {name} nq={nq} nx={len(x)} d={d} k={k}: worst |d2 - d2_f64| / m = {err.max():.3f}, undecidable {int(und.sum())} of {nq} "
          f"({100.0 * und.mean():.3f} %)")
    assert err.max() <= 1.0
    assert und.sum() <= CAP * nq, "the float64 reference alone exceeds the cap: a bad test input"
    assert np.array_equal(np.sort(idx_g[~und], 1), np.sort(idx_r[~und], 1))
    return d2_r, idx_r


CASES = [(1, 1, 1, 1), (1, 3, 5, 8), (129, 127, 5, 3), (130, 2049, 42, 8), (64, 4100, 146, 1), (16, 300, 16384, 2)]


@pytest.mark.parametrize("nq,nx,d,k", CASES)
def test_values_and_indices_match_float64(nq, nx, d, k):
    import smd_amd.metrics as M
    q, x = sets(nq, nx, d)
    d2, idx = M.nn_search(cuda(q), cuda(x), k)
    check("search", q, x, k, d2.cpu().numpy(), idx.cpu().numpy())
    if nx < k:
        assert np.all(idx.cpu().numpy()[:, nx:] == -1)
    # global numbering and self exclusion at the same shape: row j of q is candidate j of a set that begins with q
    if nq <= nx and d < 1024:
        xs = x.copy()
        xs[:nq] = q
        d2, idx = M.nn_search(cuda(q), cuda(xs), k, q_base=1000, x_base=1000, exclude_self=True)
        check("exclude_self", q, xs, k, d2.cpu().numpy(), idx.cpu().numpy(), 1000, 1000, True)


def test_equal_distances_come_back_in_index_order():
    """row 5 again at 131 (another tile), 2050 (another column split) and, through a second slab, at x_base + 7"""
    import smd_amd.metrics as M
    x = latent(2100, 42, 11)
    x[131] = x[2050] = x[5]
    slab = latent(20, 42, 12)
    slab[7] = x[5]
    q = (x[5:6] + np.float32(1e-3)).astype(np.float32)
    for k in (2, 4):
        d2, idx = M.nn_search(cuda(q), cuda(x), k)
        d2, idx = M.nn_search(cuda(q), cuda(slab), k, x_base=5000, out=(d2, idx))
        d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
        assert idx[0].tolist() == [5, 131, 2050, 5007][:k]
        assert np.all(d2[0].view(np.uint32) == d2[0, 0].view(np.uint32)) and 0 < d2[0, 0] < 1e-3
        # the other order of the slabs: the same bits
        e2, edx = M.nn_search(cuda(q), cuda(slab), k, x_base=5000)
        e2, edx = M.nn_search(cuda(q), cuda(x), k, out=(e2, edx))
        assert np.array_equal(e2.cpu().numpy().view(np.uint32), d2.view(np.uint32)) and np.array_equal(edx.cpu().numpy(), idx)


def same_bits(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("k", [1, 8])
def test_slabs_in_any_order_give_the_bits_of_one_call(k):
    import smd_amd.metrics as M
    q, x = sets(64, 4100, 42, seed=5)
    qt, xt = cuda(q), cuda(x)
    whole = M.nn_search(qt, xt, k)
    bounds = [(0, 2048), (2048, 4096), (4096, 4100)]
    for order in (bounds, bounds[::-1], [bounds[1], bounds[2], bounds[0]]):
        out = None
        for lo, hi in order:
            out = M.nn_search(qt, xt[lo:hi], k, x_base=lo, out=out)
        assert same_bits(out, whole), order
    # a slab of fewer rows than k leaves the (+inf, -1) tail for the next slab to fill
    first = M.nn_search(qt, xt[4096:4100], k, x_base=4096)
    if k > 4:
        assert bool((first[1][:, 4:] == -1).all()) and bool(torch.isposinf(first[0][:, 4:]).all())


def test_slabs_of_the_set_against_itself_with_exclude_self():
    import smd_amd.metrics as M
    x = latent(4100, 42, 6)
    x[4099] = x[17]                                     # a duplicate across slabs: found, at distance 0
    xt = cuda(x)
    k = 3
    whole = M.nn_search(xt, xt, k, exclude_self=True)
    check("self", x, x, k, whole[0].cpu().numpy(), whole[1].cpu().numpy(), exclude_self=True)
    assert int(whole[1][17, 0]) == 4099 and int(whole[1][4099, 0]) == 17 and float(whole[0][17, 0]) == 0.0 == float(whole[0][4099, 0])
    bounds = [(0, 2048), (2048, 4096), (4096, 4100)]
    for order in (bounds, bounds[::-1]):
        parts = []
        for qlo, qhi in bounds:
            out = None
            for lo, hi in order:
                out = M.nn_search(xt[qlo:qhi], xt[lo:hi], k, q_base=qlo, x_base=lo, exclude_self=True, out=out)
            parts.append(out)
        got = (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
        assert same_bits(got, whole), order
    # the bases are global: shifting both by the same amount shifts the indices and nothing else
    shifted = M.nn_search(xt, xt, k, q_base=1 << 40, x_base=1 << 40, exclude_self=True)
    assert torch.equal(shifted[0].view(torch.int32), whole[0].view(torch.int32)) and torch.equal(shifted[1] - (1 << 40), whole[1])
    # without the exclusion every row finds itself first, at distance exactly 0
    plain = M.nn_search(xt, xt, 1)
    assert bool((plain[0] == 0).all()) and torch.equal(plain[1][:4099, 0], torch.arange(4099, device="cuda"))
    assert int(plain[1][4099, 0]) == 17                 # the duplicate's lower index wins the tie


@pytest.mark.parametrize("n,d,k", [(9, 1, 8), (129, 5, 3), (4100, 42, 8)])
def test_knn_radii_are_the_bits_of_the_searchs_kth_distance(n, d, k):
    """knn_radii and nn_search follow one walk (csrc/gram_walk.h) with one distance expression (d2_of), the query owning it, so the k-th
    distance of the search of a set in itself is the radius bit for bit: a consistency condition between two entry points, both
    the code under test, no tolerance.  200 rows (3 at n = 9) are overwritten one after the other with copies of other rows
    (at n = 129 a row can be hit more than once), so exact zeros and tied distances occur."""
    import smd_amd.metrics as M
    torch.manual_seed(n)
    x = (0.25 * torch.randn(n, d)).clamp(-1, 1)
    copies = 3 if n == 9 else 200
    dst, off = torch.randint(n, (copies,)), torch.randint(1, n, (copies,))
    for a, b in zip(dst.tolist(), ((dst + off) % n).tolist()):        # b != a
        x[a] = x[b]
    xt = x.cuda()
    r2 = M.knn_radii(xt, k)
    d2, idx = M.nn_search(xt, xt, k, exclude_self=True)
    assert bool((idx >= 0).all()) and bool((d2[:, 0] == 0).any())
    assert torch.equal(r2.view(torch.int32), d2[:, k - 1].contiguous().view(torch.int32))


def test_footprint_padding_and_repeatability(dev):
    """only d2_out, idx_out and the workspace are written; NaN in the ld > d padding changes nothing; two calls, the same bits"""
    import smd_amd.lib as lib
    from test_gpu_footprint import P, both, ck, st, ws_arena
    L = lib.get_lib()
    nq, nx, d, k = 130, 2100, 42, 3
    q, x = sets(nq, nx, d, seed=7)
    need = L.smd_nn_search_workspace_bytes(nq, nx, k)
    need2 = L.smd_nn_search_workspace_bytes(nq, 100, k)

    def body(r):
        qd, xd = r.inp(torch.from_numpy(q), ld=d + 3), r.inp(torch.from_numpy(x), ld=d + 5)
        for name in ("a", "b"):
            ws = r.out("workspace_" + name, (need,), torch.uint8)
            ck(L.smd_nn_search(P(qd), d + 3, nq, 0, P(xd), d + 5, nx, 0, d, k, 0, 0, P(ws), need, P(r.out("d2_" + name, (nq, k))),
                               P(r.out("idx_" + name, (nq, k), torch.int64)), st()))
        # accumulating: the first 2000 candidates, then the last 100 into the same outputs
        d2, idx, ws = r.out("d2_acc", (nq, k)), r.out("idx_acc", (nq, k), torch.int64), ws_arena(r, need)
        ck(L.smd_nn_search(P(qd), d + 3, nq, 0, P(xd), d + 5, 2000, 0, d, k, 0, 0, P(ws), need, P(d2), P(idx), st()))
        ck(L.smd_nn_search(P(qd), d + 3, nq, 0, P(xd[2000:]), d + 5, 100, 2000, d, k, 0, 1, P(ws), need2, P(d2), P(idx), st()))

    got, _ = both(dev, body, unwritten=("workspace", "workspace_a", "workspace_b"))
    check("footprint", q, x, k, got["d2_a"].numpy(), got["idx_a"].numpy())
    for other in ("b", "acc"):
        assert torch.equal(got["d2_a"].view(torch.int32), got["d2_" + other].view(torch.int32)) and torch.equal(got["idx_a"], got["idx_" + other])


def test_strided_inputs_are_read_as_their_values():
    import smd_amd.metrics as M
    base = cuda(latent(300, 84, 8))
    xs = base[:, ::2]                                   # columns not unit-strided: copied by the wrapper
    rows = cuda(latent(200, 64, 9))[:, :42]             # rows 64 apart: read in place
    want = M.nn_search(rows.contiguous(), xs.contiguous(), 3)
    assert same_bits(M.nn_search(rows, xs, 3), want)


def test_argument_errors_raise_and_launch_nothing():
    import smd_amd.lib as lib
    import smd_amd.metrics as M
    L = lib.get_lib()
    q, x = torch.rand(10, 4, device="cuda"), torch.rand(12, 4, device="cuda")
    for k in (0, 9):
        with pytest.raises(ValueError, match=r"k=\d must be in \[1, 8\]"):
            M.nn_search(q, x, k)
    with pytest.raises(ValueError, match="d mismatch"):
        M.nn_search(q, torch.rand(12, 5, device="cuda"))
    with pytest.raises(ValueError, match="integer k"):
        M.nn_search(q, x, 1.5)
    with pytest.raises(ValueError, match="out must be"):
        M.nn_search(q, x, 2, out=(torch.zeros(10, 3, device="cuda"), torch.zeros(10, 3, dtype=torch.int64, device="cuda")))
    with pytest.raises(ValueError, match="out must be"):
        M.nn_search(q, x, 2, out=(torch.zeros(10, 2, device="cuda"), torch.zeros(10, 2, dtype=torch.int32, device="cuda")))
    need = L.smd_nn_search_workspace_bytes(10, 12, 3)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    d2 = torch.full((10, 3), -7.0, device="cuda")
    idx = torch.full((10, 3), -7, dtype=torch.int64, device="cuda")

    def call(qp=q.data_ptr(), xp=x.data_ptr(), k=3, wsp=ws.data_ptr(), wsb=need, dp=d2.data_ptr(), ip=idx.data_ptr(), ldx=4, xb=0):
        return L.smd_nn_search(qp, 4, 10, 0, xp, ldx, 12, xb, 4, k, 0, 0, wsp, wsb, dp, ip, None)

    for kw, word in ((dict(k=0), b"k=0"), (dict(k=9), b"k=9"), (dict(qp=q.data_ptr() + 2), b"aligned"), (dict(xp=x.data_ptr() + 1), b"aligned"),
                     (dict(dp=d2.data_ptr() + 2), b"aligned"), (dict(ip=idx.data_ptr() + 4), b"aligned"), (dict(wsp=ws.data_ptr() + 4), b"aligned"),
                     (dict(wsb=need - 8), b"workspace"), (dict(ldx=3), b"row stride"), (dict(xp=None), b"null"), (dict(xb=-5), b"x_base=-5")):
        assert call(**kw) < 0 and word in L.smd_last_error(), kw
    torch.cuda.synchronize()
    assert bool((d2 == -7.0).all()) and bool((idx == -7).all()) and bool((ws == 0).all())     # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((idx >= 0).all()) and bool((d2 >= 0).all())
