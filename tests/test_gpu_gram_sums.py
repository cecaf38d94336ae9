"""smd_pair_kernel_sums and smd_moments (csrc/metrics.hip) to the resolution of one pair and one covariance element
(tests/_gram_sums_ref.py holds the lattices, the float64 references, the derivation of the bounds, the regimes and the planted
faults; tests/test_gram_sums_ref_host.py shows on the CPU that an fp32 emulation of the kernels is inside every bound and that
each planted fault is caught).  Through smd_amd.metrics.pair_kernel_sums / moments / kernel_mmds; a row stride above d is a column
view of a wider buffer whose other columns are NaN.

Exact, no tolerance: the number of zero-distance pairs on integer lattices (full mode: the planted duplicates; symmetric mode:
n + 2 per planted pair; Y = roll(X, s) for every s in 0 .. 256 at 3 x 3 tiles), the polynomial sum on integer lattices against
int64 (coef0 in {0, 1, -3}, degree 1 .. 4, negative bases at odd degrees), the covariance of +- paired integer rows against
(X^T X) / (n - 1), bit for bit and equal to its transpose, mean exactly 0.  Shapes: n in {1, 127, 128, 129, 257, 513}, 129 x 257 and
257 x 513, d in {1, 15, 16, 17, 33}, grids of 1, 3, 4, 6, 9, 15, 25, 289 (full) and 276 (symmetric) tiles; moments at
n in {2, 3, 16, 17, 33, 1024, 1025, 2049, 16385, 20001} x d in {1, 127, 128, 129, 1024}.

Derived bounds, nothing fitted: the rbf sum inside [sum of the per-pair lower ends, sum of the upper ends], the polynomial sum
within the sum of the per-pair bounds, every covariance element within its own bound, the mean within its own, a constant column
exactly 0; kernel_mmds of a 1e-3 perturbation within the composed bound.

Worst |err| / bound against the float64 reference, measured on MI355X (the last test prints this table); every exact test passed
at zero tolerance and the 257 launches of the slot sweep took 0.04 s in all:
    pair sums   clamp          poly 0.014    rbf 0.443
                flat           poly 0.001    rbf 0.000
                latent         poly 0.002    rbf 0.045
                poly_cancel    poly 0.001    rbf 0.001
                poly_neg       poly 0.002    rbf 0.051
                saturate       poly 0.001    rbf 0.003
    moments     collapsed      cov 0.126     mean 0.000
                mixed          cov 0.130     mean 0.000
                offset         cov 0.120     mean 0.000
    kernel_mmds perturbation   mmd_polynomial 8.3e-05   mmd_rbf 2.0e-05
(The ratios are those of the CPU emulation of tests/test_gram_sums_ref_host.py to every printed digit: the kernels round where the
emulation does.  They are small because a bound for n roundings in any order allows n U where a real chain accumulates about
sqrt(n) U; `clamp` is the regime in which the d2 error, not the summation, decides, and it sits at 0.44.  The three sums of an MMD
share their arithmetic, so their errors cancel far below the composed bound; the mean's fp64 sum is correctly rounded here.)
"""
import time

import numpy as np
import pytest
import torch

import _gram_sums_ref as R

pytestmark = pytest.mark.gpu

WORST = {}                 # (kernel, regime) -> worst |err| / bound
PAD = 3


def on_gpu(a, pad=0):
    """the rows of `a` on the device: contiguous, or as the first d columns of a buffer of d + pad columns filled with NaN"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if not pad:
        return t
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :t.shape[1]] = t
    v = buf[:, :t.shape[1]]
    assert v.stride(0) == t.shape[1] + pad
    return v


def sums(x, y, *params):
    import smd_amd.metrics as M
    return M.pair_kernel_sums(x, y, *params).cpu().numpy()


def note(kernel, regime, r, where):
    WORST[(kernel, regime)] = max(WORST.get((kernel, regime), 0.0), r)
    print(f"{kernel} {regime} {where}: worst |err| / bound {r:.3g}")
    assert r <= 1.0, f"{kernel} {regime} {where}: at {r:.3g} of its bound"


# ------------------------------------------------------------------------------------------------ exact: pair sums
@pytest.mark.parametrize("d", R.EXACT_D)
@pytest.mark.parametrize("nx,ny", R.FULL_SHAPES)
def test_duplicate_count_full(nx, ny, d):
    x, y, want, planted = R.dup_full(nx, ny, d)
    for pad in (0, PAD):
        got = sums(on_gpu(x, pad), on_gpu(y, pad), R.GAMMA_COUNT, 1.0, 0.0, 1)[0]
        assert got == want, (nx, ny, d, pad, got, want, planted)


@pytest.mark.parametrize("d", R.EXACT_D)
@pytest.mark.parametrize("n", R.EXACT_N)
def test_duplicate_count_symmetric(n, d):
    x, want, planted = R.dup_symmetric(n, d)
    for pad in (0, PAD):
        got = sums(on_gpu(x, pad), None, R.GAMMA_COUNT, 1.0, 0.0, 1)[0]
        assert got == want, (n, d, pad, got, want, planted)


def test_duplicate_count_beyond_256_tiles():
    """289 tiles in the full mode and 276 in the symmetric one: the strided loop of reduce_pairs_kernel"""
    x, y, want, _ = R.dup_full(R.BIG_FULL, R.BIG_FULL, R.BIG_D)
    assert R.tiles_launched(len(x), len(y), False) > 256
    assert sums(on_gpu(x, PAD), on_gpu(y), R.GAMMA_COUNT, 1.0, 0.0, 1)[0] == want
    x, want, _ = R.dup_symmetric(R.BIG_SYM, R.BIG_D)
    assert R.tiles_launched(len(x), len(x), True) > 256
    assert sums(on_gpu(x, PAD), None, R.GAMMA_COUNT, 1.0, 0.0, 1)[0] == want


def test_slot_sweep():
    """Y = roll(X, s), s = 0 .. 256, at 257 rows (3 x 3 tiles): every row of X meets its copy once, in every (row in tile, column
    in tile) offset, with its own norms; the count is 257 every time"""
    x = on_gpu(R.sweep_rows())
    import smd_amd.metrics as M
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = torch.stack([M.pair_kernel_sums(x, torch.roll(x, s, 0), R.GAMMA_COUNT, 1.0, 0.0, 1) for s in range(R.SWEEP_N)]).cpu().numpy()
    dt = time.perf_counter() - t0
    print(f"slot sweep: {R.SWEEP_N} launches in {dt:.2f} s")
    bad = [(s, outs[s, 0]) for s in range(R.SWEEP_N) if outs[s, 0] != R.SWEEP_N]
    assert not bad, bad[:8]


def _poly_check(nx, ny, d, symmetric):
    for c0 in R.POLY_COEF0:
        for deg in R.POLY_DEGREES:
            x, y, want, neg = R.poly_case(nx, ny, d, c0, deg, symmetric)
            if deg % 2 and nx >= 127 and d > 1 and c0 <= 0:
                assert neg                                   # negative bases at odd degrees
            for pad in (0, PAD):
                got = sums(on_gpu(x, pad), None if symmetric else on_gpu(y, pad), 1.0, 1.0, float(c0), deg)[1]
                assert got == want, (nx, ny, d, symmetric, c0, deg, pad, got, want)


@pytest.mark.parametrize("d", R.EXACT_D)
@pytest.mark.parametrize("nx,ny", R.FULL_SHAPES)
def test_polynomial_sum_full(nx, ny, d):
    _poly_check(nx, ny, d, False)


@pytest.mark.parametrize("d", R.EXACT_D)
@pytest.mark.parametrize("n", R.EXACT_N)
def test_polynomial_sum_symmetric(n, d):
    _poly_check(n, n, d, True)


def test_polynomial_sum_beyond_256_tiles():
    _poly_check(R.BIG_FULL, R.BIG_FULL, R.BIG_D, False)
    _poly_check(R.BIG_SYM, R.BIG_SYM, R.BIG_D, True)


# ------------------------------------------------------------------------------------------------ exact: moments
@pytest.mark.parametrize("d", R.MOM_EXACT_D)
@pytest.mark.parametrize("n", R.MOM_EXACT_N)
def test_moments_exact(n, d):
    import smd_amd.metrics as M
    x = R.moment_rows(n, d)
    want = R.moment_exact(x)
    for pad in (0, PAD):
        mean, cov = (t.cpu().numpy() for t in M.moments(on_gpu(x, pad)))
        assert not mean.any(), (n, d, pad)
        assert np.array_equal(cov, want), (n, d, pad, float(np.abs(cov - want).max()))
        assert np.array_equal(cov, cov.T)


def test_moments_still_refuse_d_1025_and_one_row():
    import smd_amd.metrics as M
    with pytest.raises(ValueError):
        M.moments(torch.zeros(4, 1025, device="cuda"))
    with pytest.raises(ValueError):
        M.moments(torch.zeros(1, 4, device="cuda"))


# ------------------------------------------------------------------------------------------------ bounds: pair sums
def _pair_cases():
    for nx, ny, d in R.PAIR_SHAPES:
        for name in (R.PAIR_REGIMES if d != 512 else ("latent", "clamp")):
            for sym in (False, True):
                yield pytest.param(name, nx, ny, d, sym, id=f"{name}-{nx}x{ny}x{d}-{'symmetric' if sym else 'full'}")


@pytest.mark.parametrize("name,nx,ny,d,sym", list(_pair_cases()))
def test_pair_sums_inside_their_bounds(name, nx, ny, d, sym):
    pr = R.pair_regime(name, nx, ny, d)
    if name == "clamp":                                       # the raw fp32 d2 really goes negative in front of the clamp
        assert (R.raw_d2_32(pr["x"], pr["x"] if sym else pr["y"]) < 0).mean() > 0.1
    for pad in (0, PAD):
        x, y = on_gpu(pr["x"], pad), (None if sym else on_gpu(pr["y"], pad))
        for gr, gp, c0, deg in pr["params"]:
            ref = R.pair_reference(pr["x"], None if sym else pr["y"], sym, gr, gp, c0, deg)
            got = sums(x, y, gr, gp, c0, deg)
            where = f"{nx}x{ny}x{d} {'symmetric' if sym else 'full'} pad {pad} ({gr:g}, {gp:g}, {c0:g}, {deg})"
            print(f"  rbf {got[0]!r} ref {ref['rbf']!r} in [{ref['rbf_lo']!r}, {ref['rbf_hi']!r}]; poly {got[1]!r} ref {ref['poly']!r} +- {ref['poly_bound']:.3g}")
            note("rbf", name, R.rbf_ratio(got[0], ref), where)
            note("poly", name, R.poly_ratio(got[1], ref), where)
            assert ref["rbf_lo"] <= got[0] <= ref["rbf_hi"] and abs(got[1] - ref["poly"]) <= ref["poly_bound"]


# ------------------------------------------------------------------------------------------------ bounds: moments
@pytest.mark.parametrize("n,d", R.MOM_SHAPES)
@pytest.mark.parametrize("name", R.MOM_REGIMES)
def test_moments_inside_their_bounds(name, n, d):
    import smd_amd.metrics as M
    x = R.moments_regime(name, n, d)
    rm, rc, dm, bound = R.moments_reference(x)
    for pad in (0, PAD):
        mean, cov = (t.cpu().numpy() for t in M.moments(on_gpu(x, pad)))
        note("mean", name, R.worst_ratio(mean, rm, dm), f"n={n} d={d} pad {pad}")
        note("cov", name, R.worst_ratio(cov, rc, bound), f"n={n} d={d} pad {pad}")
        assert (np.abs(mean - rm) <= dm).all() and (np.abs(cov - rc) <= bound).all()
        c = R.CONST_COL                                       # a constant column is exact
        assert mean[c] == np.float64(np.float32(R.CONST_VALUE)) and not cov[c].any() and not cov[:, c].any()
        assert np.array_equal(cov, cov.T)


# ------------------------------------------------------------------------------------------------ composition
def test_mmd_of_a_small_perturbation():
    """y = x + 1e-3 noise: the MMDs are far below sum|K| / n^2, the unit of the whole-sum tolerance, and inside the composed bound"""
    import smd_amd.metrics as M
    rng = np.random.default_rng(77)
    x = np.clip(0.25 * rng.standard_normal((300, 42)), -1, 1).astype(np.float32)
    y = (x + 1e-3 * rng.standard_normal(x.shape)).astype(np.float32)
    for kw in (dict(gamma_rbf=1.0, degree=2, gamma_poly=1.0, coef0=0.0), dict(gamma_rbf=0.05, degree=3, gamma_poly=0.1, coef0=1.0)):
        kw = {k: (v if k == "degree" else R.f32r(v)) for k, v in kw.items()}
        ref = R.mmd_reference(x, y, **kw)
        got = M.kernel_mmds(x, y, **kw)
        print(f"mmd_rbf {got['mmd_rbf']!r} ref {ref['rbf']!r} in [{ref['rbf_lo']!r}, {ref['rbf_hi']!r}], old unit {R.OLD_PAIR_REL * ref['rbf_unit']:.3g}; "
              f"mmd_polynomial {got['mmd_polynomial']!r} ref {ref['poly']!r} +- {ref['poly_bound']:.3g}, old unit {R.OLD_PAIR_REL * ref['poly_unit']:.3g}")
        assert abs(ref["rbf"]) < 1e-2 * ref["rbf_unit"]
        note("mmd_rbf", "perturbation", R.rbf_ratio(got["mmd_rbf"], ref), str(kw))
        note("mmd_polynomial", "perturbation", R.poly_ratio(got["mmd_polynomial"], ref), str(kw))
        assert ref["rbf_lo"] <= got["mmd_rbf"] <= ref["rbf_hi"] and abs(got["mmd_polynomial"] - ref["poly"]) <= ref["poly_bound"]


def test_zz_print_the_table():
    rows = {}
    for (kernel, regime), r in sorted(WORST.items()):
        rows.setdefault(regime, []).append(f"{kernel} {r:.3f}" if r >= 5e-4 else f"{kernel} {r:.1e}")
    for regime, cells in rows.items():
        print(f"    {regime:14s} {'   '.join(cells)}")
