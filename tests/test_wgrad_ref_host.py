"""The element-wise weight-gradient criterion (tests/_wgrad_ref.py) is sharp and has room: CPU only.

  * every planted fault -- a lost m-term, a lost ragged K-tile in one 128 x 128 tile, a split's partial added twice to one
    float4, two neighbouring elements exchanged, a bias row written into the neighbour's -- leaves the bound;
  * on a 2048 x 2048 gradient the older whole-matrix criterion (relative L2 < 3e-5) does not see the lost term.  It DOES see a
    whole lost K-tile: 40 of 1000 rows missing from one of 256 tiles is sqrt(40 / 1000) / 16 = 1.2e-2 of the matrix norm
    (measured 1.3e-2), and no ragged tail is short enough to hide -- one row of 8193 is still 7e-4.  Both figures are
    asserted as they are;
  * an fp32 emulation of the kernels' own summation order, on the inputs of the small GPU cases, stays below half the bound.
"""
import pytest
import torch

import _wgrad_ref as R

OLD_TOL = 3e-5          # tests/test_gpu_kernels.py::test_gemm_tn / test_gemm_tn256


@pytest.fixture(scope="module")
def big():
    """2048 x 2048 gradient over 1000 rows (15 K-tiles + a ragged one of 40 rows), an fp32 result with fp32-sized errors"""
    Mrows = 1000
    X, dY = R.make_problem(7, Mrows, 2048, 2048)
    ref = R.reference(X, dY)
    W = ref[0].float()          # correctly rounded: inside the bound by a wide margin
    b = ref[1].float()
    nsplit, per = 4, 4
    assert R.check(W, b, ref, Mrows, nsplit)[0] < 0.01
    return Mrows, X, dY, ref, W, b, nsplit, per


def test_a_lost_term_is_flagged_and_escapes_the_whole_matrix_criterion(big):
    Mrows, X, dY, ref, W, b, nsplit, per = big
    for k, n in ((0, 0), (777, 1301), (2047, 2046)):
        bad = R.plant_lost_term(W, X, dY, k, n)
        old = R.rel(bad, ref[0])
        bW, _ = R.bounds(ref[2], ref[3], Mrows, nsplit)
        ratio = R.worst_ratio(bad, ref[0], bW)
        print(f"lost term at ({k}, {n}): whole-matrix rel {old:.2e} (< {OLD_TOL:g}: not seen), element-wise |err| / bound {ratio:.1f}")
        assert old < OLD_TOL
        assert R.flagged(bad, b, ref, Mrows, nsplit) and ratio > 1.5


def test_a_lost_ragged_ktile_is_flagged(big):
    Mrows, X, dY, ref, W, b, nsplit, per = big
    bad = R.plant_lost_ktile(W, X, dY, 3, 9)
    old = R.rel(bad, ref[0])
    bW, _ = R.bounds(ref[2], ref[3], Mrows, nsplit)
    ratio = R.worst_ratio(bad, ref[0], bW)
    print(f"lost ragged K-tile (40 rows) in tile (3, 9): whole-matrix rel {old:.2e}, element-wise |err| / bound {ratio:.0f}")
    assert R.flagged(bad, b, ref, Mrows, nsplit) and ratio > 10
    # the whole-matrix criterion sees this one too (module docstring): sqrt(40 / 1000) / 16 of the norm
    assert 0.5e-2 < old < 2.5e-2
    # untouched tiles stay inside the bound: the criterion also says WHERE
    err = (bad.double() - ref[0]).abs() > bW
    assert bool(err[3 * 128:4 * 128, 9 * 128:10 * 128].any()) and int(err.sum()) == int(err[3 * 128:4 * 128, 9 * 128:10 * 128].sum())


def test_a_partial_added_twice_swapped_neighbours_and_a_stray_bias_row_are_flagged(big):
    Mrows, X, dY, ref, W, b, nsplit, per = big
    for split, flat4 in ((0, 0), (3, 2048 * 2048 // 4 - 1), (2, 123457)):       # the last split is the short one (4 + 4 + 4 + 4 > 15.6)
        assert R.flagged(R.plant_double_partial(W, X, dY, nsplit, per, split, flat4), b, ref, Mrows, nsplit)
    for k, n in ((0, 0), (1000, 2046), (2047, 5)):
        assert R.flagged(R.plant_swap(W, k, n), b, ref, Mrows, nsplit)
    # a group of two problems with different dY: the second one's db holds the first one's
    X2, dY2 = R.make_problem(8, Mrows, 128, 146)
    ref2 = R.reference(X2, dY2)
    biases = R.plant_bias_into_neighbour([b, ref2[1].float()], 0)
    assert not R.flagged(W, biases[0], ref, Mrows, nsplit)
    assert not R.flagged(ref2[0].float(), ref2[1].float(), ref2, Mrows, nsplit)
    assert R.flagged(ref2[0].float(), biases[1], ref2, Mrows, nsplit)


@pytest.mark.parametrize("Mrows,cap,model,plan", R.SMALL_CASES)
def test_fp32_emulation_of_the_kernels_summation_stays_below_half_the_bound(Mrows, cap, model, plan):
    nsplit, per = plan
    X, dY = R.small_problem(Mrows)
    ref = R.reference(X, dY)
    W, b = R.emulate_tn128(X, dY, nsplit, per)
    rW, rb = R.check(W, b, ref, Mrows, nsplit)
    print(f"fp32 emulation Mrows={Mrows} nsplit={nsplit} x {per} K-tiles: worst |err| / bound dW {rW:.2e} db {rb:.2e}")
    assert rW < 0.5 and rb < 0.5
    # and the emulation is no stand-in for the reference: a planted fault in it is still found
    assert R.flagged(R.plant_swap(W, 5, 6), b, ref, Mrows, nsplit)
    if nsplit > 1:
        assert R.flagged(R.plant_double_partial(W, X, dY, nsplit, per, nsplit - 1, 77), b, ref, Mrows, nsplit)
