"""The criterion of the pair sums and moments (tests/_gram_sums_ref.py) is right, has room and is sharp: CPU only.

  * the lattice preconditions hold for every shape of the exact tests' tables (integers, every partial sum below 2^24, every
    |t^degree| <= 2^20, rows pairwise distinct unless planted, negative bases at odd degrees, every 32-row moment sum below 2^24,
    grids of 6, 9, 15 and more than 256 tiles), and the fp32 emulation of the kernels gives the exact values on them;
  * the emulation (k-ordered fma chains, 16-value fp32 sub-sums in accumulator order, fp64 centring then fp32 rounding, the
    32-row flush) is inside every derived bound in every regime; the worst |err| / bound is printed per regime;
  * the `clamp` regime really has negative raw fp32 d2, `poly_cancel` really has |t| below its own error (where the first-order
    form of the power's error fails and the exact difference is needed), `saturate` really underflows;
  * every planted fault is caught where CAUGHT says, by an exact test where one applies and by a bound otherwise -- except
    `diagonal-not-zeroed`, which changes no bit: the norms are the Gram's own fma chain, so (-2 g_ii + n_i) + n_i is 0 before it
    is set to 0 (test_the_diagonal_is_zero_before_it_is_zeroed states this; no test of outputs can tell the two kernels apart);
  * which of the faults the whole-sum thresholds of tests/test_gpu_metrics.py (2e-5 sum|K|, 1e-6 in norm) let through, by
    running those assertions on that file's own data against the faulty emulations.
"""
import numpy as np

import _gram_sums_ref as R
import _metrics_ref as MR

# fault -> the named check that catches it (see the functions of the same names in tests/test_gpu_gram_sums.py)
CAUGHT = {"no-clamp": "bound: rbf, clamp regime", "mirror-weight-1": "exact: duplicate count, symmetric",
          "padded-row-counted": "exact: polynomial sum, full", "tile-dropped": "exact: polynomial sum, full",
          "tile-twice": "exact: polynomial sum, full", "neighbour-tile-norms": "exact: duplicate count, full",
          "fp32-mean": "bound: mean and cov, offset regime", "one-pass": "bound: cov, offset regime",
          "slab-fp32": "exact: moments lattice", "n-not-n-1": "exact: moments lattice"}
# what the old thresholds let through (measured by test_what_the_old_thresholds_miss, which asserts this set)
OLD_MISSES = {"no-clamp", "diagonal-not-zeroed", "fp32-mean", "one-pass", "slab-fp32"}


def test_lattice_preconditions_hold_for_every_shape():
    grids = set()
    for d in R.EXACT_D:
        for nx, ny in R.FULL_SHAPES:
            R.dup_full(nx, ny, d)
            grids.add(R.tiles_launched(nx, ny, False))
        for n in R.EXACT_N:
            R.dup_symmetric(n, d)
            grids.add(R.tiles_launched(n, n, True))
    R.dup_full(R.BIG_FULL, R.BIG_FULL, R.BIG_D)
    planted = R.dup_symmetric(R.BIG_SYM, R.BIG_D)[2]
    assert {(i // R.MT == j // R.MT) for i, j in planted} == {True, False}
    assert {6, 9, 15} <= grids and all(g % 8 for g in (6, 9, 15))
    assert R.tiles_launched(R.BIG_FULL, R.BIG_FULL, False) > 256 and R.tiles_launched(R.BIG_SYM, R.BIG_SYM, True) > 256
    shapes = [(nx, ny, d, False) for nx, ny in R.FULL_SHAPES for d in R.EXACT_D] + [(n, n, d, True) for n in R.EXACT_N for d in R.EXACT_D]
    shapes += [(R.BIG_FULL, R.BIG_FULL, R.BIG_D, False), (R.BIG_SYM, R.BIG_SYM, R.BIG_D, True)]
    for nx, ny, d, sym in shapes:
        for c0 in R.POLY_COEF0:
            for deg in R.POLY_DEGREES:
                neg = R.poly_case(nx, ny, d, c0, deg, sym)[3]                 # asserts |t^deg| <= 2^20 and the partial sums
                if deg % 2 and nx >= 127 and d > 1 and c0 <= 0:
                    assert neg, (nx, ny, d, c0, deg)
    for n in R.MOM_EXACT_N:
        for d in R.MOM_EXACT_D:
            if n * d <= 2049 * 129:                                            # the larger ones assert it where the GPU test draws them
                R.moment_rows(n, d)
    assert 32 * 724 ** 2 < 2 ** 24 <= 64 * 512 ** 2
    # the boundaries the moments kernel has: a stage, a flush, a slab, the cap of the splits
    assert [R.mom_split(n) for n in (1024, 1025, 2049, 16385, 20001)] == [(1, 1024), (2, 513), (3, 683), (16, 1025), (16, 1251)]
    x = R.sweep_rows()
    assert R.zero_pairs(x, np.roll(x, 5, 0)) == R.SWEEP_N


def test_emulation_is_exact_on_the_lattices():
    for nx, ny, d in ((129, 257, 17), (257, 257, 5), (1, 1, 1)):
        x, y, want, _ = R.dup_full(nx, ny, d)
        assert R.emu_pair_sums(x, y, False, R.GAMMA_COUNT, 1.0, 0.0, 1)[0] == want
    for n, d in ((257, 16), (129, 1), (513, 33)):
        x, want, _ = R.dup_symmetric(n, d)
        assert R.emu_pair_sums(x, None, True, R.GAMMA_COUNT, 1.0, 0.0, 1)[0] == want
    x = R.sweep_rows()
    for s in (0, 1, 127, 128, 200):
        assert R.emu_pair_sums(x, np.roll(x, s, 0), False, R.GAMMA_COUNT, 1.0, 0.0, 1)[0] == R.SWEEP_N
    for sym in (False, True):
        for c0 in R.POLY_COEF0:
            for deg in R.POLY_DEGREES:
                x, y, want, _ = R.poly_case(257, 129, 33, c0, deg, sym)
                assert R.emu_pair_sums(x, y, sym, 1.0, 1.0, c0, deg)[1] == want, (sym, c0, deg)
    for n, d in ((2, 1), (3, 5), (17, 3), (33, 17), (1025, 17), (2049, 3)):
        x = R.moment_rows(n, d)
        mean, cov = R.emu_moments(x)
        assert not mean.any() and np.array_equal(cov, R.moment_exact(x)) and np.array_equal(cov, cov.T)


def pair_cases():
    for nx, ny, d in R.PAIR_SHAPES:
        for name in (R.PAIR_REGIMES if d != 512 else ("latent", "clamp")):
            for sym in (False, True):
                yield name, nx, ny, d, sym


def test_pair_emulation_is_inside_every_bound():
    worst = {}
    for name, nx, ny, d, sym in pair_cases():
        pr = R.pair_regime(name, nx, ny, d)
        x, y = pr["x"], (None if sym else pr["y"])
        for gr, gp, c0, deg in pr["params"]:
            ref = R.pair_reference(x, y, sym, gr, gp, c0, deg)
            got = R.emu_pair_sums(x, y, sym, gr, gp, c0, deg)
            rr, rp = R.rbf_ratio(got[0], ref), R.poly_ratio(got[1], ref)
            worst[(name, "rbf")] = max(worst.get((name, "rbf"), 0.0), rr)
            worst[(name, "poly")] = max(worst.get((name, "poly"), 0.0), rp)
            assert rr <= 1.0 and rp <= 1.0, (name, nx, ny, d, sym, gr, gp, c0, deg, rr, rp)
            assert ref["first_order_not_larger"]
            if name == "flat":
                # the limits are less than half a pair away from the pair count: one pair too many or too few is outside
                assert max(ref["rbf_hi"] - ref["pairs"], ref["pairs"] - ref["rbf_lo"]) < 0.5 and ref["rbf_lo"] <= got[0] <= ref["rbf_hi"]
    for k in sorted(worst):
        print(f"emulation {k[0]:12s} {k[1]:5s} worst |err| / bound {worst[k]:.3g}")


def test_the_regimes_are_what_they_say():
    for nx, ny, d in R.PAIR_SHAPES:
        pr = R.pair_regime("clamp", nx, ny, d)
        for y in (pr["y"], pr["x"]):
            raw = R.raw_d2_32(pr["x"], y)
            exact = R.pair_reference(pr["x"], y, False, 1.0, 1.0, 0.0, 1)
            share = float((raw < 0).mean())
            print(f"clamp d={d}: {share:.1%} of the raw fp32 d2 are negative (min {raw.min():.3g})")
            assert share > 0.1 and exact["rbf"] > 0
        x64, y64 = pr["x"].astype(np.float64), pr["y"].astype(np.float64)
        true = (x64 * x64).sum(1)[:, None] + (y64 * y64).sum(1)[None, :] - 2 * x64 @ y64.T
        assert true.min() > -1e-9 and true.max() < 1e-4                     # in float64 the distances are tiny and not negative
        if d == 512:
            continue
        sat = R.pair_regime("saturate", nx, ny, d)
        gr = sat["params"][0][0]
        k = R.expf32(np.float32(-gr) * np.maximum(R.raw_d2_32(sat["x"], sat["y"]), np.float32(0)))
        assert (k == 0).mean() > 0.5 or d == 5, d
        pc = R.pair_regime("poly_cancel", nx, ny, d)
        covers = []
        for gr, gp, c0, deg in pc["params"]:
            ref = R.pair_reference(pc["x"], pc["y"], False, gr, gp, c0, deg)
            assert ref["min_abs_t"] < ref["max_dt"]                          # some |t| is below the error of t
            covers.append(ref["first_order_ok"])
        assert not all(covers[:2])              # at degree >= 2 the first-order form is below the exact difference somewhere
        pn = R.pair_regime("poly_neg", nx, ny, d)
        t = pn["x"].astype(np.float64) @ pn["y"].astype(np.float64).T - 1.0
        assert (t < 0).mean() > 0.9


def mom_cases():
    for n, d in R.MOM_SHAPES:
        for name in R.MOM_REGIMES:
            yield name, n, d


def mom_ratios(x, mean, cov):
    rm, rc, dm, bound = R.moments_reference(x)
    return R.worst_ratio(mean, rm, dm), R.worst_ratio(cov, rc, bound)


def test_moments_emulation_is_inside_every_bound():
    worst = {}
    for name, n, d in mom_cases():
        x = R.moments_regime(name, n, d)
        mean, cov = R.emu_moments(x)
        a, b = mom_ratios(x, mean, cov)
        worst[name] = tuple(max(p, q) for p, q in zip(worst.get(name, (0.0, 0.0)), (a, b)))
        assert a <= 1.0 and b <= 1.0, (name, n, d, a, b)
        c = R.CONST_COL
        assert mean[c] == np.float64(np.float32(R.CONST_VALUE)) and not cov[c].any() and not cov[:, c].any()
        assert np.array_equal(cov, cov.T)
    for k, (a, b) in sorted(worst.items()):
        print(f"emulation moments {k:10s} worst |err| / bound: mean {a:.3g}  cov {b:.3g}")


def test_the_diagonal_is_zero_before_it_is_zeroed():
    """the planted fault `diagonal-not-zeroed` changes no bit of the emulation, in any regime: |x_i|^2 is the fma chain of g_ii"""
    for name in ("latent", "clamp", "saturate"):
        pr = R.pair_regime(name, 300, 257, 42)
        gr, gp, c0, deg = pr["params"][0]
        a = R.emu_pair_sums(pr["x"], None, True, gr, gp, c0, deg)
        b = R.emu_pair_sums(pr["x"], None, True, gr, gp, c0, deg, fault="diagonal-not-zeroed")
        assert a.tobytes() == b.tobytes()
        assert not np.diagonal(R.raw_d2_32(pr["x"], pr["x"])).any()


def _planted_tile(planted, off_diagonal=None):
    for i, j in planted:
        if off_diagonal is None or (i // R.MT != j // R.MT) == off_diagonal:
            return i // R.MT, j // R.MT
    raise AssertionError("no such planted pair")


def test_every_pair_fault_is_caught():
    caught = {}
    # exact: duplicate counts
    x, y, want, planted = R.dup_full(257, 257, 17)
    tile = _planted_tile(planted)
    for fault in ("neighbour-tile-norms", "tile-dropped", "tile-twice"):
        got = R.emu_pair_sums(x, y, False, R.GAMMA_COUNT, 1.0, 0.0, 1, fault=fault, tile=tile)[0]
        caught[(fault, "exact: duplicate count, full")] = got != want
    xs, wants, ps = R.dup_symmetric(257, 17)
    tile = _planted_tile(ps, off_diagonal=True)
    for fault in ("mirror-weight-1", "tile-dropped", "tile-twice", "neighbour-tile-norms"):
        got = R.emu_pair_sums(xs, None, True, R.GAMMA_COUNT, 1.0, 0.0, 1, fault=fault, tile=tile)[0]
        caught[(fault, "exact: duplicate count, symmetric")] = got != wants
    # exact: polynomial sums (coef0 = 1, degree 2: every term is positive)
    x, y, want, _ = R.poly_case(129, 257, 17, 1, 2, False)
    for fault in ("padded-row-counted", "tile-dropped", "tile-twice"):
        got = R.emu_pair_sums(x, y, False, 1.0, 1.0, 1.0, 2, fault=fault, tile=(1, 2))[1]
        caught[(fault, "exact: polynomial sum, full")] = got != want
    x, _, want, _ = R.poly_case(257, 257, 17, 1, 2, True)
    got = R.emu_pair_sums(x, None, True, 1.0, 1.0, 1.0, 2, fault="mirror-weight-1")[1]
    caught[("mirror-weight-1", "exact: polynomial sum, symmetric")] = got != want
    # bound: the clamp
    for nx, ny, d in R.PAIR_SHAPES:
        pr = R.pair_regime("clamp", nx, ny, d)
        gr, gp, c0, deg = pr["params"][0]
        for sym in (False, True):
            y = None if sym else pr["y"]
            ref = R.pair_reference(pr["x"], y, sym, gr, gp, c0, deg)
            got = R.emu_pair_sums(pr["x"], y, sym, gr, gp, c0, deg, fault="no-clamp")
            r = R.rbf_ratio(got[0], ref)
            print(f"no-clamp d={d} {'symmetric' if sym else 'full'}: sum {got[0]:.6g} of {ref['pairs']} pairs, limit {ref['rbf_hi']:.6g}, ratio {r:.3g}")
            if d >= 42:                # at d = 5 the chains are too short for the noise of the raw d2 to lift the sum over the pair count
                caught[("no-clamp", "bound: rbf, clamp regime")] = caught.get(("no-clamp", "bound: rbf, clamp regime"), True) and r > 1.0
    # bound: the pad mask in the flat regime (every counted pair adds 1)
    pr = R.pair_regime("flat", 300, 257, 42)
    gr, gp, c0, deg = pr["params"][0]
    ref = R.pair_reference(pr["x"], pr["y"], False, gr, gp, c0, deg)
    got = R.emu_pair_sums(pr["x"], pr["y"], False, gr, gp, c0, deg, fault="padded-row-counted")
    caught[("padded-row-counted", "bound: rbf, flat regime")] = R.rbf_ratio(got[0], ref) > 1.0
    for k, v in sorted(caught.items()):
        print(f"{k[0]:22s} {k[1]:36s} {'caught' if v else 'MISSED'}")
    for fault in R.PAIR_FAULTS:
        if fault == "diagonal-not-zeroed":
            continue
        assert caught[(fault, CAUGHT[fault])], fault
    assert all(caught.values())


def test_every_moments_fault_is_caught():
    caught = {}
    x = R.moment_rows(2049, 17)
    want = R.moment_exact(x)
    for fault in ("slab-fp32", "n-not-n-1"):
        caught[(fault, "exact: moments lattice")] = not np.array_equal(R.emu_moments(x, fault)[1], want)
    for n, d in ((1025, 42), (4097, 42)):
        x = R.moments_regime("offset", n, d)
        for fault in ("fp32-mean", "one-pass", "n-not-n-1"):
            a, b = mom_ratios(x, *R.emu_moments(x, fault))
            print(f"{fault} offset n={n}: mean at {a:.3g}, cov at {b:.3g} of the bound")
            key = (fault, "bound: mean and cov, offset regime" if fault == "fp32-mean" else "bound: cov, offset regime")
            caught[key] = caught.get(key, True) and (b > 1.0 and (a > 1.0 or fault != "fp32-mean"))
    for fault in R.MOM_FAULTS:
        assert caught[(fault, CAUGHT[fault])], fault
    assert all(caught.values()), caught


def test_what_the_old_thresholds_miss():
    """the assertions of tests/test_gpu_metrics.py (test_pair_kernel_sums_match_float64 at (1000, 777, 146), test_padded_rows_are_masked,
    test_moments_match_np_cov at (4097, 146)) on that file's own data, against the faulty emulations"""
    data = lambda n, d, seed, lo=-1.0, hi=1.0: np.random.default_rng(seed).uniform(lo, hi, (n, d)).astype(np.float32)
    nx, ny, d = 1000, 777, 146
    x, y = data(nx, d, 1), data(ny, d, 2, -0.9, 1.0)
    params = ((1.0, 1, 0.0), (1.0 / d, 2, 0.5), (0.1 / d, 3, 1.0))

    def old_pair_ok(fault, tile):
        ok = True
        for sym in (False, True):
            if sym and fault == "padded-row-counted":
                continue
            for gamma, degree, coef0 in params:
                got = R.emu_pair_sums(x, None if sym else y, sym, gamma, 1.0, coef0, degree, fault=fault, tile=tile)
                ref = MR.kernel_sums(x, y, sym, gamma, 1.0, coef0, degree)
                floor = nx * (nx if sym else ny) * R.FLT_MIN
                ok &= abs(got[0] - ref[0]) <= R.OLD_PAIR_REL * ref[1] + floor and abs(got[1] - ref[2]) <= R.OLD_PAIR_REL * ref[3]
        return bool(ok)

    def old_pad_ok(fault):
        a, b = data(129, 5, 3), data(130, 5, 4)
        got = R.emu_pair_sums(a, b, False, 1e-12, 1.0, 1.0, 1, fault=fault)
        ref = MR.kernel_sums(a, b, False, 1e-12, 1.0, 1.0, 1)
        return bool(abs(got[0] - 129 * 130) < 1e-3 and abs(got[1] - ref[2]) <= R.OLD_PAIR_REL * ref[3])

    assert old_pair_ok(None, (0, 0)) and old_pad_ok(None)
    missed = set()
    for fault in R.PAIR_FAULTS:
        ok = old_pair_ok(fault, (1, 2)) and (fault != "padded-row-counted" or old_pad_ok(fault))
        print(f"old thresholds, {fault:22s}: {'MISSED' if ok else 'caught'}")
        if ok:
            missed.add(fault)
    n, dm = 4097, 146
    rng = np.random.default_rng(n)
    xm = (rng.uniform(-1, 1, (n, dm)) * rng.uniform(0.1, 1.0, dm) + rng.uniform(-0.5, 0.5, dm)).astype(np.float32)
    x64 = xm.astype(np.float64)
    rmu, rcov = x64.mean(0), np.cov(x64, rowvar=False)
    for fault in (None,) + R.MOM_FAULTS:
        mu, cov = R.emu_moments(xm, fault)
        ok = bool(np.linalg.norm(mu - rmu) <= R.OLD_MOM_REL * np.linalg.norm(rmu) and np.linalg.norm(cov - rcov) <= R.OLD_MOM_REL * np.linalg.norm(rcov)
                  and np.array_equal(cov, cov.T))
        print(f"old thresholds, {str(fault):22s}: {'MISSED' if ok else 'caught'}  (mean {np.linalg.norm(mu - rmu) / np.linalg.norm(rmu):.2e}, "
              f"cov {np.linalg.norm(cov - rcov) / np.linalg.norm(rcov):.2e})")
        if fault is None:
            assert ok
        elif ok:
            missed.add(fault)
    assert missed == OLD_MISSES, sorted(missed)
