"""Element-wise criterion for the weight-gradient GEMMs  dW = X^T dY,  db = colsum(dY)  on bf16 operands (no GPU needed).

Reference: float64 of the bf16 operands (``reference``).

Bound, per element (``bounds``), with u = 2^-24 the unit roundoff of fp32:

    bound_W[k, n] = 2 (Mrows + nsplit)           u  (|X|^T |dY|)[k, n]
    bound_b[n]    = 2 (Mrows + nsplit * tiles_k) u  colsum(|dY|)[n]

Derivation.  A product of two bf16 numbers has 16 significant bits: it is exact in fp32, so the only errors are those of the
additions.  Summing t terms in fp32 in ANY order (any tree) with round-to-nearest gives |err| <= gamma_{t-1} sum|term|,
gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  An element of dW is the sum
of Mrows products, cut into nsplit partial sums that the slab reduce adds: at most Mrows + nsplit - 1 additions lie on any
path, and (Mrows + nsplit) u covers gamma for every Mrows below 2^20.  An element of db made by the 256 x 256 kernel is summed
from nsplit * tiles_k partial rows (1 per split for the 128-wide kernel, tiles_k = 1).  The factor 2 covers the matrix core's
internal summation, which is not specified to round to nearest after every addition: a truncating adder loses up to 2 u per
addition.  It is derived, not fitted, and is not to be widened: the fp32 emulation of tests/test_wgrad_ref_host.py stays
below 0.5, so the hardware has room and a lost term has none.  ``check`` asserts |got - ref| <= bound everywhere and returns
the worst ratio.

What the bound can see.  One lost term x y shows where |x y| > bound, about 2 Mrows u * Mrows mean|x y|: every typical term
up to Mrows of about 2000, none at Mrows = 8192 -- there the split / slab / tile faults below are what it is for.

``plant_*``: the faults a split-K / slab-reduce rewrite produces, planted into a correct result.
"""
import numpy as np
import torch

U = 2.0 ** -24
KM = 64            # m rows per K-tile, both kernels (smd_plan::TN128_KM, TN256_KM)
KSTEP = 16         # m rows per MFMA 32x32x16


def bf(x):
    return x.to(torch.bfloat16)


def make_problem(seed, Mrows, Kd, N, ldx=None, ldy=None):
    """(X [Mrows][ldx], dY [Mrows][ldy]) bf16 on the CPU: X ~ N(0, 1), dY ~ 0.1 N(0, 1) + 0.01 in the logical columns; the padding
    columns hold finite garbage (about 5, nothing like the data), never zeros: a kernel that sums the padding in shows."""
    ldx, ldy = ldx or Kd, ldy or N
    g = torch.Generator().manual_seed(seed)
    X = 5.0 + torch.randn(Mrows, ldx, generator=g)
    Y = -5.0 + torch.randn(Mrows, ldy, generator=g)
    X[:, :Kd] = torch.randn(Mrows, Kd, generator=g)
    Y[:, :N] = torch.randn(Mrows, N, generator=g) * 0.1 + 0.01
    return bf(X), bf(Y)


def reference(X, dY):
    """float64 (dW, db, |X|^T |dY|, colsum |dY|) of the logical operands (tensors on any device)"""
    Xd, Yd = X.double(), dY.double()
    return Xd.t() @ Yd, Yd.sum(0), Xd.abs().t() @ Yd.abs(), Yd.abs().sum(0)


def bounds(absW, absb, Mrows, nsplit, tiles_k=1):
    return 2.0 * (Mrows + nsplit) * U * absW, 2.0 * (Mrows + nsplit * tiles_k) * U * absb


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; inf where the bound is not met at an element whose bound is 0, or got is not finite"""
    got, ref, bound = (torch.as_tensor(t).double() for t in (got, ref, bound))
    err = (got.to(ref.device) - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


def check(got_W, got_b, ref, Mrows, nsplit, tiles_k=1, what=""):
    """asserts the element-wise criterion for dW (and db unless got_b is None); returns (worst ratio dW, worst ratio db)"""
    refW, refb, absW, absb = ref
    bW, bb = bounds(absW, absb, Mrows, nsplit, tiles_k)
    rW = worst_ratio(got_W, refW, bW)
    rb = worst_ratio(got_b, refb, bb) if got_b is not None else 0.0
    assert rW <= 1.0, f"{what}: dW leaves the element-wise bound, worst |err| / bound = {rW:.3g}"
    assert rb <= 1.0, f"{what}: db leaves the element-wise bound, worst |err| / bound = {rb:.3g}"
    return rW, rb


def flagged(got_W, got_b, ref, Mrows, nsplit, tiles_k=1):
    try:
        check(got_W, got_b, ref, Mrows, nsplit, tiles_k)
    except AssertionError:
        return True
    return False


def rel(a, b):
    """the whole-matrix criterion of the older tests: relative L2"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def split_ranges(Mrows, nsplit, per):
    """m-row range of every split: `per` K-tiles of 64 rows each, the last split (and its last K-tile) may be short"""
    total_kt = -(-Mrows // KM)
    assert (nsplit - 1) * per < total_kt <= nsplit * per, (Mrows, nsplit, per)
    return [(s * per * KM, min((s + 1) * per * KM, Mrows)) for s in range(nsplit)]


def _partial(Xf, Yf, lo, hi):
    """one workgroup's fp32 accumulators over rows lo .. hi: one MFMA (16 m rows) after the other, K-tiles in order"""
    acc = np.zeros((Xf.shape[1], Yf.shape[1]), np.float32)
    accb = np.zeros(Yf.shape[1], np.float32)
    for m in range(lo, hi, KSTEP):
        e = min(m + KSTEP, hi)
        acc = acc + (Xf[m:e].T @ Yf[m:e]).astype(np.float32)
        accb = accb + Yf[m:e].sum(0, dtype=np.float32)
    return acc, accb


def reduce_slabs(parts):
    """reduce_slabs_kernel (gemm_tn.hip): slice sl = 0..3 adds slabs sl, sl + 8, ... into s0 and sl + 4, sl + 12, ... into s1,
    its sum is s0 + s1, and the four slices are combined as (a0 + a1) + (a2 + a3); all fp32"""
    ns = len(parts)
    zero = np.zeros_like(parts[0])
    a = []
    for sl in range(4):
        s0, s1, s = zero.copy(), zero.copy(), sl
        while s + 4 < ns:
            s0 = s0 + parts[s]
            s1 = s1 + parts[s + 4]
            s += 8
        if s < ns:
            s0 = s0 + parts[s]
        a.append(s0 + s1)
    return (a[0] + a[1]) + (a[2] + a[3])


def emulate_tn128(X, dY, nsplit, per):
    """(dW, db) fp32 as the 128-wide kernel + reduce_slabs_kernel sum them (nsplit == 1: the kernel writes directly)"""
    Xf, Yf = X.float().numpy(), dY.float().numpy()
    parts = [_partial(Xf, Yf, lo, hi) for lo, hi in split_ranges(Xf.shape[0], nsplit, per)]
    if nsplit == 1:
        return torch.from_numpy(parts[0][0]), torch.from_numpy(parts[0][1])
    return torch.from_numpy(reduce_slabs([p[0] for p in parts])), torch.from_numpy(reduce_slabs([p[1] for p in parts]))


# the single 128 x 128 problem of the GPU cases: (Mrows, slab capacity in splits or None = the engine's workspace, tn_split_model,
# the (nsplit, ktiles_per_split) smd_plan::tn128_split answers) -- less than one K-tile, exactly one, a ragged second, a ragged
# last, 32 K-tiles; the cap of 32 splits; a capacity of 3 splits; no capacity at all
SMALL_CASES = [(8, None, 1, (1, 1)), (64, None, 1, (1, 1)), (96, None, 1, (2, 1)), (1000, None, 1, (8, 2)), (2048, None, 1, (8, 4)),
               (2048, None, 0, (32, 1)), (2048, 3, 1, (3, 11)), (2048, 0, 1, (1, 32))]


def small_problem(Mrows):
    return make_problem(1000 + Mrows, Mrows, 128, 128)


# ------------------------------------------------------------------------------------------------ fault planters
def plant_lost_term(W, X, dY, k, n, m=None):
    """one m-term missing from element (k, n); m defaults to the term of median magnitude (a typical one, not the largest)"""
    terms = X[:, k].double() * dY[:, n].double()
    if m is None:
        m = int(terms.abs().argsort()[terms.numel() // 2])
    out = W.clone()
    out[k, n] = (out[k, n].double() - terms[m]).to(W.dtype)
    return out


def plant_lost_ktile(W, X, dY, tk, tn, tile=128):
    """the last (ragged) K-tile's contribution missing from output tile (tk, tn)"""
    Mrows = X.shape[0]
    lo = (Mrows - 1) // KM * KM
    ks, ns = slice(tk * tile, (tk + 1) * tile), slice(tn * tile, (tn + 1) * tile)
    out = W.clone()
    out[ks, ns] = (out[ks, ns].double() - X[lo:, ks].double().t() @ dY[lo:, ns].double()).to(W.dtype)
    return out


def plant_double_partial(W, X, dY, nsplit, per, split, flat4):
    """split `split`'s partial added twice to the float4 at flat index 4 * flat4 of the row-major dW"""
    lo, hi = split_ranges(X.shape[0], nsplit, per)[split]
    out = W.clone().contiguous()
    flat = out.view(-1)
    N = W.shape[1]
    for i in range(4 * flat4, 4 * flat4 + 4):
        k, n = divmod(i, N)
        flat[i] = (flat[i].double() + (X[lo:hi, k].double() * dY[lo:hi, n].double()).sum()).to(W.dtype)
    return out


def plant_swap(W, k, n):
    """elements (k, n) and (k, n + 1) exchanged"""
    out = W.clone()
    out[k, n], out[k, n + 1] = W[k, n + 1], W[k, n]
    return out


def plant_bias_into_neighbour(biases, i):
    """problem i's bias row written into problem i + 1's (as far as both reach)"""
    out = [b.clone() for b in biases]
    n = min(out[i].numel(), out[i + 1].numel())
    out[i + 1][:n] = biases[i][:n]
    return out
