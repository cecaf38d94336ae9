"""Sample-quality distances of the reference's evaluation (utils/metrics.py:24-77, used by sample_ncsn.py:69-186) on the GPU.

``frechet_distance``, ``mmd_rbf`` and ``mmd_polynomial`` keep the reference's signatures and semantics on (n, d) inputs; an
array of more dimensions is read as frames of its last axis (an (N, S, C) latent set is N*S frames of C).  Inputs may be
numpy arrays or torch tensors on any device; they are taken to the GPU as contiguous fp32.  The pairwise sums and the
moments run in csrc/metrics.hip on exact-fp32 MFMA with fp64 accumulation; the N x N kernel matrices sklearn builds are
never formed.  As sklearn's ``X is Y``, passing the SAME object as ``real`` and ``fake`` takes the symmetric path whose
diagonal distances are exactly zero (and the MMD is exactly 0).

The Frechet trace term tr sqrtm(S1 S2) is evaluated on the host in float64 as sum sqrt(max(eig(S1^1/2 S2 S1^1/2), 0)) with
``numpy.linalg.eigh``: equal for covariance matrices, and real on rank-deficient inputs where scipy's sqrtm can go complex.
Only the eigenvalues that a covariance of n <= d rows has to be zero (beyond rank n - 1) are set to zero.

``precision_recall``, ``realism_scores`` and ``f1_score`` are the nearest-neighbour metrics the reference's evaluate() logs as
improved_precision / improved_recall / improved_f1 / ipr_realism (sample_ncsn.py:148-157) and its utils/metrics.py does not
define: Kynkaanniemi et al. 2019 as fixed in DESIGN.md section 14, on csrc/nn_metrics.hip (``knn_radii``, ``ball_cover``).

``precision_recall_distribution``, ``prd_f_beta_score`` and ``ndb_score`` are the remaining four scalars of that evaluate()
(precision / recall / f1 from the PRD histogram of Sajjadi et al. 2018, sample_ncsn.py:141-146; ndb of Richardson & Weiss 2018,
:160) as fixed in DESIGN.md section 15, on the full-batch Lloyd ``kmeans`` of csrc/kmeans.hip (``kmeans_assign``,
``kmeans_update``); the histograms, the PRD curve and the two-proportion test are host float64.

``nn_search``, ``TrainIndex``, ``authenticity`` and ``copy_report`` (``copy_metrics`` for frames and sequences together) ask what
none of the scores above can: which TRAINING row a sample is closest to and whether it is closer than unseen data is -- the
authenticity score of Alaa et al. 2022 and the nearest-training-neighbour distances, as fixed in DESIGN.md section 24, on
csrc/nn_search.hip.  The training set is streamed slab by slab and may stay on the host.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import lib as _lib


def _device(*arrays) -> torch.device:
    for a in arrays:
        if torch.is_tensor(a) and a.is_cuda:
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


def as_frames(a, device=None) -> torch.Tensor:
    """(..., d) numpy array or tensor -> contiguous fp32 (n, d) tensor on ``device`` (1-D input: n frames of 1)."""
    device = _device(a) if device is None else torch.device(device)
    t = torch.from_numpy(np.asarray(a)) if not torch.is_tensor(a) else a
    t = t.to(device=device, dtype=torch.float32)
    t = t.reshape(-1, 1) if t.dim() == 1 else t.reshape(-1, t.shape[-1])
    return t.contiguous()


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _rows(t: torch.Tensor) -> torch.Tensor:
    """The kernels take rows of unit-strided columns, at least d apart: any other layout (t[:, ::2], an expanded tensor) is
    copied to a contiguous one."""
    ok = (t.shape[1] <= 1 or t.stride(1) == 1) and t.stride(0) >= t.shape[1]
    return t if ok else t.contiguous()


def _workspace(nbytes: int, device):
    """(scratch tensor, nbytes) for one library call.  A size the library refuses (negative) still gets a buffer: the call
    itself then reports what is wrong with the arguments."""
    return torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device), nbytes


def _degree(degree) -> int:
    if int(degree) != degree:
        raise ValueError(f"degree={degree!r}: the polynomial kernel takes an integer degree")
    return int(degree)


def pair_kernel_sums(x: torch.Tensor, y: Optional[torch.Tensor] = None, gamma_rbf: float = 1.0, gamma_poly: float = 1.0,
                     coef0: float = 0.0, degree: int = 2) -> torch.Tensor:
    """Device fp64 tensor [sum_ij exp(-gamma_rbf |x_i - y_j|^2), sum_ij (gamma_poly <x_i, y_j> + coef0)^degree] over all
    pairs of the fp32 (n, d) cuda tensors ``x`` and ``y``; ``y=None`` is Y = X with a zero diagonal (symmetric mode).
    Enqueued on the current stream, nothing waits."""
    L = _lib.get_lib()
    sym = y is None
    if x.dim() != 2 or (not sym and y.dim() != 2):
        raise ValueError("pair_kernel_sums takes (n, d) tensors")
    if x.dtype != torch.float32 or not x.is_cuda or (not sym and (y.dtype != torch.float32 or y.device != x.device)):
        raise ValueError("pair_kernel_sums takes fp32 cuda tensors on one device")
    x = _rows(x)
    y = None if sym else _rows(y)
    nx, d = x.shape
    ny, dy = (nx, d) if sym else y.shape
    if dy != d:
        raise ValueError(f"pair_kernel_sums: d mismatch ({d} vs {dy})")
    ws, ws_bytes = _workspace(L.smd_pair_kernel_sums_workspace_bytes(nx, ny, int(sym)), x.device)
    out = torch.empty(2, dtype=torch.float64, device=x.device)
    _lib.check(L.smd_pair_kernel_sums(x.data_ptr(), x.stride(0), nx, None if sym else y.data_ptr(), x.stride(0) if sym else y.stride(0),
                                      ny, d, int(sym), float(gamma_rbf), float(gamma_poly), float(coef0), _degree(degree),
                                      ws.data_ptr(), ws_bytes, out.data_ptr(), _stream(x.device)), "smd_pair_kernel_sums")
    return out


def _check_rows(name: str, *ts: torch.Tensor) -> None:
    for t in ts:
        if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.device != ts[0].device:
            raise ValueError(f"{name} takes fp32 (n, d) cuda tensors on one device")


def knn_radii(x: torch.Tensor, k: int = 3) -> torch.Tensor:
    """Device fp32 tensor r2[n]: the squared distance from each row of the fp32 (n, d) cuda tensor ``x`` to its k-th nearest
    OTHER row (self excluded by index: a duplicated row gives 0).  1 <= k <= 8 and n >= k + 1.  Enqueued on the current
    stream, nothing waits; two calls give the same bits."""
    L = _lib.get_lib()
    _check_rows("knn_radii", x)
    if int(k) != k:
        raise ValueError(f"k={k!r}: knn_radii takes an integer k")
    x = _rows(x)
    n, d = x.shape
    ws, ws_bytes = _workspace(L.smd_knn_radii_workspace_bytes(n, int(k)), x.device)
    r2 = torch.empty(n, dtype=torch.float32, device=x.device)
    _lib.check(L.smd_knn_radii(x.data_ptr(), x.stride(0), n, d, int(k), ws.data_ptr(), ws_bytes, r2.data_ptr(), _stream(x.device)),
               "smd_knn_radii")
    return r2


def ball_cover(q: torch.Tensor, x: torch.Tensor, r2: torch.Tensor, keep: Optional[torch.Tensor] = None,
               exclude_diagonal: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """One pass over the pairs of the queries ``q`` (nq, d) and the centres ``x`` (nx, d) with squared radii ``r2`` (nx):
    (covered, realism2) = (uint8[nq]: some centre j has |q - x_j|^2 <= r2[j];  fp32[nq]: max over the centres with ``keep[j]``
    (None: all) of r2[j] / max(|q - x_j|^2, FLT_MIN)).  ``exclude_diagonal`` (q is x): pair (i, i) takes no part."""
    L = _lib.get_lib()
    _check_rows("ball_cover", q, x)
    q, x = _rows(q), _rows(x)
    nq, d = q.shape
    nx, dx = x.shape
    if dx != d:
        raise ValueError(f"ball_cover: d mismatch ({d} vs {dx})")
    if r2.shape != (nx,) or r2.dtype != torch.float32 or r2.device != x.device:
        raise ValueError(f"ball_cover: r2 must be an fp32 tensor of {nx} squared radii on the centres' device")
    r2 = r2.contiguous()
    if keep is not None:
        if keep.shape != (nx,) or keep.device != x.device:
            raise ValueError(f"ball_cover: keep must be a mask of {nx} centres on their device")
        keep = (keep != 0).to(torch.uint8).contiguous()
    ws, ws_bytes = _workspace(L.smd_ball_cover_workspace_bytes(nq, nx), x.device)
    covered = torch.empty(nq, dtype=torch.uint8, device=x.device)
    realism2 = torch.empty(nq, dtype=torch.float32, device=x.device)
    _lib.check(L.smd_ball_cover(q.data_ptr(), q.stride(0), nq, x.data_ptr(), x.stride(0), nx, d, r2.data_ptr(),
                                None if keep is None else keep.data_ptr(), int(bool(exclude_diagonal)), ws.data_ptr(), ws_bytes,
                                covered.data_ptr(), realism2.data_ptr(), _stream(x.device)), "smd_ball_cover")
    return covered, realism2


def median_keep_mask(r2: torch.Tensor) -> torch.Tensor:
    """The paper's pruning of the largest spheres for the realism score: uint8 mask of the rows whose radius sqrt(r2) is at
    most ``numpy.median`` of the radii (the mean of the two middle ones for an even count)."""
    r = np.sqrt(r2.cpu().numpy().astype(np.float64))
    return torch.from_numpy((r <= np.median(r)).astype(np.uint8)).to(r2.device)


KMEANS_MAX_K = 128        # SMD_KMEANS_MAX_K of include/smd_hip.h: the centres are one tile of the Gram pass


def _check_k(name: str, k) -> int:
    if int(k) != k or not 1 <= int(k) <= KMEANS_MAX_K:
        raise ValueError(f"{name}: k={k!r} must be an integer in [1, {KMEANS_MAX_K}]")
    return int(k)


def _check_centres(name: str, x: torch.Tensor, centres: torch.Tensor) -> torch.Tensor:
    _check_rows(name, x, centres)
    _check_k(name, centres.shape[0])
    if centres.shape[1] != x.shape[1]:
        raise ValueError(f"{name}: d mismatch ({x.shape[1]} vs {centres.shape[1]})")
    return centres.contiguous()


def _kmeans_assign(x: torch.Tensor, centres: torch.Tensor, prev_labels: Optional[torch.Tensor]):
    """kmeans_assign with (inertia, changed) as they are written: int64[2] on the device, [inertia's fp64 bits, changed]"""
    L = _lib.get_lib()
    centres = _check_centres("kmeans_assign", x, centres)
    x = _rows(x)
    n, d = x.shape
    k = centres.shape[0]
    if prev_labels is not None and (prev_labels.shape != (n,) or prev_labels.dtype != torch.int32 or prev_labels.device != x.device
                                    or not prev_labels.is_contiguous()):
        raise ValueError(f"kmeans_assign: prev_labels must be a contiguous int32 tensor of {n} labels on the rows' device")
    labels = torch.empty(n, dtype=torch.int32, device=x.device) if prev_labels is None else prev_labels
    ws, ws_bytes = _workspace(L.smd_kmeans_assign_workspace_bytes(n, k), x.device)
    min_d2 = torch.empty(n, dtype=torch.float32, device=x.device)
    out = torch.empty(2, dtype=torch.int64, device=x.device)          # [inertia as fp64 bits, changed]
    _lib.check(L.smd_kmeans_assign(x.data_ptr(), x.stride(0), n, d, centres.data_ptr(), k, int(prev_labels is not None), ws.data_ptr(),
                                   ws_bytes, labels.data_ptr(), min_d2.data_ptr(), out.data_ptr(), out.data_ptr() + 8,
                                   _stream(x.device)), "smd_kmeans_assign")
    return labels, min_d2, out


def kmeans_assign(x: torch.Tensor, centres: torch.Tensor, prev_labels: Optional[torch.Tensor] = None):
    """One Gram pass of the fp32 (n, d) cuda rows ``x`` against the (k, d) ``centres``, k <= 128: (labels int32[n]: arg min_j
    -2 <x_i, c_j> + |c_j|^2, ties to the lowest j;  min_d2 fp32[n]: the squared distance to that centre;  inertia: their fp64
    sum;  changed int64: how many labels differ from ``prev_labels``, or n without them), the last two 0-dim device tensors that
    share one 16-byte buffer.  ``prev_labels`` (int32[n], contiguous) is OVERWRITTEN and returned as ``labels``.  Enqueued on the
    current stream, nothing waits; two calls give the same bits."""
    labels, min_d2, out = _kmeans_assign(x, centres, prev_labels)
    return labels, min_d2, out[:1].view(torch.float64)[0], out[1]


def kmeans_update(x: torch.Tensor, labels: torch.Tensor, centres: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(new centres fp32 (k, d), counts int64[k]): the mean of the rows of ``x`` with each label, summed in fp64 in a fixed order;
    a cluster without rows keeps its row of ``centres`` bit for bit.  Enqueued on the current stream, nothing waits; two calls
    give the same bits."""
    L = _lib.get_lib()
    centres = _check_centres("kmeans_update", x, centres)
    x = _rows(x)
    n, d = x.shape
    k = centres.shape[0]
    if labels.shape != (n,) or labels.dtype != torch.int32 or labels.device != x.device:
        raise ValueError(f"kmeans_update: labels must be an int32 tensor of {n} labels on the rows' device")
    labels = labels.contiguous()
    ws, ws_bytes = _workspace(L.smd_kmeans_update_workspace_bytes(n, d, k), x.device)
    new = torch.empty_like(centres)
    counts = torch.empty(k, dtype=torch.int64, device=x.device)
    _lib.check(L.smd_kmeans_update(x.data_ptr(), x.stride(0), n, d, labels.data_ptr(), centres.data_ptr(), k, ws.data_ptr(), ws_bytes,
                                   new.data_ptr(), counts.data_ptr(), _stream(x.device)), "smd_kmeans_update")
    return new, counts


def _seed_words(seed, init: int) -> List[int]:
    return [int(v) for v in np.atleast_1d(seed).ravel()] + [int(init)]


def kmeans_seeds(x: torch.Tensor, k: int, u: np.ndarray) -> torch.Tensor:
    """k-means++ row indices (int64[k], device) from the uniforms ``u`` (k of them in [0, 1)): the first is row floor(u_0 n);
    centre j is the row at the inverse CDF of the float64 cumulative D^2 at u_j * total, D^2 the running minimum of min_d2 from
    a k = 1 assign against the newest centre (a chosen row has D^2 = 0 exactly and is never drawn again); a total of 0 (fewer
    distinct rows than k) takes the lowest-index row not yet chosen.  Nothing waits."""
    n = x.shape[0]
    idx = torch.empty(k, dtype=torch.int64, device=x.device)
    idx[0] = min(int(u[0] * n), n - 1)
    chosen = torch.zeros(n, dtype=torch.bool, device=x.device)
    d2 = None
    for j in range(1, k):
        chosen.index_fill_(0, idx[j - 1:j], True)
        m = _kmeans_assign(x, x.index_select(0, idx[j - 1:j]), None)[1]
        d2 = m if d2 is None else torch.minimum(d2, m)
        cum = torch.cumsum(d2.double(), 0)
        drawn = torch.searchsorted(cum, (cum[-1] * float(u[j])).reshape(1), right=True).clamp_(max=n - 1)[0]
        free = torch.searchsorted(torch.cumsum((~chosen).to(torch.int64), 0), torch.ones(1, dtype=torch.int64, device=x.device))[0]
        idx[j] = torch.where(cum[-1] > 0, drawn, free)
    return idx


def kmeans(x: torch.Tensor, k: int, seed=0, n_init: int = 1, max_iter: int = 100, trace: Optional[list] = None):
    """Full-batch Lloyd k-means of the fp32 (n, d) cuda rows ``x``: (centres fp32 (k, d), labels int32[n], inertia float, n_iter).
    Run ``init`` of ``n_init`` seeds with k-means++ (``kmeans_seeds``) from numpy.random.default_rng([*seed, init]).random(k), then
    alternates ``kmeans_assign`` and ``kmeans_update`` until an assignment changes no label (n_iter = the updates done) or
    ``max_iter`` updates, after which one more assignment makes the labels those of the returned centres.  The run of the lowest
    inertia wins, ties to the lowest ``init``.  An empty cluster keeps its centre.  The host waits for one scalar pair per
    iteration.  ``trace`` (a list): receives one dict per assignment -- init, centres, labels (a copy), inertia, changed -- and
    the seeds of every run as {"init", "seeds"}; for the tests."""
    _check_rows("kmeans", x)
    k = _check_k("kmeans", k)
    n = x.shape[0]
    if n < k:
        raise ValueError(f"kmeans: n={n} rows cannot seed k={k} clusters")
    if n_init < 1 or max_iter < 1:
        raise ValueError(f"kmeans: n_init={n_init} and max_iter={max_iter} must be >= 1")
    x = _rows(x)
    best = None
    for init in range(int(n_init)):
        seeds = kmeans_seeds(x, k, np.random.default_rng(_seed_words(seed, init)).random(k))
        if trace is not None:
            trace.append({"init": init, "seeds": seeds.cpu().numpy()})
        centres = x[seeds].contiguous()
        labels, n_iter = None, 0
        while True:
            labels, _, out = _kmeans_assign(x, centres, labels)
            out = out.cpu()                                     # the one wait of an iteration
            inertia, changed = float(out[:1].view(torch.float64)[0]), int(out[1])
            if trace is not None:
                trace.append({"init": init, "centres": centres, "labels": labels.clone(), "inertia": inertia, "changed": changed})
            if changed == 0 or n_iter == max_iter:
                break
            centres = kmeans_update(x, labels, centres)[0]
            n_iter += 1
        if best is None or inertia < best[2]:
            best = (centres, labels, inertia, n_iter)
    return best


def moments(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """np.mean(x, axis=0), np.cov(x, rowvar=False) (ddof = 1) of an fp32 (n, d) cuda tensor as fp64 device tensors."""
    L = _lib.get_lib()
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("moments takes an fp32 (n, d) cuda tensor")
    x = _rows(x)
    n, d = x.shape
    ws, ws_bytes = _workspace(L.smd_moments_workspace_bytes(n, d), x.device)
    mean = torch.empty(d, dtype=torch.float64, device=x.device)
    cov = torch.empty(d, d, dtype=torch.float64, device=x.device)
    _lib.check(L.smd_moments(x.data_ptr(), x.stride(0), n, d, ws.data_ptr(), ws_bytes, mean.data_ptr(), cov.data_ptr(),
                             _stream(x.device)), "smd_moments")
    return mean, cov


def cov_rank(n: int, d: int) -> int:
    """The largest rank a ddof = 1 covariance of n rows in d dimensions can have: min(n - 1, d)."""
    return max(min(n - 1, d), 0)


def _keep_top(w: np.ndarray, rank: Optional[int]) -> np.ndarray:
    """Ascending eigenvalues with negative round-off set to 0 and, given ``rank``, all but the ``rank`` largest set to 0.
    A covariance of n <= d rows is exactly singular: the d - rank smallest eigenvalues are zero in exact arithmetic and only
    round-off in a computed one, which the square root would lift to ~sqrt(round-off) each.  Nothing else is clipped, so a
    full-rank covariance keeps every eigenvalue however small."""
    w = np.clip(w, 0.0, None)
    if rank is not None and rank < len(w):
        w[:len(w) - rank] = 0.0
    return w


def sqrt_psd(s: np.ndarray, rank: Optional[int] = None) -> np.ndarray:
    """S^1/2 of a symmetric positive semi-definite float64 matrix of at most ``rank`` (None: d)."""
    s = np.asarray(s, np.float64)
    w, v = np.linalg.eigh((s + s.T) / 2)
    return (v * np.sqrt(_keep_top(w, rank))) @ v.T


def trace_sqrt_product(s1: np.ndarray, s2: np.ndarray, s1_sqrt: Optional[np.ndarray] = None,
                       rank1: Optional[int] = None, rank2: Optional[int] = None) -> float:
    """tr sqrtm(S1 S2) for symmetric positive semi-definite S1, S2 (float64): S1 S2 is similar to S1^1/2 S2 S1^1/2, whose
    eigenvalues are real and >= 0, so the trace is the sum of their square roots.  ``rank1`` / ``rank2``: the ranks the
    covariances have in exact arithmetic (cov_rank; None: full), which bound the rank of S1^1/2 S2 S1^1/2 by their minimum.
    ``s1_sqrt``: sqrt_psd(S1, rank1) when the caller has it already."""
    r = sqrt_psd(s1, rank1) if s1_sqrt is None else s1_sqrt
    m = r @ np.asarray(s2, np.float64) @ r
    ranks = [k for k in (rank1, rank2) if k is not None]
    ev = _keep_top(np.linalg.eigvalsh((m + m.T) / 2), min(ranks) if ranks else None)
    return float(np.sqrt(ev).sum())


def frechet_from_moments(mu1, s1, mu2, s2, s1_sqrt=None, rank1=None, rank2=None) -> float:
    """utils/metrics.py:49-53: |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2), in float64."""
    diff = np.asarray(mu1, np.float64) - np.asarray(mu2, np.float64)
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * trace_sqrt_product(s1, s2, s1_sqrt, rank1, rank2))


class ReferenceSet:
    """One side of every comparison (the eval set of evaluate()), taken to the GPU once: its frames, moments and K(X, X) sums
    are computed on first use and reused by every ``frechet_distance`` / ``kernel_mmds`` call that is given this object."""

    def __init__(self, data, device=None):
        self.source = data
        self.frames = as_frames(data, device)
        self._moments = None
        self._sqrt = None
        self._kxx: Dict[tuple, np.ndarray] = {}
        self._radii: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._bins: Dict[tuple, Tuple[torch.Tensor, np.ndarray]] = {}

    def moments(self) -> Tuple[np.ndarray, np.ndarray]:
        if self._moments is None:
            mu, cov = moments(self.frames)
            self._moments = (mu.cpu().numpy(), cov.cpu().numpy())
        return self._moments

    def cov_sqrt(self) -> np.ndarray:
        if self._sqrt is None:
            self._sqrt = sqrt_psd(self.moments()[1], self.rank())
        return self._sqrt

    def rank(self) -> int:
        return cov_rank(*self.frames.shape)

    def kxx(self, key: tuple) -> np.ndarray:
        if key not in self._kxx:
            self._kxx[key] = pair_kernel_sums(self.frames, None, *key).cpu().numpy()
        return self._kxx[key]

    def radii(self, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(r2, keep): the squared k-NN radii of the frames and the mask of those at most the median radius"""
        if k not in self._radii:
            r2 = knn_radii(self.frames, k)
            self._radii[k] = (r2, median_keep_mask(r2))
        return self._radii[k]

    def ndb_bins(self, k: int, seed=0) -> Tuple[torch.Tensor, np.ndarray]:
        """(centres, p_r): the NDB bins of the frames -- kmeans(frames, k, seed, n_init=3) -- and the share of the frames in each"""
        key = (int(k), tuple(_seed_words(seed, 0)[:-1]))
        if key not in self._bins:
            centres, labels, _, _ = kmeans(self.frames, k, seed, n_init=3)
            self._bins[key] = (centres, label_histogram(labels, k))
        return self._bins[key]

    def is_same(self, other) -> bool:
        return other is self or other is self.source


def _ref(real, device=None) -> ReferenceSet:
    return real if isinstance(real, ReferenceSet) else ReferenceSet(real, device)


def frechet_distance(real, fake) -> float:
    """utils/metrics.py:24-54 (lower is better).  ``real`` may be a ReferenceSet."""
    ref = _ref(real, _device(real, fake))
    mu1, s1 = ref.moments()
    if ref.is_same(fake):
        mu2, s2, rank2 = mu1, s1, ref.rank()
    else:
        y = as_frames(fake, ref.frames.device)
        mu, cov = moments(y)
        mu2, s2, rank2 = mu.cpu().numpy(), cov.cpu().numpy(), cov_rank(*y.shape)
    return frechet_from_moments(mu1, s1, mu2, s2, ref.cov_sqrt(), ref.rank(), rank2)


def kernel_mmds(real, fake, gamma_rbf: float = 1.0, degree: int = 2, gamma_poly: float = 1, coef0: float = 0) -> Dict[str, float]:
    """Both kernel distances of utils/metrics.py:57-77 from one pass over each pair of sets: mean K(X,X) + mean K(Y,Y)
    - 2 mean K(X,Y) for the RBF and the polynomial kernel (sklearn's biased estimator, diagonal included).  ``real`` may be
    a ReferenceSet, whose K(X, X) sums are then computed once for all calls.  gamma None: 1 / d (sklearn's default)."""
    ref = _ref(real, _device(real, fake))
    x = ref.frames
    d = x.shape[1]
    key = (1.0 / d if gamma_rbf is None else float(gamma_rbf), 1.0 / d if gamma_poly is None else float(gamma_poly),
           float(coef0), _degree(degree))
    kxx = ref.kxx(key)
    nx = x.shape[0]
    if ref.is_same(fake):
        kyy = kxy = kxx
        ny = nx
    else:
        y = as_frames(fake, x.device)
        if y.shape[1] != d:
            raise ValueError(f"kernel_mmds: d mismatch ({d} vs {y.shape[1]})")
        ny = y.shape[0]
        kyy_t = pair_kernel_sums(y, None, *key)
        kxy_t = pair_kernel_sums(x, y, *key)
        kyy, kxy = kyy_t.cpu().numpy(), kxy_t.cpu().numpy()
    mmd = kxx / (nx * nx) + kyy / (ny * ny) - 2.0 * (kxy / (nx * ny))
    return {"mmd_rbf": float(mmd[0]), "mmd_polynomial": float(mmd[1])}


def mmd_rbf(real, fake, gamma: float = 1.0) -> float:
    """utils/metrics.py:57-65 (lower is better)."""
    return kernel_mmds(real, fake, gamma_rbf=gamma)["mmd_rbf"]


def mmd_polynomial(real, fake, degree: int = 2, gamma: float = 1, coef0: float = 0) -> float:
    """utils/metrics.py:68-77 (lower is better)."""
    return kernel_mmds(real, fake, degree=degree, gamma_poly=gamma, coef0=coef0)["mmd_polynomial"]


def f1_score(p: float, r: float) -> float:
    """2 p r / (p + r), and 0 when p + r = 0."""
    return 2.0 * p * r / (p + r) if p + r > 0 else 0.0


def _against_real_balls(ref: ReferenceSet, fake, k: int):
    """(covered, realism2, fake frames or None when ``fake`` is the reference set itself): the fake rows against the real rows'
    k-NN balls, coverage and realism from one pass"""
    x = ref.frames
    r2x, keep = ref.radii(k)
    if ref.is_same(fake):
        return ball_cover(x, x, r2x, keep, exclude_diagonal=True) + (None,)
    y = as_frames(fake, x.device)
    if y.shape[1] != x.shape[1]:
        raise ValueError(f"nearest-neighbour metrics: d mismatch ({x.shape[1]} vs {y.shape[1]})")
    return ball_cover(y, x, r2x, keep) + (y,)


def _recall(ref: ReferenceSet, y: Optional[torch.Tensor], cov: torch.Tensor, k: int) -> float:
    if y is None:                       # the reference set against itself: recall is precision
        return float(cov.double().mean())
    return float(ball_cover(ref.frames, y, knn_radii(y, k))[0].double().mean())


def improved_metrics(real, fake, k: int = 3) -> Dict[str, float]:
    """improved_precision, improved_recall, improved_f1 and ipr_realism (the mean realism score) of one comparison (DESIGN.md
    section 14) from three passes: the fake set's radii, fake against the real balls (precision and realism together) and real
    against the fake balls (recall).  ``real`` may be a ReferenceSet, whose radii and median mask are then computed once for all
    calls.  When ``fake`` is the reference set itself, pair (i, i) is excluded: the leave-one-out scores of the real data."""
    ref = _ref(real, _device(real, fake))
    cov, real2, y = _against_real_balls(ref, fake, int(k))
    p, r = float(cov.double().mean()), _recall(ref, y, cov, int(k))
    return {"improved_precision": p, "improved_recall": r, "improved_f1": f1_score(p, r),
            "ipr_realism": float(np.sqrt(real2.cpu().numpy().astype(np.float64)).mean())}


def precision_recall(real, fake, k: int = 3) -> Tuple[float, float]:
    """(improved_precision, improved_recall): the share of fake rows inside some real row's k-NN ball, and of real rows inside
    some fake row's (the reference's sample_ncsn.py:148; higher is better)."""
    ref = _ref(real, _device(real, fake))
    cov, _, y = _against_real_balls(ref, fake, int(k))
    return float(cov.double().mean()), _recall(ref, y, cov, int(k))


def realism_scores(real, fake, k: int = 3) -> np.ndarray:
    """Per fake row (float64): max over the real rows of at most the median radius of r_k(x_j) / |q - x_j| (the reference's
    sample_ncsn.py:153 logs the mean as ipr_realism; higher is better)."""
    ref = _ref(real, _device(real, fake))
    return np.sqrt(_against_real_balls(ref, fake, int(k))[1].cpu().numpy().astype(np.float64))


def label_histogram(labels: torch.Tensor, k: int) -> np.ndarray:
    """float64[k]: the share of the labels in each of k bins"""
    return np.bincount(labels.cpu().numpy(), minlength=k).astype(np.float64) / labels.numel()


def prd_curve(ref_hist, eval_hist, num_angles: int = 1001, epsilon: float = 1e-10) -> Tuple[np.ndarray, np.ndarray]:
    """Sajjadi et al. 2018, algorithm 1, in float64: for slopes = tan(linspace(epsilon, pi/2 - epsilon, num_angles)),
    precision = sum_b min(ref_b slope, eval_b) and recall = precision / slope, both clipped to [0, 1]."""
    if not 0 < epsilon < 0.1 or not 3 <= num_angles <= 1e6:
        raise ValueError(f"prd_curve: epsilon={epsilon} must be in (0, 0.1) and num_angles={num_angles} in [3, 1e6]")
    ref, ev = np.asarray(ref_hist, np.float64), np.asarray(eval_hist, np.float64)
    slopes = np.tan(np.linspace(epsilon, np.pi / 2 - epsilon, num=num_angles))
    precision = np.minimum(ref[None, :] * slopes[:, None], ev[None, :]).sum(axis=1)
    recall = precision / slopes
    return np.clip(precision, 0.0, 1.0), np.clip(recall, 0.0, 1.0)


def precision_recall_distribution(real, samples, num_clusters: int = 20, num_angles: int = 1001, num_runs: int = 10,
                                  seed=0) -> Tuple[np.ndarray, np.ndarray]:
    """The PRD curve (precision[num_angles], recall[num_angles]) of ``samples`` with respect to ``real`` (which may be a
    ReferenceSet): the mean over ``num_runs`` runs of ``prd_curve`` on the two label histograms of
    kmeans(real frames followed by sample frames, num_clusters, seed=[seed, run])."""
    ref = _ref(real, _device(real, samples))
    x = ref.frames
    y = x if ref.is_same(samples) else as_frames(samples, x.device)
    if y.shape[1] != x.shape[1]:
        raise ValueError(f"precision_recall_distribution: d mismatch ({x.shape[1]} vs {y.shape[1]})")
    k = _check_k("precision_recall_distribution", num_clusters)
    if num_runs < 1:
        raise ValueError(f"precision_recall_distribution: num_runs={num_runs} must be >= 1")
    union = torch.cat((x, y))
    precision, recall = np.zeros(num_angles), np.zeros(num_angles)
    for run in range(int(num_runs)):
        labels = kmeans(union, k, _seed_words(seed, run))[1]
        p, r = prd_curve(label_histogram(labels[:x.shape[0]], k), label_histogram(labels[x.shape[0]:], k), num_angles)
        precision += p
        recall += r
    return precision / num_runs, recall / num_runs


def prd_f_beta_score(prd, beta: float = 8, epsilon: float = 1e-10) -> Tuple[float, float]:
    """(max F_beta, max F_1/beta) over the curve ``prd`` = (precision, recall), F_b = (1 + b^2) p r / (b^2 p + r + epsilon).  The
    reference unpacks the pair as (recall, precision) (sample_ncsn.py:142): F_8 weighs recall, F_1/8 precision."""
    if not beta > 0:
        raise ValueError(f"prd_f_beta_score: beta={beta} must be positive")
    p, r = (np.asarray(v, np.float64) for v in prd)
    f = lambda b: float(((1 + b * b) * p * r / (b * b * p + r + epsilon)).max())
    return f(float(beta)), f(1.0 / float(beta))


Z_TWO_SIDED_05 = 1.959963984540054       # the standard normal's 0.975 quantile


def ndb_from_proportions(p_r, p_s, n_r: int, n_s: int, z_threshold: float = Z_TWO_SIDED_05) -> float:
    """Richardson & Weiss 2018 in float64: the share of the bins whose proportions differ by the pooled two-proportion z-test,
    P = (n_r p_r + n_s p_s) / (n_r + n_s), SE = sqrt(P (1 - P) (1 / n_r + 1 / n_s)), different when SE > 0 and
    |p_r - p_s| / SE > z_threshold."""
    p_r, p_s = np.asarray(p_r, np.float64), np.asarray(p_s, np.float64)
    pooled = (n_r * p_r + n_s * p_s) / (n_r + n_s)
    se = np.sqrt(pooled * (1.0 - pooled) * (1.0 / n_r + 1.0 / n_s))
    z = np.abs(p_r - p_s) / np.where(se > 0, se, 1.0)
    return float(((se > 0) & (z > z_threshold)).sum()) / len(p_r)


def ndb_score(real, samples, k: int = 50, seed=0) -> float:
    """The number of statistically different bins over k (lower is better; no whitening, the paper's default): the bins are
    kmeans(real frames, k, seed, n_init=3) -- cached on a ReferenceSet -- p_r the share of the real frames in each and p_s that
    of the sample frames from one ``kmeans_assign``.  Frames of one sequence are not independent draws: a score, not a test."""
    ref = _ref(real, _device(real, samples))
    k = _check_k("ndb_score", k)
    centres, p_r = ref.ndb_bins(k, seed)
    y = ref.frames if ref.is_same(samples) else as_frames(samples, ref.frames.device)
    if y.shape[1] != centres.shape[1]:
        raise ValueError(f"ndb_score: d mismatch ({centres.shape[1]} vs {y.shape[1]})")
    p_s = label_histogram(kmeans_assign(y, centres)[0], k)
    return ndb_from_proportions(p_r, p_s, ref.frames.shape[0], y.shape[0])


def cluster_metrics(real, samples, prd_clusters: int = 20, prd_runs: int = 10, ndb_bins: int = 50, seed=0) -> Dict[str, float]:
    """precision, recall, f1 and ndb of one comparison as the reference's evaluate() names them (sample_ncsn.py:141-146,160;
    DESIGN.md section 15).  ``real`` may be a ReferenceSet, whose NDB bins are then computed once for all calls."""
    ref = _ref(real, _device(real, samples))
    prd = precision_recall_distribution(ref, samples, num_clusters=prd_clusters, num_runs=prd_runs, seed=seed)
    recall, precision = prd_f_beta_score(prd, beta=8)
    return {"precision": precision, "recall": recall, "f1": f1_score(precision, recall),
            "ndb": ndb_score(ref, samples, k=ndb_bins, seed=seed)}


# ---------------------------------------------------------------------------------------------------- copying
KNN_MAX_K = 8             # SMD_KNN_MAX_K of include/smd_hip.h
COPY_METRICS_VERSION = "copy-metrics-1 (DESIGN.md section 24: authenticity d2 >= r1_sq[i*], ties to the lower index, medians of distances)"


def nn_search(q: torch.Tensor, x: torch.Tensor, k: int = 1, *, q_base: int = 0, x_base: int = 0, exclude_self: bool = False,
              out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d2 fp32 (nq, k), idx int64 (nq, k)) on the device: for every row of the fp32 (nq, d) cuda tensor ``q`` the k rows of ``x``
    (nx, d) with the smallest (squared distance, global index) in lexicographic order, the global index of row i of ``x`` being
    ``x_base + i``; ascending, equal distances by the lower index.  Where fewer than k candidates exist the tail is (+inf, -1).
    ``exclude_self``: the pair with q_base + j == x_base + i takes no part (by index: a duplicate of the query still counts).
    ``out=(d2, idx)``, a previous result for the same queries and k: the rows of ``x`` are merged into it, in place, and it is
    returned -- one call on all candidates and calls on any partition of them into slabs, in any order, give the same bits.
    1 <= k <= 8.  Enqueued on the current stream, nothing waits; two calls give the same bits."""
    L = _lib.get_lib()
    _check_rows("nn_search", q, x)
    if int(k) != k:
        raise ValueError(f"k={k!r}: nn_search takes an integer k")
    k = int(k)
    q, x = _rows(q), _rows(x)
    nq, d = q.shape
    nx, dx = x.shape
    if dx != d:
        raise ValueError(f"nn_search: d mismatch ({d} vs {dx})")
    if out is None:
        d2 = torch.empty((nq, max(k, 1)), dtype=torch.float32, device=q.device)
        idx = torch.empty((nq, max(k, 1)), dtype=torch.int64, device=q.device)
    else:
        d2, idx = out
        for t, dt in ((d2, torch.float32), (idx, torch.int64)):
            if tuple(t.shape) != (nq, k) or t.dtype != dt or t.device != q.device or not t.is_contiguous():
                raise ValueError(f"nn_search: out must be contiguous (d2 fp32, idx int64) tensors of shape ({nq}, {k}) on the queries' device")
    ws, ws_bytes = _workspace(L.smd_nn_search_workspace_bytes(nq, nx, k), q.device)
    _lib.check(L.smd_nn_search(q.data_ptr(), q.stride(0), nq, int(q_base), x.data_ptr(), x.stride(0), nx, int(x_base), d, k,
                               int(bool(exclude_self)), int(out is not None), ws.data_ptr(), ws_bytes, d2.data_ptr(), idx.data_ptr(),
                               _stream(q.device)), "smd_nn_search")
    return d2, idx


class TrainIndex:
    """The training set of the copy metrics as an iterable of slabs (numpy arrays or tensors, on the host or the device; one
    array is one slab), searched exhaustively slab by slab: a host slab is uploaded when its turn comes and dropped after it, so
    device memory holds at most two slabs and the outputs.  A slab of more than two dimensions is read as frames of its last
    axis, or with ``sequences`` as one row per leading index (an (N, S, C) slab: N*S rows of C, or N rows of S*C).  Global row
    indices count through the slabs in order.  Kept on the device: ``r1_sq[n]``, every training row's squared distance to its
    nearest OTHER training row (``nn_search`` of every slab against every slab, self excluded by index), ``nn1_idx[n]``, that
    row, and ``norm[n]`` (float64), the rows' Euclidean norms."""

    def __init__(self, slabs, device=None, sequences: bool = False):
        self.source = slabs
        self.sequences = bool(sequences)
        if torch.is_tensor(slabs) or isinstance(slabs, np.ndarray):
            slabs = [slabs]
        slabs = list(slabs)
        self.device = _device(*slabs) if device is None else torch.device(device)
        self._slabs = [s if torch.is_tensor(s) else torch.from_numpy(np.asarray(s)) for s in slabs]
        sizes = [int(self._view(s).shape[0]) for s in self._slabs]
        self.offsets = [0] + [int(v) for v in np.cumsum(sizes)]
        self.n = self.offsets[-1]
        dims = {int(self._view(s).shape[1]) for s in self._slabs}
        if len(dims) != 1:
            raise ValueError(f"TrainIndex: the slabs must agree in their row length (got {sorted(dims)})")
        self.d = dims.pop()
        if self.n < 2:
            raise ValueError(f"TrainIndex: {self.n} training rows: a nearest OTHER row needs two")
        self.r1_sq = torch.empty(self.n, dtype=torch.float32, device=self.device)
        self.nn1_idx = torch.empty(self.n, dtype=torch.int64, device=self.device)
        self.norm = torch.empty(self.n, dtype=torch.float64, device=self.device)
        for a in range(len(self._slabs)):
            xa = self.slab(a)
            lo, hi = self.offsets[a], self.offsets[a + 1]
            d2, idx = self.query(xa, 1, exclude_self=True, q_base=lo, resident=(a, xa))
            self.r1_sq[lo:hi] = d2[:, 0]
            self.nn1_idx[lo:hi] = idx[:, 0]
            self.norm[lo:hi] = xa.double().pow(2).sum(1).sqrt()

    def _view(self, t: torch.Tensor) -> torch.Tensor:
        if t.dim() <= 1:
            return t.reshape(-1, 1)
        return t.reshape(t.shape[0], -1) if self.sequences else t.reshape(-1, t.shape[-1])

    def rows(self, a) -> torch.Tensor:
        """``a`` (numpy or tensor) as this index reads it: contiguous fp32 (n, d) rows on its device"""
        t = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
        return self._view(t).to(device=self.device, dtype=torch.float32).contiguous()

    def slab(self, a: int) -> torch.Tensor:
        return self.rows(self._slabs[a])

    def query(self, rows, k: int = 1, exclude_self: bool = False, q_base: int = 0, resident=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(d2, idx) of ``nn_search`` for ``rows`` against ALL slabs, accumulated slab by slab.  ``exclude_self``: ``rows`` are
        the training rows q_base, q_base + 1, ...: each leaves itself out.  ``resident=(a, tensor)``: slab a is on the device
        already."""
        q = rows if torch.is_tensor(rows) and rows.is_cuda and rows.dim() == 2 and rows.dtype == torch.float32 else self.rows(rows)
        if q.shape[1] != self.d:
            raise ValueError(f"TrainIndex.query: d mismatch ({self.d} vs {q.shape[1]})")
        out = None
        for b in range(len(self._slabs)):
            xb = resident[1] if resident is not None and resident[0] == b else self.slab(b)
            out = nn_search(q, xb, k, q_base=q_base, x_base=self.offsets[b], exclude_self=exclude_self, out=out)
        return out

    def is_same(self, other) -> bool:
        return other is self or other is self.source


def _nearest_train(index: TrainIndex, rows, k: int):
    """(d2, idx, norms float64) of ``rows`` against the training set; the training set itself (the index or the object it was
    built from, as ``kernel_mmds`` detects identity) is searched leave-one-out"""
    if index.is_same(rows):
        parts = [index.query(index.slab(a), k, exclude_self=True, q_base=index.offsets[a]) for a in range(len(index._slabs))]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), index.norm, True
    q = index.rows(rows)
    d2, idx = index.query(q, k)
    return d2, idx, q.double().pow(2).sum(1).sqrt(), False


def _authentic(index: TrainIndex, d2: torch.Tensor, idx: torch.Tensor, same: bool) -> torch.Tensor:
    """d2(q, x_i*) >= r1_sq[i*].  Leave-one-out (``same``): when row i is in turn the nearest other row of its i*, both sides are
    the distance of ONE pair and the row sits on the boundary, which counts -- decided by index, since the fp32 d2 of a pair is
    formed around the query's norm and its last bit can differ between the two directions."""
    nearest = idx[:, 0]
    a = d2[:, 0] >= index.r1_sq[nearest]
    if same:
        a |= index.nn1_idx[nearest] == torch.arange(index.n, device=a.device)
    return a


def authenticity(index: TrainIndex, fake) -> Dict[str, object]:
    """The authenticity score of Alaa et al. 2022: with i* the nearest training row of a fake row q (``nn_search`` order), q is
    authentic when d2(q, x_i*) >= r1_sq[i*] -- it is no closer to x_i* than x_i*'s nearest other training row is; the boundary
    counts as authentic.  {"authenticity": the mean over the fake rows, "authentic": the per-row flags (numpy bool)}.  When
    ``fake`` is the training set itself (the index, or the object it was built from) pair (i, i) is excluded: leave-one-out."""
    d2, idx, _, same = _nearest_train(index, fake, 1)
    a = _authentic(index, d2, idx, same).cpu().numpy()
    return {"authenticity": float(a.mean()), "authentic": a}


def _median_distance(d2: torch.Tensor) -> float:
    return float(np.median(np.sqrt(d2[:, 0].cpu().numpy().astype(np.float64))))


def copy_report(index: TrainIndex, held_out, fake, k: int = 1) -> Dict[str, object]:
    """How close the ``fake`` rows sit to the training set, next to how close unseen (``held_out``) rows do:
    authenticity (see ``authenticity``); median_nn_fake / median_nn_held_out, the median distance (not squared) to the nearest
    training row; copy_gap, their ratio (below 1: the samples are closer to the training data than unseen data is);
    exact_copies, the fake rows whose nearest d2 is at most the fp32 error bound (d + 4) 2^-24 (|q| + |x_i*|)^2 of that pair
     -- indistinguishable from distance 0; nn_d2, nn_idx (numpy (n, k)): the k nearest training rows of
    every fake row; k, n_train, n_fake, n_held_out, version."""
    d2, idx, qn, same = _nearest_train(index, fake, k)
    dh = _nearest_train(index, held_out, 1)[0]
    m = (index.d + 4) * 2.0 ** -24 * (qn + index.norm[idx[:, 0]]) ** 2
    mf, mh = _median_distance(d2), _median_distance(dh)
    gap = mf / mh if mh > 0 else (float("inf") if mf > 0 else float("nan"))
    return {"authenticity": float(_authentic(index, d2, idx, same).double().mean()), "median_nn_fake": mf, "median_nn_held_out": mh,
            "copy_gap": gap, "exact_copies": int((d2[:, 0].double() <= m).sum()), "nn_d2": d2.cpu().numpy(), "nn_idx": idx.cpu().numpy(),
            "k": int(k), "n_train": index.n, "n_fake": int(d2.shape[0]), "n_held_out": int(dh.shape[0]), "version": COPY_METRICS_VERSION}


COPY_SCALARS = ("authenticity", "median_nn_fake", "median_nn_held_out", "copy_gap", "exact_copies")


def copy_metrics(train_slabs, held_out, fake, k: int = 1, device=None) -> Dict[str, object]:
    """``copy_report`` at both levels of (N, S, C) sets: frames (N*S rows of C) under the plain keys and sequences (N rows of
    S*C) under the same keys with the suffix ``_seq`` -- a lifted two-bar phrase and a lifted piece are different findings.
    ``train_slabs``: a list of (n_i, S, C) arrays (walked once per level) or one array."""
    out: Dict[str, object] = {}
    for sequences, suffix in ((False, ""), (True, "_seq")):
        index = TrainIndex(train_slabs, device, sequences=sequences)
        rep = copy_report(index, held_out, fake, k)
        out.update({name + suffix: v for name, v in rep.items() if name not in ("k", "version")})
    out.update(k=int(k), version=COPY_METRICS_VERSION)
    return out
