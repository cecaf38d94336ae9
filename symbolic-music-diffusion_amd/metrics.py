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
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

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
    ws_bytes = L.smd_pair_kernel_sums_workspace_bytes(nx, ny, int(sym))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=x.device)
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
    ws_bytes = L.smd_knn_radii_workspace_bytes(n, int(k))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=x.device)
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
    ws_bytes = L.smd_ball_cover_workspace_bytes(nq, nx)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=x.device)
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


def moments(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """np.mean(x, axis=0), np.cov(x, rowvar=False) (ddof = 1) of an fp32 (n, d) cuda tensor as fp64 device tensors."""
    L = _lib.get_lib()
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("moments takes an fp32 (n, d) cuda tensor")
    x = _rows(x)
    n, d = x.shape
    ws_bytes = L.smd_moments_workspace_bytes(n, d)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=x.device)
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
