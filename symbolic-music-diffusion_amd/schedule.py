"""Noise schedule and the per-timestep constant tables uploaded once to the GPU.

``create_noise_schedule`` keeps the reference signature (utils/ebm_utils.py:62-86).  The tables are
computed in float32 on the host exactly as the reference's jnp float32 expressions
(utils/ebm_utils.py:313-358, utils/losses.py:277-281) so they are bit-exact against the oracle.
"""
from __future__ import annotations

import numpy as np

COLLECTION_STEPS = 40   # utils/ebm_utils.py:320


def create_noise_schedule(sigma_begin=1.0, sigma_end=1e-2, L=10, schedule="geometric") -> np.ndarray:
    """utils/ebm_utils.py:62-86 (float32 like jnp)."""
    f = np.float32
    if schedule == "geometric":
        s = np.exp(np.linspace(np.log(f(sigma_begin)), np.log(f(sigma_end)), L, dtype=np.float32))
    elif schedule == "linear":
        s = np.linspace(f(sigma_begin), f(sigma_end), L, dtype=np.float32)
    elif schedule == "fibonacci":
        v = [1e-6, 2e-6]
        for _ in range(L - 2):
            v.append(v[-1] + v[-2])
        s = np.array(v, dtype=np.float32)
    else:
        raise ValueError(f"Unsupported schedule: {schedule}")
    return s.astype(np.float32)


def alphas_cumprod(betas: np.ndarray) -> np.ndarray:
    """cumprod(1 - betas), float32 (utils/ebm_utils.py:315-316)."""
    betas = np.asarray(betas, dtype=np.float32)
    return np.cumprod((np.float32(1.0) - betas).astype(np.float32), dtype=np.float32)


PREDICTIONS = ("eps", "x0", "v")     # what the network's output means; the index is the engine's kind


def prediction_kind(prediction) -> int:
    """0 / 1 / 2 for "eps" / "x0" / "v" (or the integer itself): the value of the engine option "prediction"."""
    if isinstance(prediction, (int, np.integer)) and not isinstance(prediction, bool) and 0 <= int(prediction) < len(PREDICTIONS):
        return int(prediction)
    if prediction in PREDICTIONS:
        return PREDICTIONS.index(prediction)
    raise ValueError(f"prediction must be one of {PREDICTIONS}, got {prediction!r}")


def x0_coefficients(alphas_prod_like, prediction="eps"):
    """float64 (c0, c1) of x0 = c0 x_t - c1 out for a network whose output ``out`` is eps (c0 = sqrt(1/ap), c1 = sqrt(1/ap - 1)),
    x0 (c0 = 0, c1 = -1) or v = sqrt(ap) eps - sqrt(1 - ap) x0 (c0 = sqrt(ap), c1 = sqrt(1 - ap)): the first two columns of every
    sampler table, which is all the sampler kernels know about the parameterisation."""
    ap = np.asarray(alphas_prod_like, dtype=np.float64)
    kind = prediction_kind(prediction)
    if kind == 0:          # sqrt(1/ap - 1) as sqrt(1 - ap) / sqrt(ap): 1/ap - 1 cancels near ap = 1, 1 - ap is exact there
        return 1.0 / np.sqrt(ap), np.sqrt(1.0 - ap) / np.sqrt(ap)
    if kind == 1:
        return np.zeros_like(ap), -np.ones_like(ap)
    return np.sqrt(ap), np.sqrt(1.0 - ap)


def _x0_columns(betas, prediction):
    """float32 [T][2] (c0, c1) for a non-eps kind: float64 from the float32 ``alphas_cumprod``, rounded once; None for eps (the
    tables then keep the float32 expressions of the reference, bit for bit)."""
    if prediction_kind(prediction) == 0:
        return None
    c0, c1 = x0_coefficients(alphas_cumprod(betas).astype(np.float64), prediction)
    return np.stack([c0, c1], axis=1).astype(np.float32)


def min_snr_weight(alphas_prod_like, gamma: float, prediction="eps") -> np.ndarray:
    """Min-SNR-gamma loss weight (Hang et al. 2023), float64.  ``prediction`` "eps" (the default): min(SNR, gamma) / SNR with
    SNR = ap / (1 - ap), i.e. min(1, gamma (1 - ap) / ap) -- 1 where SNR <= gamma, gamma / SNR above.  ``gamma`` <= 0 or +inf: no
    weighting (all ones).  ap = 1 (SNR = inf) gives 0 and ap = 0 gives 1, never a NaN.  The weighted loss kernel evaluates the
    same expression per sample from the squared noise level q-sample stored.
    ``prediction`` "x0": min(SNR, gamma) -- gamma at ap = 1, 0 at ap = 0; "v": min(SNR, gamma) / (SNR + 1) = min(ap, gamma (1 - ap))
    -- 0 at both ends (section 26).  Where finite, w_v (SNR + 1) = w_x0 = w_eps SNR."""
    ap = np.asarray(alphas_prod_like, dtype=np.float64)
    gamma = float(gamma)
    kind = prediction_kind(prediction)
    if not (gamma > 0.0) or np.isinf(gamma):
        return np.ones_like(ap)
    if kind == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            snr = np.where(ap < 1.0, ap / (1.0 - ap), np.inf)
        return np.minimum(snr, gamma)
    if kind == 2:
        return np.minimum(ap, gamma * (1.0 - ap))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = gamma * (1.0 - ap) / ap
    return np.minimum(1.0, np.where(ap > 0.0, f, np.inf))


def reverse_coefficient_table(betas: np.ndarray, prediction="eps") -> np.ndarray:
    """[T][8] float32: sqrt(1/ap), sqrt(1-ap)*sqrt(1/ap), mu1, mu2, sigma, ap, sqrt(ap), sqrt(1-ap)
    (utils/ebm_utils.py:332-358, sigma = exp(0.5*log(max(var,1e-20))) as at :356-364).  ``prediction`` "x0" / "v": the first two
    columns are that kind's (c0, c1) of ``x0_coefficients``; nothing else changes."""
    f = np.float32
    betas = np.asarray(betas, dtype=np.float32)
    alphas = (f(1) - betas).astype(np.float32)
    ap = alphas_cumprod(betas)
    ap_prev = np.concatenate([np.ones((1,), np.float32), ap[:-1]])
    sqrt_recip = np.sqrt(f(1) / ap, dtype=np.float32)
    sqrt_m1 = (np.sqrt(f(1) - ap, dtype=np.float32) * sqrt_recip).astype(np.float32)
    mu1 = (betas * np.sqrt(ap_prev, dtype=np.float32) / (f(1) - ap)).astype(np.float32)
    mu2 = ((f(1) - ap_prev) * np.sqrt(alphas, dtype=np.float32) / (f(1) - ap)).astype(np.float32)
    var = (betas * (f(1) - ap_prev) / (f(1) - ap)).astype(np.float32)
    var_c = np.maximum(var, f(1e-20)).astype(np.float32)
    sigma = np.exp(f(0.5) * np.log(var_c, dtype=np.float32), dtype=np.float32)
    out = np.stack([sqrt_recip, sqrt_m1, mu1, mu2, sigma, ap, np.sqrt(ap, dtype=np.float32),
                    np.sqrt(f(1) - ap, dtype=np.float32)], axis=1)
    out = np.ascontiguousarray(out.astype(np.float32))
    cols = _x0_columns(betas, prediction)
    if cols is not None:
        out[:, :2] = cols
    return out


def collection_index_table(T: int) -> np.ndarray:
    """linspace(1, T, 40).astype(int32), utils/ebm_utils.py:324-325."""
    return np.linspace(np.float32(1), np.float32(T), COLLECTION_STEPS, dtype=np.float32).astype(np.int32)


def collection_slot_table(T: int) -> np.ndarray:
    """slot[t] = collection row written after the step at timestep t, or -1
    (image_idx = T - t + 1 matched against collection_idx, utils/ebm_utils.py:387-394).
    Slot 1 is never written and the final state (t=0) is never collected -- reference quirk."""
    table = collection_index_table(T)
    slot = np.full((T,), -1, dtype=np.int32)
    for t in range(T):
        hit = np.nonzero(table == (T - t + 1))[0]
        if hit.size:
            # short schedules (T < 40) repeat linspace entries and the summed index can pass the last row: the reference's
            # jax.ops.index_update then scatters out of bounds, which XLA drops
            s = int(np.sum(hit)) + 1
            slot[t] = s if s <= COLLECTION_STEPS else -1
    return slot


# ------------------------------------------------------------------ strided (DDIM) walks
def stride_timesteps(T: int, K: int) -> np.ndarray:
    """The K timesteps of a strided walk over [0, T), descending: evenly spaced, always with T - 1 and 0."""
    T, K = int(T), int(K)
    if not 2 <= K <= T:
        raise ValueError(f"a strided walk takes 2 <= steps <= {T} timesteps, got {K}")
    return np.unique(np.round(np.linspace(0, T - 1, K)).astype(int))[::-1].copy()


def strided_coefficients(betas: np.ndarray, taus, eta: float) -> dict:
    """float64 (a, b, sigma, sqrt_as, sqrt_1m_as), one entry per iteration of the descending walk ``taus``, of
    x_s = a x0 + b x_t + sigma z (Song et al. 2021, eq. 12 with eps_hat written as (x_t - sqrt(ap_t) x0) / sqrt(1 - ap_t));
    ap is the float32 cumulative product the engine's other tables use, and ap_s := 1 on the last iteration."""
    taus = np.asarray(taus, dtype=np.int64)
    ap = alphas_cumprod(betas).astype(np.float64)
    ap_t = ap[taus]
    ap_s = np.concatenate([ap[taus[1:]], np.ones(1)])
    sigma = float(eta) * np.sqrt((1 - ap_s) / (1 - ap_t)) * np.sqrt(1 - ap_t / ap_s)
    c = np.sqrt(np.maximum(1 - ap_s - sigma ** 2, 0.0)) / np.sqrt(1 - ap_t)
    return dict(a=np.sqrt(ap_s) - c * np.sqrt(ap_t), b=c, sigma=sigma, sqrt_as=np.sqrt(ap_s), sqrt_1m_as=np.sqrt(1 - ap_s))


def _walk_tables(betas, order, co, next_t, slots, clip, prediction="eps"):
    T = len(betas)
    base = reverse_coefficient_table(betas, prediction)
    coef = np.zeros((T, 8), dtype=np.float32)
    plan = np.zeros((T, 4), dtype=np.int32)
    plan[:, :3] = -1                                       # not on the walk: no next timestep, no iteration, no slot
    for j, t in enumerate(order):
        coef[t] = (base[t, 0], base[t, 1], co["a"][j], co["b"][j], co["sigma"][j], clip, co["sqrt_as"][j], co["sqrt_1m_as"][j])
        plan[t] = (next_t[j], j, slots[j], 0)
    return coef, plan


def strided_coefficient_table(betas: np.ndarray, taus, eta: float, clip: float = 1.0, prediction="eps"):
    """Tables of the strided sampler for the descending timesteps ``taus``: float32 [T][8] (sqrt_recip, sqrt_m1, a, b, sigma,
    clip, sqrt_as, sqrt_1m_as) and int32 [T][4] (next_t, iteration, slot, 0).  Columns 0 / 1 are those of
    ``reverse_coefficient_table`` (of the kind ``prediction``).  Timesteps that are not in ``taus`` have a zero row and (-1, -1, -1, 0); next_t is -1
    after the last iteration.  The slots are the reference's collection bookkeeping (``collection_slot_table``) applied to a
    walk of K = len(taus) iterations, so the collection keeps its 41 rows."""
    taus = [int(t) for t in taus]
    K = len(taus)
    slot_k = collection_slot_table(K)
    return _walk_tables(betas, taus, strided_coefficients(betas, taus, eta), taus[1:] + [-1],
                        [int(slot_k[K - 1 - j]) for j in range(K)], clip, prediction)


def inversion_coefficient_table(betas: np.ndarray, taus, prediction="eps"):
    """The same walk ascending with sigma = 0 (DDIM inversion): taus_asc[j] -> taus_asc[j + 1], no clamp (clip = +inf), nothing
    collected.  len(taus) - 1 steps are executed; the last of them has next_t = T, which is out of range, so the walk stops by
    itself and no step is executed at T - 1."""
    asc = sorted(int(t) for t in taus)
    ap = alphas_cumprod(betas).astype(np.float64)
    t_, s_ = np.asarray(asc[:-1]), np.asarray(asc[1:])
    c = np.sqrt(1 - ap[s_]) / np.sqrt(1 - ap[t_])
    co = dict(a=np.sqrt(ap[s_]) - c * np.sqrt(ap[t_]), b=c, sigma=np.zeros(len(t_)), sqrt_as=np.sqrt(ap[s_]),
              sqrt_1m_as=np.sqrt(1 - ap[s_]))
    n = len(t_)
    return _walk_tables(betas, asc[:-1], co, asc[1:-1] + [len(betas)], [-1] * n, np.inf, prediction)


# ------------------------------------------------------------------ second-order multistep walks
def half_logsnr(betas: np.ndarray) -> np.ndarray:
    """lambda_t = log(sqrt(ap_t) / sqrt(1 - ap_t)), float64 from the float32 ``alphas_cumprod``: the time variable of
    DPM-Solver (Lu et al. 2022), strictly decreasing in t."""
    ap = alphas_cumprod(betas).astype(np.float64)
    return 0.5 * (np.log(ap) - np.log1p(-ap))


def logsnr_timesteps(T: int, K: int, betas: np.ndarray) -> np.ndarray:
    """Timesteps of a walk that is uniform in lambda instead of in t, descending: K values of lambda evenly spaced from
    lambda[T-1] to lambda[0], each snapped to the timestep of nearest lambda, duplicates dropped.  Always with T - 1 and 0; near
    t = 0 the snapping merges points, so len(result) <= K (as ``stride_timesteps`` may)."""
    T, K = int(T), int(K)
    if len(betas) != T:
        raise ValueError(f"logsnr_timesteps: {len(betas)} betas for T={T}")
    if not 2 <= K <= T:
        raise ValueError(f"a strided walk takes 2 <= steps <= {T} timesteps, got {K}")
    lam = half_logsnr(betas)
    want = np.linspace(lam[T - 1], lam[0], K)
    taus = np.argmin(np.abs(lam[None, :] - want[:, None]), axis=1)       # linspace's end points are lam[T-1] and lam[0] exactly
    return np.unique(taus)[::-1].astype(int).copy()


def multistep_coefficients(betas: np.ndarray, taus, order: int) -> dict:
    """float64 (a0, a1, b, w, h, sqrt_as, sqrt_1m_as), one entry per iteration of the descending walk ``taus``, of the
    data-prediction multistep update of DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2) in the notation of
    ``strided_coefficients`` at eta = 0:  x_s = b x_t + a0 x0 + a1 x0_prev,  a0 = a (1 + w),  a1 = -a w,
    w_j = h_j / (2 h_{j-1}),  h_j = lambda_s - lambda_t.  w = 0 on the first iteration (no history) and on the last (ap_s := 1,
    h = inf: a first-order step that returns x0); ``order`` 1 is w = 0 everywhere, the strided update itself."""
    if order not in (1, 2):
        raise ValueError(f"multistep_coefficients: order={order} (1: DDIM, 2: DPM-Solver++(2M))")
    taus = np.asarray(taus, dtype=np.int64)
    co = strided_coefficients(betas, taus, 0.0)
    lam = half_logsnr(betas)
    n = len(taus)
    h = np.full(n, np.inf)
    h[:-1] = lam[taus[1:]] - lam[taus[:-1]]
    w = np.zeros(n)
    if order == 2 and n > 2:
        w[1:-1] = h[1:-1] / (2 * h[:-2])
    a1 = np.where(w == 0, 0.0, -co["a"] * w)               # an exact +0 where there is no history term: the kernel tests it
    return dict(a0=co["a"] * (1 + w), a1=a1, b=co["b"], w=w, h=h, sqrt_as=co["sqrt_as"], sqrt_1m_as=co["sqrt_1m_as"])


MULTISTEP_COLUMNS = 12    # floats per row of the multistep coefficient table: rows stay 16-byte aligned


def multistep_coefficient_table(betas: np.ndarray, taus, order: int, clip: float = 1.0, prediction="eps"):
    """Tables of the multistep sampler for the descending timesteps ``taus``: float32 [T][12] -- the eight columns of
    ``strided_coefficient_table`` at eta = 0 with a0 in place of a (sqrt_recip, sqrt_m1, a0, b, 0, clip, sqrt_as, sqrt_1m_as),
    then a1 and three zeros -- and that function's int32 [T][4] plan unchanged.  At order 1 the first eight columns ARE the
    strided table, bit for bit."""
    taus = [int(t) for t in taus]
    co = multistep_coefficients(betas, taus, order)
    base, plan = strided_coefficient_table(betas, taus, 0.0, clip, prediction)
    coef = np.zeros((len(betas), MULTISTEP_COLUMNS), dtype=np.float32)
    coef[:, :8] = base
    coef[taus, 2] = co["a0"]
    coef[taus, 8] = co["a1"]
    return coef, plan


# ------------------------------------------------------------------ third-order exponential Adams walks
ADAMS_SOLVERS = ("adams3", "adams3_pc")
_ADAMS_SERIES_BELOW = 0.5     # H under which the moments come from their series instead of the recurrence


def _exp_moments(H: float, n: int) -> np.ndarray:
    """J_k = Int_0^H e^(u - H) u^k du for k < n, float64.  J_0 = -expm1(-H) and J_k = H^k - k J_{k-1}; the recurrence subtracts
    two numbers of size H^k to leave one of size H^(k+1) / (k + 1), so below H = 0.5 every J_k comes from its own alternating
    series J_k = k! H^(k+1) sum_m (-H)^m / (m + k + 1)! instead (terms fall at least as fast as 2^-m there)."""
    H = float(H)
    J = np.empty(n, dtype=np.float64)
    if H < _ADAMS_SERIES_BELOW:
        for k in range(n):
            term = H ** (k + 1) / (k + 1)                    # m = 0: k! H^(k+1) / (k + 1)!
            total, m = 0.0, 0
            while abs(term) > 1e-19 * abs(total) or m == 0:
                total += term
                m += 1
                term *= -H / (m + k + 1)
            J[k] = total
        return J
    J[0] = -np.expm1(-H)
    for k in range(1, n):
        J[k] = H ** k - k * J[k - 1]
    return J


def exp_lagrange_weights(lam_a: float, lam_b: float, nodes) -> np.ndarray:
    """W_i = Int_{lam_a}^{lam_b} e^(l - lam_b) L_i(l) dl, float64, L_i the Lagrange basis on ``nodes`` (distinct lambdas, at most a
    handful): the weights of an exponential integrator that replaces x0(l) by its interpolant on the nodes (section 29).  With
    u = l - lam_a the basis is expanded in powers of u and integrated against the moments of ``_exp_moments``."""
    nodes = np.asarray(nodes, dtype=np.float64).reshape(-1)
    q = len(nodes)
    H = float(lam_b) - float(lam_a)
    if q < 1 or not H > 0 or not np.isfinite(H):
        raise ValueError(f"exp_lagrange_weights: {q} nodes on an interval of length {H}")
    u = nodes - float(lam_a)
    J = _exp_moments(H, q)
    W = np.empty(q, dtype=np.float64)
    for i in range(q):
        others = np.delete(u, i)
        poly = np.poly(others) / np.prod(u[i] - others) if q > 1 else np.ones(1)      # highest power first
        W[i] = float(np.dot(poly[::-1], J))
    return W


def adams_coefficients(betas: np.ndarray, taus, corrector: bool) -> dict:
    """float64 coefficients of the third-order exponential Adams walk down ``taus`` (section 29), one entry per iteration:
    x_s = b x_t + A0 x0_j + A1 x0_{j-1} + A2 x0_{j-2} + A3 x0_{j-3}, the corrector (``corrector``: redo the previous step with the
    evaluation just made, then predict) folded in.  Also the unfolded weights for the tests: ``wp`` [K][3] of the predictor on
    the nodes lambda of taus[j], taus[j-1], taus[j-2], ``wc`` [K][3] of the corrector on taus[j], taus[j-1], taus[j-2] over the
    previous step (zero rows where there is none), ``alpha_t`` / ``alpha_s``, ``b`` and ``h``.  Iteration j has min(3, j + 1) nodes;
    the last is first order on ap_s := 1 (b = 0, h = inf, weight 1: it returns x0).  Unused coefficients are exact +0."""
    taus = np.asarray(taus, dtype=np.int64)
    co = strided_coefficients(betas, taus, 0.0)
    ap = alphas_cumprod(betas).astype(np.float64)
    lam = half_logsnr(betas)[taus]
    n = len(taus)
    alpha_t, alpha_s, b = np.sqrt(ap[taus]), co["sqrt_as"], co["b"]
    h = np.full(n, np.inf)
    h[:-1] = lam[1:] - lam[:-1]
    wp, wc = np.zeros((n, 3)), np.zeros((n, 3))
    for j in range(n):
        if j == n - 1:
            wp[j, 0] = 1.0
        else:
            p = min(3, j + 1)
            wp[j, :p] = exp_lagrange_weights(lam[j], lam[j + 1], lam[j::-1][:p])
        if corrector and 1 <= j < n - 1:                       # b = 0 on the last iteration: nothing of the corrector survives
            q = min(3, j + 1)
            wc[j, :q] = exp_lagrange_weights(lam[j - 1], lam[j], lam[j::-1][:q])
    A = np.zeros((n, 4))
    for j in range(n):
        A[j, :3] = alpha_s[j] * wp[j]
        if corrector and 1 <= j < n - 1:
            g = b[j] * alpha_t[j]
            q = min(3, j + 1)
            A[j, 0] += g * wc[j, 0]
            A[j, 1] += g * (wc[j, 1] - wp[j - 1, 0])
            if q > 2:
                A[j, 2] += g * (wc[j, 2] - wp[j - 1, 1])
            if j >= 3:
                A[j, 3] = -g * wp[j - 1, 2]
    return dict(A0=A[:, 0], A1=A[:, 1], A2=A[:, 2], A3=A[:, 3], b=b, h=h, wp=wp, wc=wc, alpha_t=alpha_t, alpha_s=alpha_s,
                sqrt_as=co["sqrt_as"], sqrt_1m_as=co["sqrt_1m_as"])


def adams_coefficient_table(betas: np.ndarray, taus, corrector: bool, clip: float = 1.0, prediction="eps"):
    """Tables of the exponential Adams sampler for the descending timesteps ``taus``: float32 [T][12] -- the eight columns of
    ``strided_coefficient_table`` at eta = 0 with A0 in place of a, then A1, A2, A3 (``adams_coefficients``, rounded once) and a
    zero -- and that function's int32 [T][4] plan unchanged.  The four A columns depend on the schedule, the walk and the solver
    only and take per-iteration Python (milliseconds: as much as several iterations of a warm walk), so the last few are kept:
    a sampler that is called again with the same walk pays for them once."""
    taus = [int(t) for t in taus]
    key = (np.asarray(betas, dtype=np.float32).tobytes(), tuple(taus), bool(corrector))
    A = _ADAMS_A_CACHE.get(key)
    if A is None:
        co = adams_coefficients(betas, taus, corrector)
        A = np.stack([co[f"A{k}"] for k in range(4)], axis=1)
        if len(_ADAMS_A_CACHE) >= 16:
            _ADAMS_A_CACHE.pop(next(iter(_ADAMS_A_CACHE)))
        _ADAMS_A_CACHE[key] = A
    base, plan = strided_coefficient_table(betas, taus, 0.0, clip, prediction)
    coef = np.zeros((len(betas), MULTISTEP_COLUMNS), dtype=np.float32)
    coef[:, :8] = base
    coef[taus, 2] = A[:, 0]
    coef[taus, 8:11] = A[:, 1:]
    return coef, plan


_ADAMS_A_CACHE: dict = {}     # (betas bytes, walk, corrector) -> float64 [K][4], at most 16 entries, oldest dropped first


# ------------------------------------------------------------------ progressive distillation
DISTILL_COLUMNS = 16      # floats per row of the distillation table: one 64-byte row per student step
DISTILL_WEIGHTINGS = ("truncated_snr", "none")
DISTILL_COLUMN_NAMES = ("c0_t", "c1_t", "a", "b", "clip", "alpha_t", "sigma_t", "alpha_m", "c0_m", "c1_m", "w1", "w2", "weight",
                        "inv_sigma_t")


def _check_walk(T: int, walk, what: str) -> np.ndarray:
    w = np.asarray(walk, dtype=np.int64).reshape(-1)
    if len(w) == 0 or w[0] >= T or w[-1] < 0 or np.any(np.diff(w) >= 0):
        raise ValueError(f"{what}: a walk is strictly descending within [0, {T}), got {[int(t) for t in w]}")
    return w


def distill_walk(T: int, N: int, teacher_walk=None):
    """(teacher_walk, student_walk) of one round of progressive distillation (Salimans & Ho 2022) to a student of ``N`` steps: the
    teacher's descending walk of 2N timesteps -- ``stride_timesteps(T, 2N)`` in the first round, the walk its checkpoint
    records later -- and every second entry of it, ``teacher_walk[0::2]``.  Both end at the clean level, which is not listed."""
    T, N = int(T), int(N)
    if N < 1:
        raise ValueError(f"distill_walk: a student takes N >= 1 steps, got {N}")
    if teacher_walk is None:
        if 2 * N > T:
            raise ValueError(f"distill_walk: a student of {N} steps needs a teacher walk of {2 * N} timesteps, the schedule has {T}")
        tw = np.asarray(stride_timesteps(T, 2 * N), dtype=np.int64)
    else:
        tw = _check_walk(T, teacher_walk, "distill_walk")
    if len(tw) != 2 * N:
        raise ValueError(f"distill_walk: a student of {N} steps needs a teacher walk of {2 * N} timesteps, got {len(tw)}")
    return tw.copy(), tw[0::2].copy()


def distill_weights(ap, walk, kind, weighting: str = "truncated_snr") -> np.ndarray:
    """float64 loss weight of every step of the student walk ``walk`` (timesteps into the cumulative alphas ``ap``), for a
    student whose output is ``kind``.  "none": 1.  "truncated_snr" (Salimans & Ho 2022, section 4): max(SNR, 1) on the error in
    x space, written in the student's output space -- x0: max(SNR, 1); eps: max(1, 1 / SNR), since eps_hat - eps =
    -sqrt(SNR) (x_hat - x); v: max(SNR, 1) / (SNR + 1), since v_hat - v = -sqrt(SNR + 1) (x_hat - x).  SNR = ap / (1 - ap)."""
    if weighting not in DISTILL_WEIGHTINGS:
        raise ValueError(f"distill_weights: weighting must be one of {DISTILL_WEIGHTINGS}, got {weighting!r}")
    k = prediction_kind(kind)
    ap_t = np.asarray(ap, dtype=np.float64)[np.asarray(walk, dtype=np.int64)]
    if weighting == "none":
        return np.ones_like(ap_t)
    snr = ap_t / (1.0 - ap_t)
    if k == 1:
        return np.maximum(snr, 1.0)
    if k == 0:
        return np.maximum(1.0, 1.0 / snr)
    return np.maximum(snr, 1.0) / (snr + 1.0)


def distill_tables(betas: np.ndarray, teacher_walk, teacher_prediction="eps", student_prediction="v",
                   weighting: str = "truncated_snr", clip: float = 1.0):
    """The table of the distillation kernels for the teacher walk ``teacher_walk`` (2N timesteps, descending) and a dict of its
    float64 originals.  Student step k has the levels t = walk[2k], m = walk[2k + 1] and u = walk[2k + 2] (clean, ap = 1, after
    the last).  float32 [N][16], rounded once from float64:

      c0_t, c1_t, a, b, clip, alpha_t, sigma_t, alpha_m, c0_m, c1_m, w1, w2, weight, 1 / sigma_t, 0, 0

    (c0, c1) are ``x0_coefficients`` of the TEACHER's kind at t and at m, (a, b) ``strided_coefficients`` at eta = 0 for t -> m,
    alpha = sqrt(ap), sigma = sqrt(1 - ap), weight = ``distill_weights`` of the STUDENT's kind.  (w1, w2) is the convex form of
    the target of Salimans & Ho: with (a', b') the coefficients of m -> u and r = sigma_u / sigma_t = b' b,
    x~ = (z_u - r z_t) / (alpha_u - r alpha_t) = w1 x1 + w2 x2, w2 = a' / D, w1 = a b' / D, D = alpha_u - r alpha_t = a' + a b'.
    D is formed as that sum, so w1 + w2 = 1 to rounding however fine the walk; the last step has b' = 0: (w1, w2) = (0, 1)."""
    tw = _check_walk(len(betas), teacher_walk, "distill_tables")
    if len(tw) % 2:
        raise ValueError(f"distill_tables: a teacher walk has an even number of timesteps, got {len(tw)}")
    if not float(clip) > 0:
        raise ValueError(f"distill_tables: clip={clip} must be positive (inf: no clamp)")
    ap = alphas_cumprod(betas).astype(np.float64)
    co = strided_coefficients(betas, tw, 0.0)
    t, m = tw[0::2], tw[1::2]
    a, b, a2, b2 = co["a"][0::2], co["b"][0::2], co["a"][1::2], co["b"][1::2]
    ap_u = np.concatenate([ap[tw[2::2]], np.ones(1)])
    alpha_t, sigma_t = np.sqrt(ap[t]), np.sqrt(1.0 - ap[t])
    alpha_u, sigma_u = np.sqrt(ap_u), np.sqrt(1.0 - ap_u)
    c0_t, c1_t = x0_coefficients(ap[t], teacher_prediction)
    c0_m, c1_m = x0_coefficients(ap[m], teacher_prediction)
    n1, n2 = a * b2, a2
    D = n1 + n2
    ref = dict(c0_t=c0_t, c1_t=c1_t, a=a, b=b, clip=np.full(len(t), float(clip)), alpha_t=alpha_t, sigma_t=sigma_t,
               alpha_m=np.sqrt(ap[m]), c0_m=c0_m, c1_m=c1_m, w1=n1 / D, w2=n2 / D,
               weight=distill_weights(ap, t, student_prediction, weighting), inv_sigma_t=1.0 / sigma_t)
    table = np.zeros((len(t), DISTILL_COLUMNS), dtype=np.float32)
    for j, name in enumerate(DISTILL_COLUMN_NAMES):
        table[:, j] = ref[name]
    ref.update(a2=a2, b2=b2, D=D, r=sigma_u / sigma_t, alpha_u=alpha_u, sigma_u=sigma_u, sigma_m=np.sqrt(1.0 - ap[m]),
               t=t.copy(), m=m.copy(), u=np.concatenate([tw[2::2], -np.ones(1, dtype=np.int64)]))
    return np.ascontiguousarray(table), ref


# ------------------------------------------------------------------ variational bound
def bound_tables(betas: np.ndarray, timesteps, clip: float = 1.0, prediction="eps") -> dict:
    """Everything the per-timestep variational bound (Ho et al. 2020, eq. 5) needs from the schedule, for the timesteps
    ``timesteps`` -- all of [0, T), or ``stride_timesteps(T, K)`` -- in any order; they are walked ascending.  Built in float64
    from the float32 ``alphas_cumprod`` (as the strided tables are), with ap_prev[0] = 1, and rounded once:

      w [T] float64          L_t = w_t * sum (x0 - x0_hat)^2 for t >= 1, w_t = mu1_t^2 / (2 bt_t); w[0] = 1 / (2 var_0)
      var_0                  the decoder's variance, bt_1 (the reference's posterior variance at t = 0 is 0)
      decoder_const          (D / 2) log(2 pi var_0) per DIMENSION, i.e. 0.5 log(2 pi var_0): multiply by D
      prior_a, prior_c       L_T = 0.5 (prior_a * sum x0^2 + D * prior_c), prior_a = ap_{T-1}, prior_c = -ap_{T-1} - log(1 - ap_{T-1})
      table [T][4] float32   (sqrt(ap), sqrt(1-ap), sqrt(1/ap), sqrt(1/ap - 1)): the kernels' rows; columns 2 and 3 are the
                             (c0, c1) of ``x0_coefficients`` for the kind ``prediction``
      next_t [T] int32       the ascending walk: next_t[t] = the next timestep, -1 after the last and for timesteps off the walk
      timesteps              the walk, ascending (int64);  clip is passed through
    """
    betas64 = np.asarray(betas, dtype=np.float32).astype(np.float64)
    T = len(betas64)
    ts = np.unique(np.asarray(timesteps, dtype=np.int64))
    if len(ts) == 0 or ts[0] < 0 or ts[-1] >= T:
        raise ValueError(f"bound_tables: timesteps must lie in [0, {T})")
    if not float(clip) > 0:
        raise ValueError(f"bound_tables: clip={clip} must be positive (inf: no clamp)")
    ap = alphas_cumprod(betas).astype(np.float64)
    ap_prev = np.concatenate([np.ones(1), ap[:-1]])
    bt = betas64 * (1 - ap_prev) / (1 - ap)                       # posterior variance; bt[0] = 0
    mu1 = betas64 * np.sqrt(ap_prev) / (1 - ap)
    var_0 = float(bt[1]) if T > 1 else float(betas64[0])
    w = np.empty(T, dtype=np.float64)
    w[1:] = mu1[1:] ** 2 / (2 * bt[1:])
    w[0] = 1.0 / (2 * var_0)
    table = np.stack([np.sqrt(ap), np.sqrt(1 - ap), np.sqrt(1 / ap), np.sqrt(1 / ap - 1)], axis=1)
    if prediction_kind(prediction) != 0:
        table[:, 2], table[:, 3] = x0_coefficients(ap, prediction)
    next_t = np.full((T,), -1, dtype=np.int32)
    next_t[ts[:-1]] = ts[1:]
    return dict(w=w, var_0=var_0, decoder_const=0.5 * np.log(2 * np.pi * var_0), prior_a=float(ap[-1]),
                prior_c=float(-ap[-1] - np.log(1 - ap[-1])), table=np.ascontiguousarray(table.astype(np.float32)),
                next_t=next_t, timesteps=ts, clip=float(clip))


def bound_from_sums(tab: dict, sums: np.ndarray, D: int) -> dict:
    """The bound from the kernels' per-example sums: ``sums`` [K][N][3] = (sum (x0 - x0_hat)^2, sum (eps - eps_hat)^2, sum x0^2)
    for the K ascending timesteps of ``tab`` (bound_tables), D = S * C.  Weighted and added in float64:
    L_t = w_t q_t (+ D * decoder_const at t = 0), L_T = 0.5 (prior_a n + D prior_c), total = L_T + sum_t L_t -- only when the
    walk covers every timestep; a sub-sequence gives ``total`` (and the per-dimension scalars) None, never an interpolation."""
    ts = np.asarray(tab["timesteps"], dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 3 or sums.shape[0] != len(ts) or sums.shape[2] != 3:
        raise ValueError(f"bound_from_sums: sums of shape {sums.shape} for {len(ts)} timesteps")
    terms = tab["w"][ts][:, None] * sums[:, :, 0]
    if ts[0] == 0:
        terms[0] += D * tab["decoder_const"]
    prior = 0.5 * (tab["prior_a"] * sums[0, :, 2] + D * tab["prior_c"])
    total = prior + terms.sum(axis=0) if len(ts) == len(tab["w"]) else None
    return dict(timesteps=ts, terms=terms, eps_mse=sums[:, :, 1] / D, prior=prior, total=total,
                nats_per_dim=None if total is None else float(total.mean() / D),
                bits_per_dim=None if total is None else float(total.mean() / (D * np.log(2.0))), var_0=tab["var_0"])


# ------------------------------------------------------------------ analytic (optimal) reverse variance
ANALYTIC_MODES = ("none", "scalar", "element")


def analytic_moment_tables(betas: np.ndarray, timesteps, prediction="eps"):
    """Tables of the walk that estimates g_t = E[eps_hat^2] (Bao et al. 2022) at ``timesteps`` (any order; walked ascending):
    float32 [T][4] rows (A, B, 0, 0) with eps_hat = A x_t + B out, the network's output ``out`` in eps units, and int32
    ``next_t`` [T] (-1 after the last timestep and off the walk).  With x0 = c0 x_t - c1 out (``x0_coefficients``),
    A = (1 - sqrt(ap) c0) / sqrt(1 - ap) and B = sqrt(ap) c1 / sqrt(1 - ap), taken from their closed forms per kind -- eps
    (0, 1) exactly, x0 (1 / sqrt(1 - ap), -sqrt(ap) / sqrt(1 - ap)), v (sqrt(1 - ap), sqrt(ap)) -- in float64 from the float32
    ``alphas_cumprod``, rounded once: 1 - sqrt(ap) c0 is a cancellation that the rounded table columns would not survive."""
    T = len(betas)
    ts = np.unique(np.asarray(timesteps, dtype=np.int64))
    if len(ts) == 0 or ts[0] < 0 or ts[-1] >= T:
        raise ValueError(f"analytic_moment_tables: timesteps must lie in [0, {T})")
    ap = alphas_cumprod(betas).astype(np.float64)
    bb = 1.0 - ap
    kind = prediction_kind(prediction)
    if kind == 0:
        A, B = np.zeros(T), np.ones(T)
    elif kind == 1:
        A, B = 1.0 / np.sqrt(bb), -np.sqrt(ap) / np.sqrt(bb)
    else:
        A, B = np.sqrt(bb), np.sqrt(ap)
    table = np.zeros((T, 4), dtype=np.float32)
    table[:, 0], table[:, 1] = A, B
    next_t = np.full((T,), -1, dtype=np.int32)
    next_t[ts[:-1]] = ts[1:]
    return np.ascontiguousarray(table), next_t


def _analytic_parts(betas, taus, eta):
    """float64 per iteration of the descending walk ``taus``: lam2 = sigma_eta^2, h (the coefficient of -eps_hat in the step's
    mean), a (the coefficient of x0_hat), and the levels; ap_s := 1 on the last iteration."""
    taus = np.asarray(taus, dtype=np.int64)
    ap = alphas_cumprod(betas).astype(np.float64)
    co = strided_coefficients(betas, taus, eta)
    ap_t = ap[taus]
    ap_s = np.concatenate([ap[taus[1:]], np.ones(1)])
    bb_t, bb_s = 1.0 - ap_t, 1.0 - ap_s
    lam2 = co["sigma"] ** 2
    h = np.sqrt(bb_t * ap_s / ap_t) - np.sqrt(np.maximum(bb_s - lam2, 0.0))
    return dict(lam2=lam2, h=h, a=co["a"], ap_t=ap_t, ap_s=ap_s, bb_t=bb_t, bb_s=bb_s)


def analytic_variance(betas: np.ndarray, taus, eta: float, g, clip: float = 1.0) -> np.ndarray:
    """The optimal state-independent reverse variance of Bao et al. 2022 (Analytic-DPM, Theorem 1 in the notation of
    ``strided_coefficients``), float64, one entry per iteration of the descending walk ``taus``:

      sig2 = lam^2 + h^2 (1 - g),  lam = sigma_eta,  h = sqrt(bb_t ap_s / ap_t) - sqrt(max(bb_s - lam^2, 0))

    ``g`` [K] (scalar mode: one variance per iteration) or [K][...] (element mode: one per element), row j the statistic
    E[eps_hat^2] at taus[j], clipped here to [0, 1] (Theorem 2).  A finite ``clip`` (data in [-clip, clip]) also caps the result
    at lam^2 + a^2 clip^2, a = sqrt(ap_s) - sqrt(max(bb_s - lam^2, 0)) sqrt(ap_t / bb_t).  The last iteration keeps 0, as
    every walk here ends without noise.  The mean of the step is not touched."""
    p = _analytic_parts(betas, taus, eta)
    K = len(p["lam2"])
    g = np.clip(np.asarray(g, dtype=np.float64), 0.0, 1.0)
    if g.ndim < 1 or g.shape[0] != K:
        raise ValueError(f"analytic_variance: g of shape {g.shape} for a walk of {K} iterations")
    if not float(clip) > 0:
        raise ValueError(f"analytic_variance: clip={clip} must be positive (inf: no cap)")
    ex = (slice(None),) + (None,) * (g.ndim - 1)
    lam2, h, a = p["lam2"][ex], p["h"][ex], p["a"][ex]
    sig2 = lam2 + h ** 2 * (1.0 - g)
    if np.isfinite(clip):
        sig2 = np.minimum(sig2, lam2 + a ** 2 * float(clip) ** 2)
    sig2[-1] = 0.0
    return sig2


def analytic_sigma_table(betas: np.ndarray, taus, eta: float, g, clip: float = 1.0) -> np.ndarray:
    """float32 sqrt(``analytic_variance``) of the same arguments: for ``g`` [K][S][C] the [K][S][C] table of
    smd_engine_analytic_step (row = the plan's iteration), for ``g`` [K] the [K] values of the strided table's sigma column."""
    return np.ascontiguousarray(np.sqrt(analytic_variance(betas, taus, eta, g, clip)).astype(np.float32))


def analytic_scalar_g(g) -> np.ndarray:
    """Scalar mode's statistic: the mean of g [K][...] over everything but the iteration axis."""
    g = np.asarray(g, dtype=np.float64)
    return g.reshape(g.shape[0], -1).mean(axis=1) if g.ndim > 1 else g


def analytic_bound_from_sums(tab: dict, sums: np.ndarray, D: int, g, taus, betas) -> dict:
    """The bound of the chain that walks ``taus`` (descending, ending at timestep 0) at eta = 1 with the SCALAR optimal variance:
    ``tab`` = ``bound_tables(betas, ...)`` of the same timesteps and schedule, ``sums`` [K][N][3] as for ``bound_from_sums`` (rows ascending in t),
    ``g`` [K] in the order of ``taus``.  Every transition t -> s with t >= 1 is the KL divergence of two Gaussians of variance
    lam^2 (the posterior) and sig2 (the model):

      L_(t->s) = a^2 q_t / (2 sig2) + (D / 2) (log(sig2 / lam^2) + lam^2 / sig2 - 1)

    a, lam of ``strided_coefficients(betas, taus, 1)``, q_t = sum (x0 - x0_hat)^2; the decoder term L_0 (variance var_0 = bt_1)
    and the prior keep the conventions of ``bound_from_sums``.  This is a bound of the K-step chain itself, so ``total`` is a number for every
    K (for K = T it is the every-timestep bound with the optimal variances: a = mu1, lam^2 = bt).  g = 1 gives sig2 = lam^2 and
    the terms of ``bound_from_sums``.  No clip cap is applied (``clip`` = inf): the cap belongs to the sampler."""
    ts = np.asarray(tab["timesteps"], dtype=np.int64)
    taus = np.asarray(taus, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 3 or sums.shape[0] != len(ts) or sums.shape[2] != 3:
        raise ValueError(f"analytic_bound_from_sums: sums of shape {sums.shape} for {len(ts)} timesteps")
    if len(taus) != len(ts) or np.any(taus[::-1] != ts) or ts[0] != 0 or ts[-1] != len(tab["w"]) - 1:
        raise ValueError("analytic_bound_from_sums: taus must be the table's timesteps, descending from T - 1 to 0")
    g = np.asarray(g, dtype=np.float64)
    if g.shape != (len(taus),):
        raise ValueError(f"analytic_bound_from_sums: g of shape {g.shape} (scalar mode: one value per iteration) for {len(taus)} iterations")
    if len(betas) != len(tab["w"]):
        raise ValueError(f"analytic_bound_from_sums: {len(betas)} betas for tables of {len(tab['w'])} timesteps")
    K = len(ts)
    if K == len(tab["w"]):
        # every timestep: a = mu1 and lam^2 = bt as bound_tables forms them, from the float32 betas (the ratios of the float32
        # cumulative product are those betas only to 1e-7 / beta), and h^2 = beta^2 / (alpha bb), the same identity
        b64 = np.asarray(betas, dtype=np.float32).astype(np.float64)[taus]
        ap = alphas_cumprod(betas).astype(np.float64)
        ap_t, ap_s = ap[taus], np.concatenate([ap[taus[1:]], np.ones(1)])
        lam2 = b64 * (1 - ap_s) / (1 - ap_t)
        p = dict(lam2=lam2, a=b64 * np.sqrt(ap_s) / (1 - ap_t))
        sig2 = lam2 + b64 ** 2 / ((1 - b64) * (1 - ap_t)) * (1.0 - np.clip(g, 0.0, 1.0))
    else:
        p = _analytic_parts(betas, taus, 1.0)
        sig2 = analytic_variance(betas, taus, 1.0, g, clip=np.inf)
    terms = np.empty((K, sums.shape[1]), dtype=np.float64)
    ratio = np.ones(K)
    for j in range(K - 1):                      # iteration j: taus[j] -> taus[j + 1], taus[j] >= 1; row of sums K - 1 - j
        r = K - 1 - j
        lam2, s2 = p["lam2"][j], sig2[j]
        ratio[r] = s2 / lam2
        terms[r] = p["a"][j] ** 2 * sums[r, :, 0] / (2 * s2) + 0.5 * D * (np.log(s2 / lam2) + lam2 / s2 - 1.0)
    terms[0] = sums[0, :, 0] / (2 * tab["var_0"]) + D * tab["decoder_const"]
    prior = 0.5 * (tab["prior_a"] * sums[0, :, 2] + D * tab["prior_c"])
    total = prior + terms.sum(axis=0)
    return dict(timesteps=ts, terms=terms, prior=prior, total=total, sigma2_ratio=ratio,
                nats_per_dim=float(total.mean() / D), bits_per_dim=float(total.mean() / (D * np.log(2.0))), var_0=tab["var_0"])
