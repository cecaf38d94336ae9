"""Element-wise criterion for the optimiser kernels of csrc/optim.hip: float64 model of one optimiser call on flat arrays, the bf16
operand-pack model, derived per-element bounds, regimes that are built exactly, an fp32 emulation of the kernels' arithmetic in two
summation orders, planted faults, and a host model of the engine's parameter layout and of build_opt_tables.  numpy on the CPU only.

The call, as oracle/ddpm_oracle.py defines it (clip_grads, stepped_lr, adam_update, ema_update), every hyper-parameter being the fp32
value the kernel receives (lr0, gamma, beta1, beta2, eps, clip, mu, grad_scale; interval and step are integers):
    S = sum g^2        norm = sqrt(S) grad_scale        gmul = grad_scale (1 if norm < clip else clip / norm)
    lr = lr0 gamma^max(0, ceil(step / interval) - 1)    (the step BEFORE the increment)         t = step + 1
    gk = g gmul    m' = beta1 m + (1 - beta1) gk    v' = beta2 v + (1 - beta2) gk^2
    p' = p - lr (m' / (1 - beta1^t)) / (sqrt(v' / (1 - beta2^t)) + eps)        ema' = mu ema + (1 - mu) p'
    metrics = (norm, min(norm, clip), lr, step)         step' = step + 1
    pack: W[k][n] = Wt[n][k] = bf16_rne(p'[w_off + k N + n]) with leading dimensions ldw = round_up(N, 64), ldwt = round_up(K, 64)
fp32 semantics that float64 does not have are part of the model: where a g^2 or S exceeds the largest fp32 the norm is +inf, so gmul is
grad_scale clip / inf = 0 exactly (the JAX reference computes in fp32 and does the same).  A NaN gradient makes norm, gmul and with them
every parameter NaN; metrics[0] is NaN (nothing is hidden), metrics[1] is clip (NaN < clip is false).

Bound.  U = 2^-24; an fp32 operation costs U |result|; products of two first-order terms are covered by SECOND = 1 + 2^-10.  FL = 2^-126
is added wherever a product can fall below the smallest normal fp32 (flushed to zero or rounded on the denormal grid: at most 2^-126
absolute).  Contraction of a b + c into one fma only removes a rounding, so one bound serves both forms.
  S         every term is >= 0, so the sum is off RELATIVELY by at most depth U, depth = the largest number of roundings a term passes:
            the square (1), the thread's walk (4 per float4 and trip, trips = ceil(n / 4 / (blocks 256))), six shuffle steps and three
            LDS adds per block, then the reduction of the slots (slots / 256 sequential adds, six shuffle steps, three adds), + 2 for the
            head / tail scalars: sum_depth(n, path).  Flushed squares add n FL / S.
  norm      en = depth U / 2 + 2 SQRT_ULP U + U (sqrtf, the product with grad_scale)
  gmul      where norm (1 + en) < clip both the kernel and the model take the unclipped side and gmul = grad_scale EXACTLY (egm = 0);
            otherwise egm = en + 2 DIV_ULP U + U (the function is continuous at norm == clip, so the side taken does not matter).  In a
            regime whose fp32 sum is exact (exact_sum) depth is 0 and the decision is that of the model.  norm == inf: gmul = 0, egm = 0.
  lr        index 0: powf(gamma, 0) = 1 and lr = lr0 exactly; otherwise elr = 2 POW_ULP U + U
  1/(1-b^t) d(b^t) = b^t (2 POW_ULP U + |ln b| |fl(t) - t|)  (the second term: (float)(step + 1) rounds above 2^24, where b^t is 0 for both
            betas, so the derivation covers it);  d(bc) = d(b^t) + U bc: the cancellation -- at t = 1, beta2 = 0.999 one ulp of powf is
            magnified 1000 times, at t = 10^4 not at all: the bound is a function of t.  einv = d(bc) / (bc - d(bc)) + 2 DIV_ULP U.
  gk        dgk = |gk| (egm + U) + FL
  m'        dm = U |b1 m| + ob1 dgk + U |ob1 gk| + U |m'| + FL            (1 - beta is exact in fp32 for beta in [0.5, 1] and beta = 0)
  v'        dv = U b2 v + ob2 (2 |gk| dgk + dgk^2) + 2 U ob2 gk^2 + U v' + FL
  m^, v^    dmh = dm inv1 + |m^| (einv1 + U) + FL;  dvh = dv inv2 + v^ (einv2 + U) + FL
  sqrt      dsq = max(sqrt(v^ + dvh) - sqrt(v^), sqrt(v^) - sqrt(max(v^ - dvh, 0))) + 2 SQRT_ULP U sqrt(v^ + dvh);  den = sqrt(v^) + eps,
            dden = dsq + U (den + dsq)
  update    num = lr m^, dnum = lr dmh + |num| (elr + U) + FL;  upd = num / den,
            dupd = (dnum + |upd| dden) / (den - dden) + 2 DIV_ULP U |upd| + FL
  p'        dp = dupd + hulp32(|p'| + dupd): the final subtraction costs half an fp32 ulp OF p, which dominates where |p| >> lr; p' - p is
            thereby judged against the update's own bound plus that half ulp, never against |p|.
  ema'      dema = U |mu ema| + (1 - mu) dp + U |(1 - mu) p'| + U |ema'| + FL
Assumption (the ROCm installation at hand carries no statement of the device library's accuracy): powf within POW_ULP = 2 ulp, sqrtf and
the division within SQRT_ULP = DIV_ULP = 1 ulp (hipcc rounds both correctly by default: half of that).  DESIGN.md section 22 has the
measured ratios beside the assumption.  Nothing is fitted to GPU output.
"""
import math

import numpy as np

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
FL = 2.0 ** -126
POW_ULP, SQRT_ULP, DIV_ULP = 2.0, 1.0, 1.0
FLT_MAX = float(np.finfo(np.float32).max)
F32, F64 = np.float32, np.float64
OLD_PARAM_REL, OLD_UPDATE_REL = 1e-6, 1e-4       # tests/test_gpu_loss_inputs.py (of |w|, ema too); tests/test_gpu_engine.py (one ratio, of the update)
MAX_NORM_BLOCKS, NORM_SLOTS, NORM_HEAD_SLOTS = 1024, 2048, 1536


def f32(x):
    return float(np.float32(x))


class Hyper:
    """the nine hyper-parameters as the kernel receives them: fp32 values (held as Python floats), an integer interval"""

    def __init__(self, lr0=1e-3, gamma=0.98, interval=10000, beta1=0.9, beta2=0.999, eps=1e-8, clip=1.0, mu=0.999, gs=1.0):
        self.lr0, self.gamma, self.interval = f32(lr0), f32(gamma), int(interval)
        self.beta1, self.beta2, self.eps, self.clip, self.mu, self.gs = f32(beta1), f32(beta2), f32(eps), f32(clip), f32(mu), f32(gs)

    def args(self):
        """positional arguments of Engine.optimizer_step"""
        return (self.lr0, self.gamma, self.interval, self.clip, self.mu, self.gs, self.beta1, self.beta2, self.eps)

    def replace(self, **kw):
        h = Hyper.__new__(Hyper)
        h.__dict__.update(self.__dict__)
        for k, v in kw.items():
            setattr(h, k, int(v) if k == "interval" else f32(v))
        return h


def hulp32(x):
    """half an fp32 ulp at |x| (float64 array in and out; 2^-150 at and below the smallest normal)"""
    x = np.maximum(np.abs(np.asarray(x, dtype=F64)), 2.0 ** -126)
    _, e = np.frexp(x)
    return np.ldexp(1.0, e - 1 - 24)


def lr_index(step, interval):
    return max(0, -(-int(step) // int(interval)) - 1)


# ------------------------------------------------------------------------------------------------ the model (reference and faults)
FAULTS = ("eps-inside-sqrt", "eps-before-bias-correction", "lr-index-off-by-one", "bias-correction-from-step", "grad-scale-once",
          "norm-without-grad-scale", "sumsq-head-dropped", "sumsq-tail-twice", "tile-updated-twice", "pack-transposed-pre-update",
          "ema-mixes-old-parameter", "ema-never-moves", "v-from-unclipped-gradient", "clip-always", "metrics-step-after-increment")
# `<=` in place of `<` at norm == clip is NOT in the list: where(norm <= clip, g, g clip / norm) and where(norm < clip, ...) differ only at
# norm == clip, where clip / norm is exactly 1.0f: the two are the same function, bit for bit (test_optim_ref_host shows it).
EQUIVALENT = ("clip-le",)


def model(s, hp, fault=None, weights=None, twice=None):
    """float64 model of one call on the state s = dict(p, g, m, v, ema or None, step).  `fault` plants one of FAULTS; `weights` (0 / 1 /
    2 per element, the sumsq faults) multiplies g^2 in the norm, `twice` (index array) is updated a second time."""
    p, g, m, v = (np.asarray(s[k], dtype=F64) for k in ("p", "g", "m", "v"))
    step = int(s["step"])
    with np.errstate(all="ignore"):
        q = g * g
        S = float(np.sum(q if weights is None else q * weights))
        over = bool(np.any(q > FLT_MAX)) or S > FLT_MAX
        root = math.inf if over else (math.nan if math.isnan(S) else math.sqrt(S))
        norm = root if fault == "norm-without-grad-scale" else root * hp.gs
        unclipped = norm <= hp.clip if fault == "clip-le" else norm < hp.clip
        if fault == "clip-always":
            unclipped = False
        factor = 1.0 if unclipped else hp.clip / norm
        gmul = factor if fault == "grad-scale-once" else hp.gs * factor
        idx = max(0, step // hp.interval) if fault == "lr-index-off-by-one" else lr_index(step, hp.interval)
        lr = hp.lr0 * hp.gamma ** idx
        t = step if fault == "bias-correction-from-step" else step + 1
        bc1, bc2 = 1.0 - hp.beta1 ** t, 1.0 - hp.beta2 ** t
        ob1, ob2, omu = 1.0 - hp.beta1, 1.0 - hp.beta2, 1.0 - hp.mu

        def elem(p, g, m, v):
            gk = g * gmul
            m1 = hp.beta1 * m + ob1 * gk
            gv = g * hp.gs if fault == "v-from-unclipped-gradient" else gk
            v1 = hp.beta2 * v + ob2 * gv * gv
            if fault == "eps-inside-sqrt":
                den = np.sqrt(v1 / bc2 + hp.eps)
            elif fault == "eps-before-bias-correction":
                den = (np.sqrt(v1) + hp.eps) / math.sqrt(bc2)
            else:
                den = np.sqrt(v1 / bc2) + hp.eps
            return p - lr * (m1 / bc1) / den, m1, v1

        p1, m1, v1 = elem(p, g, m, v)
        if twice is not None:
            p1, m1, v1 = p1.copy(), m1.copy(), v1.copy()
            p1[twice], m1[twice], v1[twice] = elem(p1[twice], g[twice], m1[twice], v1[twice])
        out = dict(p=p1, m=m1, v=v1, ema=None, step=step + 1, S=S, norm=norm, gmul=gmul, lr=lr, idx=idx, t=step + 1, unclipped=unclipped)
        if s.get("ema") is not None:
            e = np.asarray(s["ema"], dtype=F64)
            src = p if fault == "ema-mixes-old-parameter" else p1
            out["ema"] = e.copy() if fault == "ema-never-moves" else e * hp.mu + src * omu
        out["metrics"] = (norm, norm if norm < hp.clip else hp.clip, lr, float(step + 1 if fault == "metrics-step-after-increment" else step))
    return out


# ------------------------------------------------------------------------------------------------ bounds
def norm_blocks_for(n):
    return int(min(max((n // 4 + 255) // 256, 1), MAX_NORM_BLOCKS))


def sum_depth(n, path):
    """roundings on the longest way of one g^2 into S: path "flat" (smd_adam_clip_ema: grad_sumsq_kernel, every block of the update
    reduces the <= 1024 partials) or "slots" (the engine: grad_sumsq_slots_kernel per slice into 2048 fixed slots, opt_prepare_kernel)"""
    if path == "flat":
        blocks, slots = norm_blocks_for(n), norm_blocks_for(n)
    else:
        blocks, slots = NORM_SLOTS - NORM_HEAD_SLOTS, NORM_SLOTS                # the slice with fewer blocks walks further
    trips = -(-max(n // 4, 1) // (blocks * 256))
    return 1 + 4 * trips + 2 + 6 + 3 + -(-slots // 256) + 6 + 3


def bounds(s, hp, ref, depth, exact_sum=False):
    """per-element bounds of p, m, v, ema of the reference ref = model(s, hp), relative bounds of the norm and the LR (en, elr), and
    whether the step counter's conversion is exact.  depth = sum_depth(...); exact_sum: the fp32 sum of squares is exact in any order."""
    p, g, m, v = (np.asarray(s[k], dtype=F64) for k in ("p", "g", "m", "v"))
    n = g.size
    norm, gmul, lr, t = ref["norm"], ref["gmul"], ref["lr"], ref["t"]
    with np.errstate(all="ignore"):
        if math.isinf(norm) or ref["S"] == 0.0:
            en = 0.0
        elif exact_sum:
            en = 0.0
        else:
            en = SECOND * (depth * U / 2 + n * FL / ref["S"] + 2 * SQRT_ULP * U + U)
        if math.isinf(norm) or (norm * (1 + en) < hp.clip):
            egm = 0.0
        else:
            egm = SECOND * (en + 2 * DIV_ULP * U + U)
        elr = 0.0 if ref["idx"] == 0 else SECOND * (2 * POW_ULP * U + U)
        dt = abs(float(np.float32(t)) - t)
        inv, einv = [], []
        for b in (hp.beta1, hp.beta2):
            pw = b ** t
            dpw = pw * (2 * POW_ULP * U + abs(math.log(b)) * dt) if b > 0 else 0.0
            bc = 1.0 - pw
            dbc = dpw + U * bc
            inv.append(1.0 / bc)
            einv.append(SECOND * (dbc / (bc - dbc) + 2 * DIV_ULP * U) if bc > dbc else math.inf)
        ob1, ob2, omu = 1.0 - hp.beta1, 1.0 - hp.beta2, 1.0 - hp.mu
        gk = g * gmul
        dgk = np.abs(gk) * (egm + U) + FL
        m1, v1 = ref["m"], ref["v"]
        dm = SECOND * (U * np.abs(hp.beta1 * m) + ob1 * dgk + U * np.abs(ob1 * gk) + U * np.abs(m1)) + FL
        dv = SECOND * (U * hp.beta2 * v + ob2 * (2 * np.abs(gk) * dgk + dgk * dgk) + 2 * U * ob2 * gk * gk + U * v1) + FL
        mh, vh = m1 * inv[0], v1 * inv[1]
        dmh = SECOND * (dm * inv[0] + np.abs(mh) * (einv[0] + U)) + FL
        dvh = SECOND * (dv * inv[1] + vh * (einv[1] + U)) + FL
        sq = np.sqrt(vh)
        dsq = np.maximum(np.sqrt(vh + dvh) - sq, sq - np.sqrt(np.maximum(vh - dvh, 0.0))) + 2 * SQRT_ULP * U * np.sqrt(vh + dvh)
        den = sq + hp.eps
        dden = dsq + U * (den + dsq)
        num = lr * mh
        dnum = SECOND * (lr * dmh + np.abs(num) * (elr + U)) + FL
        upd = num / den
        room = den - dden
        dupd = np.where(room > 0, SECOND * ((dnum + np.abs(upd) * dden) / np.where(room > 0, room, 1.0) + 2 * DIV_ULP * U * np.abs(upd)) + FL, np.inf)
        p1 = ref["p"]
        dp = dupd + hulp32(np.abs(p1) + dupd)
        B = dict(p=dp, m=dm, v=dv, upd=dupd, en=en, egm=egm, elr=elr, einv=einv, step_exact=dt == 0.0)
        if ref["ema"] is not None:
            e = np.asarray(s["ema"], dtype=F64)
            B["ema"] = SECOND * (U * np.abs(hp.mu * e) + omu * dp + U * np.abs(omu * p1) + U * np.abs(ref["ema"])) + FL
    return B


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite while ref is, or the bound is not finite"""
    got, ref, bound = (np.asarray(a, dtype=F64).ravel() for a in (got, ref, bound))
    if got.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        r = np.abs(got - ref) / np.maximum(bound, 1e-300)
    r = np.where(np.isfinite(got) & np.isfinite(bound), r, np.inf)
    return float(r.max())


def ratios(got, ref, B):
    """{output: worst |err| / bound} over p, m, v and (if present) ema"""
    out = {k: worst_ratio(got[k], ref[k], B[k]) for k in ("p", "m", "v")}
    if ref["ema"] is not None:
        out["ema"] = worst_ratio(got["ema"], ref["ema"], B["ema"])
    return out


# ------------------------------------------------------------------------------------------------ the operand pack
def bf16_bits(x):
    """round-to-nearest-even bf16 of fp32 values, as uint16 bit patterns (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def pack_model(p32, dense, before, fault=None, p_old=None):
    """the operand pack after a call: `before` (uint16 [n_wpack]) with W and Wt of every Dense kernel of `dense` (layout()["dense"])
    rewritten from the fp32 parameters p32; pad columns keep what `before` held"""
    out = np.array(before, dtype=np.uint16, copy=True)
    for d in dense:
        K, N = d["K"], d["N"]
        w = bf16_bits(p32[d["w_off"]:d["w_off"] + K * N]).reshape(K, N)
        out[d["W_off"]:d["W_off"] + K * d["ldw"]].reshape(K, d["ldw"])[:, :N] = w
        if fault == "pack-transposed-pre-update":
            w = bf16_bits(p_old[d["w_off"]:d["w_off"] + K * N]).reshape(K, N)
        out[d["Wt_off"]:d["Wt_off"] + N * d["ldwt"]].reshape(N, d["ldwt"])[:, :K] = w.T
    return out


# ------------------------------------------------------------------------------------------------ layout and work tables
def _up(x, q):
    return (x + q - 1) // q * q


def layout(arch, C, L, K, M, E=128, F=128):
    """SmdEngine::build_layout restated: tensor_table [(name, offset, shape)], head_off (where the output-stage slice begins), n_params,
    n_wpack and the Dense kernels with their pack offsets.  arch "TransformerDDPM" (L encoder layers, K DenseResBlocks) or "DenseDDPM" (L
    blocks; K is ignored, as the engine ignores num_mlp_layers there)."""
    tab, dense = [], []
    off = woff = 0

    def add_dense(name, Kd, Nd):
        nonlocal off, woff
        d = dict(name=name, K=Kd, N=Nd, w_off=off, ldw=_up(Nd, 64), ldwt=_up(Kd, 64))
        tab.append((name + ".kernel", off, (Kd, Nd)))
        off += Kd * Nd
        tab.append((name + ".bias", off, (Nd,)))
        off += Nd
        d["W_off"] = woff
        woff += Kd * d["ldw"]
        d["Wt_off"] = woff
        woff += Nd * d["ldwt"]
        woff = _up(woff, 128)
        dense.append(d)

    def add_ln(name, D):
        nonlocal off
        tab.append((name + ".scale", off, (D,)))
        off += D
        tab.append((name + ".bias", off, (D,)))
        off += D

    if arch == "DenseDDPM":
        add_dense("in_proj", C, M)
        head, nb = off, L
    else:
        add_dense("in_proj", C, E)
        for l in range(L):
            pre = f"enc.{l}"
            add_ln(pre + ".ln1", E)
            add_dense(pre + ".attn.qkv", E, 3 * E)
            add_dense(pre + ".attn.out", E, E)
            add_ln(pre + ".ln2", E)
            add_dense(pre + ".mlp.fc1", E, M)
            add_dense(pre + ".mlp.fc2", M, E)
        head, nb = off, K
        add_ln("ln_f", E)
        add_dense("up", E, M)
    for k in range(nb):
        f, r = f"film.{k}", f"res.{k}"
        add_dense(f + ".fc1", F, 4 * F)
        add_dense(f + ".fc2", 4 * F, 4 * F)
        add_dense(f + ".ss", 4 * F, 2 * M)
        add_ln(r + ".ln1", M)
        add_dense(r + ".fc1", M, M)
        add_ln(r + ".ln2", M)
        add_dense(r + ".fc2", M, M)
    add_ln("ln_o", M)
    add_dense("out_proj", M, C)
    return dict(tensor_table=tab, head_off=head, n_params=off, n_wpack=woff, dense=dense)


FAST, EDGE, FLAT = 0, 1, 2
OPT_DENSE_MAX, OPT_FLAT_MAX = 60, 64


def opt_tables(lay):
    """SmdEngine::build_opt_tables restated from DESIGN.md section 6 and the comments of csrc/optim.hip: two slices (stem [0, head_off),
    output stage [head_off, n_params)); in each, every Dense kernel as 64 x 64 tiles (a workgroup per tile; a full tile of a kernel whose
    offsets, row length and pack leading dimensions are all multiples of 4 elements takes the vector path, every other tile goes element
    by element), then everything between two kernels (biases, LayerNorm scale / bias) as flat runs cut into 1024-element workgroups.
    Returns, per slice: blocks [(form, index array)] in workgroup order, and the head scalars / tail of its norm pass (the scalars in
    front of the first 16-byte boundary and behind the last whole float4; the buffers are 256-byte aligned, so alignment is that of the
    offset); and `form` [n_params] (FAST / EDGE / FLAT) with `count` [n_params], how many workgroups own each element."""
    n = lay["n_params"]
    form = np.full(n, -1, dtype=np.int8)
    count = np.zeros(n, dtype=np.int32)
    parts = []
    for lo, hi in ((0, lay["head_off"]), (lay["head_off"], n)):
        blocks, cur, runs = [], lo, []
        ds = [d for d in lay["dense"] if lo <= d["w_off"] < hi]
        for d in ds:
            K, N = d["K"], d["N"]
            aligned = ((d["w_off"] | N | d["W_off"] | d["ldw"] | d["Wt_off"] | d["ldwt"]) & 3) == 0
            for k0 in range(0, K, 64):
                for n0 in range(0, N, 64):
                    kk, nn = np.arange(k0, min(k0 + 64, K)), np.arange(n0, min(n0 + 64, N))
                    idx = (d["w_off"] + kk[:, None] * N + nn[None, :]).ravel()
                    blocks.append((FAST if aligned and k0 + 64 <= K and n0 + 64 <= N else EDGE, idx))
            runs.append((cur, d["w_off"]))
            cur = d["w_off"] + K * N
        runs.append((cur, hi))
        n_dense_blocks = len(blocks)
        flats = [(a, b) for a, b in runs if b > a]
        for a, b in flats:
            for c in range(a, b, 1024):
                blocks.append((FLAT, np.arange(c, min(c + 1024, b))))
        for kind, idx in blocks:
            form[idx] = kind
            np.add.at(count, idx, 1)
        h = min((4 - (lo & 3)) & 3, hi - lo)
        tail = (hi - lo - h) % 4
        parts.append(dict(lo=lo, hi=hi, blocks=blocks, n_dense_blocks=n_dense_blocks, flats=flats, n_dense=len(ds),
                          head=np.arange(lo, lo + h), tail=np.arange(hi - tail, hi)))
    fused = all(p["n_dense"] <= OPT_DENSE_MAX and len(p["flats"]) <= OPT_FLAT_MAX for p in parts)
    return dict(parts=parts, form=form, count=count, fused=fused)


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def _butterfly(v):
    """xor-shuffle all-reduce over the last axis (64 lanes), as wave_sum: every lane ends with the same bits"""
    idx = np.arange(v.shape[-1])
    o = v.shape[-1] // 2
    while o:
        v = v + v[..., idx ^ o]
        o //= 2
    return v[..., 0]


def _block_sums(g, blocks, head, tail_lane0):
    """partial[b] of grad_sumsq_kernel (head = 0, tail on threads 0..) / grad_sumsq_slots_kernel (head scalars on threads 0.., tail on
    threads 64..) over the fp32 array g: float4 trips in grid-stride order, (x x + y y + z z) + w w left to right, block 0 takes the scalars"""
    g = np.asarray(g, dtype=F32)
    n = g.size
    h = min(head, n)
    n4 = (n - h) // 4
    per = blocks * 256
    trips = -(-n4 // per) if n4 else 0
    body = np.zeros(trips * per * 4, dtype=F32)
    body[:n4 * 4] = g[h:h + n4 * 4]
    q = (body * body).reshape(trips, blocks, 256, 4)
    acc = np.zeros((blocks, 256), dtype=F32)
    for j in range(trips):
        acc = acc + (((q[j, :, :, 0] + q[j, :, :, 1]) + q[j, :, :, 2]) + q[j, :, :, 3])
    for i in range(h):
        acc[0, i] = acc[0, i] + g[i] * g[i]
    for i in range(n - h - n4 * 4):
        acc[0, tail_lane0 + i] = acc[0, tail_lane0 + i] + g[h + n4 * 4 + i] * g[h + n4 * 4 + i]
    w = _butterfly(acc.reshape(blocks, 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _reduce_slots(partial):
    """the one-workgroup sum of the partials (adam_clip_ema_kernel's prologue, opt_prepare_kernel): thread t adds slots t, t + 256, ..."""
    n = partial.size
    pad = np.zeros(_up(n, 256), dtype=F32)
    pad[:n] = partial
    acc = np.zeros(256, dtype=F32)
    for row in pad.reshape(-1, 256):
        acc = acc + row
    w = _butterfly(acc.reshape(4, 64))
    return F32(((w[0] + w[1]) + w[2]) + w[3])


def emu_sumsq(g, order, head_off=0):
    """fp32 sum of squares in the order of `order`: "flat" (smd_adam_clip_ema) or "slots" (the engine: the output-stage slice
    [head_off, n) into slots 0..1535, the stem slice into slots 1536..2047, one workgroup over all 2048)"""
    g = np.asarray(g, dtype=F32)
    with np.errstate(all="ignore"):
        if order == "flat":
            return _reduce_slots(_block_sums(g, norm_blocks_for(g.size), 0, 0))
        part = np.zeros(NORM_SLOTS, dtype=F32)
        if g.size > head_off:
            part[:NORM_HEAD_SLOTS] = _block_sums(g[head_off:], NORM_HEAD_SLOTS, (4 - (head_off & 3)) & 3, 64)
        if head_off:
            part[NORM_HEAD_SLOTS:] = _block_sums(g[:head_off], NORM_SLOTS - NORM_HEAD_SLOTS, 0, 64)
        return _reduce_slots(part)


def _fma(a, b, c):
    return (np.asarray(a, dtype=F64) * np.asarray(b, dtype=F64) + np.asarray(c, dtype=F64)).astype(F32)


def emu(s, hp, order="flat", head_off=0, fma=False):
    """the kernels' arithmetic in numpy float32, statement by statement (adam_elem, opt_prepare_kernel / adam_clip_ema_kernel);
    fma: a b + c contracted the way the compiler may"""
    f = F32
    p, g, m, v = (np.asarray(s[k], dtype=F32) for k in ("p", "g", "m", "v"))
    step = int(s["step"])
    with np.errstate(all="ignore"):
        norm = np.sqrt(emu_sumsq(g, order, head_off)) * f(hp.gs)
        gmul = f(hp.gs) * (f(1.0) if norm < f(hp.clip) else f(hp.clip) / norm)
        idx = lr_index(step, hp.interval)
        lr = f(hp.lr0) * np.power(f(hp.gamma), f(idx))
        tt = f(step + 1)
        bc1, bc2 = f(1.0) - np.power(f(hp.beta1), tt), f(1.0) - np.power(f(hp.beta2), tt)
        inv1, inv2 = f(1.0) / bc1, f(1.0) / bc2
        ob1, ob2, omu = f(1.0) - f(hp.beta1), f(1.0) - f(hp.beta2), f(1.0) - f(hp.mu)
        gk = g * gmul
        if fma:
            m1 = _fma(f(hp.beta1), m, ob1 * gk)
            v1 = _fma(f(hp.beta2), v, ob2 * gk * gk)
        else:
            m1 = f(hp.beta1) * m + ob1 * gk
            v1 = f(hp.beta2) * v + ob2 * gk * gk
        p1 = p - lr * (m1 * inv1) / (np.sqrt(v1 * inv2) + f(hp.eps))
        out = dict(p=p1, m=m1, v=v1, ema=None, step=step + 1,
                   metrics=(float(norm), float(norm if norm < f(hp.clip) else f(hp.clip)), float(lr), float(f(step))), gmul=float(gmul))
        if s.get("ema") is not None:
            e = np.asarray(s["ema"], dtype=F32)
            out["ema"] = _fma(e, f(hp.mu), p1 * omu) if fma else e * f(hp.mu) + p1 * omu
    return out


# ------------------------------------------------------------------------------------------------ regimes (built exactly, not drawn)
def _frac(i, a):
    return (i.astype(F64) * a) % 1.0


def base_state(n, step=0, ema=True):
    """a state that differs at every index: |p| in (0.05, 1.05) with both signs, ema != p, m of both signs around 1e-3, v around 1e-6,
    g around 0.01 with both signs (no two neighbouring elements alike)"""
    i = np.arange(n)
    sgn = np.where((i * 7 // 3) % 2 == 0, 1.0, -1.0)
    p = (sgn * (0.05 + _frac(i, 0.6180339887498949))).astype(F32)
    g = (np.where(i % 3 == 0, -1.0, 1.0) * 0.01 * (0.25 + _frac(i, 0.7548776662466927))).astype(F32)
    m = (np.where(i % 5 < 2, -1.0, 1.0) * 1e-3 * (0.5 + _frac(i, 0.5698402909980532))).astype(F32)
    v = (1e-6 * (0.5 + _frac(i, 0.8191725133961645))).astype(F32)
    e = (0.5 * p.astype(F64) + 0.25 * np.where(i % 2 == 0, 1.0, -1.0)).astype(F32)
    return dict(p=p, g=g, m=m, v=v, ema=e if ema else None, step=int(step))


MAGS = (1e-12, 1e-11, 1e-10, 1e-9, 3e-9, 1e-8, 3e-8, 1e-7, 1e-6, 1e-4, 1e-2, 1.0, 1e2, 1e4)
STEPS4 = (0, 1, 2, 3, 4, 5, 8)                                            # interval 4: interval - 1, interval, interval + 1, 2 interval
STEPS_CFG = (0, 1, 2, 9999, 10000, 10001, 20000, 10 ** 6, 2 ** 24, 2 ** 24 + 1)       # the configuration's 10000 / 0.98; 2^24: step + 1 rounds
HP0 = Hyper(clip=1e9)                                                      # clip out of the way unless the regime is about it


def magnitude_state(n, planted_v, step):
    """element i: |g| = MAGS[i % 14] (exact zero where i % 29 == 28), sign by i % 3, against m of either sign (and m = 0 where
    i % 11 == 0), v fixed at planted_v (1e-16: sqrt(v^) meets eps = 1e-8; 0: the first step's v^ = g^2)"""
    s = base_state(n, step)
    i = np.arange(n)
    g = np.asarray(MAGS, dtype=F64)[i % len(MAGS)] * np.where(i % 3 == 0, -1.0, 1.0)
    g[i % 29 == 28] = 0.0
    s["g"] = g.astype(F32)
    s["v"] = np.full(n, planted_v, dtype=F32)
    s["m"] = np.where(i % 11 == 0, 0.0, s["m"] * 1e-3).astype(F32)
    return s


def exact_norm_state(n, step=0):
    """g = +-2^-12 at r^2 elements (r = floor(sqrt(n))), 0 at the others, spread evenly: every partial sum of squares is an integer
    multiple of 2^-24 below 2^24 of them, so the fp32 sum is exact in ANY order, and sqrtf of r^2 2^-24 is r 2^-12 exactly.
    Returns (state, norm)."""
    s = base_state(n, step)
    r = int(math.isqrt(n))
    assert r >= 1 and n < 2 ** 24
    i = np.arange(n)
    keep = (i * (r * r)) // n != ((i - 1) * (r * r)) // n                   # exactly r^2 True values, evenly spread (i = 0 included)
    assert int(keep.sum()) == r * r
    s["g"] = np.where(keep, np.where(i % 3 == 0, -1.0, 1.0) * 2.0 ** -12, 0.0).astype(F32)
    return s, r * 2.0 ** -12


def regimes(n, group):
    """[(name, state, Hyper, exact_sum)] of one group: "magnitude", "norm", "step4", "stepcfg", "scale", "ema" """
    out = []
    if group == "magnitude":
        for pv, step in ((1e-16, 999), (0.0, 0)):
            for clip in (1e9, 1.0):
                out.append((f"|g| 1e-12..1e4, v={pv:g}, step {step}, clip {clip:g}", magnitude_state(n, pv, step), Hyper(clip=clip), False))
        s = base_state(n, 5)
        s["g"] = np.zeros(n, dtype=F32)
        s["m"][::2] = 0.0
        s["v"][::2] = 0.0
        out.append(("g = 0 with zero and non-zero moments", s, HP0, True))
    elif group == "norm":
        s, norm = exact_norm_state(n, 3)
        up, dn = float(np.nextafter(F32(norm), F32(np.inf))), float(np.nextafter(F32(norm), F32(0)))
        for name, clip in (("below clip", 4 * norm), ("norm == clip", norm), ("norm one ulp below clip", up), ("norm one ulp above clip", dn),
                           ("far above clip", norm / 64)):
            out.append((name, s, Hyper(clip=clip), True))
        z = base_state(n, 3)
        z["g"] = np.zeros(n, dtype=F32)
        out.append(("all-zero gradient", z, Hyper(clip=1.0), True))
        h = base_state(n, 3)
        h["g"][n // 2] = 1e20
        out.append(("one element 1e20: sum of squares inf", h, Hyper(clip=1.0), True))
    elif group == "step4":
        out = [(f"step {k}, interval 4 / 0.5", base_state(n, k), HP0.replace(interval=4, gamma=0.5), False) for k in STEPS4]
    elif group == "stepcfg":
        out = [(f"step {k}, interval 10000 / 0.98", base_state(n, k), HP0, False) for k in STEPS_CFG]
    elif group == "scale":
        s = base_state(n, 7)
        raw = math.sqrt(float(np.sum(s["g"].astype(F64) ** 2)))
        out = [("grad_scale 1", s, Hyper(clip=2 * raw), False),
               ("grad_scale 3: raw norm below clip, scaled above", s, Hyper(clip=2 * raw, gs=3.0), False),
               ("grad_scale 1/8: raw norm above clip, scaled below", s, Hyper(clip=raw / 2, gs=0.125), False)]
    elif group == "ema":
        out = [("mu 0.999", base_state(n, 2), Hyper(), False), ("mu 0", base_state(n, 2), Hyper(mu=0.0), False),
               ("no ema", base_state(n, 2, ema=False), Hyper(), False)]
    else:
        raise KeyError(group)
    return out


GROUPS = ("magnitude", "norm", "step4", "stepcfg", "scale", "ema")
# the smallest engines that reach each form (arch, C, layers, blocks, mlp_dims): ragged in_proj / out_proj with a tail behind the last
# float4 of the output-stage slice; DenseDDPM; and M = 512, where the flat run film.ss.bias + res.ln1 holds 2048 elements
MODELS = {"tr42": ("TransformerDDPM", 42, 1, 1, 256), "tr146": ("TransformerDDPM", 146, 1, 1, 256),
          "dense42": ("DenseDDPM", 42, 1, 1, 256), "dense64": ("DenseDDPM", 64, 1, 1, 512)}


def nan_state(n):
    s = base_state(n, 3)
    s["g"][n // 3] = np.nan
    return s


# ------------------------------------------------------------------------------------------------ planted faults and their regimes
def fault_case(fault, n=4099):
    """(state, Hyper, exact_sum, kwargs of model()) of the named regime in which `fault` must leave the bound"""
    kw = {}
    if fault in ("eps-inside-sqrt",):
        return magnitude_state(n, 1e-16, 999), Hyper(clip=1e9), False, kw
    if fault == "eps-before-bias-correction":
        return magnitude_state(n, 0.0, 0), Hyper(clip=1e9), False, kw
    if fault == "lr-index-off-by-one":
        return base_state(n, 8), HP0.replace(interval=4, gamma=0.5), False, kw
    if fault == "bias-correction-from-step":
        return base_state(n, 2), HP0, False, kw
    if fault == "grad-scale-once":
        s = base_state(n, 7)
        raw = math.sqrt(float(np.sum(s["g"].astype(F64) ** 2)))
        return s, Hyper(clip=2 * raw, gs=0.125), False, kw
    if fault == "norm-without-grad-scale":
        s = base_state(n, 7)
        raw = math.sqrt(float(np.sum(s["g"].astype(F64) ** 2)))
        return s, Hyper(clip=2 * raw, gs=3.0), False, kw
    if fault in ("sumsq-head-dropped", "sumsq-tail-twice"):
        # a slice that begins at offset 5 (three head scalars) and ends three scalars behind a float4: those six carry the norm
        s = base_state(n, 3)
        w = np.ones(n)
        idx = np.arange(0, 3) if fault == "sumsq-head-dropped" else np.arange(n - 3, n)
        s["g"][idx] = 0.5
        w[idx] = 0.0 if fault == "sumsq-head-dropped" else 2.0
        return s, Hyper(clip=0.25), False, dict(weights=w)
    if fault == "tile-updated-twice":
        return base_state(n, 3), Hyper(), False, dict(twice=np.arange(64, 128))
    if fault in ("ema-mixes-old-parameter", "ema-never-moves"):
        return base_state(n, 2), Hyper(), False, kw
    if fault == "v-from-unclipped-gradient":
        s, norm = exact_norm_state(n, 3)
        return s, Hyper(clip=norm / 64), True, kw
    if fault == "clip-always":
        s, norm = exact_norm_state(n, 3)
        return s, Hyper(clip=norm * 4), True, kw
    if fault in ("metrics-step-after-increment", "pack-transposed-pre-update"):
        return base_state(n, 3), Hyper(), False, kw
    if fault == "clip-le":
        s, norm = exact_norm_state(n, 3)
        return s, Hyper(clip=norm), True, kw
    raise KeyError(fault)


def old_thresholds_notice(fault, n=100003, steps=3, seed=6):
    """(params / ema threshold notices, update threshold notices): would rel(params) < 1e-6 and rel(ema) < 1e-6 of the norm of w
    (test_mse_and_adam_entries_match_the_oracle) and the one Frobenius ratio < 1e-4 of the update (test_optimizer_step_matches_oracle)
    see the fault on the draw those tests use -- w ~ N(0, 1), g ~ N(0, 0.01), three steps from step 0, clip 1, grad_scale 1.  The
    deviation is the float64 model with the fault against the one without, so rounding plays no part.  Structural faults get what
    they would hit in a model: 3 head / tail scalars, one 64-element row of a tile."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n)
    g = 0.01 * rng.standard_normal(n)
    hp = Hyper()
    kw = {}
    if fault == "sumsq-head-dropped":
        kw["weights"] = np.ones(n)
        kw["weights"][:3] = 0.0
    elif fault == "sumsq-tail-twice":
        kw["weights"] = np.ones(n)
        kw["weights"][-3:] = 2.0
    elif fault == "tile-updated-twice":
        kw["twice"] = np.arange(64, 128)
    a = dict(p=w.copy(), g=g, m=np.zeros(n), v=np.zeros(n), ema=w.copy(), step=0)
    b = dict(a)
    worst_p = worst_e = worst_u = 0.0
    with np.errstate(all="ignore"):
        for _ in range(steps):
            ra, rb = model(a, hp), model(b, hp, fault, **kw)
            nz = lambda x: float(np.linalg.norm(np.nan_to_num(x, nan=1e30, posinf=1e30, neginf=-1e30)))
            a = dict(p=ra["p"], g=g, m=ra["m"], v=ra["v"], ema=ra["ema"], step=ra["step"])
            b = dict(p=rb["p"], g=g, m=rb["m"], v=rb["v"], ema=rb["ema"], step=rb["step"])
            worst_u = max(worst_u, nz(b["p"] - a["p"]) / nz(a["p"] - w))
            worst_p = max(worst_p, nz(b["p"] - a["p"]) / nz(a["p"]))
            worst_e = max(worst_e, nz(b["ema"] - a["ema"]) / nz(a["ema"]))
    return (worst_p >= OLD_PARAM_REL or worst_e >= OLD_PARAM_REL), worst_u >= OLD_UPDATE_REL
