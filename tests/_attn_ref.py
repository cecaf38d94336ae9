"""Element-wise criterion for the attention kernels (S = 32 tokens per sample): float64 reference, derived bounds, softmax regimes
that can be analysed exactly, selector weights for the fused entries and planted faults.  NumPy / torch float64 only, no GPU.

Per (sample, head), q, k, v [32][d] bf16, scale = d^-1/2:
    s = scale q k^T;  p = softmax_j(s);  o = p v
    dp = dO v^T;  dot_i = sum_j p_ij dp_ij;  dS = p (dp - dot);  dq = scale dS k;  dk = scale dS^T q;  dv = p^T dO      (closed form)

Rounding points of the three families ("kind"):
    "fused"   attn_block_fwd / attn_block_bwd(_ln) (encoder_fused.hip): matrix-core products with fp32 accumulation; the forward's
              logits are built from qs = bf16(fp32(q) * fp32(scale)) (``forward(..., qs_bf16=True)`` takes that as its INPUT, so the
              second rounding of q is not an error of the softmax stage; ``delta_p_fwd_bwd`` measures what it costs), the backward's
              from q with scale applied to the fp32 logits; p and dS are rounded to bf16 in front of P V, dS k, dS^T q, p^T dO;
              o, dq, dk, dv are bf16 stores.
    "plain"   attention_fwd / attention_bwd (attention.hip): fp32 VALU throughout, q scaled in fp32, only the outputs are bf16.
    "f32"     attention_f32 (net_f32.hip): fp32 in, fp32 out, no bf16 anywhere.

Bound.  u = 2^-24.  A bf16 store is round-to-nearest: its error is at most HALF THE SPACING of bf16 at the stored value,
hulp(x) = 2^(floor(log2 |x|) - 8), which lies between 2^-9 |x| (top of a binade) and 2^-8 |x| (bottom).  2^-9 |x| for every x is
not a bound a correct kernel can meet: 1 + 2^-8 is stored as 1 (tests/test_attn_ref_host.py holds the example), so hulp is used:
the tightest statement that is true.  An fp32 operation costs u |result|; a sum of n products on the matrix cores 2 (n + 2) u
sum |terms| (any order, a truncating adder allowed, as in _nt_ref).

  logits  es_ij = 2 (d + 2) u A_ij,  A = scale |q| |k|^T  (+ one bf16 step of qs times |k| where fp32(q) * fp32(scale) is within
          QS_ULPS fp32 ulps of a bf16 rounding boundary: rsqrtf is not specified to round correctly, d = 8 and 32 only)
  exp     x = s - max is formed in fp32 (u |x|) and exp(x) evaluated as exp2(x log2e): the constant and the product each move the
          ARGUMENT by u |x log2e|, i.e. the result by u |x| relatively; the exp2 instruction is documented at 1 ulp = 2 u:
          e_exp(x) = (3 |x| + 2) u -- it grows with |s - max|, which is why a sharp softmax needs its own test
  p       softmax is invariant under a common shift, so only eps_ij = es_ij + e_exp_ij matters, once directly and once through
          the denominator (a p-weighted mean, ebar_i), + 32 additions, the division and the product:
          |dp_ij| <= p_ij expm1(eps_ij + ebar_i + 35 u) + floor  [+ hulp(p) when p is rounded to bf16]
          The backward's second softmax exp(sn scale - max) / sum, rebuilt from the first one's max and sum, has the same form.
  o       |do_ic| <= sum_j |dp_ij| |v_jc| + 2 (32 + 2) u sum_j p_ij |v_jc|   [+ hulp(o) for a bf16 store]
  dS      dp, dot carry edp = 2 (d + 2) u |dO| |v|^T (+ the uncertainty of dO, when dO is itself a rounded result) and
          edot_i = sum_j (|dp_ij| ... ) below; t = dp - dot CANCELS: its absolute error edp + edot + u |t| does not shrink with t.
          |ddS| <= |dp| |t| + p (edp + edot + u |t|) + u |dS|   [+ hulp(dS)]
  dq, dk  scale (sum |ddS| |k| + 2 (32 + 2) u sum |dS| |k|) + u |dq| + hulp(dq);   dv: sum |dp| |dO| + 68 u sum p |dO| + hulp(dv)
Nothing is fitted to GPU output.
"""
import math

import torch

U = 2.0 ** -24
FLOOR = 2.0 ** -126
S = 32
QS_ULPS = 4
F64 = torch.float64
OLD_FWD_REL, OLD_BWD_REL = 6e-3, 1e-2      # the loosest whole-matrix thresholds of tests/test_gpu_kernels.py on o and on dqkv


def bf(x):
    return x.float().to(torch.bfloat16)


def hulp(x):
    """half the spacing of bf16 at |x| (float64 tensor): the largest error of a round-to-nearest bf16 store of x"""
    x = torch.as_tensor(x, dtype=F64).abs().clamp_min(FLOOR)
    _, e = torch.frexp(x)                                  # x = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e - 9)


def worst_ratio(got, ref, bound):
    got, ref, bound = (torch.as_tensor(t).double().cpu() for t in (got, ref, bound))
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def heads(x, H):
    """[rows][E] -> float64 (B, H, 32, d)"""
    rows, E = x.shape
    return x.double().view(rows // S, S, H, E // H).transpose(1, 2)


def unheads(x):
    B, H, _, d = x.shape
    return x.transpose(1, 2).reshape(B * S, H * d)


# ------------------------------------------------------------------------------------------------ reference
def scaled_q(q, d):
    """the fused forward's qs = bf16(fp32(q) * fp32(d^-1/2)), as float64"""
    return bf(q.float() * torch.tensor(d ** -0.5, dtype=torch.float32)).double()


def qs_step(q, d, ulps=QS_ULPS):
    """one bf16 step of qs where fp32(q) * fp32(scale) is within `ulps` fp32 ulps of a bf16 rounding boundary, else 0"""
    if d == 16:
        return torch.zeros_like(q)
    x = (q.float() * torch.tensor(d ** -0.5, dtype=torch.float32)).double()
    b = bf(x).double()
    off = (x - b).abs()
    h = hulp(b)
    dist = torch.minimum((h - off).abs(), (h / 2 - off).abs())          # (below a power of two the spacing halves)
    return torch.where(dist <= ulps * 2.0 ** -23 * x.abs(), 2 * h, torch.zeros_like(x))


def forward(qkv, H, qs_bf16=False):
    E = qkv.shape[1] // 3
    d = E // H
    q, k, v = (heads(qkv[:, i * E:(i + 1) * E], H) for i in range(3))
    qs = scaled_q(q, d) if qs_bf16 else q * d ** -0.5
    s = qs @ k.transpose(-1, -2)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    p = e / e.sum(-1, keepdim=True)
    o = p @ v
    return dict(H=H, d=d, q=q, k=k, v=v, qs=qs, s=s, p=p, o=o, out=unheads(o), A=qs.abs() @ k.abs().transpose(-1, -2),
                qstep=qs_step(q, d) if qs_bf16 else None)


def forward_rounded(qkv, H):
    """the fused forward with its rounding points restated: qs, p and o in bf16 (everything between them exact)"""
    fw = forward(qkv, H, qs_bf16=True)
    pb = bf(fw["p"]).double()
    return bf(unheads(pb @ fw["v"]))


def backward(qkv, dO, H):
    fw = forward(qkv, H)
    sc = fw["d"] ** -0.5
    g = heads(dO, H)
    p, q, k, v = fw["p"], fw["q"], fw["k"], fw["v"]
    dp = g @ v.transpose(-1, -2)
    dot = (p * dp).sum(-1, keepdim=True)
    dS = p * (dp - dot)
    dq, dk, dv = sc * (dS @ k), sc * (dS.transpose(-1, -2) @ q), p.transpose(-1, -2) @ g
    fw.update(g=g, dp=dp, dot=dot, dS=dS, dq=dq, dk=dk, dv=dv, out=torch.cat([unheads(dq), unheads(dk), unheads(dv)], 1))
    return fw


def backward_rounded(qkv, dO, H):
    """the fused backward with its rounding points restated: p and dS in bf16 in front of the products, bf16 outputs"""
    r = backward(qkv, dO, H)
    sc = r["d"] ** -0.5
    pb, dSb = bf(r["p"]).double(), bf(r["dS"]).double()
    dq, dk, dv = sc * (dSb @ r["k"]), sc * (dSb.transpose(-1, -2) @ r["q"]), pb.transpose(-1, -2) @ r["g"]
    return bf(torch.cat([unheads(dq), unheads(dk), unheads(dv)], 1))


# ------------------------------------------------------------------------------------------------ bounds
def exp_err(x):
    return (3.0 * x.abs() + 2.0) * U


def p_err(r, es, round_p):
    s, p = r["s"], r["p"]
    eps = es + exp_err(s - s.max(-1, keepdim=True).values)
    ebar = (p * eps).sum(-1, keepdim=True)
    e = p * torch.expm1(eps + ebar + 35 * U) + FLOOR
    return e + hulp(p + e) if round_p else e


def logit_err(r):
    es = 2 * (r["d"] + 2) * U * r["A"]
    if r.get("qstep") is not None:
        es = es + r["qstep"] @ r["k"].abs().transpose(-1, -2)
    return es


def forward_bound(fw, kind):
    """per element of `fw["out"]`; kind in fused / plain / f32"""
    av = fw["v"].abs()
    e = p_err(fw, logit_err(fw), kind == "fused") @ av + 2 * (S + 2) * U * (fw["p"] @ av)
    if kind != "f32":
        e = e + hulp(fw["o"].abs() + e)
    return unheads(e)


def backward_bound(r, kind, ddO=None):
    """per element of `r["out"]` ([dq | dk | dv]); ddO [rows][E]: uncertainty of dO where it is a rounded result itself"""
    fused = kind == "fused"
    d, p, g = r["d"], r["p"], r["g"]
    sc = d ** -0.5
    aq, ak, av, ag = r["q"].abs(), r["k"].abs(), r["v"].abs(), g.abs()
    T = lambda x: x.transpose(-1, -2)
    ep = p_err(r, logit_err(r), False)
    edp = 2 * (d + 2) * U * (ag @ T(av))
    dg = None
    if ddO is not None:
        dg = heads(ddO, r["H"])
        edp = edp + dg @ T(av)
    adp = r["dp"].abs()
    edot = (ep * adp + p * edp).sum(-1, keepdim=True) + (S + 2) * U * (p * adp).sum(-1, keepdim=True)
    t = (r["dp"] - r["dot"]).abs()
    adS = r["dS"].abs()
    edS = ep * t + p * (edp + edot + U * t) + U * adS
    epp = ep
    if fused:
        edS = edS + hulp(adS + edS)
        epp = ep + hulp(p + ep)
    acc = 2 * (S + 2) * U
    edq = sc * (edS @ ak + acc * (adS @ ak)) + U * r["dq"].abs()
    edk = sc * (T(edS) @ aq + acc * (T(adS) @ aq)) + U * r["dk"].abs()
    edv = T(epp) @ ag + acc * (T(p) @ ag)
    if dg is not None:
        edv = edv + T(p + epp) @ dg
    out = []
    for e, v in ((edq, r["dq"]), (edk, r["dk"]), (edv, r["dv"])):
        out.append(unheads(e + hulp(v.abs() + e)))
    return torch.cat(out, 1)


def gemm_bound(absprod, K, val=None, extra_adds=0, store_bf16=True):
    """C = sum of K bf16 x bf16 products on the matrix cores (+ `extra_adds` fp32 additions on the result `val`), then a bf16 store"""
    e = 2 * (K + 2) * U * absprod
    if val is not None:
        e = e + extra_adds * U * val.abs()
        if store_bf16:
            e = e + hulp(val.abs() + e)
    return e


def ln_fwd_bound(x, gamma, beta, eps=1e-6):
    """bf16(LN(x) gamma + beta) with the statistics as E[x^2] - mean^2 in fp32 (sums of n terms in any order): value, bound"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    n = x.shape[-1]
    m, ex2 = x.mean(-1, keepdim=True), (x * x).mean(-1, keepdim=True)
    dm = (n + 2) * U * x.abs().mean(-1, keepdim=True)
    var = ex2 - m * m + eps
    dvar = (n + 3) * U * ex2 + 2 * m.abs() * dm + 3 * U * (ex2 + m * m)
    rs = var.rsqrt()
    drs = rs * (dvar / (2 * var) + 4 * U)
    c = x - m
    y = c * rs * gamma + beta
    e = (dm + U * c.abs()) * rs * gamma.abs() + c.abs() * drs * gamma.abs() + 3 * U * ((c * rs * gamma).abs() + beta.abs())
    return y, e + hulp(y.abs() + e)


def ln_bwd_bound(x, gamma, parts, res, eps=1e-6):
    """dx = LN-backward((p0 + p1) + (p2 + p3); x, gamma) + res as the 128-wide kernels compute it in fp32, stored as bf16"""
    x, gamma, parts, res = x.double(), gamma.double(), parts.double(), res.double()
    n = x.shape[-1]
    mean = lambda t: t.mean(-1, keepdim=True)
    m, ex2 = mean(x), mean(x * x)
    dm = (n + 2) * U * mean(x.abs())
    var = ex2 - m * m + eps
    dvar = (n + 3) * U * ex2 + 2 * m.abs() * dm + 3 * U * (ex2 + m * m)
    rs = var.rsqrt()
    drs = rs * (dvar / (2 * var) + 4 * U)
    c = x - m
    xh = c * rs
    dxh_ = (dm + U * c.abs()) * rs + c.abs() * drs + U * xh.abs()
    da = parts.sum(0)
    dda = 3 * U * parts.abs().sum(0)
    dxh = da * gamma
    ddxh = dda * gamma.abs() + U * dxh.abs()
    t1, t2 = mean(dxh), mean(dxh * xh)
    dt1 = mean(ddxh) + (n + 2) * U * mean(dxh.abs())
    dt2 = mean(ddxh * xh.abs() + dxh.abs() * dxh_) + (n + 3) * U * mean((dxh * xh).abs())
    inner = dxh - t1 - xh * t2
    dinner = ddxh + dt1 + dxh_ * t2.abs() + xh.abs() * dt2 + 3 * U * (dxh.abs() + t1.abs() + (xh * t2).abs())
    y = rs * inner + res
    e = drs * inner.abs() + rs * dinner + 2 * U * ((rs * inner).abs() + res.abs())
    return y, e + hulp(y.abs() + e)


def delta_p_fwd_bwd(qkv, H):
    """max |p(qs as the fused forward builds it) - p(scale applied to the fp32 logits, as the backward does)|, both in float64"""
    return float((forward(qkv, H, qs_bf16=True)["p"] - forward(qkv, H)["p"]).abs().max())


# ------------------------------------------------------------------------------------------------ regimes
HEAD_REGIMES = ("uniform", "sharp8", "sharp30", "offset", "offset100", "ties2", "ties32", "routing")
REGIMES = HEAD_REGIMES + ("mixed",)
PI = [(5 * i + 3) % S for i in range(S)]                   # routing: query i selects key PI[i]
ROUTING_GAP = 18.0                                         # 31 e^-18 = 4.7e-7 << 2^-9 / 62: o_i = v_PI(i) to bf16


def _zs(x):
    return x - x.mean(-1, keepdim=True)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _keys(d, g, pool=1024):
    """32 well separated directions (greedy farthest point out of a random pool) on the radius-sqrt(d) sphere of the zero-sum
    subspace: with equal norms the matching key q_i = a k_PI(i) has the largest logit of its row for any a > 0"""
    c = _zs(_randn(g, pool, d))
    c = c / c.norm(dim=-1, keepdim=True)
    idx = [0]
    best = c @ c[0]
    for _ in range(S - 1):
        j = int(best.argmin())
        idx.append(j)
        best = torch.maximum(best, c @ c[j])
    return c[idx] * math.sqrt(d)


def _select(d, g, spread=None, gap=None):
    K = _keys(d, g)
    G = K[PI] @ K.T / math.sqrt(d)
    if spread is not None:
        a = spread / float((G.max(1).values - G.min(1).values).median())
    else:
        Gm = G.clone()
        Gm[torch.arange(S), PI] = -1e30
        a = gap / float((G[torch.arange(S), PI] - Gm.max(1).values).min())
    return a * K[PI], K


def head_regime(name, d, g, sign=1.0):
    """q, k, v, dO [32][d] float64 (not yet rounded) of one head"""
    v, dO = _randn(g, S, d), 0.5 * _randn(g, S, d)
    if name == "uniform":
        q, k, v = 0.8 * _randn(g, S, d), 0.8 * _randn(g, S, d), 0.8 * v
    elif name in ("sharp8", "sharp30"):
        q, k = _select(d, g, spread=8.0 if name == "sharp8" else 30.0)
    elif name in ("offset", "offset100"):
        # every logit of the sample near +L or -L (the sign goes with the sample), spread about 1.  fp32 exp overflows above 88.7 and
        # flushes to zero below -87.3: at L = 80 a softmax without the max subtraction is merely less accurate, at L = 100 it is
        # inf / inf or 0 / 0 -- the list carries both
        c = math.sqrt((80.0 if name == "offset" else 100.0) / math.sqrt(d))
        alt = torch.tensor([1.0, -1.0] * (d // 2), dtype=F64)
        k = c * alt + 0.25 / c * _zs(_randn(g, S, d))
        q = sign * c * alt + 0.25 / c * _zs(_randn(g, S, d))
    elif name in ("ties2", "ties32"):
        u = _keys(d, g, pool=64)[0]
        if name == "ties32":
            q, k = _zs(_randn(g, S, d)), u.expand(S, d).clone()
        else:
            q = 24.0 / math.sqrt(d) * u + 0.05 * _zs(_randn(g, S, d))
            k = -u + 0.05 * _zs(_randn(g, S, d))
            k[0] = k[1] = u
    elif name == "routing":
        q, k = _select(d, g, gap=ROUTING_GAP)
        j, c = torch.arange(S, dtype=F64)[:, None], torch.arange(d, dtype=F64)[None, :]
        v = 2 * ((j * (c + 3) + c) % 16) - 15
        v[:, 0] = 2 * j[:, 0] - 31                         # odd integers: exact in bf16, rows pairwise distinct, no zeros
    else:
        raise KeyError(name)
    return q, k, v, dO


def head_names(name, H, b=0):
    return [HEAD_REGIMES[(h + 3 * b) % len(HEAD_REGIMES)] if name == "mixed" else name for h in range(H)]


def regime(name, H, d, seed=0, b=0):
    """one sample: qkv [32][3 H d] bf16, dO [32][H d] bf16.  `b` (sample index): the sign of offset, the rotation of mixed"""
    g = torch.Generator().manual_seed(1000 * seed + 17 * H + d + 101 * b)
    parts = [head_regime(n, d, g, 1.0 if b % 2 == 0 else -1.0) for n in head_names(name, H, b)]
    q, k, v, dO = (torch.cat([p[i] for p in parts], 1) for i in range(4))
    return bf(torch.cat([q, k, v], 1)), bf(dO)


_ROWS = {}


def make_rows(name, H, d, B, seed=0):
    key = (name, H, d, B, seed)
    if key not in _ROWS:
        s = [regime(name, H, d, seed, b) for b in range(B)]
        _ROWS[key] = (torch.cat([x[0] for x in s]), torch.cat([x[1] for x in s]))
    return _ROWS[key]


# ------------------------------------------------------------------------------------------------ selector weights
def signed_perm(n, g, perm=None):
    """W [in n][out n] with W[perm[f]][f] = +-1: x W picks x[perm[f]] into column f, exactly"""
    perm = torch.randperm(n, generator=g) if perm is None else perm
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    W = torch.zeros(n, n, dtype=F64)
    W[perm, torch.arange(n)] = sign
    return W


def selector_weights(seed, sq=1.0, sk=1.0, paired=False):
    """(Wqkv [128 in][384 out], Wo [128 in][128 out]) bf16: Wqkv = [sq Pq | sk Pk | Pv], Wo = Po, signed permutations.
    paired: Pq keeps each half of the stream in place (Pq(f + 64) = Pq(f) + 64) and Pk reads the OTHER half with the same signs,
    so that a1 = [A | B] gives heads 0 .. H/2-1 q = A, k = B and the other heads q = B, k = A (fused_targets)."""
    g = torch.Generator().manual_seed(seed)
    E = 128
    if paired:
        Pq = torch.zeros(E, E, dtype=F64)
        f = torch.arange(E)
        sign = (torch.randint(0, 2, (E // 2,), generator=g).double() * 2 - 1).repeat(2)
        Pq[f, f] = sign
        Pk = torch.zeros(E, E, dtype=F64)
        Pk[(f + E // 2) % E, f] = sign
    else:
        Pq, Pk = signed_perm(E, g), signed_perm(E, g)
    Pv, Po = signed_perm(E, g), signed_perm(E, g)
    return bf(torch.cat([sq * Pq, sk * Pk, Pv], 1)), bf(Po)


def fused_targets(name, H, B, seed=0):
    """h_in [32 B][128] fp32 whose LayerNorm (gamma 1, beta 0) is a1 = [A | B] / sigma with A the queries and B the keys of heads
    0 .. H/2-1 of `name` (every head slice sums to 0 and the rows have about the same norm, so LayerNorm only divides by sigma), and
    sq, the power of two next to sigma^2, which gives the logits their intended size back (with selector_weights(paired=True))."""
    d = 128 // H
    rows = []
    for b in range(B):
        g = torch.Generator().manual_seed(1000 * seed + 31 * H + 7 * b + 5)
        qs, ks = [], []
        for n in head_names(name, H // 2, b):
            q, k, _, _ = head_regime(n, d, g, 1.0 if b % 2 == 0 else -1.0)
            q, k = _zs(q), _zs(k)
            if n == "ties32":
                # the keys of every token must come out of the LayerNorm as the SAME bits, so every row needs the same statistics, yet
                # the tokens must differ (v is a copy of a1 columns: identical rows would make o trivially exact).  q_i = the same
                # magnitudes in (+a, -a) pairs of adjacent columns, the order of each pair drawn per token: every pair sums to
                # exactly 0 and squares to the same value, so mean and variance are the same bits in every row
                a = q[0, 0::2].abs() + 0.25
                sgn = torch.randint(0, 2, (S, d // 2), generator=g).double() * 2 - 1
                q = torch.stack([sgn * a, -sgn * a], -1).reshape(S, d)
            if n == "ties2":
                q[1] = q[0]
            qs.append(q)
            ks.append(k)
        rows.append(torch.cat(qs + ks, 1))
    T = torch.cat(rows)
    var = float(T.var(-1, unbiased=False).mean())
    sq = 2.0 ** round(math.log2(var))
    shift = 0.0 if name in ("ties2", "ties32") else 0.3         # (a shift would make the two members of a pair round differently)
    return (1.7 * T / math.sqrt(var) + shift).float(), sq


# ------------------------------------------------------------------------------------------------ planted faults
def _o_from_p(fw, p, v=None):
    return unheads(p @ (fw["v"] if v is None else v))


def plant_no_max(fw):
    """exp without the max subtraction, in fp32 as the kernel would evaluate it"""
    e = torch.exp(fw["s"].float())
    return _o_from_p(fw, (e / e.sum(-1, keepdim=True)).double())


def plant_keys_swapped(fw):
    """keys 4 and 9 exchanged in the P V pairing of one head of sample 0 (an accumulator-element -> key map off by a term)"""
    p = fw["p"].clone()
    h = fw["H"] // 2
    p[0, h][:, [4, 9]] = p[0, h][:, [9, 4]]
    return _o_from_p(fw, p)


def plant_neighbour_v(fw):
    """head 1 of every sample reads head 0's v"""
    v = fw["v"].clone()
    v[:, 1] = fw["v"][:, 0]
    return _o_from_p(fw, fw["p"], v)


def plant_half_sum(fw):
    """the softmax sum over the lane's own 16 keys only (the cross-half shuffle missing)"""
    s = fw["s"]
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    Z = torch.cat([e[..., :16].sum(-1, keepdim=True).expand(-1, -1, -1, 16), e[..., 16:].sum(-1, keepdim=True).expand(-1, -1, -1, 16)], -1)
    return _o_from_p(fw, e / Z)


def _bwd_out(r, dS, dk_scale=None):
    sc = r["d"] ** -0.5
    dq, dk = sc * (dS @ r["k"]), (sc if dk_scale is None else dk_scale) * (dS.transpose(-1, -2) @ r["q"])
    return torch.cat([unheads(dq), unheads(dk), unheads(r["dv"])], 1)


def plant_half_dot(r):
    """the row dot product of dS over the lane's own 16 keys only"""
    pd = r["p"] * r["dp"]
    dot = torch.cat([pd[..., :16].sum(-1, keepdim=True).expand(-1, -1, -1, 16), pd[..., 16:].sum(-1, keepdim=True).expand(-1, -1, -1, 16)], -1)
    return _bwd_out(r, r["p"] * (r["dp"] - dot))


def plant_dk_unscaled(r):
    return _bwd_out(r, r["dS"], dk_scale=1.0)


def plant_last_sample_from_first(r):
    """the last sample computed from the first sample's rows (a row0 that is not applied); forward or backward result"""
    out = r["out"].clone()
    out[-S:] = out[:S]
    return out


FWD_FAULTS = {"no-max-subtraction": plant_no_max, "pv-keys-swapped": plant_keys_swapped, "neighbour-head-v": plant_neighbour_v,
              "sum-over-one-half": plant_half_sum, "fwd-last-sample-from-first": plant_last_sample_from_first}
BWD_FAULTS = {"dot-over-one-half": plant_half_dot, "dk-scale-dropped": plant_dk_unscaled,
              "bwd-last-sample-from-first": plant_last_sample_from_first}
