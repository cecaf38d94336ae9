"""Interleaved A/B of the D = 2048 LayerNorm kernels of the training and sampling steps between csrc/libsmd_hip_old.so (the
previous commit, built by tools/build_old_lib.sh) and the shipped library in one process, 8192 rows: the five instantiations of
the training step (FiLM + swish forward from a bf16 row, plain forward, and the three all-bf16 backward forms) and the sample
step's two (4096 rows: a half-batch chain).  The shipped library runs as the engine runs it: the forward saves the row
statistics, the backward reads them.  Every output is compared with the old library's (rel-L2; the results are no longer
bit-identical: folded FiLM constants, xhat as one FMA).  python tools/ln_diet_ab.py [--once [--only old|new]]
--once: one launch per form (8192 rows only) for a counter-collection run, --only: of one library, so that the per-kernel means of
tools/pmc_summary.py belong to one build (the shipped library's plain forward then has two dispatches: one fills the statistics)"""
import ctypes as C
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import smd_amd.lib as lib
new = lib.get_lib()
old = C.CDLL(os.path.join(ROOT, "symbolic-music-diffusion_amd", "csrc", "libsmd_hip_old.so"))
for name, (res, args) in lib._SIGS.items():
    if hasattr(old, name):
        fn = getattr(old, name)
        fn.restype, fn.argtypes = res, args
once = "--once" in sys.argv
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
libs = [(k, L) for k, L in (("old", old), ("new", new)) if only in (None, k)]
dev = "cuda:0"
st = torch.cuda.current_stream().cuda_stream
D = 2048
P = lambda t: None if t is None else t.data_ptr()
rel = lambda a, b: float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
g0 = torch.Generator().manual_seed(0)
NSET = 3


def run(R, tag):
    x = torch.randn(R, D, generator=g0).to(dev)
    xbf = x.to(torch.bfloat16)
    g, b = (1 + 0.1 * torch.randn(D, generator=g0)).to(dev), (0.1 * torch.randn(D, generator=g0)).to(dev)
    ss = torch.cat([1 + 0.3 * torch.randn(R // 32, D, generator=g0), 0.2 * torch.randn(R // 32, D, generator=g0)], 1).to(dev)
    dout = torch.randn(R, D, generator=g0).to(torch.bfloat16).to(dev)
    dresb = torch.randn(R, D, generator=g0).to(torch.bfloat16).to(dev)
    outs = [torch.empty(R, D, dtype=torch.bfloat16, device=dev) for _ in range(NSET)]
    dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    dss = torch.zeros(R // 32, 2 * D, device=dev)
    part = torch.empty(R * 2 * D // 16, device=dev)
    stats = torch.empty(R, 2, device=dev)
    fwd_forms = [("fwd FiLM + swish (bf16 x)", xbf, None, 1), ("fwd plain (bf16 x)", xbf, None, 0)]
    if tag == "sample":
        fwd_forms = [("fwd FiLM + swish (fp32 x)", None, x, 1), ("fwd FiLM + swish (bf16 x)", xbf, None, 1)]
    bwd_forms = [] if tag == "sample" else [("bwd res.ln2 <2048,true,0> (FiLM + swish)", None, 1),
                                            ("bwd res.ln1 <2048,true,2> (FiLM + swish, bf16 dres)", dresb, 1), ("bwd ln_o (plain)", None, 0)]
    calls = []
    for name, xb, xf, fs in fwd_forms:
        def call(L, i=0, xb=xb, xf=xf, fs=fs):
            fa = (P(ss), ss[:, D:].data_ptr()) if fs else (None, None)
            if L is new:
                rc = L.smd_layernorm_fwd_stats(P(xf), P(xb), R, D, P(g), P(b), fa[0], fa[1], 2 * D, 32, fs, P(outs[i % NSET]), None, None,
                                               P(stats) if tag == "train" else None, st)
            else:
                rc = L.smd_layernorm_fwd_ex(P(xf), P(xb), R, D, P(g), P(b), fa[0], fa[1], 2 * D, 32, fs, P(outs[i % NSET]), st)
            assert rc == 0, new.smd_last_error()
        calls.append((name, call, lambda: (outs[0].clone(),)))
    for name, res, fs in bwd_forms:
        def call(L, i=0, res=res, fs=fs):
            fa = (P(ss), ss[:, D:].data_ptr()) if fs else (None, None)
            da = (P(dss), dss[:, D:].data_ptr()) if fs else (None, None)
            args = (None, P(xbf), R, D, P(g), P(b), fa[0], fa[1], 2 * D, 32, fs, P(dout), None, P(res), None, P(outs[i % NSET]), P(dg), P(db),
                    da[0], da[1], 0, P(part), part.numel())
            rc = L.smd_layernorm_bwd_stats(*args, P(stats), st) if L is new else L.smd_layernorm_bwd_film(*args, st)
            assert rc == 0, new.smd_last_error()
        calls.append((name, call, lambda: (outs[0].clone(), dg.clone(), db.clone(), dss.clone())))
    # the statistics the backward forms read: one forward of the shipped library on the same rows
    if only != "old":
        new.smd_layernorm_fwd_stats(None, P(xbf), R, D, P(g), P(b), None, None, 2 * D, 32, 0, P(outs[0]), None, None, P(stats), st)
    for name, call, snap in calls:
        def timeit(L, reps=40):
            for i in range(4):
                call(L, i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(reps):
                call(L, i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3
        t = {"old": [], "new": []}
        if not once:
            for rnd in range(5):
                for k, L in (("old", old), ("new", new)):
                    t[k].append(timeit(L))
        got = {}
        for k, L in libs:
            call(L, 0)
            torch.cuda.synchronize()
            got[k] = snap()
        if once:
            print(f"ln_diet_ab {tag} rows={R} {name}: one launch of {' and '.join(k for k, _ in libs)}")
            continue
        err = max(rel(u.float(), v.float()) for u, v in zip(got["new"], got["old"]))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        spread = max((max(v) - min(v)) / med[k] for k, v in t.items()) * 100      # widest round-to-round range of one library
        print(f"ln_diet_ab {tag} rows={R} {name}: old {med['old']:.2f} us (min {min(t['old']):.2f})  new {med['new']:.2f} us (min {min(t['new']):.2f})  "
              f"{(med['new'] / med['old'] - 1) * 100:+.1f} %   same-library spread {spread:.1f} %   new vs old rel {err:.2e}")


run(8192, "train")
if not once:
    run(4096, "sample")
