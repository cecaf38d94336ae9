"""Interleaved A/B of the three fused sampler steps between two builds of the library in one process: csrc/libsmd_hip_old.so
(tools/build_old_lib.sh) against the shipped one, or any two with --old / --new (the same file twice gives the noise floor).

  reverse     smd_reverse_step_lab (the kernel alone), Philox noise, also at the small shapes of the per-element tests
  strided     smd_engine_strided_step, part 2 (output stage + update) of a small network, eta = 0.7, Philox noise
  multistep   smd_engine_multistep_step, part 2, order 2 with a history that is read

Every call runs with metrics, collection, the bf16 copy and the in-kernel timestep store; once in mode "noise" and once in
mode "infill" (masks, samples, Philox infill draws).  The plan of the table-driven steps points every timestep at itself, so
repeated calls stay at one timestep.  State, history, collection, metric partials, bf16 copy and the timestep are compared bit
for bit; times are medians of interleaved rounds.  python tools/reverse_step_ab.py [--old A.so --new B.so] [--json OUT]"""
import argparse
import ctypes as C
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import smd_amd.lib as lib
import smd_amd.ncsn as N
import smd_amd.schedule as S
from smd_amd.engine import NetConfig

CSRC = os.path.join(ROOT, "symbolic-music-diffusion_amd", "csrc")
ap = argparse.ArgumentParser()
ap.add_argument("--old", default=os.path.join(CSRC, "libsmd_hip_old.so"))
ap.add_argument("--new", default=None, help="default: the shipped library")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--json", default=None)
args = ap.parse_args()


def load(path):
    L = C.CDLL(path)
    for name, (res, argt) in lib._SIGS.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, argt
    return L


LIBS = {"old": load(args.old), "new": load(args.new) if args.new else lib.get_lib()}
dev = "cuda:0"
st = lambda: torch.cuda.current_stream().cuda_stream
P = lambda t: None if t is None else t.data_ptr()
T, K = 1000, 20
BETAS = np.asarray(S.create_noise_schedule(1e-6, 0.01, T, "linear"), dtype=np.float32)
BIG = [(256, 32, 512), (256, 32, 146), (4096, 1, 512)]
SMALL = [(3, 32, 512), (2, 5, 516), (2, 4, 1024), (2, 7, 8), (3, 32, 42), (2, 6, 130), (2, 4, 1), (5, 1, 512), (3, 1, 1028),
         (2, 3, 64), (5, 1, 42), (3, 1, 146), (2, 3, 42), (4, 1, 1)]      # tests/_diffusion_ref.py REVERSE_SHAPES, unpadded
g = torch.Generator().manual_seed(0)
rows = []


def bits_equal(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def ab(kernel, shape, mode, call, outputs, reset):
    """call(k) runs one step of library k on its own buffers; outputs(k) lists them; reset(k) restores the inputs"""
    def timeit(k):
        for _ in range(3):
            call(k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            call(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps * 1e3
    res = {"old": [], "new": []}
    for _ in range(args.rounds):
        for k in ("old", "new"):
            res[k].append(timeit(k))
    for k in ("old", "new"):
        reset(k)
        call(k)
    torch.cuda.synchronize()
    same = bits_equal(outputs("old"), outputs("new"))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    rows.append(dict(kernel=kernel, shape=list(shape), mode=mode, old_us=round(med["old"], 3), new_us=round(med["new"], 3),
                     ratio=round(med["new"] / med["old"], 4), bitwise_equal=same, arrays=len(outputs("new"))))
    print(f"{kernel:9s} {str(shape):16s} {mode:6s} old {med['old']:8.2f} us  new {med['new']:8.2f} us  {(med['new'] / med['old'] - 1) * 100:+5.1f} %  "
          f"bitwise equal: {same} ({len(outputs('new'))} arrays)", flush=True)


# ------------------------------------------------------------------------------------------------ reverse step: the lab entry
coef_r = torch.from_numpy(S.reverse_coefficient_table(BETAS)).to(dev)
slots_r = torch.full((T,), 5, dtype=torch.int32, device=dev)            # every timestep is collected, in row 5
for shape in BIG + SMALL:
    B, Sq, Cc = shape
    Cp = (Cc + 7) // 8 * 8
    for mode in ("noise", "infill"):
        x0, eh = torch.randn(B, Sq, Cc, generator=g).to(dev), torch.randn(B, Sq, Cc, generator=g).to(dev)
        samples = torch.clamp(0.25 * torch.randn(B, Sq, Cc, generator=g), -1, 1).to(dev) if mode == "infill" else None
        masks = (torch.rand(B, Sq, Cc, generator=g) < 0.5).float().to(dev) if mode == "infill" else None
        buf = {k: dict(x=x0.clone(), xb=torch.zeros(B * Sq, Cp, dtype=torch.int16, device=dev), met=torch.zeros(T, B, 3, device=dev),
                       coll=torch.zeros(41, B, Sq, Cc, device=dev), t=torch.tensor([500], dtype=torch.int32, device=dev),
                       tn=torch.zeros(1, dtype=torch.int32, device=dev), arrive=torch.zeros(1, dtype=torch.int32, device=dev))
               for k in LIBS}

        def call(k):
            b, a = buf[k], lib.ReverseStepLabArgs()
            a.x, a.eps_hat, a.B, a.S, a.C, a.Cp, a.T = P(b["x"]), P(eh), B, Sq, Cc, Cp, T
            a.coef, a.t_ptr, a.t_advance, a.arrive = P(coef_r), P(b["t"]), P(b["tn"]), P(b["arrive"])     # t stays, t - 1 goes to tn
            a.seed_lo, a.seed_hi = 11, 22
            a.infill_samples, a.infill_masks = P(samples), P(masks)
            a.x_bf16, a.metrics_partial, a.collection, a.slot_table = P(b["xb"]), P(b["met"]), P(b["coll"]), P(slots_r)
            rc = LIBS[k].smd_reverse_step_lab(C.byref(a), None, st())
            assert rc == 0, LIBS[k].smd_last_error()

        def reset(k):
            buf[k]["x"].copy_(x0)
        ab("reverse", shape, mode, call, lambda k: [buf[k][n] for n in ("x", "xb", "met", "coll", "tn", "arrive")], reset)


# ------------------------------------------------------------------------------------------------ table-driven steps: the engine
def engine_of(k, shape):
    B, Sq, Cc = shape
    cfg = (NetConfig(data_channels=Cc, num_layers=2, num_heads=8, num_mlp_layers=1, num_timesteps=T) if Sq > 1 else
           NetConfig(architecture="DenseDDPM", data_channels=Cc, num_layers=3, num_heads=8, num_mlp_layers=2, num_timesteps=T))
    keep, lib._LIB = lib._LIB, LIBS[k]          # the engine keeps the library it was created with
    try:
        eng = N.Model(cfg, dev, seed=0).engine
    finally:
        lib._LIB = keep
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(B, training=False)
    eng.prepare_sampler()
    return eng


def bf16_input(eng, x):
    """the engine's bf16 network input: where load_state(x) left bf16(x), zero padded, in its workspace"""
    Cc, Cp = eng.C, int(eng.L.smd_engine_padded_channels(eng.h))
    r = x.reshape(-1, Cc)
    img = torch.zeros((r.shape[0], Cp), dtype=torch.bfloat16, device=x.device)
    img[:, :Cc] = r.to(torch.bfloat16)
    want = img.view(torch.uint8).reshape(-1)
    ws = eng.workspace
    base = (-ws.data_ptr()) % 256
    n = (ws.numel() - base - want.numel()) // 256 + 1
    head = ws[base:base + n * 256].view(n, 256)[:, :64]
    cand = torch.nonzero((head == want[:64]).all(dim=1)).flatten().tolist()
    hits = [base + 256 * i for i in cand if torch.equal(ws[base + 256 * i:base + 256 * i + want.numel()], want)]
    assert len(hits) == 1, hits
    return hits[0], want.numel()


taus = S.stride_timesteps(T, K)
TS = int(taus[K // 2])              # a mid-walk timestep
tables = {"strided": S.strided_coefficient_table(BETAS, taus, 0.7, 1.0), "multistep": S.multistep_coefficient_table(BETAS, taus, 2, 1.0)}
for shape in BIG:
    B, Sq, Cc = shape
    sshape = (B, Sq, Cc) if Sq > 1 else (B, Cc)
    engs = {k: engine_of(k, shape) for k in LIBS}
    for kernel, (coef, plan) in tables.items():
        plan = plan.copy()
        plan[plan[:, 1] >= 0, 0] = np.nonzero(plan[:, 1] >= 0)[0]           # every timestep of the walk points at itself
        plan[plan[:, 1] >= 0, 2] = 5                                        # and is collected, in row 5
        assert kernel != "multistep" or coef[TS, 8] != 0.0                  # the history is read
        coef_d, plan_d = torch.from_numpy(coef).to(dev), torch.from_numpy(plan).to(dev)
        sp = lib.StridePlan() if kernel == "strided" else lib.MultistepPlan()
        sp.coef, sp.plan, sp.T = P(coef_d), P(plan_d), T
        for mode in ("noise", "infill"):
            x0 = torch.randn(*sshape, generator=g).to(dev)
            h0 = torch.clamp(torch.randn(*sshape, generator=g), -1, 1).to(dev)
            samples = torch.clamp(0.25 * torch.randn(*sshape, generator=g), -1, 1).to(dev) if mode == "infill" else None
            masks = (torch.rand(*sshape, generator=g) < 0.5).float().to(dev) if mode == "infill" else None
            buf = {k: dict(x=x0.clone(), hist=h0.clone(), met=torch.zeros(T, B, 3, device=dev), coll=torch.zeros(41, *sshape, device=dev),
                           t=torch.tensor([TS], dtype=torch.int32, device=dev)) for k in LIBS}
            where = {}

            def reset(k):
                buf[k]["x"].copy_(x0)
                buf[k]["hist"].copy_(h0)
                engs[k].load_state(buf[k]["x"])
                if k not in where:
                    torch.cuda.synchronize()
                    where[k] = bf16_input(engs[k], x0)
                step(k, 1)                      # the stem; part 2 below is the output stage and the update

            def step(k, part):
                b, io = buf[k], lib.SampleIO()
                io.x, io.t_ptr, io.seed_lo, io.seed_hi = P(b["x"]), P(b["t"]), 11, 22
                io.infill_samples, io.infill_masks = P(samples), P(masks)
                io.metrics_partial, io.collection = P(b["met"]), P(b["coll"])
                if kernel == "strided":
                    engs[k].strided_step(io, sp, part)
                else:
                    engs[k].multistep_step(io, sp, b["hist"], part)

            def outputs(k):
                off, nbytes = where[k]
                return [buf[k][n] for n in ("x", "hist", "met", "coll", "t")] + [engs[k].workspace[off:off + nbytes], engs[k].last_pred()]
            for k in LIBS:
                reset(k)
            ab(kernel, shape, mode, lambda k: step(k, 2), outputs, reset)
    del engs
    torch.cuda.empty_cache()

bad = [r for r in rows if not r["bitwise_equal"]]
print(f"{len(rows)} comparisons, {sum(r['arrays'] for r in rows)} arrays, {len(bad)} differ")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(old=os.path.basename(args.old), new=os.path.basename(args.new or "libsmd_hip.so"), rounds=args.rounds, reps=args.reps,
                       rows=rows), f, indent=1)
sys.exit(1 if bad else 0)
