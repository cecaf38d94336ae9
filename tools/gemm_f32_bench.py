"""Times the reference-precision path (engine option "fp32": csrc/gemm_f32.hip, net_f32.hip).

  python tools/gemm_f32_bench.py [--reps 20] [--sets 4] [--walk-batch 256] [--out profiles/fp32_bench.json]

(a) smd_gemm_f32 on the Dense shapes of the base network at B = 256 (8192 token rows): the DenseResBlock shape
    8192 x 2048 x 2048 (77 % of the pass's flops) and the skinny ones, against the 157.3 TF fp32-MFMA peak
    (MI355X_MICROARCH.md).  Operands rotate over `--sets` buffer sets (8192 x 2048 fp32 = 64 MiB each, so four sets exceed
    the 256 MiB last-level cache) and every shape is warmed up first; median and best of `--reps` event-timed calls.
(b) a T = 1000 reverse walk of B = 256 base sequences (Philox draws, graph replay) on an fp32 engine and on a bf16 engine of
    the same build: wall time of the second walk (the first pays capture and instantiation).
One JSON line per measurement; everything is also written to --out.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smd_amd  # noqa: E402,F401
import smd_amd.lib as lib  # noqa: E402

PEAK_TF = 157.3
SHAPES = [(8192, 2048, 2048, "DenseResBlock fc1 / fc2"), (8192, 128, 2048, "encoder mlp.fc1 / up"), (8192, 2048, 128, "encoder mlp.fc2"),
          (8192, 128, 384, "attention qkv"), (8192, 128, 128, "attention out"), (8192, 2048, 512, "out_proj"), (8192, 512, 128, "in_proj")]


def bench_gemm(L, M, K, N, reps, sets):
    dev = "cuda"
    A = [torch.randn(M, K, device=dev) for _ in range(sets)]
    W = [torch.randn(K, N, device=dev) / math.sqrt(K) for _ in range(sets)]
    b = torch.randn(N, device=dev)
    out = [torch.empty(M, N, device=dev) for _ in range(sets)]
    st = torch.cuda.current_stream().cuda_stream

    def call(i):
        j = i % sets
        lib.check(L.smd_gemm_f32(A[j].data_ptr(), K, W[j].data_ptr(), N, M, N, K, b.data_ptr(), 0, None, 0, 0, out[j].data_ptr(), N, st))
    for i in range(2 * sets):
        call(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        call(i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = [ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i in range(reps)]
    flop = 2.0 * M * N * K
    med, best = float(np.median(ts)), float(min(ts))
    return dict(us_median=med * 1e6, us_best=best * 1e6, tflops_median=flop / med * 1e-12, tflops_best=flop / best * 1e-12,
                fraction_of_fp32_mfma_peak=flop / med * 1e-12 / PEAK_TF)


def bench_walk(dtype, B, walks=3):
    import smd_amd.ncsn as N
    from smd_amd.engine import NetConfig
    from smd_amd import schedule
    model = N.Model(NetConfig(dtype=dtype), "cuda:0", seed=0)
    betas = schedule.create_noise_schedule(1e-6, 0.01, 1000, schedule="linear")
    init = torch.randn(B, 32, 512, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    ts = []
    for i in range(walks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, _, _ = N.diffusion_dynamics(N.PRNGKey(i), model, betas, init)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    assert bool(torch.isfinite(x).all())
    return dict(dtype=dtype, batch=B, steps=1000, walk_s_first=ts[0], walk_s=float(min(ts[1:])), arrangement=model.sampler_arrangement)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--walk-batch", type=int, default=256)
    ap.add_argument("--no-walk", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp32_bench.json"))
    a = ap.parse_args()
    L = lib.get_lib()
    res = dict(device=torch.cuda.get_device_name(0), peak_tf=PEAK_TF, gemm=[], walk=[])
    for M, K, N, what in SHAPES:
        r = dict(M=M, K=K, N=N, layer=what, **bench_gemm(L, M, K, N, a.reps, a.sets))
        res["gemm"].append(r)
        print(json.dumps(r), flush=True)
    if not a.no_walk:
        for dt in ("fp32", "bf16"):
            r = bench_walk(dt, a.walk_batch)
            res["walk"].append(r)
            print(json.dumps(r), flush=True)
        res["walk_ratio_fp32_over_bf16"] = res["walk"][0]["walk_s"] / res["walk"][1]["walk_s"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
