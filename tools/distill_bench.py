"""Cost of a progressive-distillation step on the base network (ddpm-mel-32seq-512: TransformerDDPM L6 H8 K2,
C = 512, T = 1000) at the bench batch.  Writes profiles/distill_bench.json.
    python tools/distill_bench.py [--batch 256] [--steps 40] [--warmup 8] [--repeats 3]

(a) Wall time per step between device synchronisations, arms interleaved block by block as in tools/prediction_bench.py:
    plain      trainer.train_step, --prediction=v
    distill    trainer.distill_step, v teacher -> v student of N = 8 steps (teacher walk of 16 timesteps)
    forward    one inference forward of the teacher handle at the same batch, alone
    The step's cost is stated as distill - plain, to be compared with 2 forwards + the three element-wise kernels.
(b) Each of the three kernels alone, through the C-ABI: `launches` back-to-back launches between two HIP events, three times.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smd_amd.lib as lib  # noqa: E402
import smd_amd.ncsn as N  # noqa: E402
import smd_amd.schedule as S  # noqa: E402
from smd_amd.trainer import DistillTables, create_optimizer, distill_step, train_step  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--student_steps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_bench.json"))
    a = ap.parse_args()
    B, T, dev = a.batch, 1000, torch.device("cuda:0")
    betas = S.create_noise_schedule(1e-6, 0.01, T, "linear")
    kwargs = dict(num_layers=6, num_heads=8, num_mlp_layers=2, mlp_dims=2048)
    out = dict(device=torch.cuda.get_device_name(0), network="TransformerDDPM L6 H8 K2 C512 (ddpm-mel-32seq-512)", T=T, batch=B,
               steps=a.steps, warmup=a.warmup, repeats=a.repeats, student_steps=a.student_steps)

    make = lambda seed: N.create_model(N.PRNGKey(seed), (32, 512), kwargs, architecture="TransformerDDPM", num_timesteps=T)
    plain_model, teacher, student = make(0), make(1), make(1)
    plain_opt = create_optimizer(plain_model, 3e-4, ema=True)
    opt = create_optimizer(student, 3e-4, ema=True)
    tw, _ = S.distill_walk(T, a.student_steps)
    tab = DistillTables(betas, tw, "v", "v", "truncated_snr", device=dev)
    x0 = torch.clamp(0.25 * torch.randn(B, 32, 512, generator=torch.Generator().manual_seed(1)), -1, 1).to(dev)
    level = torch.full((B,), 0.7, device=dev)
    it = [0]

    def one(arm):
        it[0] += 1
        if arm == "plain":
            train_step(N.diffusion_loss, x0, plain_opt, betas, N.PRNGKey(it[0]), 3e-4, lr_gamma=0.98, lr_interval=10000, prediction="v")
        elif arm == "distill":
            distill_step(x0, opt, teacher, tab, N.PRNGKey(it[0]), 3e-4, lr_gamma=0.98, lr_interval=10000)
        else:
            teacher.engine.forward(x0, level)

    def block(arm, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            one(arm)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    names = ("plain", "distill", "forward")
    for arm in names:
        block(arm, a.warmup)
    times = {arm: [] for arm in names}
    for _ in range(a.repeats):
        for arm in names:
            times[arm].append(block(arm, a.steps))
    arms = {}
    for arm in names:
        med = statistics.median(times[arm])
        arms[arm] = dict(ms_blocks=[1e3 * t for t in times[arm]], ms_median=1e3 * med, min_ms=1e3 * min(times[arm]),
                         max_ms=1e3 * max(times[arm]))
        print(f"{arm:8s}: {1e3 * med:.3f} ms [{1e3 * min(times[arm]):.3f}, {1e3 * max(times[arm]):.3f}]", flush=True)

    # ---------------------------------------------------------------- (b) the kernels alone
    L = lib.get_lib()
    st = torch.cuda.current_stream().cuda_stream
    S_, C, Ns = 32, 512, a.student_steps
    arr = [torch.randn(B, S_, C, device=dev) for _ in range(5)]
    o = [torch.empty(B, S_, C, device=dev) for _ in range(3)]
    k = torch.randint(0, Ns, (B,), device=dev).int()
    lv, ls, w = (torch.empty(B, device=dev) for _ in range(3))
    inv = 1.0 / (B * S_ * C)
    P = lambda t: t.data_ptr()
    calls = {
        "distill_noise (eps read)": lambda: L.smd_distill_noise(P(arr[0]), B, S_, C, P(tab.table), Ns, P(k), P(arr[1]), 0, 0, 0, 0, 0, None,
                                                                P(o[0]), P(lv), st),
        "distill_noise (Philox)": lambda: L.smd_distill_noise(P(arr[0]), B, S_, C, P(tab.table), Ns, P(k), P(o[1]), 1, 7, 0, 0, 0, None,
                                                              P(o[0]), P(lv), st),
        "distill_mid": lambda: L.smd_distill_mid(P(arr[0]), P(arr[1]), B, S_, C, P(tab.table), Ns, P(k), P(o[0]), P(o[1]), P(lv), st),
        "distill_loss (v)": lambda: L.smd_distill_loss(P(arr[0]), P(arr[1]), P(arr[2]), P(arr[3]), P(arr[4]), 2, B, S_, C, P(tab.table),
                                                       Ns, P(k), None, inv, P(ls), P(w), P(o[0]), None, st),
    }
    kern = {}
    for name, fn in calls.items():
        for _ in range(10):
            lib.check(fn(), name)
        per = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            per.append(1e3 * e0.elapsed_time(e1) / a.launches)
        kern[name] = dict(us_per_launch=per, median_us=statistics.median(per))
        print(f"{name:26s}: {statistics.median(per):.2f} us per launch {np.round(per, 2).tolist()}", flush=True)

    extra = arms["distill"]["ms_median"] - arms["plain"]["ms_median"]
    three = 1e-3 * (kern["distill_noise (Philox)"]["median_us"] + kern["distill_mid"]["median_us"] + kern["distill_loss (v)"]["median_us"])
    expect = 2 * arms["forward"]["ms_median"] + three
    out["step"] = dict(method="wall time between device synchronisations, arms interleaved block by block; median block", arms=arms,
                       distill_minus_plain_ms=extra, expected_ms=expect,
                       expected_is="2 x the inference forward alone + the three kernels alone (Philox noise, mid, loss)",
                       plain_spread_us=1e3 * (arms["plain"]["max_ms"] - arms["plain"]["min_ms"]))
    out["kernels"] = dict(method=f"{a.launches} back-to-back launches between two HIP events, three times; B = {B}, S = 32, C = 512",
                          kernels=kern)
    print(f"distill - plain = {extra:.3f} ms; expected 2 forwards + three kernels = {expect:.3f} ms", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
