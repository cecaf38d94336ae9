"""Cost of x0- / v-parameterised training on the base network (ddpm-mel-32seq-512: TransformerDDPM L6 H8 K2,
C = 512, T = 1000) at the bench batch.  Writes profiles/prediction_bench.json.
    python tools/prediction_bench.py [--batch 256] [--steps 40] [--warmup 8] [--repeats 3]

(a) Train steps/s of trainer.train_step for the arms eps, x0 and v on ONE optimiser (the kind is a handle option, settable at any
time).  Per arm: `warmup` steps, then `repeats` blocks of `steps` steps between two device synchronisations; the median block.
The arms are interleaved block by block (eps, x0, v, eps, ...) so that drift of the device hits all of them alike.  The eps arm
of the parent commit is measured by running this tool's --eps_only mode there (the parent knows no other arm) in the same
session, and is passed in with --parent_json to be quoted beside this build's.
(b) The loss kernels alone, through the C-ABI: `launches` back-to-back launches between two HIP events, three times (bandwidth-bound
kernels on 16.8 MB arrays: three fp32 reads for v, two for x0 and eps, one bf16 write).
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
from smd_amd.trainer import create_optimizer, train_step  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--eps_only", action="store_true", help="the eps arm alone, with no --prediction argument: runs on the parent commit")
    ap.add_argument("--parent_json", default="", help="the file an --eps_only run of the parent commit wrote")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prediction_bench.json"))
    a = ap.parse_args()
    B, T, dev = a.batch, 1000, torch.device("cuda:0")
    betas = S.create_noise_schedule(1e-6, 0.01, T, "linear")
    arms_names = ("eps",) if a.eps_only else ("eps", "x0", "v")
    out = dict(device=torch.cuda.get_device_name(0), network="TransformerDDPM L6 H8 K2 C512 (ddpm-mel-32seq-512)", T=T, batch=B,
               steps=a.steps, warmup=a.warmup, repeats=a.repeats)

    # ---------------------------------------------------------------- (a) train steps/s
    model = N.create_model(N.PRNGKey(0), (32, 512), dict(num_layers=6, num_heads=8, num_mlp_layers=2, mlp_dims=2048),
                           architecture="TransformerDDPM", num_timesteps=T)
    opt = create_optimizer(model, 3e-4, ema=True)
    x0 = torch.clamp(0.25 * torch.randn(B, 32, 512, generator=torch.Generator().manual_seed(1)), -1, 1).to(dev)
    kw = {"eps": {}} if a.eps_only else {k: dict(prediction=k) for k in arms_names}
    it = [0]

    def block(arm, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            it[0] += 1
            train_step(N.diffusion_loss, x0, opt, betas, N.PRNGKey(it[0]), 3e-4, lr_gamma=0.98, lr_interval=10000, **kw[arm])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for arm in arms_names:
        block(arm, a.warmup)
    times = {arm: [] for arm in arms_names}
    for _ in range(a.repeats):
        for arm in arms_names:
            times[arm].append(block(arm, a.steps))
    arms = {}
    for arm in arms_names:
        med = statistics.median(times[arm])
        arms[arm] = dict(step_ms_blocks=[1e3 * t for t in times[arm]], step_ms_median=1e3 * med, steps_per_s=1.0 / med,
                         min_ms=1e3 * min(times[arm]), max_ms=1e3 * max(times[arm]))
        print(f"{arm:4s}: {1e3 * med:.3f} ms per step [{1e3 * min(times[arm]):.3f}, {1e3 * max(times[arm]):.3f}] = {1.0 / med:.1f} steps/s", flush=True)
    d = arms["eps"]
    for arm in arms_names[1:]:
        arms[arm]["minus_eps_us"] = 1e3 * (arms[arm]["step_ms_median"] - d["step_ms_median"])
    out["train"] = dict(method="trainer.train_step wall time between device synchronisations, arms interleaved block by block; median block",
                        eps_spread_us=1e3 * (d["max_ms"] - d["min_ms"]), arms=arms)
    if a.parent_json:
        with open(a.parent_json) as f:
            out["train"]["parent_eps"] = json.load(f)["train"]["arms"]["eps"]

    # ---------------------------------------------------------------- (b) the kernels alone
    if not a.eps_only:
        L = lib.get_lib()
        st = torch.cuda.current_stream().cuda_stream
        S_, C = 32, 512
        pred, eps, xx = (torch.randn(B, S_, C, device=dev) for _ in range(3))
        s, iw = 0.05 + 0.9 * torch.rand(B, device=dev), 0.5 + torch.rand(B, device=dev)
        loss, w = torch.empty(B, device=dev), torch.empty(B, device=dev)
        dp = torch.zeros(B * S_, C, dtype=torch.bfloat16, device=dev)
        inv = 1.0 / (B * S_ * C)
        P = lambda t: t.data_ptr()
        calls = {"weighted_mse_loss_grad (eps)": lambda: L.smd_weighted_mse_fwd_bwd(P(pred), P(eps), P(s), P(iw), 5.0, B, S_, C, C, inv,
                                                                                  P(loss), P(w), P(dp), st)}
        for kind, name in ((1, "x0"), (2, "v")):
            calls[f"param_mse_loss_grad ({name})"] = lambda kind=kind: L.smd_param_mse_fwd_bwd(
                P(pred), P(eps), P(xx), P(s), P(iw), 5.0, kind, B, S_, C, C, inv, P(loss), P(w), P(dp), st)
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
            print(f"{name:30s}: {statistics.median(per):.2f} us per launch {np.round(per, 2).tolist()}", flush=True)
        out["kernels"] = dict(method=f"{a.launches} back-to-back launches between two HIP events, three times; B = {B}, S = 32, C = 512",
                              kernels=kern)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
