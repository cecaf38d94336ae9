"""Times the variational-bound walk of sample_ncsn.py --compute_bound (csrc/bound.hip, ncsn.variational_bound).

  python tools/bound_bench.py [--batch 256] [--warm 3] [--reps 200] [--out profiles/bound_bench.json]

Base network (32 x 512 latents, 6 layers, mlp 2048 x 2), T = 1000, in ONE process:
  * the whole bound walk -- first call (schedule tables, FiLM tables, warm-up step, graph capture) and the median of --warm
    later calls on the cached graphs, host clock around work that ends in a device synchronise;
  * the every-timestep sampler walk (ncsn.diffusion_dynamics) on the same batch, the same way: the yardstick, one eps-net
    forward per (timestep, sample) as well;
  * the noise kernel and the term kernel alone beside the fused reverse step alone, device events around each call, median of
    --reps calls.  Every timed call takes the next of several operand sets, so no call finds its inputs in the cache from the call
    before.  Comparable traffic: three fp32 arrays each (noise: x0, eps in, x_t out + the bf16 copy; terms: x0, eps, eps_hat in;
    reverse step: x, eps_hat in, x out + the bf16 copy, z drawn).  GB/s counts 3 B S C 4 bytes.
One JSON document.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smd_amd  # noqa: E402,F401
import smd_amd.lib as lib  # noqa: E402
import smd_amd.ncsn as N  # noqa: E402
import smd_amd.schedule as S  # noqa: E402
from smd_amd.engine import NetConfig  # noqa: E402

SETS = 4
T = 1000


def timed(fn, reps, warmup=4):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn(warmup + i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(reps)]
    return float(np.median(ts)), float(min(ts))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bound_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    B, Sq, Cn = a.batch, 32, 512
    betas = S.create_noise_schedule(1e-6, 1e-2, T, "linear")
    model = N.Model(NetConfig(data_channels=Cn, num_layers=6, num_heads=8, num_mlp_layers=2, num_timesteps=T), dev, seed=0)
    g = torch.Generator().manual_seed(0)
    x0 = torch.clamp(0.25 * torch.randn(B, Sq, Cn, generator=g), -1, 1).to(dev)
    res = dict(device=torch.cuda.get_device_name(0), batch=B, shape=[Sq, Cn], timesteps=T, dtype="bf16")

    out = {}
    first = wall(lambda: out.update(N.variational_bound(N.PRNGKey(1), model, betas, x0)))
    warm = [wall(lambda i=i: N.variational_bound(N.PRNGKey(2 + i), model, betas, x0)) for i in range(a.warm)]
    res["bound_walk"] = dict(first_call_s=first, warm_median_s=float(np.median(warm)), warm_s=warm, bits_per_dim=out["bits_per_dim"])
    model.drop_sampler_cache()
    init = torch.randn(B, Sq, Cn, generator=g).to(dev)
    first = wall(lambda: N.diffusion_dynamics(N.PRNGKey(1), model, betas, init))
    warm = [wall(lambda i=i: N.diffusion_dynamics(N.PRNGKey(2 + i), model, betas, init)) for i in range(a.warm)]
    res["sampler_walk"] = dict(first_call_s=first, warm_median_s=float(np.median(warm)), warm_s=warm,
                               arrangement=getattr(model, "sampler_arrangement", None))
    model.drop_sampler_cache()

    L = lib.get_lib()
    st = lambda: torch.cuda.current_stream().cuda_stream
    tab = S.bound_tables(betas, np.arange(T))
    table = torch.from_numpy(tab["table"]).to(dev)
    coef = torch.from_numpy(S.reverse_coefficient_table(betas)).to(dev)
    tp = torch.tensor([500], dtype=torch.int32, device=dev)
    Cp = Cn
    sets = [dict(x0=x0.clone(), eps=torch.randn_like(x0), eh=torch.randn_like(x0), xt=torch.empty_like(x0), x=torch.randn_like(x0),
                 bf=torch.empty((B * Sq, Cp), dtype=torch.bfloat16, device=dev), part=torch.zeros((T, B, 3), device=dev)) for _ in range(SETS)]

    def noise(i):
        s = sets[i % SETS]
        lib.check(L.smd_bound_noise(s["x0"].data_ptr(), B, Sq, Cn, Cp, table.data_ptr(), T, tp.data_ptr(), s["eps"].data_ptr(), 0, 0, 0,
                                    None, 0, s["xt"].data_ptr(), s["bf"].data_ptr(), st()), "bound_noise")

    def noise_draw(i):
        s = sets[i % SETS]
        lib.check(L.smd_bound_noise(s["x0"].data_ptr(), B, Sq, Cn, Cp, table.data_ptr(), T, tp.data_ptr(), s["eps"].data_ptr(), 1, 7, 0,
                                    None, 0, s["xt"].data_ptr(), s["bf"].data_ptr(), st()), "bound_noise")

    def terms(i):
        s = sets[i % SETS]
        lib.check(L.smd_bound_terms(s["x0"].data_ptr(), s["eps"].data_ptr(), s["eh"].data_ptr(), B, Sq, Cn, table.data_ptr(), T, 1.0,
                                    tp.data_ptr(), None, None, s["part"].data_ptr(), st()), "bound_terms")

    def reverse(i):
        s = sets[i % SETS]
        lib.check(L.smd_ddpm_reverse_step(s["x"].data_ptr(), s["eh"].data_ptr(), B, Sq, Cn, coef.data_ptr(), T, tp.data_ptr(), None, 7, 0,
                                          0, None, None, None, st()), "reverse_step")

    nbytes = 3 * B * Sq * Cn * 4
    res["kernels"] = {}
    for name, fn in (("reverse_step", reverse), ("bound_noise", noise), ("bound_noise_philox", noise_draw), ("bound_terms", terms)):
        med, best = timed(fn, a.reps)
        res["kernels"][name] = dict(median_us=med, best_us=best, gb_per_s=nbytes / med * 1e-3)
    rs = res["kernels"]["reverse_step"]["median_us"]
    for name in ("bound_noise", "bound_noise_philox", "bound_terms"):
        res["kernels"][name]["vs_reverse_step"] = res["kernels"][name]["median_us"] / rs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
