"""Cost and solver error of the second-order multistep sampler (DPM-Solver++(2M)) on the base network
(L6 H8 K2, C = 512, T = 1000).  Writes profiles/multistep_sampler_bench.json.
    python tools/multistep_sampler_bench.py [--repeats 7] [--batch 256] [--error_batch 8]

(a) Wall time.  Whole N.sample() calls at B = `batch` (bf16) between two device synchronisations, as
tools/strided_sampler_bench.py measures them: one cold call per configuration, then `repeats` warm calls with other seeds that
reuse the cached graphs; the median of the warm calls.  Configurations: (order 1, uniform) = the strided kernel, (order 2,
uniform) = the multistep kernel on the SAME timesteps, (order 1, logsnr), (order 2, logsnr).  The cost of the multistep update
over the strided one is the difference of the two uniform walks divided by their (equal) number of iterations.

(b) Solver error.  Under --dtype=fp32 at B = `error_batch`: rel-L2 of the final state against the K = T, eta = 0 walk from the
same start, for K = 10, 20, 50.  This is the error of the ODE solver on a freshly initialised network, NOT sample quality.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smd_amd.ncsn as N  # noqa: E402
import smd_amd.schedule as S  # noqa: E402
from smd_amd.engine import NetConfig  # noqa: E402

CONFIGS = (("order1_uniform", 1, "uniform"), ("order2_uniform", 2, "uniform"), ("order1_logsnr", 1, "logsnr"), ("order2_logsnr", 2, "logsnr"))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--error_batch", type=int, default=8)
    ap.add_argument("--steps", type=int, nargs="*", default=[20, 50])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistep_sampler_bench.json"))
    a = ap.parse_args()
    B, T = a.batch, 1000
    betas = S.create_noise_schedule(1e-6, 0.01, T, "linear")
    out = dict(device=torch.cuda.get_device_name(0), T=T, network="TransformerDDPM L6 H8 K2 C512", repeats=a.repeats)

    # ---------------------------------------------------------------- (a) wall time, bf16, B = batch
    model = N.Model(NetConfig(architecture="TransformerDDPM", data_channels=512, seq_len=32, num_timesteps=T), "cuda:0", seed=0)
    seed = [100]

    def call(**kw):
        seed[0] += 1
        gen, _, _ = N.sample(model, betas, N.PRNGKey(seed[0]), (32, 512), num_samples=B, sampling="ddpm", **kw)
        assert bool(torch.isfinite(gen).all())

    walks = {}
    for K in a.steps:
        for name, order, spacing in CONFIGS:
            kw = dict(ddim_steps=K, ddim_eta=0.0, ddim_order=order, ddim_spacing=spacing)
            first = timed(lambda: call(**kw))
            warm = [timed(lambda: call(**kw)) for _ in range(a.repeats)]
            n = model.sampler_arrangement["iterations"]
            r = dict(first_call_s=first, warm_s=warm, median_s=statistics.median(warm), min_s=min(warm), max_s=max(warm), iterations=n,
                     per_iteration_ms=1e3 * statistics.median(warm) / n, kernel=model.sampler_arrangement["walk"],
                     arrangement=dict(model.sampler_arrangement))
            walks[f"K{K}_{name}"] = r
            print(f"K = {K:3d} {name:15s} ({n} iterations, {r['kernel']} kernel): first {first:.3f} s, warm median {r['median_s'] * 1e3:.2f} ms "
                  f"[{r['min_s'] * 1e3:.2f}, {r['max_s'] * 1e3:.2f}] = {r['per_iteration_ms']:.3f} ms per iteration", flush=True)
        s1, s2 = walks[f"K{K}_order1_uniform"], walks[f"K{K}_order2_uniform"]
        d_med = 1e6 * (s2["median_s"] - s1["median_s"]) / K
        d_min = 1e6 * (s2["min_s"] - s1["min_s"]) / K
        walks[f"K{K}_update_cost"] = dict(multistep_minus_strided_us_per_iteration_median=d_med, multistep_minus_strided_us_per_iteration_min=d_min,
                                          spread_of_one_walk_us_per_iteration=1e6 * (s1["max_s"] - s1["min_s"]) / K)
        print(f"K = {K:3d} multistep update - strided update: {d_med:+.2f} us per iteration (medians), {d_min:+.2f} us (minima); "
              f"the strided walk alone spreads over {1e6 * (s1['max_s'] - s1['min_s']) / K:.2f} us per iteration", flush=True)
    out["wall_time"] = dict(batch=B, dtype="bf16", method="N.sample() wall time between device synchronisations; first call captures, warm "
                            "calls reuse the cached graphs (other seeds); median of the warm calls", walks=walks)
    model.drop_sampler_cache()
    del model

    # ---------------------------------------------------------------- (b) solver error, fp32
    Be = a.error_batch
    m32 = N.Model(NetConfig(architecture="TransformerDDPM", data_channels=512, seq_len=32, num_timesteps=T, dtype="fp32"), "cuda:0", seed=0)
    init = torch.randn(Be, 32, 512, generator=torch.Generator().manual_seed(1)).cuda()
    full, _, _ = N.strided_dynamics(N.PRNGKey(0), m32, betas, init, T, 0.0)
    rel = lambda x: float((x.double() - full.double()).norm() / full.double().norm())
    err = {}
    for K in (10, 20, 50):
        for name, order, spacing in (CONFIGS[0], CONFIGS[2], CONFIGS[3]):
            x, _, _ = N.strided_dynamics(N.PRNGKey(0), m32, betas, init, K, 0.0, order=order, spacing=spacing)
            err[f"K{K}_{name}"] = dict(rel_l2=rel(x), iterations=m32.sampler_arrangement["iterations"])
        print(f"K = {K:3d} rel-L2 against the K = T walk: " + ", ".join(f"{n} {err[f'K{K}_{n}']['rel_l2']:.3e} ({err[f'K{K}_{n}']['iterations']} it.)"
                                                                      for n in ("order1_uniform", "order1_logsnr", "order2_logsnr")), flush=True)
    out["solver_error"] = dict(batch=Be, dtype="fp32", reference="strided_dynamics(K = T = 1000, eta = 0) from the same start",
                               what="error of the ODE solver on a freshly initialised network (seed 0): NOT sample quality", rel_l2=err)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
