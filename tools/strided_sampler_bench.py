"""Wall time of the strided (DDIM) sampler at B = 256 on the base network (L6 H8 K2, C = 512, T = 1000) for K = 10, 20, 50, 100,
250 timesteps, next to the every-timestep walk of the same process, and the fixed cost a call pays around its network
evaluations.  Writes profiles/strided_sampler_bench.json.      python tools/strided_sampler_bench.py [--repeats 5] [--batch 256]

How it measures: whole N.sample() calls between two device synchronisations (what a user waits for: initial draw, schedule
tables, FiLM tables, the walk, the copies out).  Per K: one cold call (capture of the K's graphs; its time is the "first_call"),
then `repeats` warm calls with other seeds that reuse the cached graphs; the median and the spread of the warm calls are
reported.  The fixed cost is measured part by part on the warm handle: prepare_sampler alone, the warm-up iteration and the
capture of uncached calls (timers inside the walker), and a K = 2 walk (2 evaluations).
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, nargs="*", default=[10, 20, 50, 100, 250])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strided_sampler_bench.json"))
    a = ap.parse_args()
    B, T = a.batch, 1000
    model = N.Model(NetConfig(architecture="TransformerDDPM", data_channels=512, seq_len=32, num_timesteps=T), "cuda:0", seed=0)
    betas = S.create_noise_schedule(1e-6, 0.01, T, "linear")
    seed = [100]

    def call(**kw):
        seed[0] += 1
        gen, _, _ = N.sample(model, betas, N.PRNGKey(seed[0]), (32, 512), num_samples=B, sampling="ddpm", **kw)
        assert bool(torch.isfinite(gen).all())

    def series(**kw):
        first = timed(lambda: call(**kw))
        warm = [timed(lambda: call(**kw)) for _ in range(a.repeats)]
        return dict(first_call_s=first, warm_s=warm, median_s=statistics.median(warm), min_s=min(warm), max_s=max(warm),
                    arrangement={k: v for k, v in model.sampler_arrangement.items()})

    out = dict(device=torch.cuda.get_device_name(0), batch=B, T=T, network="TransformerDDPM L6 H8 K2 C512 bf16", repeats=a.repeats,
               method="N.sample() wall time between device synchronisations; first call captures, warm calls reuse the cached graphs "
                      "(other seeds); median of the warm calls", walks={})
    full = series()
    out["walks"]["every_timestep_1000"] = full
    print(f"every timestep (1000 evaluations): first {full['first_call_s']:.3f} s, warm median {full['median_s']:.4f} s", flush=True)
    for K in a.steps:
        for eta in (0.0, 1.0):
            r = series(ddim_steps=K, ddim_eta=eta)
            r["speedup_vs_1000"] = full["median_s"] / r["median_s"]
            r["per_evaluation_ms"] = 1e3 * r["median_s"] / K
            out["walks"][f"K{K}_eta{eta:g}"] = r
            print(f"K = {K:4d} eta = {eta:g}: first {r['first_call_s']:.3f} s, warm median {r['median_s']:.4f} s "
                  f"[{r['min_s']:.4f}, {r['max_s']:.4f}] = {r['per_evaluation_ms']:.3f} ms per evaluation, {r['speedup_vs_1000']:.1f}x the 1000-step walk",
                  flush=True)
    # fixed cost of a call, each part on its own: FiLM tables for all T levels (prepare_sampler, once per chain and call); the
    # warm-up iteration as plain launches and the capture + instantiation of the graphs (timed inside the walker, which blocks
    # the host around them: SMD_SAMPLER_TIMING, on a dropped cache, so these calls are not part of the series above); and
    # everything but the evaluations of a warm call (a K = 2 walk)
    n_chains = model.sampler_arrangement["chains"]
    eng = model.chain_engines(n_chains)[0] if n_chains > 1 else model.engine     # a handle the walks above bound and scheduled
    prep = [timed(eng.prepare_sampler) for _ in range(a.repeats)]
    os.environ["SMD_SAMPLER_TIMING"] = "1"
    parts = {}
    for K in (20, 100):
        warm_up, capture, first = [], [], []
        for _ in range(a.repeats):
            model.drop_sampler_cache()
            first.append(timed(lambda: call(ddim_steps=K, ddim_eta=0.0)))
            warm_up.append(model._sampler_timing["warmup_s"])
            capture.append(model._sampler_timing["capture_s"])
        parts[f"K{K}"] = dict(uncached_call_s=statistics.median(first), warmup_iteration_s=statistics.median(warm_up),
                              capture_s=statistics.median(capture))
    os.environ.pop("SMD_SAMPLER_TIMING")
    model.drop_sampler_cache()
    k2 = series(ddim_steps=2, ddim_eta=0.0)
    out["fixed_cost"] = dict(prepare_sampler_s=statistics.median(prep), prepare_sampler_calls_per_walk=model.sampler_arrangement["chains"],
                             uncached=parts, k2_walk_first_call_s=k2["first_call_s"], k2_walk_warm_median_s=k2["median_s"],
                             note="uncached: graphs dropped before every call, host blocked around warm-up and capture; "
                                  "warmup_iteration_s = the first iteration of both chains as plain launches; capture_s = capture + "
                                  "instantiation of both chains' graphs (8 iterations each)")
    print(f"fixed cost: prepare_sampler {out['fixed_cost']['prepare_sampler_s'] * 1e3:.2f} ms per chain; " +
          "; ".join(f"{k}: warm-up {v['warmup_iteration_s'] * 1e3:.2f} ms, capture {v['capture_s'] * 1e3:.2f} ms, uncached call {v['uncached_call_s'] * 1e3:.1f} ms"
                    for k, v in parts.items()) +
          f"; K = 2 walk warm {k2['median_s'] * 1e3:.2f} ms (first call {k2['first_call_s'] * 1e3:.1f} ms)", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
