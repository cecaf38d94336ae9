"""Times the analytic reverse variance (csrc/analytic.hip, ncsn.estimate_score_moments, strided_dynamics(analytic=...)).

  python tools/analytic_bench.py [--batch 256] [--warm 3] [--reps 200] [--kernels-only] [--out profiles/analytic_bench.json]

Base network (32 x 512 latents, 6 layers, mlp 2048 x 2), T = 1000, bf16, in ONE process:
  * the estimator walk over all T timesteps against the bound walk on the same batch: first call (tables, FiLM tables, warm-up
    step, graph capture) and the median of --warm later calls on the cached graphs, host clock around work that ends in a device
    synchronise;
  * smd_score_moments alone beside smd_bound_terms alone, device events around each call, median of --reps calls, every call
    on the next of several operand sets (no call finds its inputs in the cache from the call before).  score_moments reads two
    fp32 arrays (and writes B / 8 partial rows), bound_terms reads three;
  * one iteration of smd_engine_analytic_step beside one of smd_engine_strided_step (the network forward + the fused update:
    the library has no entry for either update alone), the same way; the difference of the two medians is the difference of
    the update kernels -- the expectation is one L2-shared read of S C floats per sample;
  * a K = 20 element-mode sampling run against the same run without the variance, first call and warm median.
One JSON document.  --kernels-only skips the walks (and takes a random g): the run to put under
`rocprofv3 --kernel-trace --stats`, whose per-kernel durations separate the two fused updates from the network in front of them
(profiles/analytic_bench_kernel_stats.txt).
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
K = 20


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
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analytic_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    B, Sq, Cn = a.batch, 32, 512
    betas = S.create_noise_schedule(1e-6, 1e-2, T, "linear")
    model = N.Model(NetConfig(data_channels=Cn, num_layers=6, num_heads=8, num_mlp_layers=2, num_timesteps=T), dev, seed=0)
    g = torch.Generator().manual_seed(0)
    x0 = torch.clamp(0.25 * torch.randn(B, Sq, Cn, generator=g), -1, 1).to(dev)
    res = dict(device=torch.cuda.get_device_name(0), batch=B, shape=[Sq, Cn], timesteps=T, dtype="bf16")

    taus = S.stride_timesteps(T, K)
    ge = np.random.default_rng(0).uniform(0.2, 0.95, (K, Sq, Cn))
    if not a.kernels_only:
        # ---- walks
        first = wall(lambda: N.variational_bound(N.PRNGKey(1), model, betas, x0))
        warm = [wall(lambda i=i: N.variational_bound(N.PRNGKey(2 + i), model, betas, x0)) for i in range(a.warm)]
        res["bound_walk"] = dict(first_call_s=first, warm_median_s=float(np.median(warm)), warm_s=warm)
        model.drop_sampler_cache()
        out = {}
        first = wall(lambda: out.update(g=N.estimate_score_moments(model, betas, x0, np.arange(T), rng=N.PRNGKey(1), batch=B)[0]))
        warm = [wall(lambda i=i: N.estimate_score_moments(model, betas, x0, np.arange(T), rng=N.PRNGKey(2 + i), batch=B)) for i in range(a.warm)]
        res["estimator_walk"] = dict(first_call_s=first, warm_median_s=float(np.median(warm)), warm_s=warm,
                                     vs_bound_walk=float(np.median(warm)) / res["bound_walk"]["warm_median_s"],
                                     g_mean=float(np.clip(out["g"], 0, 1).mean()))
        model.drop_sampler_cache()

        # ---- the K = 20 sampling run, element mode against none
        ge = out["g"][taus]
        init = torch.randn(B, Sq, Cn, generator=g).to(dev)
        for name, kw in (("sampling_none", {}), ("sampling_element", dict(analytic=("element", ge)))):
            first = wall(lambda: N.strided_dynamics(N.PRNGKey(1), model, betas, init, K, 1.0, **kw))
            warm = [wall(lambda i=i: N.strided_dynamics(N.PRNGKey(2 + i), model, betas, init, K, 1.0, **kw)) for i in range(a.warm)]
            res[name] = dict(first_call_s=first, warm_median_s=float(np.median(warm)), warm_s=warm, arrangement=dict(model.sampler_arrangement))
            model.drop_sampler_cache()
        res["sampling_element"]["vs_none"] = res["sampling_element"]["warm_median_s"] / res["sampling_none"]["warm_median_s"]

    # ---- kernels alone
    L = lib.get_lib()
    st = lambda: torch.cuda.current_stream().cuda_stream
    table = torch.from_numpy(S.bound_tables(betas, np.arange(T))["table"]).to(dev)
    mtab = torch.from_numpy(S.analytic_moment_tables(betas, np.arange(T), "eps")[0]).to(dev)
    tp = torch.tensor([500], dtype=torch.int32, device=dev)
    chunks = (B + lib.MOMENT_CHUNK - 1) // lib.MOMENT_CHUNK
    sets = [dict(x0=x0.clone(), eps=torch.randn_like(x0), eh=torch.randn_like(x0), xt=torch.randn_like(x0),
                 part=torch.zeros((T, B, 3), device=dev), mpart=torch.zeros((chunks, Sq, Cn), device=dev),
                 sums=torch.zeros((T, Sq, Cn), device=dev)) for _ in range(SETS)]

    def terms(i):
        s = sets[i % SETS]
        lib.check(L.smd_bound_terms(s["x0"].data_ptr(), s["eps"].data_ptr(), s["eh"].data_ptr(), B, Sq, Cn, table.data_ptr(), T, 1.0,
                                    tp.data_ptr(), None, None, s["part"].data_ptr(), st()), "bound_terms")

    def moments(i):
        s = sets[i % SETS]
        lib.check(L.smd_score_moments(s["xt"].data_ptr(), s["eh"].data_ptr(), B, Sq, Cn, mtab.data_ptr(), T, tp.data_ptr(), None, None,
                                      s["mpart"].data_ptr(), s["sums"].data_ptr(), st()), "score_moments")

    per = B * Sq * Cn * 4
    res["kernels"] = {}
    for name, fn, nbytes in (("bound_terms", terms, 3 * per), ("score_moments", moments, 2 * per + 2 * chunks * Sq * Cn * 4)):
        med, best = timed(fn, a.reps)
        res["kernels"][name] = dict(median_us=med, best_us=best, gb_per_s=nbytes / med * 1e-3, launches=2 if name == "score_moments" else 1)
    res["kernels"]["score_moments"]["vs_bound_terms"] = res["kernels"]["score_moments"]["median_us"] / res["kernels"]["bound_terms"]["median_us"]

    # ---- one engine iteration: network forward + fused update
    eng = model.engine
    N._ensure_schedule(eng, betas, with_sampler=True)
    eng.bind(B, training=False)
    eng.refresh_weights()
    eng.prepare_sampler()
    coef, plan = S.strided_coefficient_table(betas, taus, 1.0)
    c_on = coef.copy()
    c_on[taus, 4] = 1.0
    keep = [torch.from_numpy(v).to(dev) for v in (coef, plan, c_on)]
    sp, spa = lib.StridePlan(), lib.StridePlan()
    sp.coef, sp.plan, sp.T = keep[0].data_ptr(), keep[1].data_ptr(), T
    spa.coef, spa.plan, spa.T = keep[2].data_ptr(), keep[1].data_ptr(), T
    sig = torch.from_numpy(S.analytic_sigma_table(betas, taus, 1.0, ge)).to(dev)
    sgt = lib.SigmaTable()
    sgt.sig, sgt.K = sig.data_ptr(), K
    t_mid = int(taus[K // 2])
    states = [torch.randn_like(x0) for _ in range(SETS)]
    ios = []
    for x in states:
        io = lib.SampleIO()
        io.x, io.t_ptr, io.seed_lo = x.data_ptr(), tp.data_ptr(), 7
        ios.append(io)

    def strided(i):
        tp.fill_(t_mid)
        eng.strided_step(ios[i % SETS], sp)

    def analytic(i):
        tp.fill_(t_mid)
        eng.analytic_step(ios[i % SETS], spa, sgt)

    eng.load_state(states[0])
    res["iteration"] = {}
    for name, fn in (("strided_step", strided), ("analytic_step", analytic), ("strided_step_again", strided)):
        med, best = timed(fn, a.reps)
        res["iteration"][name] = dict(median_us=med, best_us=best)
    it = res["iteration"]
    it["analytic_minus_strided_us"] = it["analytic_step"]["median_us"] - 0.5 * (it["strided_step"]["median_us"] + it["strided_step_again"]["median_us"])
    it["note"] = "network forward + fused update per call (plus one 4-byte fill of the timestep); the updates alone have no entry point"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
