"""Cost and solver error of the third-order exponential Adams sampler on the base network (L6 H8 K2,
C = 512, T = 1000).  Writes profiles/adams_sampler_bench.json.
    python tools/adams_sampler_bench.py [--repeats 9] [--batch 256] [--error_batch 8]

(a) Wall time.  Whole N.sample() calls at B = `batch` (bf16) between two device synchronisations, on the lambda grid: the
second-order walk (the baseline: the multistep kernel, one history array), adams3 and adams3_pc (the Adams kernel, a ring of three)
on the SAME timesteps, in one process.  The two Adams solvers share one cache slot, so each is measured beside the order-2 walk
on its own: one cold call per configuration (it captures the graphs) and one discarded warm call, then `repeats` rounds that
visit the pair in turn, so a drift of the clocks falls on both alike; the median of each configuration's warm calls, the
difference to its baseline per iteration, and that baseline's own spread.

Every call builds its coefficient table on the host before it looks at the graph cache, so the host time of one table build --
the first (Python loops over the iterations) and a repeated one (the A columns kept by schedule.adams_coefficient_table) -- is
measured and reported on its own, beside the order-2 table's.

(b) Solver error.  Under --dtype=fp32 at B = `error_batch`: rel-L2 of the final state against the K = T, eta = 0 walk from the same
start, for K = 10, 20, 50.  This is the error of the ODE solver on a freshly initialised network, NOT sample quality.
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

CONFIGS = (("order2", dict(ddim_order=2)), ("adams3", dict(ddim_solver="adams3")), ("adams3_pc", dict(ddim_solver="adams3_pc")))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def host_timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--error_batch", type=int, default=8)
    ap.add_argument("--steps", type=int, nargs="*", default=[20, 50])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adams_sampler_bench.json"))
    a = ap.parse_args()
    B, T = a.batch, 1000
    betas = S.create_noise_schedule(1e-6, 0.01, T, "linear")
    out = dict(device=torch.cuda.get_device_name(0), T=T, network="TransformerDDPM L6 H8 K2 C512", repeats=a.repeats)

    # ---------------------------------------------------------------- (a) wall time, bf16, B = batch
    model = N.Model(NetConfig(architecture="TransformerDDPM", data_channels=512, seq_len=32, num_timesteps=T), "cuda:0", seed=0)
    seed = [100]

    def call(**kw):
        seed[0] += 1
        gen, _, _ = N.sample(model, betas, N.PRNGKey(seed[0]), (32, 512), num_samples=B, sampling="ddpm", ddim_eta=0.0,
                             ddim_spacing="logsnr", **kw)
        assert bool(torch.isfinite(gen).all())

    # host time of the coefficient tables alone, which every strided_dynamics call builds before it looks at its graph cache: the
    # first build (Python loops over the iterations) and a later one (the A columns kept by schedule.adams_coefficient_table)
    tables = {}
    for K in a.steps:
        taus = S.logsnr_timesteps(T, K, betas)
        row = dict(order2_ms=1e3 * statistics.median(host_timed(lambda: S.multistep_coefficient_table(betas, taus, 2)) for _ in range(5)))
        for name, corr in (("adams3", False), ("adams3_pc", True)):
            S._ADAMS_A_CACHE.clear()
            row[f"{name}_first_ms"] = 1e3 * host_timed(lambda: S.adams_coefficient_table(betas, taus, corr))
            row[f"{name}_again_ms"] = 1e3 * statistics.median(host_timed(lambda: S.adams_coefficient_table(betas, taus, corr)) for _ in range(5))
        tables[f"K{K}"] = row
        print(f"K = {K:3d} host table build: order 2 {row['order2_ms']:.2f} ms | adams3 first {row['adams3_first_ms']:.2f} ms, again "
              f"{row['adams3_again_ms']:.2f} ms | adams3_pc first {row['adams3_pc_first_ms']:.2f} ms, again {row['adams3_pc_again_ms']:.2f} ms", flush=True)
    S._ADAMS_A_CACHE.clear()
    out["host_table_build"] = dict(what="host wall time of one coefficient-table build, no GPU work; the sampling walls below contain "
                                   "one 'again' build per call (the first call of a walk: one 'first' build)", tables=tables)

    walks = {}
    for K in a.steps:
        # adams3 and adams3_pc share the cache slot "adams" (keyed by the solver), so a round that visited both would capture the
        # graphs again on every call; each is paired with the order-2 walk on its own, and the entry is checked to have stayed
        for name, kw in CONFIGS[1:]:
            pair = (CONFIGS[0], (name, kw))
            first, warm, its, arr = {}, {n: [] for n, _ in pair}, {}, {}
            for n_, kw_ in pair:
                first[n_] = timed(lambda: call(ddim_steps=K, **kw_))
                timed(lambda: call(ddim_steps=K, **kw_))
                its[n_], arr[n_] = model.sampler_arrangement["iterations"], dict(model.sampler_arrangement)
            entries = {k: model._sampler_graphs[k] for k in ("multistep", "adams")}
            for _ in range(a.repeats):
                for n_, kw_ in pair:
                    warm[n_].append(timed(lambda: call(ddim_steps=K, **kw_)))
            assert all(model._sampler_graphs[k] is v for k, v in entries.items()), "a warm call captured its graphs again"
            n = its["order2"]
            assert its[name] == n
            for n_, _ in pair:
                w = warm[n_]
                tag = f"K{K}_{n_}" if n_ != "order2" else f"K{K}_order2_beside_{name}"
                walks[tag] = dict(first_call_s=first[n_], warm_s=w, median_s=statistics.median(w), min_s=min(w), max_s=max(w),
                                  iterations=n, per_iteration_ms=1e3 * statistics.median(w) / n, kernel=arr[n_]["walk"], arrangement=arr[n_])
                print(f"K = {K:3d} {tag[len(f'K{K}_'):]:24s} ({n} iterations, {arr[n_]['walk']} kernel): first {first[n_]:.3f} s, warm median "
                      f"{statistics.median(w) * 1e3:.2f} ms [{min(w) * 1e3:.2f}, {max(w) * 1e3:.2f}] = {1e3 * statistics.median(w) / n:.3f} ms per iteration",
                      flush=True)
        cost = {}
        for name in ("adams3", "adams3_pc"):
            r, base = walks[f"K{K}_{name}"], walks[f"K{K}_order2_beside_{name}"]
            cost[f"{name}_minus_order2_us_per_iteration_median"] = 1e6 * (r["median_s"] - base["median_s"]) / r["iterations"]
            cost[f"{name}_minus_order2_us_per_iteration_min"] = 1e6 * (r["min_s"] - base["min_s"]) / r["iterations"]
            cost[f"spread_of_the_order2_walk_beside_{name}_us_per_iteration"] = 1e6 * (base["max_s"] - base["min_s"]) / r["iterations"]
        walks[f"K{K}_update_cost"] = cost
        print(f"K = {K:3d} per iteration over the order-2 walk: adams3 {cost['adams3_minus_order2_us_per_iteration_median']:+.2f} us, adams3_pc "
              f"{cost['adams3_pc_minus_order2_us_per_iteration_median']:+.2f} us (medians); the order-2 walks alone spread over "
              f"{cost['spread_of_the_order2_walk_beside_adams3_us_per_iteration']:.2f} / {cost['spread_of_the_order2_walk_beside_adams3_pc_us_per_iteration']:.2f} us per iteration",
              flush=True)
    out["wall_time"] = dict(batch=B, dtype="bf16", grid="logsnr", method="N.sample() wall time between device synchronisations; per "
                            "configuration one capturing call and one discarded warm call, then rounds that visit the order-2 walk and ONE "
                            "Adams solver in turn (other seeds, cached graphs, checked not to be captured again); median of the warm calls", walks=walks)
    model.drop_sampler_cache()
    del model

    # ---------------------------------------------------------------- (b) solver error, fp32
    Be = a.error_batch
    m32 = N.Model(NetConfig(architecture="TransformerDDPM", data_channels=512, seq_len=32, num_timesteps=T, dtype="fp32"), "cuda:0", seed=0)
    init = torch.randn(Be, 32, 512, generator=torch.Generator().manual_seed(1)).cuda()
    full, _, _ = N.strided_dynamics(N.PRNGKey(0), m32, betas, init, T, 0.0)
    rel = lambda x: float((x.double() - full.double()).norm() / full.double().norm())
    err = {}
    names = ("order1", "order2", "adams3", "adams3_pc")
    for K in (10, 20, 50):
        for name, kw in (("order1", dict(order=1)), ("order2", dict(order=2)), ("adams3", dict(solver="adams3")), ("adams3_pc", dict(solver="adams3_pc"))):
            x, _, _ = N.strided_dynamics(N.PRNGKey(0), m32, betas, init, K, 0.0, spacing="logsnr", **kw)
            err[f"K{K}_{name}"] = dict(rel_l2=rel(x), iterations=m32.sampler_arrangement["iterations"])
        print(f"K = {K:3d} ({err[f'K{K}_order1']['iterations']} it., logsnr) rel-L2 against the K = T walk: " +
              ", ".join(f"{n} {err[f'K{K}_{n}']['rel_l2']:.3e}" for n in names), flush=True)
    out["solver_error"] = dict(batch=Be, dtype="fp32", grid="logsnr", reference="strided_dynamics(K = T = 1000, eta = 0) from the same start",
                               what="error of the ODE solver on a freshly initialised network (seed 0): NOT sample quality", rel_l2=err)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
