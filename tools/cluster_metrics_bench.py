"""Times the k-means metrics of sample_ncsn.py --compute_metrics --cluster_metrics (csrc/kmeans.hip).

  python tools/cluster_metrics_bench.py [--channels 42,146,512] [--reps 20] [--out profiles/cluster_metrics_bench.json]
  python tools/cluster_metrics_bench.py --evaluate-only --channels 42      (one evaluate(); the run to put under rocprofv3)

Two shapes per C: n = 64,000 rows with k = 20 (the union PRD clusters) and n = 32,000 with k = 50 (the NDB bins).  For each:
smd_kmeans_assign, smd_kmeans_update and one whole Lloyd iteration (assign, the read of `changed`, update); the fused pair sums of
csrc/metrics.hip in full mode with ny = 128 at the same n and d -- the same Gram pass with a heavier epilogue, hence the
yardstick -- and a torch baseline (cdist + argmin + index_add_).  Every timed call takes the next of several operand sets, so no
call finds its inputs in the cache from the call before; the median of --reps calls is reported.  The assign pass is bound by
reading X once: GB/s counts n C 4 bytes.  Then whole evaluate() runs at sample_size = 1000 (32,000 frames of C, 22 comparisons)
with and without cluster_metrics.  One JSON line each.
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
import smd_amd.metrics as M  # noqa: E402

SETS = 4            # rotating operand sets
SHAPES = ((64000, 20, "prd_union"), (32000, 50, "ndb"))


def timed(fn, reps, warmup=2):
    """median and best milliseconds of fn(i), i counting the calls (the operand set is i % SETS)"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn(warmup + i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]
    return float(np.median(ts)), float(min(ts))


def torch_assign(x, c):
    return torch.cdist(x, c).argmin(1)


def torch_update(x, labels, c):
    sums = torch.zeros_like(c).index_add_(0, labels, x)
    counts = torch.bincount(labels, minlength=c.shape[0])
    return torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], c)


def lloyd_iteration(x, c, labels):
    labels, _, out = M._kmeans_assign(x, c, labels)
    out.cpu()                                                   # the wait of kmeans() for `changed`
    return M.kmeans_update(x, labels, c)[0]


class _Null:
    def scalar(self, *a, **k):
        pass

    def flush(self):
        pass


def bench_evaluate(c, reps, cluster_metrics, sample_size=1000):
    import sample_ncsn
    g = torch.Generator(device="cuda").manual_seed(c)
    coll = torch.clamp(0.25 * torch.randn(41, sample_size, 32, c, device="cuda", generator=g), -1, 1)
    real = torch.clamp(0.25 * torch.randn(sample_size, 32, c, device="cuda", generator=g), -1, 1).cpu().numpy()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sample_ncsn.evaluate(_Null(), real, coll, None, real, cluster_metrics=cluster_metrics)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="42,146,512")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-evaluate", action="store_true")
    ap.add_argument("--evaluate-only", action="store_true")
    ap.add_argument("--evaluate-reps", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    chans = [int(v) for v in a.channels.split(",")]
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
        if a.out:                                               # rewritten after every row: a run cut short keeps what it measured
            with open(a.out, "w") as f:
                for q in rows:
                    f.write(json.dumps(q) + "\n")

    if a.evaluate_only:
        for c in chans:
            emit({"what": "evaluate", "cluster_metrics": True, "C": c, "sample_size": 1000, "seconds": bench_evaluate(c, 1, True)})
        return
    dev = torch.device("cuda:0")
    emit({"device": torch.cuda.get_device_properties(dev).name, "reps": a.reps, "operand_sets": SETS,
          "shapes": [{"n": n, "k": k, "use": use} for n, k, use in SHAPES]})
    for c in chans:
        for n, k, use in SHAPES:
            g = torch.Generator(device=dev).manual_seed(c * 1000 + k)
            xs = [torch.clamp(0.25 * torch.randn(n, c, device=dev, generator=g), -1, 1) for _ in range(SETS)]
            cs = [x[torch.randperm(n, device=dev, generator=g)[:k]].contiguous() for x in xs]
            ys = [torch.clamp(0.25 * torch.randn(128, c, device=dev, generator=g), -1, 1) for _ in range(SETS)]
            labs = [M.kmeans_assign(x, cc)[0] for x, cc in zip(xs, cs)]
            labs64 = [l.long() for l in labs]
            gb = n * c * 4 / 1e9

            def row(what, med, best, **extra):
                emit(dict({"what": what, "use": use, "C": c, "n": n, "k": k, "ms_median": med, "ms_best": best,
                           "x_read_gb_per_s": gb / (med * 1e-3)}, **extra))

            med_p, best_p = timed(lambda i: M.pair_kernel_sums(xs[i % SETS], ys[i % SETS], 1.0, 1.0, 0.0, 2), a.reps)
            row("pair_kernel_sums_ny128", med_p, best_p, mode="full")
            med_a, best = timed(lambda i: M._kmeans_assign(xs[i % SETS], cs[i % SETS], None), a.reps)
            row("kmeans_assign", med_a, best, times_pair_sums=med_a / med_p)
            med_u, best = timed(lambda i: M.kmeans_update(xs[i % SETS], labs[i % SETS], cs[i % SETS]), a.reps)
            row("kmeans_update", med_u, best)
            med, best = timed(lambda i: lloyd_iteration(xs[i % SETS], cs[i % SETS], labs[i % SETS]), a.reps)
            row("lloyd_iteration", med, best, assign_plus_update_ms=med_a + med_u)
            if not a.no_baseline:
                med_ta, best = timed(lambda i: torch_assign(xs[i % SETS], cs[i % SETS]), a.reps)
                row("torch_cdist_argmin", med_ta, best)
                med_tu, best = timed(lambda i: torch_update(xs[i % SETS], labs64[i % SETS], cs[i % SETS]), a.reps)
                row("torch_index_add_means", med_tu, best, torch_iteration_over_lloyd_iteration=(med_ta + med_tu) / med)
            del xs, cs, ys, labs, labs64
            torch.cuda.empty_cache()
    if not a.no_evaluate:
        for c in chans:
            for on in (False, True):
                ts = bench_evaluate(c, a.evaluate_reps, on)
                emit({"what": "evaluate", "cluster_metrics": on, "prd_clusters": 20, "prd_runs": 10, "ndb_bins": 50, "C": c,
                      "sample_size": 1000, "frames": 32000, "comparisons": 22, "seconds": ts, "seconds_best": min(ts)})


if __name__ == "__main__":
    main()
