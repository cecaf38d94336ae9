"""Times the nearest-neighbour metrics of sample_ncsn.py --compute_metrics --nn_metrics (csrc/nn_metrics.hip).

  python tools/nn_metrics_bench.py [--n 32000] [--channels 42,146,512] [--k 3] [--reps 20] [--out profiles/nn_metrics_bench.json]
  python tools/nn_metrics_bench.py --evaluate-only --channels 42      (one evaluate(); the run to put under rocprofv3)

For each C at nx = ny = n: smd_knn_radii and smd_ball_cover (coverage + realism from one pass), the fused pair sums of
csrc/metrics.hip at the same shape -- the same Gram pass, hence the yardstick -- and a chunked fp32 torch baseline that
materialises 4096 x n distance tiles (cdist + topk for the radii, cdist + compare / divide for the cover).  Every timed call
takes the next of several operand sets, so no call finds its inputs in the cache from the call before; the median of --reps
calls is reported.  Effective TF/s counts the Gram's 2 n^2 C FLOP against the 157.3 TF fp32-MFMA peak (MI355X_MICROARCH.md).
Then one whole evaluate() with nn_metrics at sample_size = 1000 (32,000 frames of C, 22 comparisons).  One JSON line each.
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

PEAK_TF = 157.3
SETS = 4            # rotating operand sets


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


def torch_knn(x, k, chunk=4096):
    """fp32 torch: cdist tiles of chunk x n, self masked by index, topk"""
    out = torch.empty(x.shape[0], device=x.device)
    for i in range(0, x.shape[0], chunk):
        d2 = torch.cdist(x[i:i + chunk], x).square_()
        rows = torch.arange(d2.shape[0], device=x.device)
        d2[rows, rows + i] = float("inf")
        out[i:i + chunk] = d2.topk(k, dim=1, largest=False).values[:, k - 1]
    return out


def torch_cover(q, x, r2, keep, chunk=4096):
    cov = torch.empty(q.shape[0], dtype=torch.bool, device=q.device)
    real2 = torch.empty(q.shape[0], device=q.device)
    rk = torch.where(keep.bool(), r2, torch.zeros_like(r2))
    for i in range(0, q.shape[0], chunk):
        d2 = torch.cdist(q[i:i + chunk], x).square_()
        cov[i:i + chunk] = (d2 <= r2[None, :]).any(1)
        real2[i:i + chunk] = (rk[None, :] / d2.clamp_(min=1.1754944e-38)).amax(1)
    return cov, real2


class _Null:
    def scalar(self, *a, **k):
        pass

    def flush(self):
        pass


def bench_evaluate(c, reps, nn_metrics, k, sample_size=1000):
    import sample_ncsn
    g = torch.Generator(device="cuda").manual_seed(c)
    coll = torch.clamp(0.25 * torch.randn(41, sample_size, 32, c, device="cuda", generator=g), -1, 1)
    real = torch.clamp(0.25 * torch.randn(sample_size, 32, c, device="cuda", generator=g), -1, 1).cpu().numpy()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sample_ncsn.evaluate(_Null(), real, coll, None, real, nn_metrics=nn_metrics, nn_k=k)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32000)
    ap.add_argument("--channels", default="42,146,512")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-evaluate", action="store_true")
    ap.add_argument("--evaluate-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    chans = [int(v) for v in a.channels.split(",")]
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    if a.evaluate_only:
        for c in chans:
            emit({"what": "evaluate", "nn_metrics": True, "k": a.k, "C": c, "sample_size": 1000, "seconds": bench_evaluate(c, 1, True, a.k)})
        return
    dev = torch.device("cuda:0")
    emit({"device": torch.cuda.get_device_properties(dev).name, "n": a.n, "k": a.k, "reps": a.reps, "operand_sets": SETS,
          "peak_tf_f32_mfma": PEAK_TF})
    n, k = a.n, a.k
    for c in chans:
        g = torch.Generator(device=dev).manual_seed(c)
        xs = [torch.clamp(0.25 * torch.randn(n, c, device=dev, generator=g), -1, 1) for _ in range(SETS)]
        ys = [torch.clamp(0.9 * 0.25 * torch.randn(n, c, device=dev, generator=g) + 0.05, -1, 1) for _ in range(SETS)]
        r2s = [M.knn_radii(x, k) for x in xs]
        keeps = [M.median_keep_mask(r2) for r2 in r2s]
        flop = 2.0 * n * n * c

        def row(what, med, best, **extra):
            emit(dict({"what": what, "C": c, "n": n, "ms_median": med, "ms_best": best,
                       "tflops_effective": flop / (med * 1e-3) / 1e12, "frac_of_peak": flop / (med * 1e-3) / 1e12 / PEAK_TF}, **extra))

        med_p, best_p = timed(lambda i: M.pair_kernel_sums(xs[i % SETS], ys[i % SETS], 1.0, 1.0, 0.0, 2), a.reps)
        row("pair_kernel_sums", med_p, best_p, mode="full")
        med, best = timed(lambda i: M.knn_radii(xs[i % SETS], k), a.reps)
        row("knn_radii", med, best, k=k, times_pair_sums=med / med_p)
        med, best = timed(lambda i: M.ball_cover(ys[i % SETS], xs[i % SETS], r2s[i % SETS], keeps[i % SETS]), a.reps)
        row("ball_cover", med, best, times_pair_sums=med / med_p)
        if not a.no_baseline:
            reps = max(3, a.reps // 4)
            med, best = timed(lambda i: torch_knn(xs[i % SETS], k), reps, warmup=1)
            row("torch_fp32_chunked_knn", med, best, k=k)
            med, best = timed(lambda i: torch_cover(ys[i % SETS], xs[i % SETS], r2s[i % SETS], keeps[i % SETS]), reps, warmup=1)
            row("torch_fp32_chunked_cover", med, best)
        del xs, ys, r2s, keeps
        torch.cuda.empty_cache()
    if not a.no_evaluate:
        for c in chans:
            for nn in (False, True):
                ts = bench_evaluate(c, 3, nn, k)
                emit({"what": "evaluate", "nn_metrics": nn, "k": k, "C": c, "sample_size": 1000, "frames": 32000, "comparisons": 22,
                      "seconds": ts, "seconds_best": min(ts)})
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
