"""Times the evaluation distances of sample_ncsn.py --compute_metrics (csrc/metrics.hip).

  python tools/metrics_bench.py [--n 32000] [--channels 42,146,512] [--reps 5] [--out profiles/metrics_bench.json]
  python tools/metrics_bench.py --evaluate-only --channels 42      (one evaluate(); the run to put under rocprofv3)

For each C: the fused pair sums (RBF + polynomial from one Gram pass) at nx = ny = n in full and symmetric mode, the moments,
and a chunked fp32 torch baseline that materialises 4096 x n tiles of the Gram and kernel matrices.  Effective TF/s counts
the Gram's 2 n^2 C FLOP (full) or n (n + 1) C (symmetric: the upper triangle) against the 157.3 TF fp32-MFMA peak
(MI355X_MICROARCH.md).  Then one whole evaluate() at sample_size = 1000 (32,000 frames of C: 20 collection points + the
random and real controls).  Prints one JSON line per measurement.
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


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    ts = []
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]
    return float(np.median(ts)), float(min(ts))


def torch_baseline(x, y, chunk=4096):
    """fp32 torch: Gram tiles of chunk x n, materialised distances and kernels, fp64 sums."""
    yy = (y * y).sum(1)
    sr = torch.zeros((), dtype=torch.float64, device=x.device)
    sp = torch.zeros((), dtype=torch.float64, device=x.device)
    for i in range(0, x.shape[0], chunk):
        xc = x[i:i + chunk]
        g = xc @ y.T
        d2 = torch.clamp((-2.0 * g + (xc * xc).sum(1)[:, None]) + yy[None, :], min=0)
        sr += torch.exp(-d2).sum(dtype=torch.float64)
        sp += (g * g).sum(dtype=torch.float64)
    return sr, sp


class _Null:
    def scalar(self, *a, **k):
        pass

    def flush(self):
        pass


def bench_evaluate(c, reps, sample_size=1000):
    import sample_ncsn
    g = torch.Generator(device="cuda").manual_seed(c)
    coll = torch.rand(41, sample_size, 32, c, device="cuda", generator=g) * 2 - 1
    real = (torch.rand(sample_size, 32, c, device="cuda", generator=g) * 2 - 1).cpu().numpy()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sample_ncsn.evaluate(_Null(), real, coll, None, real)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32000)
    ap.add_argument("--channels", default="42,146,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
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
            ts = bench_evaluate(c, 1)
            emit({"what": "evaluate", "C": c, "sample_size": 1000, "seconds": ts})
        return
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    emit({"device": props.name, "n": a.n, "peak_tf_f32_mfma": PEAK_TF})
    n = a.n
    for c in chans:
        g = torch.Generator(device=dev).manual_seed(c)
        x = torch.rand(n, c, device=dev, generator=g) * 2 - 1
        y = torch.rand(n, c, device=dev, generator=g) * 2 - 1
        for mode in ("full", "symmetric"):
            yy = None if mode == "symmetric" else y
            med, best = timed(lambda: M.pair_kernel_sums(x, yy, 1.0, 1.0, 0.0, 2), a.reps)
            flop = 2.0 * n * n * c if mode == "full" else 1.0 * n * (n + 1) * c
            pairs = n * n if mode == "full" else n * (n + 1) // 2
            emit({"what": "pair_kernel_sums", "mode": mode, "C": c, "n": n, "ms_median": med, "ms_best": best,
                  "tflops_effective": flop / (med * 1e-3) / 1e12, "frac_of_peak": flop / (med * 1e-3) / 1e12 / PEAK_TF,
                  "gpairs_per_s": pairs / (med * 1e-3) / 1e9})
        med, best = timed(lambda: M.moments(x), a.reps)
        emit({"what": "moments", "C": c, "n": n, "ms_median": med, "ms_best": best})
        if not a.no_baseline:
            med, best = timed(lambda: torch_baseline(x, y), max(2, a.reps // 2), warmup=1)
            flop = 2.0 * n * n * c
            emit({"what": "torch_fp32_chunked_baseline", "mode": "full", "C": c, "n": n, "ms_median": med, "ms_best": best,
                  "tflops_effective": flop / (med * 1e-3) / 1e12})
        del x, y
        torch.cuda.empty_cache()
    for c in chans:
        ts = bench_evaluate(c, 3)
        emit({"what": "evaluate", "C": c, "sample_size": 1000, "frames": 32000, "comparisons": 22, "seconds": ts,
              "seconds_best": min(ts)})
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
