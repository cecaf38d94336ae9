"""Times the nearest-neighbour search of sample_ncsn.py --copy_metrics (csrc/nn_search.hip).

  python tools/copy_metrics_bench.py [--n 32000] [--channels 42,146,512] [--ks 1,3,8] [--reps 20] [--out profiles/copy_metrics_bench.json]

For each C and k at nq = nx = n: smd_nn_search (self excluded, as the training set's own radii are built) against smd_knn_radii
of the same build at the same shape and k -- the same Gram pass without the indices, hence the yardstick -- and a chunked fp32
torch baseline that materialises 4096 x n distance tiles (cdist + topk with indices).  The protocol is that of
tools/nn_metrics_bench.py: every timed call takes the next of several operand sets, so no call finds its inputs in the cache
from the call before; the median of --reps calls is reported.  Effective TF/s counts the Gram's 2 n^2 C FLOP against the 157.3 TF
fp32-MFMA peak.  One JSON line each.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import smd_amd  # noqa: E402,F401
import smd_amd.metrics as M  # noqa: E402
from nn_metrics_bench import PEAK_TF, SETS, timed  # noqa: E402


def torch_search(x, k, chunk=4096):
    """fp32 torch: cdist tiles of chunk x n, self masked by index, topk with its indices"""
    d2_out = torch.empty(x.shape[0], k, device=x.device)
    idx_out = torch.empty(x.shape[0], k, dtype=torch.int64, device=x.device)
    for i in range(0, x.shape[0], chunk):
        d2 = torch.cdist(x[i:i + chunk], x).square_()
        rows = torch.arange(d2.shape[0], device=x.device)
        d2[rows, rows + i] = float("inf")
        top = d2.topk(k, dim=1, largest=False)
        d2_out[i:i + chunk], idx_out[i:i + chunk] = top.values, top.indices
    return d2_out, idx_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32000)
    ap.add_argument("--channels", default="42,146,512")
    ap.add_argument("--ks", default="1,3,8")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    dev = torch.device("cuda:0")
    n = a.n
    emit({"device": torch.cuda.get_device_properties(dev).name, "n": n, "reps": a.reps, "operand_sets": SETS, "peak_tf_f32_mfma": PEAK_TF})
    for c in [int(v) for v in a.channels.split(",")]:
        g = torch.Generator(device=dev).manual_seed(c)
        xs = [torch.clamp(0.25 * torch.randn(n, c, device=dev, generator=g), -1, 1) for _ in range(SETS)]
        flop = 2.0 * n * n * c
        for k in [int(v) for v in a.ks.split(",")]:
            def row(what, med, best, **extra):
                emit(dict({"what": what, "C": c, "n": n, "k": k, "ms_median": med, "ms_best": best,
                           "tflops_effective": flop / (med * 1e-3) / 1e12, "frac_of_peak": flop / (med * 1e-3) / 1e12 / PEAK_TF}, **extra))

            med_r, best_r = timed(lambda i: M.knn_radii(xs[i % SETS], k), a.reps)
            row("knn_radii", med_r, best_r)
            med, best = timed(lambda i: M.nn_search(xs[i % SETS], xs[i % SETS], k, exclude_self=True), a.reps)
            row("nn_search", med, best, times_knn_radii=med / med_r)
            if not a.no_baseline:
                med_t, best_t = timed(lambda i: torch_search(xs[i % SETS], k), max(3, a.reps // 4), warmup=1)
                row("torch_fp32_chunked_search", med_t, best_t, times_nn_search=med_t / med)
        del xs
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
