"""Wall time of the posterior marginals of one cross-section (quantiles 5 / 50 / 95 % and a 50-bin
histogram on [0, 50) per node), host to host, by two routes in one process:

  device  TdContext.marginals (td_rasterize_marginals): value matrix, order statistics and counts on
          the device; only the results come back
  host    what there was before it: TdContext.rasterize(..., want_values=True) brings the
          nmodels x nq value matrix to the host, then np.sort per column, Julia's quantile formula and
          floor((v - lo) / w) counted per column in numpy

at two shapes over the xz section of the shipped grid: 100 models x 5000 cells (a reference-sized
model_hist) and 10000 models x 200 cells (a densely thinned device history).  Each route: one warm-up,
then the median of --repeat runs; the device route's kernels by HIP events as well, and the quantile
kernel of the streaming regime forced at the same shape.  The two routes'
results are compared bit for bit.  One JSON line per shape, printed and appended to
profiles/marginals/marginals_rate.jsonl.

    python tools/marginals_rate.py [--repeat 10] [--shapes 100x5000,10000x200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tonga  # noqa: E402

PROBS = (0.05, 0.5, 0.95)
BINS = (50, 0.0, 50.0)
KERNELS = ("raster_brute", "raster_quantile", "raster_node_hist")


def host_marginals(V, probs, bins):
    M, nq = V.shape
    S = np.sort(V, axis=0)
    quant = np.empty((len(probs), nq))
    for i, p in enumerate(probs):
        aleph = M * p + (1 - p)
        j = min(max(int(np.trunc(aleph)), 1), max(M - 1, 1))
        g = min(max(aleph - j, 0.0), 1.0)
        a, b = S[j - 1], (S[0] if M == 1 else S[j])
        quant[i] = a + g * (b - a)
    quant[:, np.isnan(V).any(axis=0)] = np.nan
    nbins, lo, hi = bins
    w = (hi - lo) / nbins
    with np.errstate(invalid="ignore"):
        s = 1 + np.minimum(np.nan_to_num(np.floor((V - lo) / w)), nbins - 1).astype(np.int64)
        s[V < lo] = 0
        s[V >= hi] = nbins + 1
    s[np.isnan(V)] = nbins + 2
    s += np.arange(nq, dtype=np.int64) * (nbins + 3)
    hist = np.bincount(s.ravel(), minlength=nq * (nbins + 3)).reshape(nq, nbins + 3)
    return quant, hist


def median_run(fn, repeat):
    fn()  # warm-up: allocations, first launches
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [round(t, 5) for t in ts], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--shapes", default="100x5000,10000x200")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginals", "marginals_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    xv, zv = np.asarray(ds.xVec, dtype=np.float64), np.asarray(ds.zVec, dtype=np.float64)
    qx, qz = np.tile(xv, len(zv)), np.repeat(zv, len(xv))
    qy = np.full(qx.shape, 150.0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        nmodels, cells = (int(v) for v in shape.split("x"))
        models = [tt.random_model(cells, 1000 + k).cells() for k in range(nmodels)]

        def device():
            return ctx.marginals(models, qx, qy, qz, PROBS, BINS)

        def host():
            mean, std, V = ctx.rasterize(models, qx, qy, qz, want_values=True)
            quant, hist = host_marginals(V, PROBS, BINS)
            return dict(mean=mean, std=std, quantiles=quant, hist=hist)

        t_dev, all_dev, r_dev = median_run(device, a.repeat)
        t_host, all_host, r_host = median_run(host, a.repeat)
        ctx.timing(enable=True, reset=True)
        device()
        kernel_ms = {k: ctx.timing(kernel=k)[1] for k in KERNELS}
        # the same request through the streaming regime (the radix select takes over beyond
        # marginals_resident_max models; forced here to time it at the same shape)
        ctx.set_marginals_method(tt.TdContext.MARG_STREAMING)
        ctx.timing(reset=True)
        r_stream = device()
        stream_ms = ctx.timing(kernel="raster_quantile")[1]
        ctx.set_marginals_method(tt.TdContext.MARG_AUTO)
        ctx.timing(enable=False)
        equal = np.array_equal(r_stream["quantiles"], r_dev["quantiles"], equal_nan=True) and \
            all(np.array_equal(r_dev[f], r_host[f], equal_nan=True) for f in ("mean", "std", "quantiles")) and \
            np.array_equal(r_dev["hist"], r_host["hist"])
        line = json.dumps({"nmodels": nmodels, "cells": cells, "nq": len(qx), "probs": PROBS, "bins": BINS,
                           "repeat": a.repeat, "device_s": t_dev, "host_s": t_host, "host_over_device": t_host / t_dev,
                           "device_not_slower": bool(t_dev <= t_host), "kernel_ms": kernel_ms,
                           "raster_quantile_streaming_ms": stream_ms,
                           "device_all_s": all_dev, "host_all_s": all_host, "results_equal": bool(equal)})
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
