"""Wall time of the posterior covariance of device histories against a few target points on the shipped
lattice (cov and corr of every node with each target, the nodes' and the targets' mean and std), host call to
host results, by two routes in one process:

  covariance  TdContext.covariance_history (td_history_covariance): the volume's search structure, the nodes
              swept slab by slab, each slab reduced against the target series on the device (k_cov_targets);
              T x nq doubles per output come back
  yardstick   what there was before it: TdContext.volume_history(want_values=True) brings the value matrix
              V[nmodels][nq] to the host (the targets are lattice nodes, so their series are columns of it) and
              numpy reduces it: ((V - mean).T @ (A - mean_A)) / (M - 1)

numpy's matrix product associates differently: the largest differences of the two routes are reported, not
compared bit for bit.  Also reported: the covariance route's kernel times by HIP events (cov_targets,
vol_search, raster_stats, ...) and k_cov_targets' achieved bandwidth, 8 M nq ceil(T / G) bytes over its time.
Shapes: CHAINSxSAMPLESxCELLS (chains started at CELLS uniform cells, every 10th model recorded).

Each figure: one warm-up, then the median of --repeat runs (--yardstick-repeat for the yardstick).  One JSON
line per shape, printed and appended to profiles/covariance/covariance_rate.jsonl.

    python tools/covariance_rate.py [--repeat 10] [--shapes 8x1250x2000,8x1250x5000] [--targets 8] [--no-yardstick]
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

KERNELS = ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute", "raster_stats", "cov_center", "cov_targets")


def median_run(fn, repeat):
    fn()  # warm-up: allocations, first launches
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
        print("  %s %.4f s" % (fn.__name__, ts[-1]), file=sys.stderr, flush=True)
    return float(np.median(ts)), [round(t, 5) for t in ts], out


def kernel_ms(ctx, fn):
    ctx.timing(enable=True, reset=True)
    try:
        fn()
        return {k: dict(zip(("launches", "ms"), ctx.timing(kernel=k))) for k in KERNELS if ctx.timing(kernel=k)[0]}
    finally:
        ctx.timing(enable=False)


def rate(tt, ctx, ds, hists, ntargets, line, repeat, yard_repeat, out):
    xv, yv, zv = (np.asarray(v, dtype=np.float64).ravel() for v in (ds.xVec, ds.yVec, ds.zVec))
    qx = np.tile(xv, len(yv) * len(zv))
    qy = np.tile(np.repeat(yv, len(xv)), len(zv))
    qz = np.repeat(zv, len(xv) * len(yv))
    nq = len(qx)
    nmodels = sum(len(h) for h in hists)
    nodes = np.linspace(0, nq - 1, ntargets + 2).astype(np.int64)[1:-1]  # target points: lattice nodes, spread out
    targets = np.stack([qx[nodes], qy[nodes], qz[nodes]], axis=1)
    G = ctx.covariance_group()
    groups = -(-ntargets // G)

    def covariance():
        return ctx.covariance_history(hists, qx, qy, qz, targets)

    def yardstick():
        r = ctx.volume_history(hists, qx, qy, qz, want_values=True)
        V = r["values"]
        A = V[:, nodes]
        am, asd = A.mean(axis=0), A.std(axis=0, ddof=1)
        cov = (((V - r["mean"]).T @ (A - am)) / (nmodels - 1)).T
        with np.errstate(invalid="ignore", divide="ignore"):
            corr = cov / np.multiply.outer(asd, r["std"])
        return dict(cov=cov, corr=corr, mean=r["mean"], std=r["std"], target_mean=am, target_std=asd)

    plan = ctx.volume_plan(nmodels, nq)
    line.update({"nmodels": nmodels, "mean_cells": sum(h.count()[1] for h in hists) / nmodels, "nodes": nq,
                 "targets": ntargets, "group": G, "plan": plan, "repeat": repeat,
                 "bytes_to_host": 8 * (2 * ntargets * nq + 2 * nq + 2 * ntargets)})
    t, runs, r = median_run(covariance, repeat)
    ks = kernel_ms(ctx, covariance)
    line.update({"covariance_s": t, "covariance_all_s": runs, "covariance_kernel_ms": ks})
    slab_bytes = 8 * nmodels * nq * groups
    line["cov_targets_bytes"] = slab_bytes
    line["cov_targets_TB_per_s"] = slab_bytes / (ks["cov_targets"]["ms"] * 1e-3) / 1e12
    line["raster_stats_TB_per_s"] = 2 * 8 * nmodels * nq / (ks["raster_stats"]["ms"] * 1e-3) / 1e12  # (V read twice)
    if yard_repeat > 0:
        ty, runs_y, y = median_run(yardstick, yard_repeat)
        line.update({"yardstick_s": ty, "yardstick_all_s": runs_y, "yardstick_repeat": yard_repeat,
                     "yardstick_bytes_to_host": 8 * nmodels * nq, "yardstick_over_covariance": ty / t,
                     "covariance_not_slower": bool(t <= ty),
                     "mean_std_equal_bit_for_bit": bool(np.array_equal(r["mean"], y["mean"]) and
                                                        np.array_equal(r["std"], y["std"], equal_nan=True)),
                     "numpy_max_abs_diff": {f: float(np.nanmax(np.abs(r[f] - y[f]))) for f in
                                            ("cov", "corr", "target_mean", "target_std")},
                     "cov_abs_max": float(np.nanmax(np.abs(r["cov"])))})
    emit(line, out)


def shape_rate(tt, ctx, ds, shape, ntargets, repeat, yard_repeat, out):
    nchains, per, cells = (int(v) for v in shape.split("x"))
    prm = tt.define_TDstructrure().replace(max_cells=cells + 1000)
    hists = []
    for c in range(nchains):  # every 10th model of a chain started at `cells` uniform cells
        ch = tt.Chain(ctx, tt.chain_params(prm, ds, seed=2000 + c, chain=c + 1), tt.random_model(cells, 2000 + c))
        h = tt.History(ctx, per, per * (cells + 1000), with_ptS=False)
        ch.run_recorded(10 * per, 10, 10, h)
        ch.close()
        hists.append(h)
    rate(tt, ctx, ds, hists, ntargets, {"lattice": "shipped", "nchains": nchains, "models_per_chain": per, "cells": cells},
         repeat, yard_repeat, out)
    for h in hists:
        h.close()


def emit(line, out):
    line = json.dumps(line)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--yardstick-repeat", type=int, default=10)
    ap.add_argument("--shapes", default="8x1250x2000,8x1250x5000")
    ap.add_argument("--targets", type=int, default=8)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance", "covariance_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        shape_rate(tt, ctx, ds, shape, a.targets, a.repeat, 0 if a.no_yardstick else a.yardstick_repeat, a.out)


if __name__ == "__main__":
    main()
