"""Wall time of the posterior region averages of device histories on the shipped lattice (series, weight, mean,
std, quantiles, histograms, R-hat, ESS, greater), host call to host results, by two routes in one process:

  regions    TdContext.regions_history (td_history_regions): the volume's search structure, the regions' points
             swept slab by slab, each slab reduced over its columns on the device (k_region_sums), the leaves
             combined (k_region_combine), the pairs counted (k_region_greater), the statistics of the [M, R] series
             by the volume's own kernels
  yardstick  what there was before it: TdContext.volume_history(want_values=True) brings the value matrix
             V[nmodels][nq] of the lattice to the host and numpy forms the series from it (both sums in
             oracle_np.julia_mapreduce_arrays' association, so that the two routes can be compared bit for bit),
             then mean, std, quantiles and the pair counts

`series`, `weight` and `greater` of both routes are compared for equality.  Also reported: the bytes each route
brings to the host, the device route's kernel times by HIP events, the read rate of k_region_sums (8 bytes x models
x points over its time) against the 6.29 TB/s measured HBM rate, and the share of the call that is sweep, region
kernels, statistics and the rest (copies, host work).  Region sets: `layers`, one region per depth node of the
lattice (every node of the lattice once), and `boxes`, 8 boxes (the octants of the lattice's index space), both
with volume weights.
Shapes: CHAINSxSAMPLESxCELLS (chains started at CELLS uniform cells, every 10th model recorded).

Each figure: one warm-up, then the median of --repeat runs (--yardstick-repeat for the yardstick).  One JSON line
per shape and region set, printed and appended to profiles/regions/regions_rate.jsonl.

    python tools/regions_rate.py [--repeat 10] [--shapes 8x1250x2000,8x1250x5000] [--no-yardstick]
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
from oracle import oracle_np  # noqa: E402

KERNELS = ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute", "region_sums", "region_combine", "region_greater",
           "raster_stats")
HBM_TB_PER_S = 6.29
PROBS, BINS = (0.05, 0.5, 0.95), (64, 0.0, 50.0)


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


def tree(T):
    """The sum along the last axis in td_rasterize's association (tests/regions_ref.py's tree_sum)."""
    return oracle_np.julia_mapreduce_arrays([T[..., k] for k in range(T.shape[-1])])


def region_sets(tt, xv, yv, zv):
    layers = {"z %g" % z: (np.arange(len(zv)) == k).reshape(1, 1, -1) for k, z in enumerate(zv)}
    boxes = {}
    for a, (x0, x1) in enumerate(((0, len(xv) // 2), (len(xv) // 2, len(xv)))):
        for b, (y0, y1) in enumerate(((0, len(yv) // 2), (len(yv) // 2, len(yv)))):
            for c, (z0, z1) in enumerate(((0, len(zv) // 2), (len(zv) // 2, len(zv)))):
                boxes["box %d%d%d" % (a, b, c)] = tt.box_region(xv, yv, zv, (xv[x0], yv[y0], zv[z0]),
                                                                (xv[x1 - 1], yv[y1 - 1], zv[z1 - 1]))
    return {"layers": layers, "boxes": boxes}


def rate(tt, ctx, ds, hists, line, repeat, yard_repeat, out):
    xv, yv, zv = (np.asarray(v, dtype=np.float64).ravel() for v in (ds.xVec, ds.yVec, ds.zVec))
    nx, ny, nz = len(xv), len(yv), len(zv)
    nq = nx * ny * nz
    qx = np.tile(xv, ny * nz)
    qy = np.tile(np.repeat(yv, nx), nz)
    qz = np.repeat(zv, nx * ny)
    nmodels = sum(len(h) for h in hists)
    total_cells = sum(h.count()[1] for h in hists)
    for set_name, regs in region_sets(tt, xv, yv, zv).items():
        names, px, py, pz, w, off = tt.region_points(regs, xv, yv, zv, "volume")
        R, npts = len(names), len(px)
        # the flat node of every point: the yardstick's columns of V
        node = (np.searchsorted(xv, px) + nx * (np.searchsorted(yv, py) + ny * np.searchsorted(zv, pz))).astype(np.int64)

        def regions():
            return ctx.regions_history(hists, px, py, pz, off, w, True, PROBS, BINS, convergence=True)

        def volume_same_points():  # a posterior volume with the same statistics on the same points
            return ctx.volume_history(hists, px, py, pz, PROBS, BINS, convergence=True)

        def yardstick():
            V = ctx.volume_history(hists, qx, qy, qz, want_values=True)["values"]
            F = np.empty((nmodels, R))
            W = np.empty(R)
            for r in range(R):
                lo, hi = int(off[r]), int(off[r + 1])
                W[r] = tree(w[lo:hi])
                F[:, r] = tree(w[lo:hi] * V[:, node[lo:hi]]) / W[r]
            mean, std = F.mean(axis=0), F.std(axis=0, ddof=1)
            quant = np.quantile(F, PROBS, axis=0)
            greater = np.sum(F[:, :, None] > F[:, None, :], axis=0).astype(np.int64)
            return dict(series=F, weight=W, mean=mean, std=std, quantiles=quant, greater=greater)

        nodes, nslabs = ctx.regions_plan(nmodels, npts)
        ln = dict(line)
        ln.update({"regions": set_name, "nreg": R, "points": npts, "nmodels": nmodels, "mean_cells": total_cells / nmodels,
                   "lattice": [nx, ny, nz], "plan": [nodes, nslabs], "repeat": repeat,
                   "bytes_to_host": 8 * (nmodels * R + R + 2 * R + len(PROBS) * R + R * (BINS[0] + 3) + 2 * R + R * R) + 4 * R})
        t, runs, r = median_run(regions, repeat)
        ks = kernel_ms(ctx, regions)
        tv, runs_v, _ = median_run(volume_same_points, repeat)
        ln.update({"regions_s": t, "regions_all_s": runs, "regions_kernel_ms": ks, "volume_same_points_s": tv,
                   "volume_same_points_all_s": runs_v, "regions_over_volume": t / tv})
        sweep_ms = sum(ks[k]["ms"] for k in ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute") if k in ks)
        sums_ms = ks["region_sums"]["ms"]
        tail_ms = ks["region_combine"]["ms"] + ks["region_greater"]["ms"]
        stats_ms = ks["raster_stats"]["ms"]
        sums_bytes = 8 * nmodels * npts
        ln["region_sums_bytes"] = sums_bytes
        ln["region_sums_TB_per_s"] = sums_bytes / (sums_ms * 1e-3) / 1e12
        ln["region_sums_share_of_hbm_rate"] = ln["region_sums_TB_per_s"] / HBM_TB_PER_S
        call_ms = t * 1e3
        ln["share_of_call"] = {"sweep": sweep_ms / call_ms, "region_sums": sums_ms / call_ms,
                               "combine_and_greater": tail_ms / call_ms, "statistics": stats_ms / call_ms,
                               "copies_and_host": 1.0 - (sweep_ms + sums_ms + tail_ms + stats_ms) / call_ms}
        if yard_repeat > 0:
            ty, runs_y, y = median_run(yardstick, yard_repeat)
            equal = {f: bool(np.array_equal(r[f], y[f], equal_nan=True)) for f in ("series", "weight", "greater")}
            close = {f: bool(np.allclose(r[f], y[f], rtol=1e-9, atol=0, equal_nan=True)) for f in ("mean", "std", "quantiles")}
            g = r["greater"]
            ln.update({"yardstick_s": ty, "yardstick_all_s": runs_y, "yardstick_repeat": yard_repeat,
                       "yardstick_bytes_to_host": 8 * nmodels * nq + 2 * 8 * nq, "yardstick_over_regions": ty / t,
                       "equal_bit_for_bit": equal, "all_equal": all(equal.values()), "statistics_close": close,
                       "pairs_with_0_lt_greater_lt_M": int(np.sum((g > 0) & (g < nmodels))), "pairs": R * (R - 1)})
        emit(ln, out)


def shape_rate(tt, ctx, ds, shape, repeat, yard_repeat, out):
    nchains, per, cells = (int(v) for v in shape.split("x"))
    prm = tt.define_TDstructrure().replace(max_cells=cells + 1000)
    hists = []
    for c in range(nchains):  # every 10th model of a chain started at `cells` uniform cells
        ch = tt.Chain(ctx, tt.chain_params(prm, ds, seed=2000 + c, chain=c + 1), tt.random_model(cells, 2000 + c))
        h = tt.History(ctx, per, per * (cells + 1000), with_ptS=False)
        ch.run_recorded(10 * per, 10, 10, h)
        ch.close()
        hists.append(h)
    rate(tt, ctx, ds, hists, {"nchains": nchains, "models_per_chain": per, "cells": cells}, repeat, yard_repeat, out)
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
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions", "regions_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        shape_rate(tt, ctx, ds, shape, a.repeat, 0 if a.no_yardstick else a.yardstick_repeat, a.out)


if __name__ == "__main__":
    main()
