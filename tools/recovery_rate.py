"""Wall time of the posterior recovery of device histories against a checkerboard truth on the shipped lattice (the
rank counts and the error's mean and sigma per node, the mean square distance per sample and depth layer with its mean,
std, quantiles, histograms, R-hat and ESS), host call to host results, by two routes in one process:

  recovery   TdContext.recovery_history (td_history_recovery): the volume's search structure, the points swept slab
             by slab, each slab counted against the truth and turned into the error in place (k_recovery_counts),
             its columns' statistics taken (k_raster_stats), its squares reduced over the regions' columns
             (k_region_sums with the squared term), the leaves combined (k_region_combine), the statistics of the
             [M, R] series by the volume's own kernels
  yardstick  what there was before it: TdContext.volume_history(want_values=True) brings the value matrix
             V[nmodels][nq] of the lattice to the host and numpy forms the counts and the series from it (the sums in
             oracle_np.julia_mapreduce_arrays' association, so that the two routes can be compared bit for bit)

`below`, `equal`, `above` and `msd` of both routes are compared for equality.  Also reported: the bytes each route
brings to the host, the device route's kernel times by HIP events, the rates of the sums kernel (8 bytes x models x
points read over its time) and of the counting pass (16 bytes x models x points read and written over its time)
against the 6.29 TB/s measured streaming copy, and k_region_sums' rate in a TdContext.regions_history call on the same
points and slabs in the same run.  Regions: one per depth node of the lattice (every node once), volume weights.
Shapes: CHAINSxSAMPLESxCELLS (chains started at CELLS uniform cells, every 10th model recorded).

Each figure: one warm-up, then the median of --repeat runs (--yardstick-repeat for the yardstick).  One JSON line per
shape, printed and appended to profiles/recovery/recovery_rate.jsonl.

    python tools/recovery_rate.py [--repeat 10] [--shapes 8x1250x2000] [--no-yardstick]
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

KERNELS = ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute", "recovery_counts", "recovery_dstats", "recovery_sums",
           "recovery_combine", "raster_stats", "region_sums")
HBM_TB_PER_S = 6.29
PROBS, BINS = (0.05, 0.5, 0.95), (64, 0.0, 1000.0)
BLOCKS, LO, HI = (4, 2, 4), 5.0, 15.0


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


def rate(tt, ctx, ds, hists, line, repeat, yard_repeat, out):
    xv, yv, zv = (np.asarray(v, dtype=np.float64).ravel() for v in (ds.xVec, ds.yVec, ds.zVec))
    nx, ny, nz = len(xv), len(yv), len(zv)
    nq = nx * ny * nz
    qx = np.tile(xv, ny * nz)
    qy = np.tile(np.repeat(yv, nx), nz)
    qz = np.repeat(zv, nx * ny)
    nmodels = sum(len(h) for h in hists)
    total_cells = sum(h.count()[1] for h in hists)
    layers = {"z %g" % z: (np.arange(nz) == k).reshape(1, 1, -1) for k, z in enumerate(zv)}
    names, px, py, pz, w, off = tt.region_points(layers, xv, yv, zv, "volume")
    R, npts = len(names), len(px)
    assert npts == nq and np.array_equal(px, qx) and np.array_equal(py, qy) and np.array_equal(pz, qz)  # every node once
    board = tt.checkerboard_model(xv, yv, zv, BLOCKS, LO, HI)
    truth = ctx.rasterize([board.cells()], px, py, pz, want_values=True)[2][0]

    def recovery():
        return ctx.recovery_history(hists, px, py, pz, truth, off, w, True, PROBS, BINS, convergence=True)

    def regions_same_points():  # the region averages with the same statistics on the same points and slabs
        return ctx.regions_history(hists, px, py, pz, off, w, True, PROBS, BINS, convergence=True, greater=False)

    def yardstick():
        V = ctx.volume_history(hists, qx, qy, qz, want_values=True)["values"]
        F = np.empty((nmodels, R))
        below, equal, above = (np.empty(nq, dtype=np.int64) for _ in range(3))
        bias = np.empty(nq)
        for r in range(R):
            lo, hi = int(off[r]), int(off[r + 1])
            Vr, tr = V[:, lo:hi], truth[lo:hi]
            below[lo:hi], equal[lo:hi], above[lo:hi] = (Vr < tr).sum(axis=0), (Vr == tr).sum(axis=0), (Vr > tr).sum(axis=0)
            D = Vr - tr
            bias[lo:hi] = D.mean(axis=0)
            F[:, r] = tree(w[lo:hi] * (D * D)) / tree(w[lo:hi])
        return dict(below=below, equal=equal, above=above, series=F, dmean=bias, mean=F.mean(axis=0),
                    std=F.std(axis=0, ddof=1), quantiles=np.quantile(F, PROBS, axis=0))

    nodes, nslabs = ctx.regions_plan(nmodels, npts)
    ln = dict(line)
    ln.update({"nreg": R, "points": npts, "nmodels": nmodels, "mean_cells": total_cells / nmodels, "lattice": [nx, ny, nz],
               "truth": {"blocks": list(BLOCKS), "lo": LO, "hi": HI}, "plan": [nodes, nslabs], "repeat": repeat,
               "bytes_to_host": 8 * (5 * npts + nmodels * R + R + 2 * R + len(PROBS) * R + R * (BINS[0] + 3) + 2 * R) + 4 * R})
    t, runs, r = median_run(recovery, repeat)
    ks = kernel_ms(ctx, recovery)
    tv, runs_v, _ = median_run(regions_same_points, repeat)
    kr = kernel_ms(ctx, regions_same_points)
    ln.update({"recovery_s": t, "recovery_all_s": runs, "recovery_kernel_ms": ks, "regions_same_points_s": tv,
               "regions_same_points_all_s": runs_v, "recovery_over_regions": t / tv})
    sweep_ms = sum(ks[k]["ms"] for k in ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute") if k in ks)
    sums_ms, counts_ms, dstats_ms = ks["recovery_sums"]["ms"], ks["recovery_counts"]["ms"], ks["recovery_dstats"]["ms"]
    slab_bytes = 8 * nmodels * npts
    ln["slab_bytes"] = slab_bytes
    ln["recovery_sums_TB_per_s"] = slab_bytes / (sums_ms * 1e-3) / 1e12
    ln["recovery_sums_share_of_hbm_rate"] = ln["recovery_sums_TB_per_s"] / HBM_TB_PER_S
    ln["region_sums_same_slabs_TB_per_s"] = slab_bytes / (kr["region_sums"]["ms"] * 1e-3) / 1e12
    ln["recovery_counts_TB_per_s"] = 2 * slab_bytes / (counts_ms * 1e-3) / 1e12  # read and written
    ln["recovery_counts_share_of_hbm_rate"] = ln["recovery_counts_TB_per_s"] / HBM_TB_PER_S
    ln["recovery_dstats_TB_per_s"] = 2 * slab_bytes / (dstats_ms * 1e-3) / 1e12  # k_raster_stats reads the slab twice
    call_ms = t * 1e3
    tail_ms = ks["recovery_combine"]["ms"] + ks["raster_stats"]["ms"]
    ln["share_of_call"] = {"sweep": sweep_ms / call_ms, "recovery_counts": counts_ms / call_ms,
                           "recovery_dstats": dstats_ms / call_ms, "recovery_sums": sums_ms / call_ms,
                           "combine_and_statistics": tail_ms / call_ms,
                           "copies_and_host": 1.0 - (sweep_ms + counts_ms + dstats_ms + sums_ms + tail_ms) / call_ms}
    if yard_repeat > 0:
        ty, runs_y, y = median_run(yardstick, yard_repeat)
        equal = {f: bool(np.array_equal(r[f], y[f], equal_nan=True)) for f in ("below", "equal", "above", "series")}
        close = {f: bool(np.allclose(r[f], y[f], rtol=1e-9, atol=1e-12, equal_nan=True)) for f in ("dmean", "mean", "std", "quantiles")}
        ln.update({"yardstick_s": ty, "yardstick_all_s": runs_y, "yardstick_repeat": yard_repeat,
                   "yardstick_bytes_to_host": 8 * nmodels * nq + 2 * 8 * nq, "yardstick_over_recovery": ty / t,
                   "equal_bit_for_bit": equal, "all_equal": all(equal.values()), "statistics_close": close,
                   "nodes_with_0_lt_below_lt_M": int(np.sum((r["below"] > 0) & (r["below"] < nmodels))),
                   "nodes_with_equal": int(np.sum(r["equal"] > 0))})
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
    ap.add_argument("--shapes", default="8x1250x2000")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recovery", "recovery_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        shape_rate(tt, ctx, ds, shape, a.repeat, 0 if a.no_yardstick else a.yardstick_repeat, a.out)


if __name__ == "__main__":
    main()
