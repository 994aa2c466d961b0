"""Wall time of the posterior data support of device histories on the shipped rays and lattice (per cell and per
sample outputs, mean, std, the share of samples above 0.0), host call to host results, by two routes in one process:

  support    TdContext.support_history (td_history_support): the volume's search structure once, the context's ray
             points swept against every sample (I[M][P], the owners), k_sup_scatter, k_sup_finish, then the lattice
             swept slab by slab with the support in the place of zeta, k_sup_exceed and the volume's statistics
  yardstick  what there was before it: History.read(), one evaluate(want_nearest=True) per sample, numpy.bincount
             with the weights, then volume_history(want_values=True) brings V[nmodels][nq] to the host and every
             sample's row is joined to its cells through its zeta values (sorted once per sample), with running
             sums for mean and std and a count for the threshold

The yardstick sums the weights in floating point, so its supports are compared to 1e-9 relative; count, barren and
the count above 0.0 are integers and are compared for equality.  Also reported: the device route without nodes (the
ray-point phase alone), under each scatter mode, its kernel times by HIP events (td_timing_get), and the question
DESIGN 4.6j asks: k_sup_scatter plus the traffic of I (written by the sweep, read by the scatter: 16 bytes x
models x points at the measured HBM rate) against the two sweeps together.
Shapes: CHAINSxSAMPLESxCELLS (chains started at CELLS uniform cells, every 10th model recorded).

Each figure: one warm-up, then the median of --repeat runs (--yardstick-repeat for the yardstick).  One JSON line
per shape, printed and appended to profiles/support/support_rate.jsonl.

    python tools/support_rate.py [--repeat 10] [--yardstick-repeat 10] [--shapes 8x1250x5000,8x1250x2000]
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

KERNELS = ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute", "sup_index", "sup_scatter", "sup_finish",
           "sup_exceed", "raster_stats")
HBM_TB_PER_S = 6.29
THR = (0.0,)


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


def rate(tt, ctx, ds, hists, line, repeat, yard_repeat, out):
    xv, yv, zv = (np.asarray(v, dtype=np.float64).ravel() for v in (ds.xVec, ds.yVec, ds.zVec))
    nx, ny, nz = len(xv), len(yv), len(zv)
    nq = nx * ny * nz
    qx = np.tile(xv, ny * nz)
    qy = np.tile(np.repeat(yv, nx), nz)
    qz = np.repeat(zv, nx * ny)
    M = sum(len(h) for h in hists)
    total = sum(h.count()[1] for h in hists)
    w = tt.support_weights(ds, "tstar")
    P = ctx.P

    def support():
        return ctx.support_history(hists, w, qx, qy, qz, thresholds=THR)

    def support_cells_only():
        return ctx.support_history(hists, w)

    def volume_same_nodes():  # a posterior volume's mean and std on the same lattice
        return ctx.volume_history(hists, qx, qy, qz)

    def yardstick():
        cell, count, barren = [], [], []
        for h in hists:
            for m in h.read():
                near = ctx.evaluate(m.cells(), want_nearest=True)[3]
                nc = len(m.xCell)
                has = near >= 0
                cell.append(np.bincount(near[has], weights=w[has], minlength=nc))
                count.append(np.bincount(near[has], minlength=nc).astype(np.int64))
                barren.append(int(np.sum(count[-1] == 0)))
        V = ctx.volume_history(hists, qx, qy, qz, want_values=True)["values"]
        s1, s2, above = np.zeros(nq), np.zeros(nq), np.zeros(nq, dtype=np.int64)
        k = 0
        for h in hists:
            zeta = h.read_arrays()
            for j in range(len(h)):
                z = zeta["zeta"][zeta["off"][j]:zeta["off"][j + 1]]
                order = np.argsort(z, kind="stable")
                u = cell[k][order[np.searchsorted(z[order], V[k])]]
                s1 += u
                s2 += u * u
                above += u > THR[0]
                k += 1
        mean = s1 / M
        std = np.sqrt(np.maximum(s2 - M * mean * mean, 0.0) / (M - 1))
        return dict(cell=np.concatenate(cell), count=np.concatenate(count), barren=np.array(barren, dtype=np.int64),
                    mean=mean, std=std, exceed=above[None, :])

    ln = dict(line)
    ln.update({"nmodels": M, "mean_cells": total / M, "points": P, "lattice": [nx, ny, nz], "repeat": repeat,
               "plan_points": list(ctx.volume_plan(M, P)), "plan_nodes": list(ctx.volume_plan(M, nq)),
               "lds_cells": ctx.support_lds_cells(),
               "bytes_to_host": 8 * (2 * total + 2 * M + 2 * nq + len(THR) * nq)})
    t, runs, r = median_run(support, repeat)
    ks = kernel_ms(ctx, support)
    t1, runs1, _ = median_run(support_cells_only, repeat)
    ks1 = kernel_ms(ctx, support_cells_only)
    tv, runs_v, _ = median_run(volume_same_nodes, repeat)
    ln.update({"support_s": t, "support_all_s": runs, "support_kernel_ms": ks, "cells_only_s": t1, "cells_only_all_s": runs1,
               "cells_only_kernel_ms": ks1, "volume_same_nodes_s": tv, "volume_same_nodes_all_s": runs_v,
               "support_over_volume": t / tv})
    modes = {}
    for name, mode in (("lds", ctx.SUP_LDS), ("global", ctx.SUP_GLOBAL)):
        ctx.set_support_scatter(mode)
        try:
            tm, _, rm = median_run(support_cells_only, repeat)
            km = kernel_ms(ctx, support_cells_only)
        finally:
            ctx.set_support_scatter(ctx.SUP_AUTO)
        modes[name] = {"cells_only_s": tm, "sup_scatter_ms": km["sup_scatter"]["ms"],
                       "equal_to_auto": bool(np.array_equal(rm["cell"], r["cell"]) and np.array_equal(rm["count"], r["count"]))}
    ln["scatter_modes"] = modes
    search = lambda k: sum(k[n]["ms"] for n in ("vol_search", "raster_brute") if n in k)  # noqa: E731
    sweep_points_ms, sweeps_ms = search(ks1), search(ks)
    traffic_ms = 16.0 * M * P / (HBM_TB_PER_S * 1e12) * 1e3
    ln.update({"sweep_points_ms": sweep_points_ms, "sweep_nodes_ms": sweeps_ms - sweep_points_ms, "sweeps_ms": sweeps_ms,
               "sup_scatter_ms": ks["sup_scatter"]["ms"], "I_traffic_ms_at_hbm_rate": traffic_ms,
               "scatter_plus_I_over_sweeps": (ks["sup_scatter"]["ms"] + traffic_ms) / sweeps_ms,
               "scatter_plus_I_over_point_sweep": (ks["sup_scatter"]["ms"] + traffic_ms) / sweep_points_ms,
               "barren_share_mean": float(np.mean(r["barren"] / np.concatenate([h.traces()[:, 1] for h in hists]))),
               "nodes_owned_by_a_barren_cell": float(np.mean(1.0 - r["exceed"][0] / M))})
    if yard_repeat > 0:
        ty, runs_y, y = median_run(yardstick, yard_repeat)
        equal = {f: bool(np.array_equal(r[f], y[f])) for f in ("count", "barren", "exceed")}
        close = {f: bool(np.allclose(r[f], y[f], rtol=1e-9, atol=1e-12)) for f in ("cell", "mean", "std")}
        ln.update({"yardstick_s": ty, "yardstick_all_s": runs_y, "yardstick_repeat": yard_repeat,
                   "yardstick_bytes_to_host": 8 * M * nq + 4 * M * P + 8 * 4 * total, "yardstick_over_support": ty / t,
                   "equal_integers": equal, "close_sums": close})
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
    ap.add_argument("--shapes", default="8x1250x5000,8x1250x2000")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "support", "support_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        shape_rate(tt, ctx, ds, shape, a.repeat, 0 if a.no_yardstick else a.yardstick_repeat, a.out)


if __name__ == "__main__":
    main()
