"""Wall time of a posterior volume (mean, std, quantiles 5/50/95, split R-hat, ESS and lags at every
node of the shipped 58 x 34 x 34 lattice) of device histories, host call to host results, by two routes
in one process:

  volume    TdContext.volume_history (td_history_volume): one search structure for all models, the nodes
            swept slab by slab
  sections  what there was before it, asked for all nodes at once: TdContext.marginals_history plus
            TdContext.convergence_history (each sweeps the models again; where nq x mean cells exceeds
            2^28 they read the histories back and search model by model)

and, with --crossover, the two sweeps of ONE slab against each other over the mean cells per model:
k_vol_search (plus k_vol_grid_build, amortised over the slabs of the whole lattice) and k_raster_brute, by
HIP events -- the table kVolGridMinMeanCells (csrc/volume.hip) is read from.

Each figure: one warm-up, then the median of --repeat runs.  One JSON line per shape, printed and
appended to profiles/volume/volume_rate.jsonl.

    python tools/volume_rate.py [--repeat 10] [--shapes 8x1250x2000,8x1250x5000] [--crossover] [--no-sections]
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
KERNELS = ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute", "nn_grid_build", "nn_grid", "raster_quantile",
           "conv_moments", "conv_autocov", "conv_geyer")
SWEEP = (50, 100, 200, 400, 800, 2000, 5000)


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


def lattice(ds):
    xv, yv, zv = (np.asarray(v, dtype=np.float64) for v in (ds.xVec, ds.yVec, ds.zVec))
    return (np.tile(xv, len(yv) * len(zv)), np.tile(np.repeat(yv, len(xv)), len(zv)), np.repeat(zv, len(xv) * len(yv)))


def volume_rate(tt, ctx, ds, shape, repeat, sections, out):
    nchains, per, cells = (int(v) for v in shape.split("x"))
    qx, qy, qz = lattice(ds)
    prm = tt.define_TDstructrure().replace(max_cells=cells + 1000)
    hists = []
    for c in range(nchains):  # every 10th model of a chain started at `cells` uniform cells
        ch = tt.Chain(ctx, tt.chain_params(prm, ds, seed=2000 + c, chain=c + 1), tt.random_model(cells, 2000 + c))
        h = tt.History(ctx, per, per * (cells + 1000), with_ptS=False)
        ch.run_recorded(10 * per, 10, 10, h)
        ch.close()
        hists.append(h)
    ncell = [h.count()[1] / per for h in hists]

    def volume():
        return ctx.volume_history(hists, qx, qy, qz, PROBS, convergence=True)

    def sections_marginals():
        return ctx.marginals_history(hists, qx, qy, qz, PROBS)

    def sections_convergence():
        return ctx.convergence_history(hists, qx, qy, qz)

    line = {"nchains": nchains, "models_per_chain": per, "cells": cells, "mean_cells": float(np.mean(ncell)),
            "nq": len(qx), "repeat": repeat, "plan": ctx.volume_plan(nchains * per, len(qx))}
    t_vol, all_vol, r = median_run(volume, repeat)
    line.update({"volume_s": t_vol, "volume_all_s": all_vol, "volume_kernel_ms": kernel_ms(ctx, volume)})
    ctx.set_volume_counting(True)
    try:
        volume()
        line["counters"] = ctx.volume_counters()
    finally:
        ctx.set_volume_counting(False)
    if sections:
        t_m, all_m, rm = median_run(sections_marginals, repeat)
        t_c, all_c, rc = median_run(sections_convergence, repeat)
        equal = all(np.array_equal(r[f], rm[f], equal_nan=True) for f in ("mean", "std", "quantiles")) and \
            all(np.array_equal(r[f], rc[f], equal_nan=True) for f in ("rhat", "ess", "lags"))
        line.update({"sections_s": t_m + t_c, "sections_marginals_s": t_m, "sections_convergence_s": t_c,
                     "sections_marginals_all_s": all_m, "sections_convergence_all_s": all_c,
                     "sections_kernel_ms": {"marginals": kernel_ms(ctx, sections_marginals),
                                            "convergence": kernel_ms(ctx, sections_convergence)},
                     "sections_over_volume": (t_m + t_c) / t_vol, "volume_not_slower": bool(t_vol <= t_m + t_c),
                     "equal_bit_for_bit": bool(equal)})
    for h in hists:
        h.close()
    emit(line, out)


def crossover(tt, ctx, ds, repeat, nmodels, out):
    """One slab of the lattice as 10^4 models would see it, `nmodels` models of c uniform cells each."""
    qx, qy, qz = lattice(ds)
    nodes, _ = ctx.volume_plan(10 ** 4, len(qx))
    slabs = len(qx) / nodes  # the build is paid once per volume
    qx, qy, qz = qx[:nodes], qy[:nodes], qz[:nodes]
    ctx.set_volume_slab_nodes(nodes)
    rows = []
    try:
        for cells in SWEEP:
            models = [tt.random_model(cells, 3000 + k).cells() for k in range(nmodels)]
            ms = {}
            for name, method in (("grid", ctx.VOL_GRID), ("brute", ctx.VOL_BRUTE)):
                ctx.set_volume_method(method)
                ctx.volume(models, qx, qy, qz)  # warm-up
                runs = [kernel_ms(ctx, lambda: ctx.volume(models, qx, qy, qz)) for _ in range(repeat)]
                ms[name] = {k: float(np.median([r[k]["ms"] for r in runs])) for k in runs[0]}
            ctx.set_volume_method(ctx.VOL_GRID)  # the instance that counts its paths
            ctx.set_volume_counting(True)
            ctx.volume(models, qx, qy, qz)
            runs = [kernel_ms(ctx, lambda: ctx.volume(models, qx, qy, qz)) for _ in range(repeat)]
            counting = float(np.median([r["vol_search"]["ms"] for r in runs]))
            counters = ctx.volume_counters()
            ctx.set_volume_counting(False)
            grid = ms["grid"]["vol_search"] + (ms["grid"]["vol_grid_build"] + ms["grid"]["vol_boxes"]) / slabs
            row = {"cells": cells, "nmodels": nmodels, "nodes": int(nodes), "vol_search_ms": ms["grid"]["vol_search"],
                   "vol_search_counting_ms": counting,
                   "vol_grid_build_ms": ms["grid"]["vol_grid_build"], "vol_boxes_ms": ms["grid"]["vol_boxes"],
                   "grid_ms_amortised": grid, "raster_brute_ms": ms["brute"]["raster_brute"],
                   "brute_over_grid": ms["brute"]["raster_brute"] / grid, "counters": counters,
                   "pairs_per_s_grid": nmodels * nodes / (ms["grid"]["vol_search"] * 1e-3)}
            print("  " + json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
    finally:
        ctx.set_volume_counting(False)
        ctx.set_volume_method(ctx.VOL_AUTO)
        ctx.set_volume_slab_nodes(0)
    emit({"crossover": rows, "repeat": repeat}, out)


def emit(line, out):
    line = json.dumps(line)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--shapes", default="8x1250x2000,8x1250x5000")
    ap.add_argument("--no-sections", dest="sections", action="store_false")
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--crossover-models", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume", "volume_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.crossover:
        crossover(tt, ctx, ds, a.repeat, a.crossover_models, a.out)
    for shape in [s for s in a.shapes.split(",") if s]:
        volume_rate(tt, ctx, ds, shape, a.repeat, a.sections, a.out)


if __name__ == "__main__":
    main()
