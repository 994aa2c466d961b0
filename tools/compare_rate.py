"""Wall time of the posterior comparison of two sets of device histories on the shipped lattice -- a posterior ensemble
against a debug_prior = 1 ensemble of the same size: all pair counts, two exceedance pairs, Kolmogorov-Smirnov, both
sides' mean and std -- host call to host results, by two routes in one process:

  compare    TdContext.compare_history (td_history_compare): the two sides as one ensemble in the volume's search
             structure, the nodes swept slab by slab, each side's statistics by the volume's kernels, each column of
             each side sorted in LDS (k_compare_sort) and the ranks counted (k_compare_count)
  baseline   what there was before it: TdContext.volume_history(want_values=True) once per side brings both value
             matrices to the host, and numpy sorts every column and counts with searchsorted (one run)

Every integer output and ks_at of the two routes are compared for equality.  Also reported: the bytes each route brings
to the host, the device route's kernel times by HIP events, and the rates of the two new kernels against the bytes of
the slabs they read (k_compare_sort: 8 bytes x models x nodes read, as many written; k_compare_count: the sorted copy
read once per pass) as a share of the 6.29 TB/s measured streaming copy -- both kernels are bound by LDS traffic and
compares, not by HBM, and the share says how far.  --forms runs the device route once per form PLAIN:SORT:COUNT of
TdContext.set_compare_form (the placement of the sort kernel's columns and the threads of the two kernels; 0:0:0 is the
product's).
Shapes: CHAINSxSAMPLESxCELLS a side (chains started at CELLS uniform cells, every 10th model recorded).

Each figure: one warm-up, then the median of --repeat runs.  One JSON file per shape in profiles/compare/.

    python tools/compare_rate.py [--repeat 10] [--shapes 8x1250x2000,8x1250x5000] [--no-baseline]
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

KERNELS = ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute", "compare_side_stats", "compare_sort", "compare_count")
HBM_TB_PER_S = 6.29
EXCEED = ((1.0, 0.0), (1.5, 0.0))
INTS = ("less", "equal", "greater", "exceed", "ks_plus", "ks_minus")


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


def host_counts(VA, VB):
    """The contract on two host value matrices, column by column with np.sort and np.searchsorted."""
    (MA, nq), MB = VA.shape, VB.shape[0]
    out = {f: np.zeros(nq, dtype=np.int64) for f in INTS if f != "exceed"}
    out["exceed"] = np.zeros((len(EXCEED), nq), dtype=np.int64)
    out["ks_at"] = np.full(nq, np.nan)
    for q in range(nq):
        if q % 8192 == 0:
            print("  baseline: column %d of %d" % (q, nq), file=sys.stderr, flush=True)
        a, b = (np.sort(np.where(v == 0, 0.0, v)[~np.isnan(v)]) for v in (VA[:, q], VB[:, q]))
        lo, hi = np.searchsorted(b, a, "left"), np.searchsorted(b, a, "right")
        out["greater"][q], out["equal"][q], out["less"][q] = lo.sum(), (hi - lo).sum(), (len(b) - hi).sum()
        for k, (s, t) in enumerate(EXCEED):
            f = s * b
            f = f + t
            out["exceed"][k, q] = np.searchsorted(f, a, "left").sum()
        X = np.concatenate((a, b))
        T = (np.concatenate((np.searchsorted(a, a, "right"), np.searchsorted(a, b, "right"))).astype(np.int64) * MB -
             np.concatenate((hi, np.searchsorted(b, b, "right"))).astype(np.int64) * MA)
        if len(T):
            out["ks_plus"][q], out["ks_minus"][q] = max(0, T.max()), max(0, (-T).max())
            best = max(out["ks_plus"][q], out["ks_minus"][q])
            if best > 0:
                out["ks_at"][q] = X[np.abs(T) == best].min()
    return out


def rate(tt, ctx, ds, ha, hb, line, repeat, baseline, forms, out_dir):
    xv, yv, zv = (np.asarray(v, dtype=np.float64).ravel() for v in (ds.xVec, ds.yVec, ds.zVec))
    nx, ny, nz = len(xv), len(yv), len(zv)
    nq = nx * ny * nz
    qx = np.tile(xv, ny * nz)
    qy = np.tile(np.repeat(yv, nx), nz)
    qz = np.repeat(zv, nx * ny)
    MA, MB = sum(len(h) for h in ha), sum(len(h) for h in hb)

    def compare():
        return ctx.compare_history(ha, hb, qx, qy, qz, EXCEED)

    def baseline_route():
        va = ctx.volume_history(ha, qx, qy, qz, want_values=True)
        vb = ctx.volume_history(hb, qx, qy, qz, want_values=True)
        r = host_counts(va["values"], vb["values"])
        r.update(mean_a=va["mean"], std_a=va["std"], mean_b=vb["mean"], std_b=vb["std"])
        return r

    nodes, nslabs = ctx.volume_plan(MA + MB, nq)
    ln = dict(line)
    ln.update({"MA": MA, "MB": MB, "nq": nq, "lattice": [nx, ny, nz], "exceed": [list(p) for p in EXCEED], "plan": [nodes, nslabs],
               "repeat": repeat, "bytes_to_host": 8 * nq * (5 + len(EXCEED) + 1 + 4)})
    slab_bytes = 8 * (MA + MB) * nq
    ln["slab_bytes"] = slab_bytes
    r = None
    for form in forms:
        ctx.set_compare_form(*form)
        tag = "form_%d:%d:%d" % form
        t, runs, r = median_run(compare, repeat)
        ks = kernel_ms(ctx, compare)
        sort_ms, count_ms = ks["compare_sort"]["ms"], ks["compare_count"]["ms"]
        sweep_ms = sum(ks[k]["ms"] for k in ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute") if k in ks)
        stats_ms = ks["compare_side_stats"]["ms"]  # (both sides' mean and sigma with their copies and waits)
        ln[tag] = {"compare_s": t, "compare_all_s": runs, "kernel_ms": ks,
                   "compare_sort_TB_per_s": 2 * slab_bytes / (sort_ms * 1e-3) / 1e12,  # read and written
                   "compare_count_TB_per_s": 2 * slab_bytes / (count_ms * 1e-3) / 1e12,  # the sorted copy, once per pass
                   "share_of_call": {"sweep": sweep_ms / (t * 1e3), "side_stats": stats_ms / (t * 1e3), "compare_sort": sort_ms / (t * 1e3),
                                     "compare_count": count_ms / (t * 1e3)}}
        for k in ("compare_sort", "compare_count"):
            ln[tag][k + "_share_of_hbm_rate"] = ln[tag][k + "_TB_per_s"] / HBM_TB_PER_S
    ctx.set_compare_form()
    ln["nodes_with_ties"] = int(np.sum(r["equal"] > 0))
    ln["median_prob_greater"] = float(np.median((r["greater"] + 0.5 * r["equal"]) / (MA * MB)))
    ln["median_ks"] = float(np.median(np.maximum(r["ks_plus"], r["ks_minus"]) / (MA * MB)))
    if baseline:
        t0 = time.perf_counter()
        y = baseline_route()
        ty = time.perf_counter() - t0
        equal = {f: bool(np.array_equal(r[f], y[f])) for f in INTS}
        equal["ks_at"] = bool(np.array_equal(r["ks_at"], y["ks_at"], equal_nan=True))
        equal.update({f: bool(np.array_equal(r[f], y[f], equal_nan=True)) for f in ("mean_a", "std_a", "mean_b", "std_b")})
        first = "form_%d:%d:%d" % forms[0]
        ln.update({"baseline_s": ty, "baseline_bytes_to_host": 8 * (MA + MB) * nq + 4 * 8 * nq,
                   "baseline_over_compare": ty / ln[first]["compare_s"], "equal_bit_for_bit": equal,
                   "all_equal": all(equal.values())})
    path = os.path.join(out_dir, "compare_rate_%dx%dx%d.json" % (line["nchains"], line["models_per_chain"], line["cells"]))
    with open(path, "w") as f:
        json.dump(ln, f, indent=1)
        f.write("\n")
    print(json.dumps(ln), flush=True)


def record(tt, ctx, ds, prm, nchains, per, cells, seed):
    hists = []
    for c in range(nchains):  # every 10th model of a chain started at `cells` uniform cells
        ch = tt.Chain(ctx, tt.chain_params(prm, ds, seed=seed + c, chain=c + 1), tt.random_model(cells, seed + c))
        h = tt.History(ctx, per, per * (cells + 1000), with_ptS=False)
        ch.run_recorded(10 * per, 10, 10, h)
        ch.close()
        hists.append(h)
    return hists


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--shapes", default="8x1250x2000,8x1250x5000")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--forms", default="0:0:0", help="PLAIN:SORT_THREADS:COUNT_THREADS[,...]; the baseline is held to the first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    os.makedirs(a.out, exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        nchains, per, cells = (int(v) for v in shape.split("x"))
        prm = tt.define_TDstructrure().replace(max_cells=cells + 1000)
        ha = record(tt, ctx, ds, prm, nchains, per, cells, 2000)
        hb = record(tt, ctx, ds, prm.replace(debug_prior=1), nchains, per, cells, 3000)
        rate(tt, ctx, ds, ha, hb, {"nchains": nchains, "models_per_chain": per, "cells": cells}, a.repeat, not a.no_baseline,
             [tuple(int(v) for v in f.split(":")) for f in a.forms.split(",")], a.out)
        for h in ha + hb:
            h.close()


if __name__ == "__main__":
    main()
