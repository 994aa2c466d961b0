"""Wall time of the posterior resolution of device histories on the shipped lattice (footprint, run, extent,
censored, mean, std; corr and cov stay on the device), host call to host results, in one process:

  resolution  TdContext.resolution_history (td_history_resolution): the volume's search structure, every node swept
              once in a ring of blocks, the pairs of every block formed on the device (k_res_pairs / k_res_xruns,
              k_res_combine) and reduced by k_res_summary; with the plain form of the pair kernel for every offset,
              with the x-run form for every run and with the kept choice between them, and under window budgets of
              1, 2 and 4 GiB
  yardstick   what there was before it: TdContext.volume_history(want_values=True) brings the value matrix
              V[nmodels][nq] to the host and numpy forms one shifted product per offset over views of the centred
              matrix (one pass over it per offset), then the summaries (tests/resolution_ref.py).  numpy's sums
              associate differently from the device's, so the largest difference of corr is reported as a number and
              nothing is asserted on it; the summaries' differing nodes are counted.

Windows: `axes` (5, 3, 5) and `box` (2, 1, 2) by both routes, `box` (5, 3, 5) on the device only.  Also reported: the
bytes each route brings to the host, the device route's kernel times by HIP events (one more run), the pair kernel's
arithmetic rate (2 FP64 operations per model, node and offset with pairs on the lattice -- a product and an addition, no
FMA) against the part's 78.6 TFLOP/s FP64 vector peak (which counts an FMA as two: the roof of separate products and
additions is half of it), and the plain form's bytes (8 x models x nodes x (1 + offsets)) against the 6.29 TB/s
measured streaming rate.
Shapes: CHAINSxSAMPLESxCELLS (chains started at CELLS uniform cells, every 10th model recorded).

Each figure: one warm-up, then the median of --repeat runs (--yardstick-repeat for the yardstick).  One JSON line per
shape, printed and appended to profiles/resolution/resolution_rate.jsonl.

    python tools/resolution_rate.py [--repeat 10] [--shapes 8x1250x2000,8x1250x5000] [--yardstick-repeat 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tonga  # noqa: E402
import resolution_ref as rref  # noqa: E402

KERNELS = ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute", "raster_stats", "res_center", "res_pairs",
           "res_combine", "res_summary")
HBM_TB_PER_S = 6.29
FP64_VECTOR_TFLOPS = 78.6
SUMMARY = ("footprint", "run", "extent", "censored", "mean", "std")
WINDOWS = (("axes_5_3_5", (5, 3, 5), "axes", True), ("box_2_1_2", (2, 1, 2), "box", True), ("box_5_3_5", (5, 3, 5), "box", False))
GIB = 1 << 30


def median_run(fn, repeat, name):
    fn()  # warm-up: allocations, first launches
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
        print("  %s %.4f s" % (name, ts[-1]), file=sys.stderr, flush=True)
    return float(np.median(ts)), [round(t, 5) for t in ts], out


def kernel_ms(ctx, fn):
    ctx.timing(enable=True, reset=True)
    try:
        fn()
        return {k: dict(zip(("launches", "ms"), ctx.timing(kernel=k))) for k in KERNELS if ctx.timing(kernel=k)[0]}
    finally:
        ctx.timing(enable=False)


def host_corr(V, mean, std, nx, ny, nz, off):
    """corr [noff][nq] by shifted products over views of the centred matrix: one pass over it per offset."""
    M, nq = V.shape
    D4 = (V - mean).reshape(M, nz, ny, nx)
    s3 = std.reshape(nz, ny, nx)
    corr = np.full((len(off), nz, ny, nx), np.nan)
    for t, (di, dj, dk) in enumerate(off):
        if abs(di) >= nx or abs(dj) >= ny or dk >= nz:
            continue
        lo = (slice(0, nz - dk), slice(max(0, -dj), ny - max(0, dj)), slice(max(0, -di), nx - max(0, di)))
        hi = (slice(dk, nz), slice(max(0, dj), ny + min(0, dj)), slice(max(0, di), nx + min(0, di)))
        S = np.einsum("mkji,mkji->kji", D4[(slice(None),) + lo], D4[(slice(None),) + hi])
        with np.errstate(invalid="ignore", divide="ignore"):
            corr[(t,) + lo] = S / np.float64(M - 1) / (s3[lo] * s3[hi])
    return corr.reshape(len(off), nq)


def pair_count(nx, ny, nz, off):
    return int(sum(rref.on_lattice(nx, ny, nz, o)[0].sum() for o in off))


def rate(tt, ctx, ds, hists, line, repeat, yard_repeat, yard_windows, out):
    T = tt.TdContext
    xv, yv, zv = (np.asarray(v, dtype=np.float64).ravel() for v in (ds.xVec, ds.yVec, ds.zVec))
    nx, ny, nz = len(xv), len(yv), len(zv)
    nq = nx * ny * nz
    qx, qy, qz = rref.lattice(xv, yv, zv)
    w = tt.voxel_weights(xv, yv, zv).transpose(2, 1, 0).ravel()
    M = sum(len(h) for h in hists)
    line.update({"nmodels": M, "mean_cells": sum(h.count()[1] for h in hists) / M, "nodes": nq, "lattice": [nx, ny, nz],
                 "repeat": repeat, "bytes_to_host": 8 * nq * (1 + 3 + 2) + 4 * nq * (6 + 1)})
    for name, lags, window, yard in WINDOWS:
        off = tt.resolution_offsets(lags, window)
        reach = max(int(o[0]) + nx * (int(o[1]) + ny * int(o[2])) for o in off)
        pairs = pair_count(nx, ny, nz, off)
        res = {"offsets": len(off), "reach": reach, "pairs_on_the_lattice": pairs}

        def call():
            return ctx.resolution_history(hists, xv, yv, zv, off, 0.5, w)

        forms = {}
        for form, code in (("plain", T.RES_FORM_PLAIN), ("xruns", T.RES_FORM_XRUNS), ("kept", T.RES_FORM_KEPT)):
            ctx.set_resolution(0, code)
            t, runs, r = median_run(call, repeat, "%s %s" % (name, form))
            ks = kernel_ms(ctx, call)
            pair_ms = ks["res_pairs"]["ms"]
            forms[form] = {"s": t, "all_s": runs, "kernel_ms": ks, "plan": list(T.resolution_plan(M, nq, reach)),
                           "pairs_TFLOPS": 2.0 * M * pairs / (pair_ms * 1e-3) / 1e12,
                           "pairs_share_of_fp64_vector_peak": 2.0 * M * pairs / (pair_ms * 1e-3) / 1e12 / FP64_VECTOR_TFLOPS,
                           "plain_bytes_TB_per_s": 8.0 * M * nq * (1 + len(off)) / (pair_ms * 1e-3) / 1e12,
                           "share_of_call": {k: v["ms"] / (t * 1e3) for k, v in ks.items()}, "out": r}
        outs = {k: v.pop("out") for k, v in forms.items()}
        r = outs["kept"]
        res["all_equal_between_forms"] = all(np.array_equal(outs[k][f], r[f], equal_nan=True) for k in ("plain", "xruns") for f in SUMMARY)
        res["forms"] = forms
        res["plain_over_xruns_pair_kernel"] = forms["plain"]["kernel_ms"]["res_pairs"]["ms"] / forms["xruns"]["kernel_ms"]["res_pairs"]["ms"]
        budgets = {}
        for gib in (1, 2, 4):  # the kept form under three window budgets
            ctx.set_resolution(gib * GIB, T.RES_FORM_KEPT)
            t, runs, _ = median_run(call, repeat, "%s %d GiB" % (name, gib))
            budgets["%d_GiB" % gib] = {"s": t, "all_s": runs, "plan": list(T.resolution_plan(M, nq, reach, gib * GIB))}
        ctx.set_resolution(0, T.RES_FORM_KEPT)
        res["budgets"] = budgets
        if yard and yard_repeat > 0 and name in yard_windows:
            def yardstick():
                v = ctx.volume_history(hists, qx, qy, qz, want_values=True)
                corr = host_corr(v["values"], v["mean"], v["std"], nx, ny, nz, off)
                foot, run, cens = rref.summaries(corr, nx, ny, nz, off, 0.5, w)
                return dict(corr=corr, footprint=foot, run=run, censored=cens, extent=rref.extents(run, xv, yv, zv),
                            mean=v["mean"], std=v["std"])

            ty, runs_y, y = median_run(yardstick, yard_repeat, name + " yardstick")
            dev = ctx.resolution_history(hists, xv, yv, zv, off, 0.5, w, want=("corr",))["corr"]
            both = ~np.isnan(dev) & ~np.isnan(y["corr"])
            res.update({"yardstick_s": ty, "yardstick_all_s": runs_y, "yardstick_repeat": yard_repeat,
                        "yardstick_bytes_to_host": 8 * M * nq + 2 * 8 * nq, "yardstick_over_resolution": ty / forms["kept"]["s"],
                        "corr_largest_difference": float(np.max(np.abs(dev[both] - y["corr"][both]))) if both.any() else 0.0,
                        "corr_nan_pattern_equal": bool(np.array_equal(np.isnan(dev), np.isnan(y["corr"]))),
                        "nodes_differing": {f: int(np.sum(np.any(np.reshape(r[f] != y[f], (-1, nq)), axis=0))) for f in
                                            ("footprint", "run", "censored")},
                        "mean_std_equal": bool(np.array_equal(r["mean"], y["mean"]) and np.array_equal(r["std"], y["std"]))})
        line[name] = res
    emit(line, out)


def shape_rate(tt, ctx, ds, shape, repeat, yard_repeat, yard_windows, out):
    nchains, per, cells = (int(v) for v in shape.split("x"))
    prm = tt.define_TDstructrure().replace(max_cells=cells + 1000)
    hists = []
    for c in range(nchains):  # every 10th model of a chain started at `cells` uniform cells
        ch = tt.Chain(ctx, tt.chain_params(prm, ds, seed=2000 + c, chain=c + 1), tt.random_model(cells, 2000 + c))
        h = tt.History(ctx, per, per * (cells + 1000), with_ptS=False)
        ch.run_recorded(10 * per, 10, 10, h)
        ch.close()
        hists.append(h)
    rate(tt, ctx, ds, hists, {"nchains": nchains, "models_per_chain": per, "cells": cells}, repeat, yard_repeat, yard_windows, out)
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
    ap.add_argument("--yardstick-windows", default="axes_5_3_5,box_2_1_2", help="the windows the yardstick is run on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resolution", "resolution_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        shape_rate(tt, ctx, ds, shape, a.repeat, a.yardstick_repeat, a.yardstick_windows.split(","), a.out)


if __name__ == "__main__":
    main()
