"""Wall time of the posterior interfaces of device histories on the shipped lattice (count, any, exceed, jump,
mean, std, density), host call to host results, by two routes in one process:

  interfaces  TdContext.interfaces_history (td_history_interfaces): the volume's search structure, the nodes
              swept slab by slab with the halo of their forward neighbours, each slab reduced on the device
              (k_iface_faces, k_iface_combine), the cells counted into their voxels (k_iface_density)
  yardstick   what there was before it: TdContext.volume_history(want_values=True) brings the value matrix
              V[nmodels][nq] to the host and numpy forms the face statistics from it (the sum of |d| in
              oracle_np.julia_mapreduce_arrays' association, so that the two routes can be compared bit for
              bit); History.read() brings every sample's cells to the host and numpy counts them

The outputs of both routes are compared for equality.  Also reported: the bytes each route brings to the host,
the device route's kernel times by HIP events, the read rate of k_iface_faces (8 bytes x models x columns of
every slab over the time of k_iface_faces + k_iface_combine) against the 6.29 TB/s measured HBM rate, and the
share of the call that is sweep, face kernels, density and the rest (copies, host work).
Shapes: CHAINSxSAMPLESxCELLS (chains started at CELLS uniform cells, every 10th model recorded).

Each figure: one warm-up, then the median of --repeat runs (--yardstick-repeat for the yardstick).  One JSON
line per shape, printed and appended to profiles/interfaces/interfaces_rate.jsonl.

    python tools/interfaces_rate.py [--repeat 10] [--shapes 8x1250x2000,8x1250x5000] [--no-yardstick]
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

KERNELS = ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute", "raster_stats", "iface_faces", "iface_density")
HBM_TB_PER_S = 6.29
FIELDS = ("count", "any", "exceed", "jump", "mean", "std", "density", "skipped")


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


def host_faces(V, nx, ny, nz, thr):
    """The face statistics of V[M][nq] in numpy, axis by axis on views of V (no copy of it)."""
    M, nq = V.shape
    V4 = V.reshape(M, nz, ny, nx)
    count = np.full((3, nz, ny, nx), -1, dtype=np.int64)
    exceed = np.full((len(thr), 3, nz, ny, nx), -1, dtype=np.int64)
    jump = np.full((3, nz, ny, nx), np.nan)
    differs = np.zeros((M, nz, ny, nx), dtype=bool)
    has = np.zeros((nz, ny, nx), dtype=bool)
    for a, axis in enumerate((3, 2, 1)):
        if V4.shape[axis] < 2:
            continue
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        neq = V4[lo] != V4[hi]
        differs[lo] |= neq
        has[lo[1:]] = True
        count[(a,) + lo[1:]] = neq.sum(axis=0)
        del neq
        with np.errstate(invalid="ignore"):
            d = np.abs(V4[hi] - V4[lo])
            for t, th in enumerate(thr):
                exceed[(t, a) + lo[1:]] = (d > th).sum(axis=0)
        jump[(a,) + lo[1:]] = oracle_np.julia_mapreduce_arrays(list(d)) / np.float64(M)
        del d
    anyc = np.where(has, differs.sum(axis=0), -1).astype(np.int64)
    return count.reshape(3, nq), anyc.reshape(nq), exceed.reshape(len(thr), 3, nq), jump.reshape(3, nq)


def host_density(hists, xv, yv, zv):
    nx, ny, nz = len(xv), len(yv), len(zv)
    mids = [0.5 * (v[:-1] + v[1:]) for v in (xv, yv, zv)]
    dens = np.zeros(nx * ny * nz, dtype=np.int64)
    skipped = 0
    nbytes = 0
    for h in hists:
        for m in h.read():
            x, y, z = (np.asarray(c, dtype=np.float64) for c in m.cells()[:3])
            nbytes += 8 * 4 * len(x)
            ok = ~(np.isnan(x) | np.isnan(y) | np.isnan(z))
            skipped += int(len(x) - ok.sum())
            i, j, k = (np.searchsorted(mid, c[ok], side="right") for mid, c in zip(mids, (x, y, z)))
            np.add.at(dens, i + nx * (j + ny * k), 1)
    return dens, skipped, nbytes


def rate(tt, ctx, ds, hists, thr, line, repeat, yard_repeat, out):
    xv, yv, zv = (np.asarray(v, dtype=np.float64).ravel() for v in (ds.xVec, ds.yVec, ds.zVec))
    nx, ny, nz = len(xv), len(yv), len(zv)
    nq = nx * ny * nz
    qx = np.tile(xv, ny * nz)
    qy = np.tile(np.repeat(yv, nx), nz)
    qz = np.repeat(zv, nx * ny)
    nmodels = sum(len(h) for h in hists)
    total_cells = sum(h.count()[1] for h in hists)
    nthr = len(thr)

    def interfaces():
        return ctx.interfaces_history(hists, xv, yv, zv, thr)

    def yardstick():
        r = ctx.volume_history(hists, qx, qy, qz, want_values=True)
        count, anyc, exceed, jump = host_faces(r["values"], nx, ny, nz, thr)
        dens, skipped, cell_bytes = host_density(hists, xv, yv, zv)
        return dict(count=count, any=anyc, exceed=exceed, jump=jump, mean=r["mean"], std=r["std"], density=dens,
                    skipped=skipped, cell_bytes=cell_bytes)

    nodes, nslabs, maxcols = ctx.interfaces_plan(nmodels, nx, ny, nz)
    # the columns of every slab (its nodes and halo, clipped to the lattice): what k_iface_faces reads
    cols = 0
    for s in range(nslabs):
        q0 = s * nodes
        ns = min(nodes, nq - q0)
        r1 = min(q0 + ns + nx, nq)
        r2lo, r2hi = min(q0 + nx * ny, nq), min(q0 + ns + nx * ny, nq)
        cols += (max(r1, r2hi) - q0) if r2lo <= r1 else (r1 - q0) + (r2hi - r2lo)
    line.update({"nmodels": nmodels, "mean_cells": total_cells / nmodels, "nodes": nq, "lattice": [nx, ny, nz],
                 "thresholds": list(thr), "plan": [nodes, nslabs, maxcols], "slab_columns_in_all": cols, "repeat": repeat,
                 "bytes_to_host": 8 * nq * (3 + 1 + 3 * nthr + 3 + 2 + 1) + 8})
    t, runs, r = median_run(interfaces, repeat)
    ks = kernel_ms(ctx, interfaces)
    line.update({"interfaces_s": t, "interfaces_all_s": runs, "interfaces_kernel_ms": ks})
    sweep_ms = sum(ks[k]["ms"] for k in ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute") if k in ks)
    faces_ms, dens_ms, stats_ms = ks["iface_faces"]["ms"], ks["iface_density"]["ms"], ks["raster_stats"]["ms"]
    face_bytes = 8 * nmodels * cols
    line["iface_faces_bytes"] = face_bytes
    line["iface_faces_TB_per_s"] = face_bytes / (faces_ms * 1e-3) / 1e12
    line["iface_faces_share_of_hbm_rate"] = line["iface_faces_TB_per_s"] / HBM_TB_PER_S
    line["iface_density_TB_per_s"] = 8 * 3 * total_cells / (dens_ms * 1e-3) / 1e12
    call_ms = t * 1e3
    line["raster_stats_TB_per_s"] = 2 * face_bytes / (stats_ms * 1e-3) / 1e12  # (the slab's columns, read twice)
    line["share_of_call"] = {"sweep": sweep_ms / call_ms, "faces": faces_ms / call_ms, "density": dens_ms / call_ms,
                             "raster_stats": stats_ms / call_ms,
                             "copies_and_host": 1.0 - (sweep_ms + faces_ms + dens_ms + stats_ms) / call_ms}
    if yard_repeat > 0:
        ty, runs_y, y = median_run(yardstick, yard_repeat)
        equal = {f: bool(np.array_equal(r[f], y[f], equal_nan=np.asarray(r[f]).dtype.kind == "f")) for f in FIELDS}
        line.update({"yardstick_s": ty, "yardstick_all_s": runs_y, "yardstick_repeat": yard_repeat,
                     "yardstick_bytes_to_host": 8 * nmodels * nq + 2 * 8 * nq + y["cell_bytes"],
                     "yardstick_over_interfaces": ty / t, "equal_bit_for_bit": equal, "all_equal": all(equal.values()),
                     "faces_with_0_lt_count_lt_M": int(np.sum((r["count"] > 0) & (r["count"] < nmodels))),
                     "faces": int(np.sum(r["count"] >= 0)), "density_sum": int(r["density"].sum()), "cells_in_all": int(total_cells)})
    emit(line, out)


def shape_rate(tt, ctx, ds, shape, thr, repeat, yard_repeat, out):
    nchains, per, cells = (int(v) for v in shape.split("x"))
    prm = tt.define_TDstructrure().replace(max_cells=cells + 1000)
    hists = []
    for c in range(nchains):  # every 10th model of a chain started at `cells` uniform cells
        ch = tt.Chain(ctx, tt.chain_params(prm, ds, seed=2000 + c, chain=c + 1), tt.random_model(cells, 2000 + c))
        h = tt.History(ctx, per, per * (cells + 1000), with_ptS=False)
        ch.run_recorded(10 * per, 10, 10, h)
        ch.close()
        hists.append(h)
    rate(tt, ctx, ds, hists, thr, {"nchains": nchains, "models_per_chain": per, "cells": cells}, repeat, yard_repeat, out)
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
    ap.add_argument("--thresholds", default="5.0")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interfaces", "interfaces_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    thr = tuple(float(v) for v in a.thresholds.split(",") if v)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        shape_rate(tt, ctx, ds, shape, thr, a.repeat, 0 if a.no_yardstick else a.yardstick_repeat, a.out)


if __name__ == "__main__":
    main()
