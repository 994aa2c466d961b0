"""Wall time of the ensemble Gram and distance matrices of device histories on the shipped lattice with volume
weights (gram, dist2 [M, M], mean, std), host call to host results, by two routes in one process:

  gram       TdContext.gram_history (td_history_gram): the volume's search structure, the lattice swept slab by slab,
             each slab centred in place (k_gram_centre) and added to the M x M matrices on the device (k_gram_pairs),
             the upper triangle mirrored at the end (k_gram_mirror); under every form of the pair kernel
             (tdt_set_gram_form: the register tile) and for gram alone, dist2 alone and both
  yardstick  what there was before it: TdContext.volume_history(want_values=True) brings the value matrix
             V[nmodels][nq] to the host, numpy centres and weights it, X @ X.T (BLAS) gives gram and the identity
             d2 = g_aa + g_bb - 2 g_ab the distances; one run

The two routes' gram are compared within the bound any order of summation obeys, gamma_n sum_p |X_a X_b| with n =
np + 1 (tests/test_gram_host.py), mean and std bit for bit.  Also reported: the bytes each route brings to the host,
the device route's kernel times by HIP events, and the pair kernel's FP64 operations per second -- useful (the
M (M + 1) / 2 pairs of the lower triangle, 2 operations a point for gram, 3 for dist2) and issued (every pair of
every tile, the diagonal's tiles whole and the tiles' tails included) -- against the 39 TFLOP/s roof of separate FP64
products and additions.  With --eigh, numpy.linalg.eigh of the matrix once: the host step of
posterior_patterns, LAPACK's time.
Shapes: CHAINSxSAMPLESxCELLS (chains started at CELLS uniform cells, every 10th model recorded).

Each figure: one warm-up, then the median of --repeat runs.  One JSON line per shape, printed and appended to --out.

    python tools/gram_rate.py [--repeat 10] [--shapes 8x1250x2000,8x1250x5000] [--no-yardstick] [--eigh]
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

KERNELS = ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute", "raster_stats", "gram_centre", "gram_pairs", "gram_mirror")
ROOF_TFLOPS = 39.0
FORMS = {1: "4x4", 2: "8x8"}
OPS = {("gram", "dist2"): 5, ("gram",): 2, ("dist2",): 3}  # FP64 operations per pair and point


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


def rate(tt, ctx, ds, hists, line, repeat, yardstick, eigh, out):
    xv, yv, zv = (np.asarray(v, dtype=np.float64).ravel() for v in (ds.xVec, ds.yVec, ds.zVec))
    nx, ny, nz = len(xv), len(yv), len(zv)
    nq = nx * ny * nz
    qx = np.tile(xv, ny * nz)
    qy = np.tile(np.repeat(yv, nx), nz)
    qz = np.repeat(zv, nx * ny)
    w = tt.voxel_weights(xv, yv, zv).transpose(2, 1, 0).ravel()
    M = sum(len(h) for h in hists)
    total_cells = sum(h.count()[1] for h in hists)
    nodes, nslabs = ctx.gram_plan(M, nq)
    ln = dict(line)
    ln.update({"nmodels": M, "mean_cells": total_cells / M, "lattice": [nx, ny, nz], "points": nq, "plan": [nodes, nslabs],
               "repeat": repeat, "roof_TFLOPS": ROOF_TFLOPS, "kept_tile_rows": ctx.gram_tile(0), "forms": {}})
    kept, t_both = None, float("nan")
    for form, fname in FORMS.items():
        T = ctx.gram_tile(form)
        nt = -(-M // T)
        issued_pairs = nt * (nt + 1) // 2 * T * T
        for want in OPS:
            tt.TdContext.set_gram_form(form)
            try:
                def gram():
                    return ctx.gram_history(hists, qx, qy, qz, w, want=want)

                t, runs, r = median_run(gram, repeat)
                ks = kernel_ms(ctx, gram)
            finally:
                tt.TdContext.set_gram_form(0)
            pair_s = ks["gram_pairs"]["ms"] * 1e-3
            useful = OPS[want] * (M * (M + 1) // 2) * nq
            issued = OPS[want] * issued_pairs * nq
            sweep_ms = sum(ks[k]["ms"] for k in ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute") if k in ks)
            ln["forms"]["%s %s" % (fname, "+".join(want))] = {
                "tile_rows": T, "tiles": nt * (nt + 1) // 2, "call_s": t, "call_all_s": runs, "kernel_ms": ks,
                "pairs_useful_TFLOPS": useful / pair_s / 1e12, "pairs_issued_TFLOPS": issued / pair_s / 1e12,
                "pairs_issued_share_of_roof": issued / pair_s / 1e12 / ROOF_TFLOPS,
                "bytes_to_host": 8 * (len(want) * M * M + 2 * nq + 1),
                "share_of_call": {"sweep": sweep_ms / (t * 1e3), "raster_stats": ks["raster_stats"]["ms"] / (t * 1e3),
                                  "gram_centre": ks["gram_centre"]["ms"] / (t * 1e3), "gram_pairs": ks["gram_pairs"]["ms"] / (t * 1e3),
                                  "gram_mirror": ks["gram_mirror"]["ms"] / (t * 1e3)}}
            if form == 1 and want == ("gram", "dist2"):
                kept, t_both = r, t
            elif kept is not None:  # no answer depends on the form or on the outputs asked for
                for f in want:
                    assert np.array_equal(kept[f], r[f], equal_nan=True), (fname, want, f)
            print("%s %s: %.3f s, pairs %.1f ms" % (fname, "+".join(want), t, pair_s * 1e3), file=sys.stderr, flush=True)
    emit(dict(ln, part="device"), out)  # (the yardstick takes minutes: the device's figures are on file before it starts)
    ln = dict(line, part="yardstick", nmodels=M, points=nq)
    if yardstick:
        t0 = time.perf_counter()
        vol = ctx.volume_history(hists, qx, qy, qz, want_values=True)
        t_values = time.perf_counter() - t0
        X = vol.pop("values")  # centred and weighted in place: one subtraction, then one multiply, as on the device
        X -= vol["mean"]
        X *= np.sqrt(w)
        t_centre = time.perf_counter() - t0 - t_values
        G = X @ X.T
        t_product = time.perf_counter() - t0 - t_values - t_centre
        g = np.diag(G)
        D = g[:, None] + g[None, :] - 2.0 * G
        ty = time.perf_counter() - t0
        u = 2.0 ** -53
        n = nq + 1
        gamma = n * u / (1 - n * u)
        np.abs(X, out=X)
        bound = gamma * (X @ X.T)
        err = np.abs(kept["gram"] - G)
        ln.update({"yardstick_s": ty, "yardstick_values_s": t_values, "yardstick_centre_s": t_centre, "yardstick_product_s": t_product,
                   "yardstick_bytes_to_host": 8 * M * nq + 2 * 8 * nq, "yardstick_over_gram": ty / t_both,
                   "gram_within_twice_the_bound": bool(np.all(err <= 2 * bound)), "gram_max_error_over_bound": float(np.max(err / bound)),
                   "gram_max_relative_difference": float(np.max(err / np.maximum(np.abs(G), 1e-300))),
                   "dist2_max_difference_over_scale": float(np.max(np.abs(kept["dist2"] - D) / (g[:, None] + g[None, :]))),
                   "mean_equal_bit_for_bit": bool(np.array_equal(kept["mean"], vol["mean"], equal_nan=True)),
                   "std_equal_bit_for_bit": bool(np.array_equal(kept["std"], vol["std"], equal_nan=True))})
        del X, G, D, vol, bound, err
    if eigh:
        t0 = time.perf_counter()
        lam = np.linalg.eigh(kept["gram"])[0]
        ln.update({"host_eigh_s": time.perf_counter() - t0, "explained_first_8": (lam[::-1][:8] / lam.sum()).tolist(),
                   "participation": float(lam.sum() ** 2 / np.sum(lam * lam))})
    emit(ln, out)


def shape_rate(tt, ctx, ds, shape, repeat, yardstick, eigh, out):
    nchains, per, cells = (int(v) for v in shape.split("x"))
    prm = tt.define_TDstructrure().replace(max_cells=cells + 1000)
    hists = []
    for c in range(nchains):  # every 10th model of a chain started at `cells` uniform cells
        ch = tt.Chain(ctx, tt.chain_params(prm, ds, seed=2000 + c, chain=c + 1), tt.random_model(cells, 2000 + c))
        h = tt.History(ctx, per, per * (cells + 1000), with_ptS=False)
        ch.run_recorded(10 * per, 10, 10, h)
        ch.close()
        hists.append(h)
    print("%s: recorded" % shape, file=sys.stderr, flush=True)
    rate(tt, ctx, ds, hists, {"nchains": nchains, "models_per_chain": per, "cells": cells}, repeat, yardstick, eigh, out)
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
    ap.add_argument("--shapes", default="8x1250x2000,8x1250x5000")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--eigh", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gram", "gram_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        shape_rate(tt, ctx, ds, shape, a.repeat, not a.no_yardstick, a.eigh, a.out)


if __name__ == "__main__":
    main()
