"""Wall time of the posterior predictive data of device histories (every sample's t* on the context's rays,
its chi^2, mean, std, quantiles 5/50/95, split R-hat, ESS and lags per ray), host call to host results, by
two routes in one process:

  predict    TdContext.predict_history (td_history_predict): one search structure for all samples where they
             lie, the ray points swept slab by slab, the statistics on the device
  yardstick  what there was before it: History.read() + TdContext.evaluate_batch (a host loop of full
             evaluates) + numpy for mean, std and the quantiles + TdContext.convergence on the matrix

ptS and phi of the two routes are compared bit for bit (as are R-hat, ESS and lags, which the same kernels
compute from the same matrix); numpy's mean, std and quantiles associate differently: their largest
differences are reported.  Shapes: CHAINSxSAMPLESxCELLS on the shipped 381 rays (chains started at CELLS
uniform cells, every 10th model recorded), and with --stress N one such chain of 20 000 cells on the 10 000
synthetic rays of the bench's config 5, N samples.  Per shape also the ray-sum kernel's time with
its workgroups of model m on XCD m % 8 and without (HIP events, median).

Each figure: one warm-up, then the median of --repeat runs (--yardstick-repeat for the yardstick).  One JSON
line per shape, printed and appended to profiles/predict/predict_rate.jsonl.

    python tools/predict_rate.py [--repeat 10] [--shapes 8x1250x2000,8x1250x5000] [--stress 780] [--no-yardstick]
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
KERNELS = ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute", "pred_ray_sums", "pred_chi2", "raster_quantile",
           "conv_moments", "conv_autocov", "conv_geyer", "nn_grid_build", "nn_grid", "nn_tile", "ray_sums")


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


def rate(tt, ctx, hists, line, repeat, yard_repeat, out):
    lens = [len(h) for h in hists]
    nmodels = sum(lens)
    ncell = sum(h.count()[1] for h in hists) / nmodels
    rp = np.sum(~np.isnan(ctx._arrays[0]), axis=1)

    def predict():
        return ctx.predict_history(hists, PROBS, convergence=True)

    def yardstick():
        models = [m.cells() for h in hists for m in h.read()]
        ptS, phi, _ = ctx.evaluate_batch(models)
        r = dict(ptS=ptS, phi=phi, mean=ptS.mean(axis=0), std=ptS.std(axis=0, ddof=1),
                 quantiles=np.quantile(ptS, PROBS, axis=0))
        r.update(ctx.convergence(ptS, lens))
        return r

    line.update({"nmodels": nmodels, "mean_cells": ncell, "rays": ctx.n, "points": ctx.P, "repeat": repeat,
                 "pairs": nmodels * ctx.P, "plan": ctx.predict_plan(nmodels, rp)[:2],
                 "slabs": len(ctx.predict_plan(nmodels, rp)[2]) - 1})
    t, runs, r = median_run(predict, repeat)
    line.update({"predict_s": t, "predict_all_s": runs, "predict_kernel_ms": kernel_ms(ctx, predict),
                 "pairs_per_s_search": None})
    ks = line["predict_kernel_ms"]
    sweep = ks.get("vol_search", ks.get("raster_brute"))
    line["pairs_per_s_search"] = nmodels * ctx.P / (sweep["ms"] * 1e-3)
    place = {}
    for name, on in (("consecutive", False), ("xcd", True)):  # the ray sums' placement, by HIP events
        ctx.set_predict_placement(on)
        predict()
        place[name] = float(np.median([kernel_ms(ctx, predict)["pred_ray_sums"]["ms"] for _ in range(repeat)]))
    ctx.set_predict_placement(False)
    line["pred_ray_sums_ms"] = place
    if yard_repeat > 0:
        ty, runs_y, y = median_run(yardstick, yard_repeat)
        full = ctx.predict_history(hists, PROBS, convergence=True, want_values=True)
        equal = np.array_equal(full["ptS"], y["ptS"]) and np.array_equal(full["phi"], y["phi"]) and \
            all(np.array_equal(full[f], r[f], equal_nan=True) for f in ("phi", "mean", "std", "quantiles", "rhat", "ess", "lags"))
        conv_equal = all(np.array_equal(full[f], y[f], equal_nan=True) for f in ("rhat", "ess", "lags"))
        line.update({"yardstick_s": ty, "yardstick_all_s": runs_y, "yardstick_repeat": yard_repeat,
                     "yardstick_kernel_ms": kernel_ms(ctx, yardstick), "yardstick_over_predict": ty / t,
                     "predict_not_slower": bool(t <= ty), "ptS_phi_equal_bit_for_bit": bool(equal),
                     "rhat_ess_lags_equal_bit_for_bit": bool(conv_equal),
                     "numpy_max_abs_diff": {f: float(np.nanmax(np.abs(full[f] - y[f]))) for f in ("mean", "std", "quantiles")}})
    emit(line, out)


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
    rate(tt, ctx, hists, {"geometry": "381 rays", "nchains": nchains, "models_per_chain": per, "cells": cells}, repeat,
         yard_repeat, out)
    for h in hists:
        h.close()


def stress_rate(tt, nsamples, repeat, yard_repeat, out):
    ds = tt.synthetic_rays(10000, seed=5)
    ctx = tt.TdContext.from_datastruct(ds)
    cells = 20000
    prm = tt.define_TDstructrure().replace(max_cells=cells + 1000)
    ch = tt.Chain(ctx, tt.chain_params(prm, ds, seed=5, chain=1), tt.random_model(cells, 5))
    h = tt.History(ctx, nsamples, nsamples * (cells + 1000), with_ptS=False)
    ch.run_recorded(10 * nsamples, 10, 10, h)
    ch.close()
    rate(tt, ctx, [h], {"geometry": "config 5: 10000 synthetic rays", "nchains": 1, "models_per_chain": nsamples,
                        "cells": cells, "search_structure_bytes": 68 * h.count()[1]}, repeat, yard_repeat, out)
    h.close()
    ctx.close()


def emit(line, out):
    line = json.dumps(line)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--yardstick-repeat", type=int, default=10)
    ap.add_argument("--stress-yardstick-repeat", type=int, default=1)
    ap.add_argument("--shapes", default="8x1250x2000,8x1250x5000")
    ap.add_argument("--stress", type=int, default=0, help="samples of the config-5 line (0: skip it)")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict", "predict_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        shape_rate(tt, ctx, ds, shape, a.repeat, 0 if a.no_yardstick else a.yardstick_repeat, a.out)
    if a.stress > 0:
        stress_rate(tt, a.stress, a.repeat, 0 if a.no_yardstick else a.stress_yardstick_repeat, a.out)


if __name__ == "__main__":
    main()
