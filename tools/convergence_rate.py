"""Wall time of the convergence diagnostics of one cross-section (split R-hat, ESS and lags per node,
max_lag 0), host arrays to host results, by two routes in one process:

  device  TdContext.convergence_models (td_rasterize_convergence): value matrix, moments,
          autocovariances and Geyer's sum on the device; only the results come back
  host    what there was before it: TdContext.rasterize(..., want_values=True) brings the
          nmodels x nq value matrix to the host, then the same formulas in numpy, vectorised over
          columns, sequences and the summed index (np.sum's pairwise association: the values differ
          from the device's in the last bits, so they are compared to 1e-9, not bit for bit)

at two shapes over the xz section of the shipped grid: 8 chains x 1250 models x 200 cells (a densely
thinned ensemble) and 2 chains x 50 models x 5000 cells (a reference-sized model_hist).  Each route:
one warm-up, then the median of --repeat runs; the device route's kernels by HIP events as well, with
the number of rounds, for both lag blocks.  One JSON line per shape, printed and appended to
profiles/convergence/convergence_rate.jsonl.

    python tools/convergence_rate.py [--repeat 10] [--shapes 8x1250x200,2x50x5000]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tonga  # noqa: E402

KERNELS = ("raster_brute", "conv_moments", "conv_autocov", "conv_geyer")


def host_convergence(V, lens):
    """The formulas of include/tdstar.h, every lag up to n - 1 computed for every column (numpy has no
    cheap way to stop column by column), then Geyer's sum lag pair by lag pair."""
    n, m = min(lens) // 2, 2 * len(lens)
    T = n - 1
    X = np.empty((m, n, V.shape[1]))
    pos = 0
    for c, L in enumerate(lens):
        X[2 * c] = V[pos + L - 2 * n:pos + L - n]
        X[2 * c + 1] = V[pos + L - n:pos + L]
        pos += L
    with np.errstate(all="ignore"):
        mean = X.sum(axis=1) / n
        D = X - mean[:, None, :]
        W = ((D * D).sum(axis=1) / (n - 1)).sum(axis=0) / m
        mu = mean.sum(axis=0) / m
        Bn = ((mean - mu) ** 2).sum(axis=0) / (m - 1)
        vp = (n - 1) / n * W + Bn
        rhat = np.sqrt(vp / W)

        def rho(t):
            return 1.0 - (W - ((D[:, :n - t] * D[:, t:]).sum(axis=1) / n).sum(axis=0) / m) / vp

        Pprev = 1.0 + rho(1)
        S = Pprev.copy()
        last = np.ones(V.shape[1], dtype=np.int64)
        going = np.ones(V.shape[1], dtype=bool)
        k = 1
        while 2 * k + 1 <= T and going.any():
            P = rho(2 * k) + rho(2 * k + 1)
            going &= P > 0
            P = np.where(P > Pprev, Pprev, P)
            S = np.where(going, S + P, S)
            Pprev = np.where(going, P, Pprev)
            last = np.where(going, 2 * k + 1, last)
            k += 1
        tau = -1.0 + 2.0 * S
        floor = 1.0 / math.log10(float(m * n))
        tau = np.where(tau < floor, floor, tau)
        return dict(rhat=rhat, ess=m * n / tau, lags=np.where(going, -last, last).astype(np.int32))


def median_run(fn, repeat):
    fn()  # warm-up: allocations, first launches
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
        print("  %s %.4f s" % (fn.__name__, ts[-1]), file=sys.stderr, flush=True)
    return float(np.median(ts)), [round(t, 5) for t in ts], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--shapes", default="8x1250x200,2x50x5000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convergence", "convergence_rate.jsonl"))
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    xv, zv = np.asarray(ds.xVec, dtype=np.float64), np.asarray(ds.zVec, dtype=np.float64)
    qx, qz = np.tile(xv, len(zv)), np.repeat(zv, len(xv))
    qy = np.full(qx.shape, 150.0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for shape in [s for s in a.shapes.split(",") if s]:
        nchains, per, cells = (int(v) for v in shape.split("x"))
        lens = [per] * nchains
        # a chain's consecutive samples share most cells: each model moves a tenth of its predecessor's
        models = []
        for c in range(nchains):
            rng = np.random.default_rng(1000 + c)
            cur = [np.array(v, dtype=np.float64) for v in tt.random_model(cells, 1000 + c).cells()]
            for k in range(per):
                idx = rng.choice(cells, max(cells // 10, 1), replace=False)
                fresh = tt.random_model(len(idx), 5000 + 997 * c + k).cells()
                for j in range(4):
                    cur[j][idx] = fresh[j]
                models.append(tuple(v.copy() for v in cur))

        def device():
            return ctx.convergence_models(models, lens, qx, qy, qz)

        def host():
            mean, std, V = ctx.rasterize(models, qx, qy, qz, want_values=True)
            return dict(host_convergence(V, lens), mean=mean, std=std)

        line = {"nchains": nchains, "models_per_chain": per, "cells": cells, "nq": len(qx), "n": per // 2,
                "m": 2 * nchains, "repeat": a.repeat}
        for LB in (8, 16):
            ctx.set_convergence_lag_block(LB)
            t_dev, all_dev, r_dev = median_run(device, a.repeat)
            ctx.timing(enable=True, reset=True)
            device()
            line["lag_block_%d" % LB] = {"device_s": t_dev, "device_all_s": all_dev,
                                         "kernel_ms": {k: ctx.timing(kernel=k)[1] for k in KERNELS},
                                         "rounds": ctx.timing(kernel="conv_geyer")[0]}
            ctx.timing(enable=False)
        ctx.set_convergence_lag_block(0)
        t_dev, all_dev, r_dev = median_run(device, a.repeat)
        t_host, all_host, r_host = median_run(host, a.repeat)
        with np.errstate(all="ignore"):
            close = all(np.allclose(r_dev[f], r_host[f], rtol=1e-9, atol=0, equal_nan=True) for f in ("rhat", "ess"))
        line.update({"device_s": t_dev, "host_s": t_host, "host_over_device": t_host / t_dev,
                     "device_not_slower": bool(t_dev <= t_host), "device_all_s": all_dev, "host_all_s": all_host,
                     "mean_std_equal": bool(np.array_equal(r_dev["mean"], r_host["mean"]) and
                                            np.array_equal(r_dev["std"], r_host["std"], equal_nan=True)),
                     "rhat_ess_close_1e-9": bool(close),
                     "lags_equal_share": float(np.mean(r_dev["lags"] == r_host["lags"])),
                     "rhat_max": float(np.nanmax(r_dev["rhat"])), "ess_min": float(np.nanmin(r_dev["ess"])),
                     "lags_max": int(np.abs(r_dev["lags"]).max()), "capped_share": float(np.mean(r_dev["lags"] < 0))})
        line = json.dumps(line)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
