"""Wall time of TD_inversion_function at bench.py's config 3 (381 rays, a 5000-cell starting model,
max_cells 10000) with and without the device sample history, in one process.

For keep_each in {10, 100, 1000} (n_iter 20000, burn_in 0): the proposals per second of history=False
(one launch and one td_chain_get_model per saved model) and of history=True (the kernel records the
saved models; launches end only at the launch cap or the history's memory budget), their ratio, the
chain_run launch counts, and whether the two model_hist agree bit for bit (each run --repeat times,
alternating; the median run is reported, every run's seconds listed).  With --profile also the
in-kernel cost of a sample: the phase stamps' total cycles of a recorded run (every iteration sampled)
minus an unrecorded one, per sample, beside the cycles of a proposal -- and minus an unrecorded run
that takes every decision on the exact sums (as a sampled iteration does), which leaves the copy.
(The stamps charge a sample's copy to the next iteration's first phase, so the sample of the launch's
last iteration is in no stamp: 1 of the 2000 is missing from the sum.)  One JSON line per figure.

    python tools/history_rate.py [--n-iter 20000] [--keeps 10,100,1000] [--repeat 5] [--profile]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tonga  # noqa: E402


def same(a, b):
    return (np.array_equal(a.xCell, b.xCell) and np.array_equal(a.yCell, b.yCell) and np.array_equal(a.zCell, b.zCell)
            and np.array_equal(a.zeta, b.zeta) and a.phi == b.phi and np.array_equal(a.ptS, b.ptS)
            and a.action == b.action and a.accept == b.accept)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-iter", type=int, default=20000)
    ap.add_argument("--keeps", default="10,100,1000")
    ap.add_argument("--cells", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    model = tt.random_model(a.cells, 3)
    warm = tt.define_TDstructrure().replace(max_cells=2 * a.cells, n_iter=200.0, burn_in=0.0, keep_each=100.0,
                                            print_each=0.0)
    tt.TD_inversion_function(warm, ds, 1, seed=1000, model=model)  # first-launch costs out of the way
    for keep in [int(k) for k in a.keeps.split(",") if k]:
        prm = tt.define_TDstructrure().replace(max_cells=2 * a.cells, n_iter=float(a.n_iter), burn_in=0.0,
                                               keep_each=float(keep), print_each=0.0)
        res, hist = {}, {}
        for rep in range(a.repeat):  # the two alternate; the median trial of each is reported
            for history in (False, True):
                ctx.timing(enable=True, reset=True)
                t0 = time.perf_counter()
                hist[history] = tt.TD_inversion_function(prm, ds, 1, seed=1000, model=model, history=history)
                dt = time.perf_counter() - t0
                launches, ms = ctx.timing(kernel="chain_run")
                ctx.timing(enable=False)
                res.setdefault(history, []).append(dict(seconds=dt, proposals_per_s=a.n_iter / dt, launches=launches,
                                                        kernel_ms=ms))
        for history in (False, True):
            runs = sorted(res[history], key=lambda r: r["seconds"])
            res[history] = dict(runs[len(runs) // 2], all_seconds=[round(r["seconds"], 4) for r in runs])
        ok = len(hist[True]) == len(hist[False]) and all(same(x, y) for x, y in zip(hist[True], hist[False]))
        print(json.dumps({"keep_each": keep, "n_iter": a.n_iter, "cells": a.cells, "saved": len(hist[True]),
                          "history_false": res[False], "history_true": res[True],
                          "ratio": res[True]["proposals_per_s"] / res[False]["proposals_per_s"],
                          "model_hist_equal": bool(ok)}), flush=True)
    if a.profile:
        prm = tt.define_TDstructrure().replace(max_cells=2 * a.cells)
        iters = 2000
        tot = {}
        for kind in ("plain", "exact", "recorded"):
            ch = tt.Chain(ctx, tt.chain_params(prm, ds, seed=1000, chain=1), model)
            if kind == "exact":  # every decision on the exact sums, as a sampled iteration's is
                tt.lib().tdt_chain_set_exact_every(ch.h, 1)
            prof = (ctypes.c_int64 * 80)()
            tt.lib().tdt_chain_profile(ch.h, 1, prof)
            base = [int(x) for x in prof]
            if kind == "recorded":
                h = tt.History(ctx, iters, iters * 2 * a.cells)
                ch.run_recorded(iters, 1, 1, h)
                h.close()
            else:
                ch.run(iters)
            tt.lib().tdt_chain_profile(ch.h, 0, prof)
            tot[kind] = sum(int(prof[k]) - base[k] for k in (0, 1, 2, 3, 4, 5, 6, 12, 13))  # every phase stamp
            ch.close()
        print(json.dumps({"profile_iters": iters, "cells": a.cells, "cycles_per_proposal": tot["plain"] / iters,
                          "cycles_per_proposal_exact_decisions": tot["exact"] / iters,
                          "cycles_per_recorded_proposal": tot["recorded"] / iters,
                          "cycles_per_sample": (tot["recorded"] - tot["plain"]) / iters,
                          "cycles_per_sample_copy_only": (tot["recorded"] - tot["exact"]) / iters}), flush=True)


if __name__ == "__main__":
    main()
