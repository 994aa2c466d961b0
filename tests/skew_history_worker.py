"""Child process of tests/test_gpu_skew_history.py: run with TD_LIB_PATH = the wave-skew build
(mcmc-in-tonga_amd/libtdstar_skew.so, chain_diag.h SKEW).  Recorded runs of the device chain
(td_chain_run_recorded: the sample copy and its barrier are skew sites too) against the HOST engine
recording from its host loop, on the 8-cell model at max_cells 12 and the 200-cell one, every 1 and
every 3: one JSON line per run -- the histories equal or not, the end states equal or not, and the skew
build's spin-guard slot (nonzero: a spin wait gave up).  Stops at the first mismatch or guard trip."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tonga  # noqa: E402

tt = tonga.load()
ds = tt.load_data_Tonga()
ctx = tt.TdContext.from_datastruct(ds)
L = tt.lib()
for ncells, max_cells, iters, seed in [(8, 12, 300, 4), (200, 300, 200, 1)]:
    for every in (1, 3):
        prm = tt.define_TDstructrure().replace(max_cells=max_cells)
        model = tt.random_model(ncells, seed)
        dev = tt.Chain(ctx, tt.chain_params(prm, None, seed=seed, chain=1, engine=tt.TD_ENGINE_DEVICE), model)
        host = tt.Chain(ctx, tt.chain_params(prm, None, seed=seed, chain=1, engine=tt.TD_ENGINE_HOST), model)
        ns = iters // every + 1
        hd, hh = tt.History(ctx, ns, ns * max_cells), tt.History(ctx, ns, ns * max_cells)
        prof = (ctypes.c_int64 * 80)()
        for k in range(2):  # two launches: `first` carried over the cut
            first = every - (k * (iters // 2)) % every
            dev.run_recorded(iters // 2, first, every, hd)
            host.run_recorded(iters // 2, first, every, hh)
        L.tdt_chain_profile(dev.h, 0, prof)
        a, b = hd.read_arrays(), hh.read_arrays()
        same = len(hd) == len(hh) > 0 and all(np.array_equal(a[key], b[key]) for key in a)
        sd, sh = dev.stats(), host.stats()
        end = sd["phi"] == sh["phi"] and sd["accepted"] == sh["accepted"] and sd["ncells"] == sh["ncells"]
        print(json.dumps({"cells": ncells, "every": every, "samples": len(hd), "same": bool(same), "end": bool(end),
                          "guard": int(prof[79]),
                          "sites": [int(prof[56 + w]) for w in range(8)] if prof[79] else None}), flush=True)
        if not same or not end or prof[79]:
            sys.exit(1)
        for x in (hd, hh, dev, host):
            x.close()
