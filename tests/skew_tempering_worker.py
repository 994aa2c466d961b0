"""Child process of tests/test_gpu_skew_tempering_history.py: run with TD_LIB_PATH = the wave-skew build
(mcmc-in-tonga_amd/libtdstar_skew.so, chain_diag.h SKEW).  The recorded ladder of
tests/test_gpu_tempering_history.py (4 replicas of 12 cells at max_cells 16, K = 5, 24 rounds, rounds 3, 5,
... sampled) in both round protocols against its twin -- a non-resident ladder stepped round by round,
the cold chain's model read after each sampled round -- printing one JSON line per protocol: the history
equal or not, the trace equal or not, and the skew build's spin-guard slot summed over the replicas
(nonzero: a spin wait gave up)."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tonga  # noqa: E402
import test_gpu_tempering_history as t  # noqa: E402  (the shapes, the twin and the comparison)

tt = tonga.load()
ds = tt.load_data_Tonga()
ctx = tt.context_for(ds)
L = tt.lib()

chains = t.lds_chains(tt, ctx)
rounds, tlad = t.twin_run(tt, chains, t.ROUNDS, t.K, t.TMAX, t.SEED)
t.close_all(chains)
want = [(it, m) for r, j, it, m in rounds if r in t.sampled(t.ROUNDS, t.FIRST, t.EVERY)]
bad = False
for protocol in t.PROTOCOLS:
    chains = t.lds_chains(tt, ctx)
    lad = t.ladder(tt, chains, protocol, t.TMAX, t.SEED)
    hist = tt.History(ctx, len(want), len(want) * t.MAXC)
    lad.run(t.ROUNDS, t.K, history=hist, first=t.FIRST, every=t.EVERY)
    lad.close()
    same, why = True, None
    try:
        assert len(hist) == len(want)
        t.assert_samples(hist, want)
    except AssertionError as e:
        same, why = False, str(e)[:300]
    guard = 0
    prof = (ctypes.c_int64 * 80)()
    for c in chains:
        L.tdt_chain_profile(c.h, 0, prof)
        guard += int(prof[79])
    row = {"protocol": protocol, "same": same, "why": why, "trace": lad.trace_digest() == tlad.trace_digest(),
           "guard": guard, "samples": len(hist), "cells": [int(x) for x in np.diff(hist.read_arrays()["off"])]}
    print(json.dumps(row), flush=True)
    bad = bad or not same or not row["trace"] or guard != 0
    hist.close()
    t.close_all(chains)
sys.exit(1 if bad else 0)
