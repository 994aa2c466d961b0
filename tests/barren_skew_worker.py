"""Child process of tests/test_gpu_barren.py: run with TD_LIB_PATH = the wave-skew build
(mcmc-in-tonga_amd/libtdstar_skew.so, chain_diag.h SKEW).  The hand-placed hazard model and the 200-cell
shape, LDS and HBM layout, against the HOST engine; one JSON line per run: `same` (phi, counters, cells and
ptS), `guard` (the skew build's spin-guard slot prof[79]), `own` (tdt_chain_own_check) and `short` (proposals
taken on the short road).  Stops at the first failure (the state is then broken)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tonga  # noqa: E402
import test_gpu_barren as tb  # noqa: E402

assert "skew" in os.path.basename(os.environ.get("TD_LIB_PATH", "")), "run with TD_LIB_PATH = the skew build"
tt = tonga.load()
ds = tt.load_data_Tonga()
ctx = tt.context_for(ds)
ITERS = 600  # (a skewed iteration sleeps for several phases)
for name in ("hazard", "m200"):
    host = tb.make(tt, ds, ctx, name, tt.TD_ENGINE_HOST)
    host.run(ITERS)
    want = tb.end_state(host)
    host.close()
    for lds_mode in (0, 1):
        dev = tb.make(tt, ds, ctx, name, tt.TD_ENGINE_DEVICE, lds_mode)
        p0 = tb.profile(tt, dev, 1)
        for part in (ITERS // 2, ITERS - ITERS // 2):
            dev.run(part)
        prof = tb.profile(tt, dev, 0)
        row = {"case": name, "lds_mode": lds_mode, "same": bool(tb.same_state(tb.end_state(dev), want)),
               "guard": int(prof[79]), "own": int(tb.own_check(tt, dev)),
               "short": int(prof[35] + prof[45] - p0[35] - p0[45])}
        dev.close()
        print(json.dumps(row), flush=True)
        if not row["same"] or row["guard"] or row["own"]:
            sys.exit(1)
