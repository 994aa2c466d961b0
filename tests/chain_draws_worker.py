"""Child process of tests/test_gpu_chain_reference.py test_in_kernel_draws_follow_the_restatement: run with
TD_PRE_DRAWS=0 (read once per process, csrc/chain_kernels.hip chain_run), so that every launch of the product
library draws its uniforms inside k_chain_run instead of loading them from k_draws' table.  Case A prior 1
of tests/chain_cases.py for ITERS iterations on each free-running instance: the automatic layout and
lds_mode 1, plain and recorded, alone; lds_mode 2 and 3 as a run_batch / run_batch_recorded of two chains
(chain numbers 1 and 2); and the two recorded single-chain runs again from iteration 2^32 - 100 on, where the
kernel's own refill (iter0 + it + 1 + lane) carries the counter across 2^32.  One JSON line per run -- the
history (every iteration) where it records, the end state of each chain -- then one with
tdt_chain_launch_counts and tdt_chain_draws_launches.  The parent compares them with the restatement; here the
first error ends the process."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tonga  # noqa: E402
import chain_cases as cc  # noqa: E402

NAME, ITERS = "A-p1-T1", 200
# run -> (lds_mode, recorded, chain numbers, start_iter (0: iteration 1))
RUNS = {"auto": (0, False, [1], 0), "auto_rec": (0, True, [1], 0), "hbm": (1, False, [1], 0),
        "hbm_rec": (1, True, [1], 0), "packed_tiles": (2, False, [1, 2], 0), "packed_tiles_rec": (2, True, [1, 2], 0),
        "packed_hbm": (3, False, [1, 2], 0), "packed_hbm_rec": (3, True, [1, 2], 0),
        "auto_rec_high": (0, True, [1], cc.HIGH_START), "hbm_rec_high": (1, True, [1], cc.HIGH_START)}


def end_state(c):
    m = c.model()
    return dict(stats=c.stats(), cells=[a.tolist() for a in m.cells()], phi=m.phi, ptS=m.ptS.tolist())


def one_run(tt, ctx, run):
    """A run's JSON row; its chains and histories are closed on the way out whatever happens (they read their
    context when destroyed, so none may outlive it)."""
    lds_mode, recorded, numbers, start_iter = RUNS[run]
    _, ncells, _, max_cells, _, prior, _, seed = cc.CASES[NAME]
    chains, hists = [], []
    try:
        for number in numbers:
            p = cc.chain_params(tt, NAME, start_iter=start_iter)
            p.chain = number
            chains.append(tt.Chain(ctx, p, cc.start_model(tt, ncells, prior, seed)))
            assert tt.lib().tdt_chain_set_lds_mode(chains[-1].h, lds_mode) == 0
            if recorded:
                hists.append(tt.History(ctx, ITERS, ITERS * max_cells, with_ptS=True))
        if len(chains) == 1:
            if recorded:
                chains[0].run_recorded(ITERS, 1, 1, hists[0])
            else:
                chains[0].run(ITERS)
        elif recorded:
            tt.run_batch_recorded(chains, ITERS, 1, 1, hists)
        else:
            tt.run_batch(chains, ITERS)
        return {"run": run, "ends": [end_state(c) for c in chains],
                "histories": [{k: (None if v is None else np.asarray(v).tolist()) for k, v in h.read_arrays().items()}
                              for h in hists]}
    finally:
        for x in hists + chains:
            x.close()


def main():
    assert os.environ.get("TD_PRE_DRAWS") == "0", "run with TD_PRE_DRAWS=0"
    tt = tonga.load()
    L = tt.lib()
    ctx = tt.TdContext.from_datastruct(cc.rays(tt, cc.CASES[NAME][0]))
    try:
        for run in RUNS:
            print(json.dumps(one_run(tt, ctx, run)), flush=True)
        out, n, d = (ctypes.c_int64 * 32)(), ctypes.c_int(0), ctypes.c_int64(-1)
        assert L.tdt_chain_launch_counts(out, ctypes.byref(n)) == 0
        assert L.tdt_chain_draws_launches(ctypes.byref(d)) == 0
        print(json.dumps({"launched": [out[i] for i in range(n.value)], "draws_launches": d.value}), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
