"""What recording the cold replica of a tempering ladder costs, at bench.py's config-4 shape (8 replicas x
2000 cells, max_cells 4000, K = 10 proposals per round, 300 rounds after 20 of warm-up, T in [1, 8], seed
4242), in one process and one build.  One JSON line per figure, ms per round (median of --repeat runs,
every run listed):

  unrecorded   TemperingLadder.run(rounds, K), host-decided and device-decided swaps
  recorded     run(rounds, K, history=h, every=E) for E in --everys, both protocols, the pack included;
               beside it the pack kernel's own time (the context's "history_pack" timer) and whether the
               trace digest is the unrecorded run's  (skipped when the build has no recording)
  step_model   the only route to the same samples without it: step(K) every round and the cold chain's
               model() after each sampled round

Builds are compared by running this file once per build, alternating, each run under its own time limit:
--root names the tree whose package and library are loaded (default: this one), so a checkout of another
commit is measured by the same script.

  python tools/tempering_history_rate.py [--root DIR] [--repeat 3] [--everys 1,10,100] [--rounds 300]

--scan: no timing; the twin ladder of tests/test_gpu_tempering_history.py (4 replicas of 12 cells, max_cells
16, K = 5, 24 rounds, rounds 3, 5, ... sampled) for every (chain seed base, tmax, ladder seed) of a small
grid: which replicas hold level 0 in the sampled rounds and the samples' cell counts -- where the test's BASE,
TMAX and SEED come from.
"""
import argparse
import json
import os
import sys
import time


def chains_of(tt, ctx, ds, nrep, ncells):
    prm = tt.define_TDstructrure().replace(max_cells=2 * ncells)
    return [tt.Chain(ctx, tt.chain_params(prm, ds, seed=100 + g, chain=1 + g), tt.random_model(ncells, 100 + g))
            for g in range(nrep)]


def median(rows):
    s = sorted(rows)
    return s[len(s) // 2]


def scan(tt, ctx):
    nrep, ncells, maxc, k, rounds, first, every = 4, 12, 16, 5, 24, 3, 2
    prm = tt.define_TDstructrure().replace(max_cells=maxc)
    for base in range(300, 600, 10):  # replica j: seed base + j, model random_model(12, base + j)
        for tmax in (1.05, 1.1, 1.2):
            for seed in range(1, 7):
                chains = [tt.Chain(ctx, tt.chain_params(prm, None, seed=base + j, chain=1 + j),
                                   tt.random_model(ncells, base + j)) for j in range(nrep)]
                lad = tt.TemperingLadder(chains, tmax=tmax, seed=seed, resident=False)
                cold, sizes = [], []
                for r in range(1, rounds + 1):
                    j = lad.cold_local()
                    lad.step(k)
                    if r >= first and (r - first) % every == 0:
                        cold.append(j)
                        sizes.append(chains[j].stats()["ncells"])
                ok = len(set(cold)) >= 2 and maxc in sizes and min(sizes) < maxc
                print(json.dumps({"scan": True, "base": base, "tmax": tmax, "seed": seed, "ok": ok, "cold": cold,
                                  "ncells": sizes, "swap_rates": [round(x, 2) for x in lad.swap_rates()]}), flush=True)
                for c in chains:
                    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--everys", default="1,10,100")
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--cells", type=int, default=2000)
    ap.add_argument("--scan", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import tonga

    tt = tonga.load()
    ds = tt.load_data_Tonga()
    ctx = tt.context_for(ds)
    if a.scan:
        return scan(tt, ctx)
    has_rec = hasattr(tt.lib(), "td_rounds_temper_recorded")
    base = {"root": os.path.abspath(a.root), "replicas": a.replicas, "cells": a.cells, "k": a.k, "rounds": a.rounds}
    everys = [int(e) for e in a.everys.split(",") if e]

    def ladder(device_swaps):
        chains = chains_of(tt, ctx, ds, a.replicas, a.cells)
        lad = tt.TemperingLadder(chains, tmax=8.0, seed=4242, device_swaps=device_swaps)
        lad.run(a.warm, a.k)
        return chains, lad

    def done(chains, lad):
        lad.close()
        for c in chains:
            c.close()

    digest = {}
    for proto, dev in (("host_decided", False), ("device_swaps", True)):
        ms = []
        for _ in range(a.repeat):
            chains, lad = ladder(dev)
            t0 = time.perf_counter()
            lad.run(a.rounds, a.k)
            ms.append((time.perf_counter() - t0) / a.rounds * 1e3)
            digest[proto] = lad.trace_digest()
            done(chains, lad)
        print(json.dumps(dict(base, what="unrecorded", protocol=proto, ms_per_round=round(median(ms), 5),
                              all_ms=[round(x, 5) for x in ms])), flush=True)
    for every in everys if has_rec else []:
        ns = len(range(1, a.rounds + 1, every))
        for proto, dev in (("host_decided", False), ("device_swaps", True)):
            ms, pack, same = [], [], True
            for _ in range(a.repeat):
                chains, lad = ladder(dev)
                hist = tt.History(ctx, ns, ns * 2 * a.cells, with_ptS=True)
                ctx.timing(enable=True, reset=True)
                t0 = time.perf_counter()
                lad.run(a.rounds, a.k, history=hist, first=1, every=every)
                ms.append((time.perf_counter() - t0) / a.rounds * 1e3)
                pack.append(ctx.timing(kernel="history_pack")[1])
                ctx.timing(enable=False)
                same = same and lad.trace_digest() == digest[proto] and len(hist) == ns
                hist.close()
                done(chains, lad)
            print(json.dumps(dict(base, what="recorded", protocol=proto, every=every, samples=ns,
                                  slot_cells=2 * a.cells, ms_per_round=round(median(ms), 5),
                                  all_ms=[round(x, 5) for x in ms], history_pack_ms=round(median(pack), 4),
                                  all_history_pack_ms=[round(x, 4) for x in pack], trace_as_unrecorded=same)),
                  flush=True)
    for every in everys:
        ms = []
        for _ in range(a.repeat):
            chains, lad = ladder(False)
            kept = []
            t0 = time.perf_counter()
            for r in range(1, a.rounds + 1):
                j = lad.cold_local()
                lad.step(a.k)
                if (r - 1) % every == 0:
                    kept.append(chains[j].model())
            ms.append((time.perf_counter() - t0) / a.rounds * 1e3)
            done(chains, lad)
        print(json.dumps(dict(base, what="step_model", protocol="host_decided", every=every, samples=len(kept),
                              ms_per_round=round(median(ms), 5), all_ms=[round(x, 5) for x in ms])), flush=True)


if __name__ == "__main__":
    main()
