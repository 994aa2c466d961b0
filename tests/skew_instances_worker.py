"""Child process of tests/test_gpu_skew_instances.py: run with TD_LIB_PATH = the wave-skew build
(mcmc-in-tonga_amd/libtdstar_skew.so, chain_diag.h SKEW) and the names of the cases to run.  One case per
k_chain_run instance and run-time mode that the three older skew workers do not reach, each against the
HOST engine (a full td_evaluate per proposal: no chain kernel, so nothing the skew build changes), at the
smallest shapes that reach the code.  One JSON line per case: `same` (the end state -- phi, accepted,
proposed, ncells and the models cell for cell; histories and trace digests where the case has them),
`guard` (the skew build's spin-guard slot prof[79], summed over the case's chains; nonzero: a spin wait
gave up) and `sites` (where the waves were then), `launched` (tdt_chain_launch_counts over the case's
device launches) and `twin_launched` (over everything else in the case: 0), and the figures of the
reference runs that the parent holds against a minimum: `accepted` (per action, the least over the case's
twins), `swaps`, `long_shifts`.  Stops at the first case that fails (the state is then broken)."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tonga  # noqa: E402
import test_gpu_incremental as ti  # noqa: E402  (the edit walk)
import test_gpu_tempering_history as th  # noqa: E402  (the recorded ladder's shapes, twin and comparison)

assert "skew" in os.path.basename(os.environ.get("TD_LIB_PATH", "")), "run with TD_LIB_PATH = the skew build"
tt = tonga.load()
L = tt.lib()
DS = tt.load_data_Tonga()
DEVICE, HOST, DROPIN = tt.TD_ENGINE_DEVICE, tt.TD_ENGINE_HOST, tt.TD_ENGINE_DROPIN

# the two shapes every free-running case runs (cells, max_cells, iterations, seed): tests/skew_worker.py's
# 8-cell model at max_cells 12, whose births at the cap are inactive proposals, and the 200-cell one
SMALL = [(8, 12, 600, 4), (200, 300, 400, 1)]
# the large models whose accepted deaths shift the order in HBM over more than one round of the block: the
# round's entries, then the shape
LONG8 = (8 * 512, (9000, 9100, 240, 3))
LONG4 = (8 * 256, (5000, 5100, 400, 3))
# the smallest ray count (a multiple of 50) of tt.synthetic_rays(N, seed=8) at which the drop-in path's shadow
# chain of a 300-cell model takes the HBM layout: 450 rays still launch instance 1
HBM_RAYS = 500


def launches():
    out = (ctypes.c_int64 * 32)()
    n = ctypes.c_int(0)
    assert L.tdt_chain_launch_counts(out, ctypes.byref(n)) == 0
    return np.array([out[i] for i in range(n.value)], dtype=np.int64)


class Case:
    """A case's row: the device launches are made through dev(), so that their table entries are counted
    apart from whatever else the case runs."""

    def __init__(self, name):
        self.name, self.same, self.why = name, True, None
        self.guard, self.sites = 0, None
        self.accepted = self.swaps = self.long_shifts = None
        self.t0 = time.perf_counter()
        self.start = launches()
        self.launched = np.zeros_like(self.start)

    def dev(self, f, *a, **k):
        before = launches()
        out = f(*a, **k)
        self.launched += launches() - before
        return out

    def check(self, ok, why):
        if not ok and self.same:
            self.same, self.why = False, why

    def twin_stats(self, st):
        acc = [int(x) for x in st["accepted"]]
        self.accepted = acc if self.accepted is None else [min(a, b) for a, b in zip(self.accepted, acc)]

    def read_guard(self, chains=(), ctxs=()):
        prof = (ctypes.c_int64 * 80)()
        for kind, x in [(0, c) for c in chains] + [(1, c) for c in ctxs]:
            rc = L.tdt_chain_profile(x.h, 0, prof) if kind == 0 else L.tdt_shadow_profile(x.h, prof)
            self.check(rc == 0, "no profile to read the guard from")
            if prof[79] and self.sites is None:
                self.sites = [int(prof[56 + w]) for w in range(8)] + [int(prof[64])]
            self.guard += int(prof[79])

    def row(self):
        total = launches() - self.start
        return {"case": self.name, "same": bool(self.same), "why": self.why, "guard": self.guard, "sites": self.sites,
                "launched": [int(x) for x in self.launched], "twin_launched": int((total - self.launched).sum()),
                "accepted": self.accepted, "swaps": self.swaps, "long_shifts": self.long_shifts,
                "seconds": round(time.perf_counter() - self.t0, 2)}


def chain(ctx, ncells, max_cells, seed, engine, lds_mode=0, chain_no=1, model_seed=None):
    prm = tt.define_TDstructrure().replace(max_cells=max_cells)
    c = tt.Chain(ctx, tt.chain_params(prm, None, seed=seed, chain=chain_no, engine=engine),
                 tt.random_model(ncells, seed if model_seed is None else model_seed))
    if engine == DEVICE and lds_mode:
        assert L.tdt_chain_set_lds_mode(c.h, lds_mode) == 0
    return c


def same_models(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("xCell", "yCell", "zCell", "zeta"))


def same_end(a, b):
    sa, sb = a.stats(), b.stats()
    return (all(sa[k] == sb[k] for k in ("phi", "accepted", "proposed", "ncells", "iterations")) and
            same_models(a.model(), b.model()))


def run_counting_long_shifts(host, iters, span):
    """host.run(iters), one proposal at a time -> the accepted deaths whose Julia index i leaves more than
    `span` entries to shift (i + 1 + span < ncells before the death: a second round of the block).  The
    host model is in Julia order, so i is where the models before and after first differ."""
    count = 0
    prev = host.model()
    for _ in range(iters):
        before = sum(host.stats()["accepted"])
        host.run(1)
        st = host.stats()
        if sum(st["accepted"]) == before:
            continue
        cur = host.model()
        n = len(prev.xCell)
        if len(cur.xCell) == n - 1:
            eq = ((prev.xCell[:n - 1] == cur.xCell) & (prev.yCell[:n - 1] == cur.yCell) &
                  (prev.zCell[:n - 1] == cur.zCell) & (prev.zeta[:n - 1] == cur.zeta))
            i = n - 1 if eq.all() else int(np.argmin(eq))
            count += i + 1 + span < n
        prev = cur
    return int(count)


def ctx381():
    return tt.context_for(DS)


# ---------------------------------------------------------------- free-running: instances 2, 4, 5 ----
def hbm_free():
    """Instance 2: lds_mode 1, one chain per launch, each against its HOST twin."""
    c, ctx = Case("hbm_free"), ctx381()
    span, big = LONG8
    c.long_shifts = 0
    for ncells, max_cells, iters, seed in SMALL + [big]:
        dev, host = (chain(ctx, ncells, max_cells, seed, e, 1) for e in (DEVICE, HOST))
        for part in (iters // 3, iters - iters // 3):
            c.dev(dev.run, part)
        if (ncells, max_cells, iters, seed) == big:
            c.long_shifts += run_counting_long_shifts(host, iters, span)
        else:
            host.run(iters)
        c.check(same_end(dev, host), "%d cells: %r / %r" % (ncells, dev.stats(), host.stats()))
        c.twin_stats(host.stats())
        c.read_guard([dev])
        dev.close()
        host.close()
    return c


def packed(name, lds_mode):
    """Instances 4 and 5: a run_batch of three chains of lds_mode 3 / 2 (the 4-wave kernel: all in HBM / the
    tiles in LDS), each against its HOST twin."""
    c, ctx = Case(name), ctx381()
    span, big = LONG4
    iters = big[2]
    specs = [(n, m, s) for n, m, _, s in SMALL + [big]]
    devs = [chain(ctx, n, m, s, DEVICE, lds_mode, chain_no=1 + j) for j, (n, m, s) in enumerate(specs)]
    hosts = [chain(ctx, n, m, s, HOST, chain_no=1 + j) for j, (n, m, s) in enumerate(specs)]
    for part in (iters // 3, iters - iters // 3):
        c.dev(tt.run_batch, devs, part)
    c.long_shifts = run_counting_long_shifts(hosts[-1], iters, span)
    for h in hosts[:-1]:
        h.run(iters)
    for d, h, (n, _, _) in zip(devs, hosts, specs):
        c.check(same_end(d, h), "%d cells: %r / %r" % (n, d.stats(), h.stats()))
        c.twin_stats(h.stats())
    c.read_guard(devs)
    for x in devs + hosts:
        x.close()
    return c


# ------------------------------------------------------------- recorded: instances 9, 10, 11 ----
def recorded(name, lds_mode):
    """The recorded forms of the two small shapes, every 1 and 3, over two launches with `first` carried
    over the cut (tests/skew_history_worker.py's runs in another layout), against the HOST engine's
    run_recorded."""
    c, ctx = Case(name), ctx381()
    for ncells, max_cells, iters, seed in SMALL:
        for every in (1, 3):
            dev, host = (chain(ctx, ncells, max_cells, seed, e, lds_mode) for e in (DEVICE, HOST))
            ns = iters // every + 1
            hd, hh = tt.History(ctx, ns, ns * max_cells), tt.History(ctx, ns, ns * max_cells)
            for k in range(2):
                first = every - (k * (iters // 2)) % every
                c.dev(dev.run_recorded, iters // 2, first, every, hd)
                host.run_recorded(iters // 2, first, every, hh)
            a, b = hd.read_arrays(), hh.read_arrays()
            c.check(len(hd) == len(hh) > 0 and all(np.array_equal(a[k], b[k]) for k in a),
                    "%d cells every %d: histories of %d / %d samples differ" % (ncells, every, len(hd), len(hh)))
            c.check(same_end(dev, host), "%d cells every %d: %r / %r" % (ncells, every, dev.stats(), host.stats()))
            c.twin_stats(host.stats())
            c.read_guard([dev])
            for x in (hd, hh, dev, host):
                x.close()
    return c


# ------------------------------------------------------------------- scripted: instances 1, 3 ----
def edit_kind(cur, prop):
    if len(prop[0]) != len(cur[0]):
        return 0 if len(prop[0]) > len(cur[0]) else 1
    return 2 if not np.array_equal(prop[3], cur[3]) else 3


def dropin(name, ds, shapes, walk_cells):
    """Instances 1 and 3: a DROPIN chain (the host loop calling td_evaluate; the context follows it with
    its resident server, fed scripted steps through the mailbox) against the HOST engine on a context of
    its own; then a context with a k_chain_run launch per td_evaluate (tdt_set_incremental 1) through
    100 steps of tests/test_gpu_incremental.py's edit walk against a context with the incremental path
    off -- the twin of that test: a td_evaluate has no HOST engine, and the full evaluate is what the HOST
    engine runs.  `accepted` counts the walk's kept edits by action beside the chains' accepted proposals."""
    c = Case(name)
    for ncells, max_cells, iters, seed in shapes:
        ca, cb = tt.TdContext.from_datastruct(ds), tt.TdContext.from_datastruct(ds)
        dev, host = chain(ca, ncells, max_cells, seed, DROPIN), chain(cb, ncells, max_cells, seed, HOST)
        for part in (iters // 3, iters - iters // 3):
            c.dev(dev.run, part)
        host.run(iters)
        c.check(same_end(dev, host) and np.array_equal(dev.model().ptS, host.model().ptS),
                "%d cells: %r / %r" % (ncells, dev.stats(), host.stats()))
        c.twin_stats(host.stats())
        c.read_guard(ctxs=[ca])
        for x in (dev, host, ca, cb):
            x.close()
    ca, cb = tt.TdContext.from_datastruct(ds), tt.TdContext.from_datastruct(ds)
    assert L.tdt_set_incremental(ca.h, 1) == 0 and L.tdt_set_incremental(cb.h, 0) == 0
    rng = np.random.default_rng(11)
    cur = tt.random_model(walk_cells, 11).cells()
    kept = [0, 0, 0, 0]
    c.dev(ca.evaluate, cur)
    for step in range(100):
        prop = ti.edit(rng, cur, tt.box())
        a, b = c.dev(ca.evaluate, prop), cb.evaluate(prop)
        c.check(a[1] == b[1] and np.array_equal(a[0], b[0]) and a[2] == b[2], "edit walk, step %d" % step)
        if rng.random() < 0.55:
            kept[edit_kind(cur, prop)] += 1
            cur = prop
    c.twin_stats({"accepted": kept})
    c.read_guard(ctxs=[ca])
    ca.close()
    cb.close()
    return c


# -------------------------------------------------- rounds: instances 0 and 2 with sa.rb, 6, 7, 13 ----
def ladder(name, lds_mode, device_swaps, calls):
    """Three replicas of 200 cells at max_cells 300 in a resident ladder (host-decided rounds, or the
    kernel's own exchange rounds) against a ladder of HOST-engine chains stepped round by round."""
    c, ctx = Case(name), ctx381()
    tmax, seed = 2.0, 77

    def chains(engine):
        return [chain(ctx, 200, 300, 30 + j, engine, lds_mode, chain_no=1 + j) for j in range(3)]

    hosts = chains(HOST)
    twin = tt.TemperingLadder(hosts, tmax=tmax, seed=seed, resident=False)
    for rounds, k in calls:
        for _ in range(rounds):
            twin.step(k)
    devs = chains(DEVICE)
    lad = tt.TemperingLadder(devs, tmax=tmax, seed=seed, device_swaps=device_swaps)
    assert lad.resident and lad.device_swaps == device_swaps and not twin.resident
    for rounds, k in calls:
        c.dev(lad.run, rounds, k)
    lad.close()
    c.check(lad.trace_digest() == twin.trace_digest() and list(lad.levels) == list(twin.levels) and
            list(lad.tried) == list(twin.tried) and list(lad.accepted) == list(twin.accepted),
            "the ladders' traces differ: levels %r / %r" % (list(lad.levels), list(twin.levels)))
    for j, (d, h) in enumerate(zip(devs, hosts)):
        c.check(same_end(d, h), "replica %d: %r / %r" % (j, d.stats(), h.stats()))
    c.swaps = int(np.sum(twin.accepted))
    c.read_guard(devs)
    for x in devs + hosts:
        x.close()
    return c


def ladder_rec_hbm():
    """Instance 13: tests/skew_tempering_worker.py's recorded ladder with its chains' lds_mode 1, both
    round protocols, against that test's twin built of HOST-engine chains."""
    c, ctx = Case("ladder_rec_hbm"), ctx381()
    prm = tt.define_TDstructrure().replace(max_cells=th.MAXC)
    hosts = [tt.Chain(ctx, tt.chain_params(prm, None, seed=th.BASE + j, chain=1 + j, engine=HOST),
                      tt.random_model(th.NCELLS, th.BASE + j)) for j in range(th.NREP)]
    rounds, twin = th.twin_run(tt, hosts, th.ROUNDS, th.K, th.TMAX, th.SEED)
    want = [(it, m) for r, j, it, m in rounds if r in th.sampled(th.ROUNDS, th.FIRST, th.EVERY)]
    c.swaps = int(np.sum(twin.accepted))
    for protocol in th.PROTOCOLS:
        devs = th.lds_chains(tt, ctx)
        for d in devs:
            assert L.tdt_chain_set_lds_mode(d.h, 1) == 0
        lad = th.ladder(tt, devs, protocol, th.TMAX, th.SEED)
        hist = tt.History(ctx, len(want), len(want) * th.MAXC)
        c.dev(lad.run, th.ROUNDS, th.K, history=hist, first=th.FIRST, every=th.EVERY)
        lad.close()
        try:
            assert len(hist) == len(want)
            th.assert_samples(hist, want)
        except AssertionError as e:
            c.check(False, "%s: the history differs: %s" % (protocol, str(e)[:300]))
        c.check(lad.trace_digest() == twin.trace_digest() and list(lad.levels) == list(twin.levels),
                "%s: the ladders' traces differ" % protocol)
        for j, (d, h) in enumerate(zip(devs, hosts)):
            c.check(same_end(d, h), "%s, replica %d: %r / %r" % (protocol, j, d.stats(), h.stats()))
        c.read_guard(devs)
        hist.close()
        th.close_all(devs)
    th.close_all(hosts)
    return c


RUN = {
    "hbm_free": hbm_free,
    "hbm_rb": lambda: ladder("hbm_rb", 1, False, [(12, 5)]),
    "rec_hbm": lambda: recorded("rec_hbm", 1),
    "packed_hbm": lambda: packed("packed_hbm", 3),
    "packed_tiles": lambda: packed("packed_tiles", 2),
    "rec_packed_hbm": lambda: recorded("rec_packed_hbm", 3),
    "rec_packed_tiles": lambda: recorded("rec_packed_tiles", 2),
    "dropin_lds": lambda: dropin("dropin_lds", DS, SMALL, 400),
    "dropin_hbm": lambda: dropin("dropin_hbm", tt.synthetic_rays(HBM_RAYS, seed=8), [(300, 400, 300, 5)], 300),
    "lds_rb": lambda: ladder("lds_rb", 0, False, [(12, 5)]),
    "xch_lds": lambda: ladder("xch_lds", 0, True, [(8, 5), (5, 3)]),
    "xch_hbm": lambda: ladder("xch_hbm", 1, True, [(8, 5), (5, 3)]),
    "ladder_rec_hbm": ladder_rec_hbm,
}

if __name__ == "__main__":
    for name in sys.argv[1:]:
        row = RUN[name]().row()
        print(json.dumps(row), flush=True)
        if not row["same"] or row["guard"]:
            sys.exit(1)
