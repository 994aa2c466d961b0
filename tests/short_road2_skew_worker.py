"""Child process of tests/test_gpu_short_road2.py: run with TD_LIB_PATH = the wave-skew build
(mcmc-in-tonga_amd/libtdstar_skew.so, chain_diag.h SKEW) and the names of the cases to run.  One case per
free-running k_chain_run instance -- every one of them reads an unknown point count at the loop top, and the
LDS-layout ones run the short road's death without phase B's barrier -- against the HOST engine, in the rows
of tests/skew_instances_worker.py (its Case, and its recorded and ladder runs under this file's names).  The
plain free-running cases run with the profile on, in launches of 1 + 64 + 65 proposals and then the rest, and
add to their row `barren_full` (changes and deaths that owned no point and took the full path) and `top`
(point counts read at the loop top); the other rows carry None there.  Stops at the first case that fails."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skew_instances_worker as siw  # noqa: E402  (asserts the skew build is the one loaded)
import test_gpu_tempering_history as th  # noqa: E402

tt, L, DEVICE, HOST = siw.tt, siw.L, siw.DEVICE, siw.HOST
# (cells, max_cells, iterations, seed): tests/skew_instances_worker.py's two small shapes
SHAPES = siw.SMALL
HBM_SHAPE = (300, 400, 300, 5)  # on siw.HBM_RAYS synthetic rays: the launcher takes the HBM layout by itself
FIRST = (1, 64, 65)


def parts(iters):
    return list(FIRST) + [iters - sum(FIRST)]


def counts(chain, before):
    out = (ctypes.c_int64 * 80)()
    assert L.tdt_chain_profile(chain.h, 0, out) == 0
    d = np.array(out[:], dtype=np.int64) - before
    return int(d[35] >> 32) + int(d[45] >> 32), sum(int(d[k] & 0xffffffff) + int(d[k] >> 32) for k in (7, 75))


def profile_on(chain):
    out = (ctypes.c_int64 * 80)()
    assert L.tdt_chain_profile(chain.h, 1, out) == 0
    return np.array(out[:], dtype=np.int64)


def free(name, ctx, shapes, lds_mode):
    """One chain per launch, each against its HOST twin."""
    c = siw.Case(name)
    c.barren_full = c.top = 0
    for ncells, max_cells, iters, seed in shapes:
        dev, host = (siw.chain(ctx, ncells, max_cells, seed, e, lds_mode) for e in (DEVICE, HOST))
        p0 = profile_on(dev)
        for part in parts(iters):
            c.dev(dev.run, part)
            c.check(L.tdt_chain_own_check(dev.h) == 0, "%d cells: the point counts are off" % ncells)
        host.run(iters)
        c.check(siw.same_end(dev, host) and np.array_equal(dev.model().ptS, host.model().ptS),
                "%d cells: %r / %r" % (ncells, dev.stats(), host.stats()))
        c.twin_stats(host.stats())
        b, t = counts(dev, p0)
        c.barren_full += b
        c.top += t
        c.read_guard([dev])
        dev.close()
        host.close()
    return c


def packed(name, lds_mode):
    """The two small shapes in one run_batch of the 4-wave kernel."""
    c, ctx = siw.Case(name), siw.ctx381()
    c.barren_full = c.top = 0
    iters = min(s[2] for s in SHAPES)
    devs = [siw.chain(ctx, n, m, s, DEVICE, lds_mode, chain_no=1 + j) for j, (n, m, _, s) in enumerate(SHAPES)]
    hosts = [siw.chain(ctx, n, m, s, HOST, chain_no=1 + j) for j, (n, m, _, s) in enumerate(SHAPES)]
    p0 = [profile_on(d) for d in devs]
    for part in parts(iters):
        c.dev(tt.run_batch, devs, part)
        c.check(all(L.tdt_chain_own_check(d.h) == 0 for d in devs), "the point counts are off")
    for d, h, q in zip(devs, hosts, p0):
        h.run(iters)
        c.check(siw.same_end(d, h) and np.array_equal(d.model().ptS, h.model().ptS), "%r / %r" % (d.stats(), h.stats()))
        c.twin_stats(h.stats())
        b, t = counts(d, q)
        c.barren_full += b
        c.top += t
    c.read_guard(devs)
    for x in devs + hosts:
        x.close()
    return c


def ladder_rec(name, lds_mode):
    """tests/skew_tempering_worker.py's recorded ladder (lds_mode 0: instance 12; 1: instance 13), both round
    protocols, against that test's twin built of HOST-engine chains."""
    c, ctx = siw.Case(name), siw.ctx381()
    prm = tt.define_TDstructrure().replace(max_cells=th.MAXC)
    hosts = [tt.Chain(ctx, tt.chain_params(prm, None, seed=th.BASE + j, chain=1 + j, engine=HOST),
                      tt.random_model(th.NCELLS, th.BASE + j)) for j in range(th.NREP)]
    rounds, twin = th.twin_run(tt, hosts, th.ROUNDS, th.K, th.TMAX, th.SEED)
    want = [(it, m) for r, j, it, m in rounds if r in th.sampled(th.ROUNDS, th.FIRST, th.EVERY)]
    c.swaps = int(np.sum(twin.accepted))
    for protocol in th.PROTOCOLS:
        devs = th.lds_chains(tt, ctx)
        for d in devs:
            if lds_mode:
                assert L.tdt_chain_set_lds_mode(d.h, lds_mode) == 0
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
            c.check(siw.same_end(d, h), "%s, replica %d: %r / %r" % (protocol, j, d.stats(), h.stats()))
        c.read_guard(devs)
        hist.close()
        th.close_all(devs)
    th.close_all(hosts)
    return c


def hbm_rays(name):
    ds = tt.synthetic_rays(siw.HBM_RAYS, seed=8)
    ctx = tt.TdContext.from_datastruct(ds)
    c = free(name, ctx, [HBM_SHAPE], 0)
    ctx.close()
    return c


RUN = {
    "road_lds": lambda: free("road_lds", siw.ctx381(), SHAPES, 0),
    "road_hbm": lambda: free("road_hbm", siw.ctx381(), SHAPES, 1),
    "road_hbm_rays": lambda: hbm_rays("road_hbm_rays"),
    "road_packed_hbm": lambda: packed("road_packed_hbm", 3),
    "road_packed_tiles": lambda: packed("road_packed_tiles", 2),
    "road_rec_lds": lambda: siw.recorded("road_rec_lds", 0),
    "road_rec_hbm": lambda: siw.recorded("road_rec_hbm", 1),
    "road_rec_packed_hbm": lambda: siw.recorded("road_rec_packed_hbm", 3),
    "road_rec_packed_tiles": lambda: siw.recorded("road_rec_packed_tiles", 2),
    "road_xch_lds": lambda: siw.ladder("road_xch_lds", 0, True, [(8, 5), (5, 3)]),
    "road_xch_hbm": lambda: siw.ladder("road_xch_hbm", 1, True, [(8, 5), (5, 3)]),
    "road_ladder_rec_lds": lambda: ladder_rec("road_ladder_rec_lds", 0),
    "road_ladder_rec_hbm": lambda: ladder_rec("road_ladder_rec_hbm", 1),
}

if __name__ == "__main__":
    for name in sys.argv[1:]:
        c = RUN[name]()
        row = c.row()
        row["barren_full"], row["top"] = getattr(c, "barren_full", None), getattr(c, "top", None)
        print(json.dumps(row), flush=True)
        if not row["same"] or row["guard"] or row["barren_full"]:
            sys.exit(1)
