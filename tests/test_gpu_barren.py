"""The chain kernel's short road: a change or death whose cell owns no ray point skips the
tile pass and phases C-E.  What makes that right is the per-slot point count own[] (csrc/chain_dev.h) and the
rule for trusting the count a guessed proposal read; both are held here to the HOST engine, which runs a full
td_evaluate per proposal and has none of it:

  * parity with == on cells, ptS, phi and counters over 3000 proposals -- the bench's 5000-cell model at
    max_cells 10000 (nearly every change and death barren), 200 cells at max_cells 300, and a hand-placed
    10-cell model (min_cells 5, max_cells 14) that provokes the stale-count hazard: an accepted move hands
    points to a cell that owned none, and the next proposal selects that cell;
  * lds_mode 0, 1, 2 and 3, a recorded run and a host-decided ladder (tests/skew_instances_worker.py's shapes);
  * own[s] == #{q : best_s[q] == s} after every run and at a launch boundary in the middle
    (tdt_chain_own_check);
  * the road is taken (its counters, tdt_chain_profile), and the stale count is met and cleared;
  * the hazard and the 200-cell model again in the wave-skew build, in a child process.

The hazard is counted from the restatement of the reference's loop alone (oracle/chain_ref.py): iterations k
whose accepted death or move raises the point count of some OTHER cell from 0, followed by a change or death
of that cell at k + 1."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKEW = os.path.join(ROOT, "mcmc-in-tonga_amd", "libtdstar_skew.so")
ITERS = 3000
# (name: cells or None for the hand-placed model, min_cells, max_cells, seed, temperature)
# The hazard needs an accepted death or move to be followed at once by a change or death of one particular
# cell of 5-14: a few per cent of those iterations.  At T = 1 a 10-cell model accepts some 150 moves and 60
# deaths in 3000 proposals, few of which uncover a barren cell, and the reference's run holds the hazard 0 or
# 1 times at any seed tried; the chain's temperature (the build's one extension of the reference's decision,
# oracle/chain_ref.py) is therefore 1e6 for this shape -- nearly every move is accepted, so ownership changes
# hands all the time (1 to 9 such iterations at most seeds) -- and the seed is the first of 1, 2, ..., 550 at
# which the run holds it HAZARD_MIN times (11).
SHAPES = {"bench": (5000, 5, 10000, 3, 1.0), "m200": (200, 5, 300, 1, 1.0), "hazard": (None, 5, 14, 550, 1e6)}
HAZARD_MIN = 10  # stale-count events the hazard model's reference run must hold


def hazard_model(tt, ds):
    """Ten cells: three among the rays (at ray points a third of the way along three rays spread over the
    set) and seven crowded into the box's corner farthest from the rays' centre -- none of those owns a
    point while a near cell stands, and each is the next owner once the near cells move away."""
    X, Y, Z = (np.asarray(a, dtype=np.float64) for a in (ds.rayX, ds.rayY, ds.rayZ))
    n = X.shape[1]
    near = []
    for r in (n // 6, n // 2, (5 * n) // 6):
        k = int(np.count_nonzero(~np.isnan(X[:, r]))) // 3
        near.append((X[k, r], Y[k, r], Z[k, r]))
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    m = ~np.isnan(X)
    cx, cy, cz = X[m].mean(), Y[m].mean(), Z[m].mean()
    corner = (xmin if cx - xmin > xmax - cx else xmax, ymin if cy - ymin > ymax - cy else ymax,
              zmin if cz - zmin > zmax - cz else zmax)
    far = []
    for j in range(7):  # a fixed lattice, 2 % of the box apart, inside the corner
        f = 0.02 * np.array([1 + j % 2, 1 + (j // 2) % 2, 1 + j // 4])
        far.append(tuple(c + (lo + hi - 2 * c) * t for c, lo, hi, t in
                         zip(corner, (xmin, ymin, zmin), (xmax, ymax, zmax), f)))
    pts = np.array(near + far)
    zeta = np.linspace(5.0, 45.0, len(pts))
    m0 = tt.random_model(len(pts), 1)
    m0.xCell[:], m0.yCell[:], m0.zCell[:], m0.zeta[:] = pts[:, 0], pts[:, 1], pts[:, 2], zeta
    return m0


def start_model(tt, ds, name):
    cells = SHAPES[name][0]
    return hazard_model(tt, ds) if cells is None else tt.random_model(cells, SHAPES[name][3])


def td_prm(tt, name):
    return tt.define_TDstructrure().replace(min_cells=SHAPES[name][1], max_cells=SHAPES[name][2])


def make(tt, ds, ctx, name, engine, lds_mode=0, chain_no=1):
    p = tt.chain_params(td_prm(tt, name), None, seed=SHAPES[name][3], chain=chain_no, engine=engine,
                        temperature=SHAPES[name][4])
    c = tt.Chain(ctx, p, start_model(tt, ds, name))
    if engine == tt.TD_ENGINE_DEVICE and lds_mode:
        assert tt.lib().tdt_chain_set_lds_mode(c.h, lds_mode) == 0
    return c


def end_state(c):
    st, m = c.stats(), c.model()
    return ({k: st[k] for k in ("phi", "accepted", "proposed", "ncells", "iterations")},
            [np.array(getattr(m, f)) for f in ("xCell", "yCell", "zCell", "zeta", "ptS")])


def same_state(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def own_check(tt, c):
    return tt.lib().tdt_chain_own_check(c.h)


def stale_count_events(orc, ds, start_cells, steps, draws, min_cells):
    """From the reference's run alone: iterations k that are an accepted death or move after which some cell
    other than the moved one owns points and owned none before, with k + 1 a change or an entered death of
    that cell."""
    def counts(cells):
        near = orc.evaluate(ds.rayX, ds.rayY, ds.rayZ, ds.rayL, ds.rayU, ds.tS, ds.allSig, cells)["nearest"]
        return np.bincount(near[near >= 0], minlength=len(cells[0]))

    events = 0
    prev = start_cells
    for k, s in enumerate(steps[:-1]):
        before, prev = prev, s.cells
        if not (s.accept == 1 and s.action in (2, 4)):
            continue
        nb = len(before[0])
        sel = int(math.floor(draws(s.iter)[6] * nb))  # the killed / moved position (TD_inversion_function.jl:128, :222)
        cb, ca = counts(before), counts(s.cells)
        if s.action == 2:
            cb = np.delete(cb, sel)  # the survivors keep their order
            raised = set(np.nonzero((cb == 0) & (ca > 0))[0])
        else:
            raised = set(np.nonzero((cb == 0) & (ca > 0))[0]) - {sel}
        nxt = steps[k + 1]
        na = len(s.cells[0])
        if nxt.action == 3 or (nxt.action == 2 and na > min_cells):
            events += int(math.floor(draws(nxt.iter)[6] * na)) in raised
    return events


_HOST_END = {}


def host_end(tt, ds, name):
    """The HOST engine's state after ITERS proposals of a shape (computed once, shared: read-only)."""
    if name not in _HOST_END:
        h = make(tt, ds, tt.context_for(ds), name, tt.TD_ENGINE_HOST)
        h.run(ITERS)
        _HOST_END[name] = end_state(h)
        h.close()
    return _HOST_END[name]


def profile(tt, c, enable):
    out = (ctypes.c_int64 * 80)()
    assert tt.lib().tdt_chain_profile(c.h, enable, out) == 0
    return np.array(out[:], dtype=np.int64)


def test_hazard_model_holds_the_stale_count_hazard(tt, orc, ds):
    """The reference alone: the hand-placed model's run meets the hazard at least HAZARD_MIN times."""
    name = "hazard"
    p = tt.chain_params(td_prm(tt, name), None, seed=SHAPES[name][3], chain=1, engine=tt.TD_ENGINE_HOST,
                        temperature=SHAPES[name][4])
    m = start_model(tt, ds, name)
    ref = cc.restate(tt, ds, p, m, ITERS)
    n = stale_count_events(orc, ds, m.cells(), ref["steps"], cc.draws_of(tt, p.seed, p.chain), SHAPES[name][1])
    print("stale-count events:", n, "accepted:", ref["accepted"])
    assert n >= HAZARD_MIN


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("lds_mode", [0, 1])
def test_one_chain_follows_host(tt, ds, name, lds_mode):
    """Instances 0 and 2 (the LDS and the HBM layout), two launches with the invariant checked at the boundary;
    the road's counters on the LDS layout."""
    ctx = tt.context_for(ds)
    dev = make(tt, ds, ctx, name, tt.TD_ENGINE_DEVICE, lds_mode)
    assert own_check(tt, dev) == 0
    p0 = profile(tt, dev, 1)
    dev.run(ITERS // 2)
    assert own_check(tt, dev) == 0
    dev.run(ITERS - ITERS // 2)
    assert own_check(tt, dev) == 0
    prof = profile(tt, dev, 0) - p0
    got = end_state(dev)
    dev.close()
    assert same_state(got, host_end(tt, ds, name)), (got[0], host_end(tt, ds, name)[0])
    print(name, lds_mode, "short road deaths/changes:", prof[35], prof[45], "adopted barren:", prof[55],
          "cleared:", prof[25])
    if name == "bench":
        assert prof[35] > 0 and prof[45] > 0
        assert prof[35] + prof[45] >= ITERS // 10
    if name == "hazard":
        assert prof[25] > 0


@pytest.mark.parametrize("lds_mode", [2, 3])
def test_packed_batch_follows_host(tt, ds, lds_mode):
    """Instances 5 and 4 (the 4-wave kernel, tiles in LDS / all in HBM): the three shapes in one run_batch."""
    ctx = tt.context_for(ds)
    devs = [make(tt, ds, ctx, name, tt.TD_ENGINE_DEVICE, lds_mode) for name in SHAPES]
    for part in (ITERS // 2, ITERS - ITERS // 2):
        tt.run_batch(devs, part)
        assert [own_check(tt, d) for d in devs] == [0] * len(devs)
    got = [end_state(d) for d in devs]
    for d in devs:
        d.close()
    for name, g in zip(SHAPES, got):
        assert same_state(g, host_end(tt, ds, name)), (name, g[0], host_end(tt, ds, name)[0])


@pytest.mark.parametrize("name", ["m200", "hazard"])
def test_recorded_run_follows_host(tt, ds, name):
    """Instance 8 (a recorded launch): every third model of two launches, history and end state."""
    ctx = tt.context_for(ds)
    every, maxc = 3, SHAPES[name][2]
    dev, host = (make(tt, ds, ctx, name, e) for e in (tt.TD_ENGINE_DEVICE, tt.TD_ENGINE_HOST))
    ns = ITERS // every + 1
    hd, hh = tt.History(ctx, ns, ns * maxc), tt.History(ctx, ns, ns * maxc)
    for k in range(2):
        first = every - (k * (ITERS // 2)) % every
        dev.run_recorded(ITERS // 2, first, every, hd)
        host.run_recorded(ITERS // 2, first, every, hh)
        assert own_check(tt, dev) == 0
    a, b = hd.read_arrays(), hh.read_arrays()
    assert len(hd) == len(hh) > 0 and all(np.array_equal(a[k], b[k]) for k in a)
    assert same_state(end_state(dev), end_state(host))
    assert same_state(end_state(dev), host_end(tt, ds, name))
    for x in (hd, hh, dev, host):
        x.close()


def test_host_decided_ladder_follows_host(tt, ds):
    """Instance 0 with resident host-decided rounds: three replicas of the 200-cell shape, 100 rounds of 10."""
    ctx = tt.context_for(ds)
    tmax, seed, calls = 2.0, 77, [(100, 10)]

    def chains(engine):
        out = []
        for j in range(3):
            p = tt.chain_params(td_prm(tt, "m200"), None, seed=30 + j, chain=1 + j, engine=engine)
            out.append(tt.Chain(ctx, p, tt.random_model(200, 30 + j)))
        return out

    hosts = chains(tt.TD_ENGINE_HOST)
    twin = tt.TemperingLadder(hosts, tmax=tmax, seed=seed, resident=False)
    for rounds, k in calls:
        for _ in range(rounds):
            twin.step(k)
    devs = chains(tt.TD_ENGINE_DEVICE)
    lad = tt.TemperingLadder(devs, tmax=tmax, seed=seed, device_swaps=False)
    assert lad.resident
    for rounds, k in calls:
        lad.run(rounds, k)
    lad.close()
    assert lad.trace_digest() == twin.trace_digest() and list(lad.levels) == list(twin.levels)
    for d, h in zip(devs, hosts):
        assert own_check(tt, d) == 0
        assert same_state(end_state(d), end_state(h))
    for x in devs + hosts:
        x.close()


@pytest.mark.timeout(240)
def test_short_road_under_wave_skew():
    """The hazard and the 200-cell shape in the wave-skew build against HOST (a child process, as
    tests/test_gpu_skew.py); no spin wait gives up."""
    assert os.path.exists(SKEW), "the skew build is made by __graft_entry__.build() (make all)"
    env = dict(os.environ, TD_LIB_PATH=SKEW)
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "barren_skew_worker.py")], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=220, cwd=ROOT)
    text = p.stdout.decode(errors="replace")
    rows = [json.loads(x) for x in text.splitlines() if x.startswith("{")]
    assert p.returncode == 0 and len(rows) == 4, text[-3000:]
    assert all(r["same"] and r["guard"] == 0 and r["own"] == 0 for r in rows), rows
    assert all(r["short"] > 0 for r in rows), rows
