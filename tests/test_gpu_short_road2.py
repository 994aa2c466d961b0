"""The chain kernel's short road, second part: a change or death whose barren flag is not up --
a launch's first proposal, every 64th, every proposal wave 0 makes again at an iteration's end -- reads the
cell's point count (DevChain::own) at the loop top and takes the short road when it is 0, so no change or
death of a cell that owns no ray point walks the tiles any more.  Held to the HOST engine (a full td_evaluate
per proposal, none of this) with == on cells, ptS, phi and counters:

  * 8 cells at max_cells 12 (inactive proposals, proposals made again every few steps) and 200 cells at
    max_cells 300, launches of 1, 63, 64, 65 and 130 proposals (across the every-64th ones), and the 130 as
    launches of 1 + 64 + 65, whose stats -- bytes too -- are the one launch's;
  * 300 cells on 500 synthetic rays (the HBM layout) and a run_batch of both small shapes in each of the two
    4-wave instances, the instance taken checked (tdt_chain_launch_counts);
  * with tdt_chain_profile on: no change or death that owned no point took the full path; the short road's
    proposals and those whose count was read at the loop top and found above 0 are all the evaluated changes
    and deaths of the restatement of the reference's loop (oracle/chain_ref.py) over the same draws;
    tdt_chain_own_check after every launch;
  * the same shapes in the wave-skew build, every free-running instance (tests/short_road2_skew_worker.py),
    judged by tests/test_gpu_skew_instances.py's judge()."""
import ctypes
import json
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest

import chain_cases as cc
import test_gpu_skew_instances as tsi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "short_road2_skew_worker.py")
# name: (cells, max_cells, seed, synthetic rays or 0 for the 381 shipped ones)
SHAPES = {"m8": (8, 12, 4, 0), "m200": (200, 300, 1, 0), "hbm300": (300, 400, 5, 500)}
LENGTHS = (1, 63, 64, 65, 130)
SPLIT = (1, 64, 65)
# the launcher's table (csrc/chain_kernels.hip kChainInstances): free-running LDS layout, HBM layout, and the
# 4-wave kernel all in HBM (lds_mode 3) / with the tiles in LDS (lds_mode 2)
INST_LDS, INST_HBM, INST_PACKED = 0, 2, {3: 4, 2: 5}


def rays(tt, ds, name):
    n = SHAPES[name][3]
    return tt.synthetic_rays(n, seed=8) if n else ds


def make(tt, ds, ctx, name, engine, lds_mode=0):
    cells, max_cells, seed, _ = SHAPES[name]
    prm = tt.define_TDstructrure().replace(max_cells=max_cells)
    c = tt.Chain(ctx, tt.chain_params(prm, None, seed=seed, chain=1, engine=engine), tt.random_model(cells, seed))
    if engine == tt.TD_ENGINE_DEVICE and lds_mode:
        assert tt.lib().tdt_chain_set_lds_mode(c.h, lds_mode) == 0
    return c


def end_state(c):
    st, m = c.stats(), c.model()
    return ({k: st[k] for k in ("phi", "accepted", "proposed", "ncells", "iterations")},
            [np.array(getattr(m, f)) for f in ("xCell", "yCell", "zCell", "zeta", "ptS")])


def same_state(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


_HOST, _REF, _CTX = {}, {}, {}


def context(tt, ds, name):
    """One context per ray set (shared)."""
    key = SHAPES[name][3]
    if key not in _CTX:
        r = rays(tt, ds, name)
        _CTX[key] = (r, tt.context_for(r) if key == 0 else tt.TdContext.from_datastruct(r))
    return _CTX[key]


def host_states(tt, ds, name):
    """The HOST engine's state after each of LENGTHS proposals of a shape (one run, computed once; read-only)."""
    if name not in _HOST:
        _, ctx = context(tt, ds, name)
        h = make(tt, ds, ctx, name, tt.TD_ENGINE_HOST)
        out, done = {}, 0
        for n in LENGTHS:
            h.run(n - done)
            done = n
            out[n] = end_state(h)
        h.close()
        _HOST[name] = out
    return _HOST[name]


def evaluated_changes_and_deaths(tt, ds, name, n):
    """From the restatement of the reference's loop alone: the changes and deaths among the first n proposals
    that were entered and valid -- the ones the kernel takes down one road or the other."""
    from oracle import chain_ref

    if name not in _REF:
        r, _ = context(tt, ds, name)
        cells, max_cells, seed, _ = SHAPES[name]
        prm = tt.define_TDstructrure().replace(max_cells=max_cells)
        p = tt.chain_params(prm, None, seed=seed, chain=1, engine=tt.TD_ENGINE_HOST)
        _REF[name] = cc.restate(tt, r, p, tt.random_model(cells, seed), max(LENGTHS))["steps"]
    return sum(1 for s in _REF[name][:n] if s.action in (2, 3) and s.outcome == chain_ref.EVALUATED)


def profile(tt, c, enable):
    out = (ctypes.c_int64 * 80)()
    assert tt.lib().tdt_chain_profile(c.h, enable, out) == 0
    return np.array(out[:], dtype=np.int64)


def launches(tt):
    out, n = (ctypes.c_int64 * 32)(), ctypes.c_int(0)
    assert tt.lib().tdt_chain_launch_counts(out, ctypes.byref(n)) == 0
    return np.array(out[:n.value], dtype=np.int64)


def roads(prof):
    """The slots' counts, two to a slot (csrc/chain_dev.h): proposals on the short road, on the full path though the
    cell owned no point, and counts read at the loop top that were 0 / above 0 -- deaths and changes together."""
    lo, hi = (lambda k: int(prof[k]) & 0xffffffff), (lambda k: int(prof[k]) >> 32)
    return dict(short=lo(35) + lo(45), barren_full=hi(35) + hi(45), top_none=lo(7) + lo(75), top_some=hi(7) + hi(75))


def run_checked(tt, ds, name, parts, lds_mode=0, instance=INST_LDS):
    """A DEVICE chain of the shape through launches of `parts` proposals, the profile on: the invariant after
    every launch, the instance taken, the roads' counts -> (end state, stats, counts)."""
    _, ctx = context(tt, ds, name)
    dev = make(tt, ds, ctx, name, tt.TD_ENGINE_DEVICE, lds_mode)
    assert tt.lib().tdt_chain_own_check(dev.h) == 0
    p0, l0 = profile(tt, dev, 1), launches(tt)
    for n in parts:
        dev.run(n)
        assert tt.lib().tdt_chain_own_check(dev.h) == 0
    took = launches(tt) - l0
    r = roads(profile(tt, dev, 0) - p0)
    got, st = end_state(dev), dev.stats()
    dev.close()
    assert took[instance] == len(parts) and took.sum() == len(parts), took
    print(name, parts, "lds_mode", lds_mode, r)
    assert r["barren_full"] == 0
    assert r["top_none"] <= r["short"]
    assert r["short"] + r["top_some"] == evaluated_changes_and_deaths(tt, ds, name, sum(parts))
    return got, st, r


@pytest.mark.parametrize("name", ["m8", "m200"])
@pytest.mark.parametrize("length", LENGTHS)
def test_one_launch_follows_host(tt, ds, name, length):
    got, _, r = run_checked(tt, ds, name, [length])
    want = host_states(tt, ds, name)[length]
    assert same_state(got, want), (got[0], want[0])
    if length == 130:  # (the road is met, and so is a count read at the loop top)
        assert r["short"] + r["top_some"] > 0 and r["top_none"] + r["top_some"] > 0


@pytest.mark.parametrize("name", ["m8", "m200"])
def test_split_launches_equal_one_launch(tt, ds, name):
    """1 + 64 + 65 proposals: every launch's first proposal asks at the loop top; the stats, bytes among them,
    are those of the 130 in one launch."""
    one, st_one, _ = run_checked(tt, ds, name, [sum(SPLIT)])
    got, st, _ = run_checked(tt, ds, name, list(SPLIT))
    assert same_state(got, host_states(tt, ds, name)[sum(SPLIT)]) and same_state(got, one)
    assert st == st_one, (st, st_one)


def test_hbm_layout_follows_host(tt, ds):
    """300 cells on 500 synthetic rays: the per-ray arrays do not fit in LDS (instance 2, chosen by the launcher)."""
    name = "hbm300"
    one, st_one, _ = run_checked(tt, ds, name, [sum(SPLIT)], instance=INST_HBM)
    got, st, _ = run_checked(tt, ds, name, list(SPLIT), instance=INST_HBM)
    want = host_states(tt, ds, name)[sum(SPLIT)]
    assert same_state(one, want) and same_state(got, want), (one[0], got[0], want[0])
    assert st == st_one, (st, st_one)


@pytest.mark.parametrize("lds_mode", [2, 3])
def test_four_wave_batch_follows_host(tt, ds, lds_mode):
    """Both small shapes in one run_batch (two chains per CU: instance 5 with the tiles in LDS, 4 all in HBM)."""
    names = ["m8", "m200"]
    _, ctx = context(tt, ds, names[0])
    devs = [make(tt, ds, ctx, n, tt.TD_ENGINE_DEVICE, lds_mode) for n in names]
    p0, l0 = [profile(tt, d, 1) for d in devs], launches(tt)
    for part in SPLIT:
        tt.run_batch(devs, part)
        assert [tt.lib().tdt_chain_own_check(d.h) for d in devs] == [0] * len(devs)
    took = launches(tt) - l0
    assert took[INST_PACKED[lds_mode]] == len(SPLIT) and took.sum() == len(SPLIT), took
    for n, d, q in zip(names, devs, p0):
        r = roads(profile(tt, d, 0) - q)
        got = end_state(d)
        d.close()
        print(n, "lds_mode", lds_mode, r)
        assert same_state(got, host_states(tt, ds, n)[sum(SPLIT)]), (n, got[0])
        assert r["barren_full"] == 0
        assert r["short"] + r["top_some"] == evaluated_changes_and_deaths(tt, ds, n, sum(SPLIT))


# the skew worker's cases for tests/test_gpu_skew_instances.py's judge(): the instance each must launch, and that
# its reference accepts a proposal of every action
SKEW_CASES = {
    "road_lds": (0, "road", {"accepted": 1}),
    "road_hbm": (2, "road", {"accepted": 1}),
    "road_hbm_rays": (2, "road", {"accepted": 1}),
    "road_packed_hbm": (4, "road", {"accepted": 1}),
    "road_packed_tiles": (5, "road", {"accepted": 1}),
    "road_rec_lds": (8, "road", {"accepted": 1}),
    "road_rec_hbm": (9, "road", {"accepted": 1}),
    "road_rec_packed_hbm": (10, "road", {"accepted": 1}),
    "road_rec_packed_tiles": (11, "road", {"accepted": 1}),
    "road_xch_lds": (6, "road", {"swaps": 1}),
    "road_xch_hbm": (7, "road", {"swaps": 1}),
    "road_ladder_rec_lds": (12, "road", {"swaps": 1}),
    "road_ladder_rec_hbm": (13, "road", {"swaps": 1}),
}


@pytest.mark.timeout(60)
def test_every_free_running_instance_under_wave_skew():
    """The shapes above in the wave-skew build, one case per free-running instance (all twelve read the count at
    the loop top), in a child process; each launched its instance, equals the HOST engine's run and tripped no
    spin guard -- judge() of tests/test_gpu_skew_instances.py over this file's cases."""
    assert os.path.exists(tsi.SKEW), "the skew build is made by __graft_entry__.build() (make all)"
    env = dict(os.environ, TD_LIB_PATH=tsi.SKEW)
    p = subprocess.run([sys.executable, "-u", WORKER] + list(SKEW_CASES), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=50, cwd=ROOT)
    text = p.stdout.decode(errors="replace")
    rows = [json.loads(x) for x in text.splitlines() if x.startswith("{")]
    assert p.returncode == 0, text[-3000:]
    with mock.patch.dict(tsi.CASES, SKEW_CASES):
        assert tsi.judge(rows, list(SKEW_CASES)) == [], text[-3000:]
    counted = [r for r in rows if r["barren_full"] is not None]  # (the plain free-running cases: the profile on)
    assert len(counted) == 5 and all(r["barren_full"] == 0 and r["top"] > 0 for r in counted), rows
