"""Every chain engine against a restatement of the reference's loop (oracle/chain_ref.py,
TD_inversion_function.jl:69-288), decision for decision.

The other chain tests tie the DEVICE engine, the drop-in path, the ladders and the histories to the HOST
engine bit for bit -- and the HOST engine (csrc/chain.cpp host_iteration) to nothing once the data are in
play: both were written from one reading of the Julia.  Here the HOST engine, the DEVICE engine in its
automatic layout and with lds_mode 1, and (case A prior 1) the drop-in path each record EVERY iteration of
the cases of tests/chain_cases.py (run_recorded(iters, 1, 1, History(with_ptS=True))), and every sample must
equal the restatement's model after that iteration with ==: action, accept, iter, nCells, phi, ptS and the four
cell arrays; at the end the per-action accepted and proposed counts.  tests/test_chain_reference.py shows
(without a GPU) that the restatement's runs visit every branch and contain no near tie.  What stays the
build's own definition: the RNG stream (tdt_draws, Philox KATs), the inverse-CDF normals (tdt_normal_quantile,
scipy at 1e-14), the log-domain form of the decision, and T.

tdt_chain_launch_counts says which k_chain_run instance each run took; every test asserts the ones it meant.

Each test was timed once on an MI355X (its whole call, written in its docstring); its pytest.mark.timeout is about
four times that plus a process's start -- a cold first launch, a busy shared machine."""
import contextlib
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "chain_draws_worker.py")
NINST = 14


def launches(tt):
    out, n = (ctypes.c_int64 * 32)(), ctypes.c_int(0)
    assert tt.lib().tdt_chain_launch_counts(out, ctypes.byref(n)) == 0 and n.value == NINST
    return np.array([out[i] for i in range(NINST)], dtype=np.int64)


def draws_launches(tt):
    d = ctypes.c_int64(-1)
    assert tt.lib().tdt_chain_draws_launches(ctypes.byref(d)) == 0
    return d.value


def took(instance=None, count=1):
    v = np.zeros(NINST, dtype=np.int64)
    if instance is not None:
        v[instance] = count
    return v


@pytest.fixture(scope="module")
def contexts(tt):
    made = {}

    def get(rname):
        if rname not in made:
            made[rname] = tt.TdContext.from_datastruct(cc.rays(tt, rname))
        return made[rname]

    yield get
    for c in made.values():
        c.close()


def engines(tt):
    """(label, engine, lds_mode, the instance a recorded launch takes, a plain launch takes)"""
    return [("HOST", tt.TD_ENGINE_HOST, 0, None, None), ("DEVICE", tt.TD_ENGINE_DEVICE, 0, 8, 0),
            ("DEVICE lds_mode 1", tt.TD_ENGINE_DEVICE, 1, 9, 2)]


@contextlib.contextmanager
def make_chain(tt, ctx, name, engine, lds_mode=0, start_iter=0):
    """The case's chain, closed on the way out whatever happens: td_chain_destroy reads its context, so a chain
    that a failed assertion's traceback keeps alive must not outlive the context the fixture then closes."""
    _, ncells, _, _, _, prior, _, seed = cc.CASES[name]
    c = tt.Chain(ctx, cc.chain_params(tt, name, engine, start_iter), cc.start_model(tt, ncells, prior, seed))
    try:
        if lds_mode:
            assert tt.lib().tdt_chain_set_lds_mode(c.h, lds_mode) == 0
        yield c
    finally:
        c.close()


def record(tt, ctx, c, name, pieces):
    """run_recorded every iteration of each piece into one history -> (read_arrays(), the launches it took)"""
    total = sum(pieces)
    h = tt.History(ctx, total, total * cc.CASES[name][3], with_ptS=True)
    try:
        before = launches(tt)
        for k in pieces:
            c.run_recorded(k, 1, 1, h)
        used = launches(tt) - before
        return h.read_arrays(), used
    finally:
        h.close()


def check_end(c, steps, label, iterations=None):
    m = c.model()
    bad = cc.end_diff(c.stats(), m.cells(), m.phi, m.ptS, steps, iterations)
    assert bad is None, (label, bad)


def follow(tt, ctx, name, label, engine, lds_mode, instance, steps, start_iter=0, pieces=None):
    with make_chain(tt, ctx, name, engine, lds_mode, start_iter) as c:
        m0 = c.model()
        a, used = record(tt, ctx, c, name, pieces or [len(steps)])
        bad = cc.history_diff(a, steps)
        assert bad is None, (name, label, bad)
        check_end(c, steps, (name, label))
        assert np.array_equal(used, took(instance, len(pieces or [0]))), (name, label, used)
    return m0


@pytest.mark.timeout(5)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_engines_follow_the_restatement(tt, orc, contexts, name):
    """HOST, DEVICE (instance 8) and DEVICE with lds_mode 1 (instance 9), every iteration of the case.  The
    starting model's phi and ptS are the restatement's too (build_starting's evaluate, MCsub.jl:118).
    Measured: 0.40-0.71 s per case (C-p1 and the module's first case the longest)."""
    ref = cc.reference(tt, name)
    ctx = contexts(cc.CASES[name][0])
    for label, engine, lds_mode, rec_inst, _ in engines(tt):
        m0 = follow(tt, ctx, name, label, engine, lds_mode, rec_inst, ref["steps"])
        assert m0.phi == ref["start"][0] and np.array_equal(m0.ptS, ref["start"][1]), (name, label)


@pytest.mark.timeout(4)
def test_dropin_follows_the_restatement(tt, orc):
    """Case A prior 1 through the drop-in path: the host loop calling td_evaluate, which follows the chain with
    its resident server (instance 1) on a context of its own.  Measured: 0.40 s."""
    name = "A-p1-T1"
    ref = cc.reference(tt, name)
    ctx = tt.TdContext.from_datastruct(cc.rays(tt, cc.CASES[name][0]))
    try:
        with make_chain(tt, ctx, name, tt.TD_ENGINE_DROPIN) as c:
            a, used = record(tt, ctx, c, name, [len(ref["steps"])])
            bad = cc.history_diff(a, ref["steps"])
            assert bad is None, bad
            check_end(c, ref["steps"], "DROPIN")
            assert used[1] >= 1 and used.sum() == used[1], used  # (the server is started again after an idle time-out)
    finally:
        ctx.close()


@pytest.mark.timeout(3)
def test_unrecorded_pieces_follow_the_restatement(tt, orc, contexts):
    """Case A prior 1 as run() pieces of 1, 63, 64, 65 and the rest -- lengths around the 64-draw refill of the
    plain instances (0, and 2 with lds_mode 1) -- model and stats after each piece.  Every plain DEVICE launch
    here loads its draws from k_draws' table: tdt_chain_draws_launches counts one per launch (the child of
    test_in_kernel_draws_follow_the_restatement must count none).  Measured: 0.15 s."""
    name = "A-p1-T1"
    steps = cc.reference(tt, name)["steps"]
    ctx = contexts(cc.CASES[name][0])
    pieces = [1, 63, 64, 65]
    pieces.append(len(steps) - sum(pieces))
    for label, engine, lds_mode, _, plain_inst in engines(tt):
        with make_chain(tt, ctx, name, engine, lds_mode) as c:
            before, dbefore = launches(tt), draws_launches(tt)
            done = 0
            for k in pieces:
                c.run(k)
                done += k
                check_end(c, steps[:done], (label, done))
            assert np.array_equal(launches(tt) - before, took(plain_inst, len(pieces))), label
            assert draws_launches(tt) - dbefore == (len(pieces) if plain_inst is not None else 0), label


@pytest.mark.timeout(3)
def test_iterations_above_2_32_follow_the_restatement(tt, orc, contexts):
    """Case A prior 1 started at iteration 2^32 - 100 (td_chain_params.start_iter) for 200 iterations: the Philox
    counter's high word, k_draws' d.st->iter + i, the kernel's iter0 + it + 1 + lane and the history's iter
    header carry values above 2^32.  Every sample's iter is the absolute index; the run split 100 + 100 across
    the boundary is the same run.  Measured: 0.11 s."""
    name = "A-p1-T1"
    steps = cc.reference(tt, name, cc.HIGH_ITERS, cc.HIGH_START)["steps"]
    assert steps[0].iter == 2 ** 32 - 100 and steps[-1].iter == 2 ** 32 + 99
    ctx = contexts(cc.CASES[name][0])
    for label, engine, lds_mode, rec_inst, _ in engines(tt):
        for pieces in ([cc.HIGH_ITERS], [100, 100]):
            follow(tt, ctx, name, (label, pieces), engine, lds_mode, rec_inst, steps, cc.HIGH_START, pieces)


@pytest.mark.timeout(3)
def test_driver_saves_the_restatements_models(tt, orc):
    """TD_inversion_function with n_iter 300, burn_in 100, keep_each 20 on case A prior 1: model_hist is the
    restatement's (:275-288) -- the models after iterations 119, 139, ..., 299 themselves, not only ten of
    them -- on the DEVICE engine (recorded by the kernel, and one launch per saved model) and the HOST engine.
    Measured: 0.04 s."""
    name = "A-p1-T1"
    rname, ncells, _, _, _, prior, _, seed = cc.CASES[name]
    ref = cc.driver_reference(tt)
    by_iter = {s.iter: s for s in ref["steps"]}
    assert len(ref["saved"]) == 10
    prm = cc.td_parameters(tt, name, **cc.DRIVER)
    for engine, history in ((tt.TD_ENGINE_DEVICE, True), (tt.TD_ENGINE_DEVICE, False), (tt.TD_ENGINE_HOST, True)):
        hist = tt.TD_inversion_function(prm, cc.rays(tt, rname), cc.CHAIN, seed=seed,
                                        model=cc.start_model(tt, ncells, prior, seed), engine=engine, history=history)
        assert len(hist) == len(ref["saved"]), (engine, history, len(hist))
        for m, it in zip(hist, ref["saved"]):
            s = by_iter[it]
            assert m.nCells == s.ncells and m.phi == s.phi and np.array_equal(m.ptS, s.ptS), (engine, history, it)
            assert all(np.array_equal(a, b) for a, b in zip(m.cells(), s.cells)), (engine, history, it)
            assert (m.action, m.accept) == (s.action, s.accept), (engine, history, it)


@pytest.mark.timeout(6)
def test_in_kernel_draws_follow_the_restatement(tt, orc):
    """The draws made inside k_chain_run (csrc/chain_kernels.hip: a launch without a precomputed table) on the
    eight free-running instances, which otherwise take that branch only when a launch's draws would exceed
    256 MB: tests/chain_draws_worker.py, a child with TD_PRE_DRAWS=0 (read once per process), runs case A
    prior 1 for 200 iterations on instances 0, 8, 2, 9 (alone) and 5, 11, 4, 10 (two chains per launch, chain
    numbers 1 and 2), then on 8 and 9 again from iteration 2^32 - 100 on (the kernel's own refill carries the
    counter across 2^32), and its histories and end states must be the restatement's.  That the child drew in the
    kernel is not taken from the environment variable alone: tdt_chain_draws_launches, a host-side count of
    k_draws launches, is 0 there (test_unrecorded_pieces_follow_the_restatement sees it count in a normal
    process).  Measured: 0.46 s, the child's start included, with the first eight of its ten runs;
    with all ten, below 1.4 s within the whole suite."""
    import chain_draws_worker as w

    name = w.NAME
    rname, ncells, _, _, _, prior, _, seed = cc.CASES[name]
    want = {1: cc.reference(tt, name)["steps"][:w.ITERS]}
    p2 = cc.chain_params(tt, name)
    p2.chain = 2
    want[2] = cc.restate(tt, cc.rays(tt, rname), p2, cc.start_model(tt, ncells, prior, seed), w.ITERS)["steps"]
    assert [s.action for s in want[1]] != [s.action for s in want[2]]
    assert w.ITERS == cc.HIGH_ITERS
    high = cc.reference(tt, name, cc.HIGH_ITERS, cc.HIGH_START)["steps"]
    p = subprocess.run([sys.executable, "-u", WORKER], env=dict(os.environ, TD_PRE_DRAWS="0"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=4, cwd=ROOT)
    text = p.stdout.decode(errors="replace")
    assert p.returncode == 0, text[-3000:]
    rows = [json.loads(x) for x in text.splitlines() if x.startswith("{")]
    runs = {r["run"]: r for r in rows if "run" in r}
    assert sorted(runs) == sorted(w.RUNS)
    for run, (_, recorded, numbers, start_iter) in w.RUNS.items():
        r = runs[run]
        assert len(r["ends"]) == len(numbers) and len(r["histories"]) == (len(numbers) if recorded else 0), run
        for k, number in enumerate(numbers):
            e = r["ends"][k]
            steps = high if start_iter else want[number]
            bad = cc.end_diff(e["stats"], e["cells"], e["phi"], e["ptS"], steps)
            assert bad is None, (run, number, bad)
            if recorded:
                a = {key: (None if v is None else np.asarray(v)) for key, v in r["histories"][k].items()}
                bad = cc.history_diff(a, steps)
                assert bad is None, (run, number, bad)
    tail = rows[-1]
    assert tail["draws_launches"] == 0, tail  # no launch of the child loaded precomputed draws
    launched = tail["launched"]
    assert len(launched) == NINST
    for instance, count in ((0, 1), (2, 1), (8, 2), (9, 2), (4, 1), (5, 1), (10, 1), (11, 1)):
        assert launched[instance] == count, (instance, launched)
    assert sum(launched) == 10, launched
