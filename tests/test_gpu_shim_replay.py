"""The Julia shim's call order replayed against the restated loop.

The "host" is the restatement of the reference's loop (oracle/chain_ref.py, TD_inversion_function.jl:69-288) on
the build's uniforms, with its two forward calls replaced by the transliterated shim of INTEGRATION.md section 2
(tests/shim_replay.py: ctypes statements on the library, no TdContext): cc.restate(..., forward=shim.forward(ds)).
So the library sees what an unchanged Julia host sends it, which the DROPIN engine (csrc/chain.cpp host_iteration,
test_gpu_chain_reference.py test_dropin_follows_the_restatement) does not send:
  * a change is evaluated at :191 BEFORE the validity check of :195 / :206: td_evaluate gets models the host then
    discards unseen, and the next call is an edit of the model before;
  * under prior 2 a death is evaluated twice (:141, :159) and then interpolated on the reduced model;
  * the first td_interpolate may come before any td_evaluate (debug_prior = 1; a resumed chain, :41-67);
  * a pmap worker keeps its context for the life of the process and runs chain after chain on it.
csrc/incremental.cpp recognises "one edit from B or from Q" from that sequence alone.  Every step of every replay
must equal the restatement's own run (the C oracle in the forward calls' place) with == (cc.steps_diff: iter,
action, accept, outcome, nCells, phi, ptS, the four cell arrays, accepted, proposed, the starting model).
tests/test_chain_reference.py shows on the CPU that those runs contain the distinguishing sequences.

What this does not show: that the Julia text itself runs.  Only its transliteration has
(tests/test_shim_text_host.py ties the two together line by line).

Each test was timed once on an MI355X (its whole call, written in its docstring); its pytest.mark.timeout is about
four times that plus a process's start, as in tests/test_gpu_chain_reference.py."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import chain_cases as cc
import shim_replay

pytestmark = pytest.mark.gpu

NINST = 14


def launches(tt):
    out, n = (ctypes.c_int64 * 32)(), ctypes.c_int(0)
    assert tt.lib().tdt_chain_launch_counts(out, ctypes.byref(n)) == 0 and n.value == NINST
    return np.array([out[i] for i in range(NINST)], dtype=np.int64)


@contextlib.contextmanager
def worker(tt):
    """One worker process's shim; its contexts are destroyed on the way out whatever happens."""
    shim = shim_replay.Shim(tt)
    try:
        yield shim
    finally:
        shim.close()


def replay(tt, shim, name, iters=None, debug_prior=0):
    """The case's chain with the shim in the forward calls' place -> (the run, td_evaluate calls, td_interpolate
    calls, the launches it took)"""
    rname, ncells, _, _, n, prior, _, seed = cc.CASES[name]
    e0, i0, l0 = shim.calls["td_evaluate"], shim.calls["td_interpolate"], launches(tt)
    ds = cc.rays(tt, rname)
    run = cc.restate(tt, ds, cc.chain_params(tt, name), cc.start_model(tt, ncells, prior, seed),
                     n if iters is None else iters, debug_prior=debug_prior, forward=shim.forward(ds, debug_prior))
    return run, shim.calls["td_evaluate"] - e0, shim.calls["td_interpolate"] - i0, launches(tt) - l0


def entered(steps, actions):
    from oracle import chain_ref

    return sum(s.action in actions and s.outcome != chain_ref.SKIPPED for s in steps)


def check_data_run(name, ref, run, nev, nint):
    from oracle import chain_ref

    bad = cc.steps_diff(run, ref)
    assert bad is None, (name, bad)
    # the reference's order: every evaluate of the loop reached the library, and more of them than the DROPIN
    # engine makes (1 + one per EVALUATED step): changes evaluated and then invalid, prior 2's second evaluate
    assert nev == run["evaluations"] == ref["evaluations"], (name, nev, run["evaluations"], ref["evaluations"])
    assert nint == entered(ref["steps"], (1, 2)), (name, nint)
    return sum(s.outcome == chain_ref.EVALUATED for s in ref["steps"])


@pytest.mark.timeout(5)
@pytest.mark.parametrize("name", ["A-p1-T1", "A-p2-T1", "A-p3-T1", "B-p2", "C-p1"])
def test_replay_follows_the_restatement(tt, orc, name):
    """The whole case on a fresh worker.  td_evaluate is called ref["evaluations"] times, strictly more than 1 +
    the EVALUATED steps (test_restatement_visits_every_branch's conditions guarantee it: an invalid change under
    priors 1 and 3, >= 20 twice-evaluated deaths under prior 2), and the launches are the resident server's
    (instance 1) alone: the incremental path really ran.  Measured: 0.21-0.36 s per case (the module's first
    case the longest of those), C-p1 0.58 s."""
    ref = cc.reference(tt, name)
    with worker(tt) as shim:
        run, nev, nint, used = replay(tt, shim, name)
        evaluated = check_data_run(name, ref, run, nev, nint)
        print(name, "td_evaluate %d (1 + %d EVALUATED steps), td_interpolate %d, launches %s"
              % (nev, evaluated, nint, used))
        assert nev > 1 + evaluated, (name, nev, evaluated)
        assert used[1] >= 1 and used.sum() == used[1], (name, used)
        assert shim.calls["td_create"] == 1 and shim.TDCTX0.value is None


@pytest.mark.timeout(4)
def test_chain_after_chain_on_one_worker(tt, orc):
    """A-p1-T1 whole, then A-p3-T1 whole on the same shim: the same rays, the same cached TDCTX, and a second
    starting model that has nothing to do with the shadow chain the first run left.  Measured: 0.29 s."""
    with worker(tt) as shim:
        for name in ("A-p1-T1", "A-p3-T1"):
            run, nev, nint, used = replay(tt, shim, name)
            check_data_run(name, cc.reference(tt, name), run, nev, nint)
            assert used[1] >= 1 and used.sum() == used[1], (name, used)
        assert shim.calls["td_create"] == 1


PRIOR_ITERS = 600


@functools.lru_cache(maxsize=None)
def prior_reference(tt):
    """A-p1-T1's rays and start under debug_prior = 1: the run that test_restatement_agrees_with_chain_np_on_the_prior
    (tests/test_chain_reference.py) holds to oracle/chain_np.py."""
    name = "A-p1-T1"
    rname, ncells, _, _, _, prior, _, seed = cc.CASES[name]
    return cc.restate(tt, cc.rays(tt, rname), cc.chain_params(tt, name), cc.start_model(tt, ncells, prior, seed),
                      PRIOR_ITERS, debug_prior=1)


@pytest.mark.timeout(3)
@pytest.mark.parametrize("after", [None, "A-p1-T1"], ids=["fresh", "after-a-data-run"])
def test_debug_prior_needs_no_evaluate(tt, orc, after):
    """debug_prior = 1 for 600 iterations: the shim's evaluate returns before td_evaluate, so the library sees
    td_create and then one-point td_interpolate calls only -- on a fresh worker the first is its first call after
    td_create; after a data run (300 iterations of A-p1-T1) they meet a context whose shadow chain holds an
    unrelated model.  No td_evaluate, no launch of the chain kernel, every phi 1.0, the model's ptS never
    touched, and one td_interpolate per birth and death the loop ENTERED: a birth interpolates at :81 before its
    zeta is judged at :92, so the births that are then invalid (:103) count too -- not only the evaluated ones.
    Measured: 0.05 s fresh, 0.07 s after the data run."""
    from oracle import chain_ref

    name = "A-p1-T1"
    ref = prior_reference(tt)
    assert all(s.phi == 1.0 for s in ref["steps"])
    with worker(tt) as shim:
        if after:
            head, nev, nint, used = replay(tt, shim, after, 300)
            want = cc.reference(tt, after)
            want = dict(want, steps=want["steps"][:300])
            want["accepted"], want["proposed"] = cc.counts(want["steps"])
            bad = cc.steps_diff(head, want)
            assert bad is None, bad
            assert nev == head["evaluations"] > 300 // 2 and used[1] >= 1
        run, nev, nint, used = replay(tt, shim, name, PRIOR_ITERS, debug_prior=1)
        bad = cc.steps_diff(run, ref, with_ptS=False)
        assert bad is None, bad
        assert nev == 0 and not used.any(), (nev, used)
        births_deaths = [s for s in ref["steps"] if s.action in (1, 2)]
        n_entered = entered(ref["steps"], (1, 2))
        n_evaluated = sum(s.outcome == chain_ref.EVALUATED for s in births_deaths)
        assert nint == n_entered >= n_evaluated >= 100, (nint, n_entered, n_evaluated)
        assert all(s.phi == 1.0 and s.ptS is None for s in run["steps"]) and run["start"] == (1.0, None)
        assert run["evaluations"] == ref["evaluations"]  # the host called evaluate as often; the shim returned
        assert shim.calls["td_create"] == 1 and shim.TDCTX.value is not None and shim.TDCTX0.value is None


RESUME_ITERS = 300


@pytest.mark.timeout(3)
@pytest.mark.parametrize("action", [1, 2], ids=["birth-first", "death-first"])
def test_resumed_chain(tt, orc, action):
    """A chain loaded from its checkpoint (:41-67): a fresh worker, no evaluate of a starting model, the model
    after iteration k of A-p1-T1 with its saved phi and ptS, k the first >= 100 whose iteration k + 1 is a birth
    (a death) that is not skipped; 300 iterations, equal to steps[k:k + 300].  Birth first: the library's first
    call after the ray-less td_create is td_interpolate (:81), the worker's context is made by the evaluate that
    follows, and that evaluate's phi is what catches a ray-less context left in TDCTX.  Death first: evaluate
    (:141) comes before Interpolation (:146), so no ray-less context is made at all.  Measured: 0.05 s."""
    from oracle import chain_ref

    name = "A-p1-T1"
    steps = cc.reference(tt, name)["steps"]
    k = next(k for k in range(100, len(steps))
             if steps[k].action == action and steps[k].outcome != chain_ref.SKIPPED)
    assert steps[k].iter == k + 1 and k + RESUME_ITERS <= len(steps)
    want = cc.window(steps, k, RESUME_ITERS)
    ds = cc.rays(tt, cc.CASES[name][0])
    with worker(tt) as shim:
        run = cc.restate(tt, ds, cc.chain_params(tt, name), steps[k - 1].cells, RESUME_ITERS, start_iter=k + 1,
                         forward=shim.forward(ds), resume=want["start"])
        bad = cc.steps_diff(run, want)
        assert bad is None, (k, bad)
        assert shim.calls["td_evaluate"] == run["evaluations"]  # none for a starting model
        assert shim.calls["td_create"] == (2 if action == 1 else 1)
        assert (shim.TDCTX0.value is not None) == (action == 1) and shim.TDCTX.value is not None
        assert shim.TDCTX.value != shim.TDCTX0.value


@pytest.mark.timeout(3)
def test_one_point_queries_that_tie(tt, orc):
    """No death of B-p2 queries a tie or a site of its reduced model (tests/test_shim_text_host.py
    test_no_death_of_the_replayed_cases_queries_a_tie shows it from the reference's steps alone), so: six calls
    on a 12-cell model of the 24 synthetic rays, each against the C oracle: evaluate; the birth of
    a cell exactly on cell 5's site, evaluated; Interpolation at that site on the proposal (13 cells, cells 5 and
    12 at distance 0: v_nearest's strict < keeps cell 5) and on the model; the host accepts, and the death of
    cell 5, evaluated; Interpolation at the killed site on the reduced model, where it lands on the twin's site
    (now cell 11).  Measured: 0.01 s."""
    import oracle

    ds = cc.rays(tt, "syn24")
    x, y, z, zeta = (np.array(a, dtype=np.float64) for a in tt.random_model(12, 3).cells())
    model = (x, y, z, zeta)
    born = (np.append(x, x[5]), np.append(y, y[5]), np.append(z, z[5]), np.append(zeta, zeta[5] + 7.0))
    reduced = tuple(np.delete(a, 5) for a in born)
    site = ([x[5]], [y[5]], [z[5]])

    def evaluate(shim, cells):
        phi, ptS, valid = shim.evaluate(cells, ds, 0)
        r = oracle.evaluate(ds.rayX, ds.rayY, ds.rayZ, ds.rayL, ds.rayU, ds.tS, ds.allSig, cells)
        assert valid == 1 and phi == r["phi"] and np.array_equal(ptS, r["ptS"]), len(cells[0])

    def interpolate(shim, cells, value):
        got = shim.Interpolation(cells, *site)
        assert np.array_equal(got, oracle.interpolation(cells, *site)[0]) and got.shape == (1,)
        assert got[0] == value

    with worker(tt) as shim:
        evaluate(shim, model)
        evaluate(shim, born)
        interpolate(shim, born, zeta[5])  # the tie goes to the lower position, not to the newborn
        interpolate(shim, model, zeta[5])
        evaluate(shim, reduced)
        interpolate(shim, reduced, zeta[5] + 7.0)  # the twin, now the only cell on the site
        assert reduced[3][11] == zeta[5] + 7.0
        assert shim.calls == {"td_create": 1, "td_evaluate": 3, "td_interpolate": 3}
