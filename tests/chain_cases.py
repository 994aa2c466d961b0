"""The cases of tests/test_chain_reference.py (CPU: the conditions on the restatement alone) and
tests/test_gpu_chain_reference.py (GPU: every chain engine against it; tests/test_gpu_shim_replay.py: the Julia
shim's transliteration in its forward calls' place), and the restatement's run of each
(oracle/chain_ref.py on the build's own uniforms, tdt_draws), computed once per process and never modified.

A: synthetic_rays(24, seed=1), random_model(8, .), min_cells 5, max_cells 12, 1500 iterations, priors
   1, 2, 3 x T in {1, 2.5} -- births skipped at max_cells, deaths skipped at min_cells;
B: the same rays, 40 cells, max_cells 60, 1500 iterations, priors 1-3 at T = 1;
C: the 381 shipped rays, 60 cells, max_cells 80, 600 iterations, prior 1.
Prior 2 starts from normal(0, 50) zeta, as tests/test_gpu_chain.py test_priors_device_follows_host does.

`seed` is the chain's RNG seed and the starting model's: the first of 1, 2, 3, ... (case C: of 7, 8, ...) at
which the restatement's run meets every condition of tests/test_chain_reference.py, each case by itself.  Two
cases passed seeds over; tests/test_chain_reference.py says which and why."""
import ctypes
import functools

import numpy as np

#        name: (rays, cells, min_cells, max_cells, iterations, prior, T, seed)
CASES = {
    "A-p1-T1": ("syn24", 8, 5, 12, 1500, 1, 1.0, 1),
    "A-p1-T2.5": ("syn24", 8, 5, 12, 1500, 1, 2.5, 1),
    "A-p2-T1": ("syn24", 8, 5, 12, 1500, 2, 1.0, 6),
    "A-p2-T2.5": ("syn24", 8, 5, 12, 1500, 2, 2.5, 1),
    "A-p3-T1": ("syn24", 8, 5, 12, 1500, 3, 1.0, 1),
    "A-p3-T2.5": ("syn24", 8, 5, 12, 1500, 3, 2.5, 6),
    "B-p1": ("syn24", 40, 5, 60, 1500, 1, 1.0, 1),
    "B-p2": ("syn24", 40, 5, 60, 1500, 2, 1.0, 1),
    "B-p3": ("syn24", 40, 5, 60, 1500, 3, 1.0, 1),
    "C-p1": ("rays381", 60, 5, 80, 600, 1, 1.0, 7),
}
CHAIN = 1  # the chain number of every case (the Philox counter's fourth word)


@functools.lru_cache(maxsize=None)
def rays(tt, name):
    return tt.synthetic_rays(24, seed=1) if name == "syn24" else tt.load_data_Tonga()


def start_model(tt, ncells, prior, seed):
    m = tt.random_model(ncells, seed)
    if prior == 2:
        m.zeta[:] = np.random.default_rng(seed).normal(0.0, 50.0, ncells)  # the normal prior's start
    return m


def td_parameters(tt, name, **more):
    _, _, min_cells, max_cells, _, prior, _, _ = CASES[name]
    return tt.define_TDstructrure().replace(prior=prior, min_cells=min_cells, max_cells=max_cells, **more)


def chain_params(tt, name, engine=None, start_iter=0):
    """The td_chain_params of a case (the box is data.box(): dataStruct None, as the chain tests make theirs)."""
    T, seed = CASES[name][6], CASES[name][7]
    p = tt.chain_params(td_parameters(tt, name), None, seed=seed, chain=CHAIN, temperature=T,
                        engine=tt.TD_ENGINE_DEVICE if engine is None else engine)
    p.start_iter = start_iter
    return p


def draws_of(tt, seed, chain):
    """iteration -> the build's seven uniforms of (seed, chain, iteration)"""
    L = tt.lib()
    out = (ctypes.c_double * 7)()

    def draws(it):
        L.tdt_draws(seed, chain, it, out)
        return tuple(out)

    return draws


def restate(tt, ds, p, model, iters, start_iter=1, burn_in=None, keep_each=None, debug_prior=0, forward=None,
            resume=None):
    """oracle.chain_ref.run for the chain that td_chain_params `p` describes, from `model` (a Model, or the four
    cell arrays of a Step); `forward` and `resume` as chain_ref.run takes them."""
    from oracle import chain_ref

    prm = chain_ref.Params((p.xmin, p.xmax, p.ymin, p.ymax, p.zmin, p.zmax), prior=p.prior, sig=p.sig,
                           zeta_scale=p.zeta_scale, max_cells=p.max_cells, min_cells=p.min_cells,
                           debug_prior=debug_prior, temperature=p.temperature, burn_in=burn_in, keep_each=keep_each)
    cells = model.cells() if hasattr(model, "cells") else model
    return chain_ref.run(ds, prm, cells, iters, draws_of(tt, p.seed, p.chain), tt.lib().tdt_normal_quantile,
                         start_iter=start_iter, forward=forward, resume=resume)


@functools.lru_cache(maxsize=None)
def reference(tt, name, iters=None, start_iter=1):
    """The restatement's run of a case (shared: treat as read-only)."""
    rname, ncells, _, _, n, prior, _, seed = CASES[name]
    return restate(tt, rays(tt, rname), chain_params(tt, name), start_model(tt, ncells, prior, seed),
                   n if iters is None else iters, start_iter)


# case A prior 1 across the iteration counter's 32-bit boundary
HIGH_START, HIGH_ITERS = 2 ** 32 - 100, 200
# the driver's run (TD_inversion_function with these TD_parameters on case A prior 1's rays and start)
DRIVER = dict(n_iter=300.0, burn_in=100.0, keep_each=20.0, print_each=100.0)


@functools.lru_cache(maxsize=None)
def driver_reference(tt):
    """The restatement of TD_inversion_function(td_parameters(A-p1-T1, **DRIVER), rays, 1, seed, model): the box
    is the dataStruct's (xVec, yVec, zVec: :30-32), `saved` the iterations of model_hist."""
    name = "A-p1-T1"
    rname, ncells, _, _, _, prior, T, seed = CASES[name]
    ds = rays(tt, rname)
    p = tt.chain_params(td_parameters(tt, name, **DRIVER), ds, seed=seed, chain=CHAIN, temperature=T)
    return restate(tt, ds, p, start_model(tt, ncells, prior, seed), int(DRIVER["n_iter"]), 1, DRIVER["burn_in"],
                   DRIVER["keep_each"])


def history_diff(a, steps):
    """What differs between a History's read_arrays() of one sample per iteration and the restatement's steps
    (==: every header, phi, ptS and cell of every iteration), or None."""
    n = len(steps)
    if len(a["phi"]) != n:
        return "%d samples, %d iterations" % (len(a["phi"]), n)
    want = {"iter": [s.iter for s in steps], "action": [s.action for s in steps], "accept": [s.accept for s in steps],
            "phi": [s.phi for s in steps]}
    for key, w in want.items():
        bad = np.flatnonzero(np.asarray(a[key]) != np.asarray(w))
        if bad.size:
            k = int(bad[0])
            return "%s differs first at sample %d (iteration %d, action %d): %r, restatement %r" % (
                key, k, steps[k].iter, steps[k].action, np.asarray(a[key])[k].item(), w[k])
    off = np.concatenate([[0], np.cumsum([s.ncells for s in steps])])
    if not np.array_equal(a["off"], off):
        k = int(np.flatnonzero(np.diff(a["off"]) != np.diff(off))[0])
        return "nCells differs first at iteration %d" % steps[k].iter
    for j, key in enumerate(("x", "y", "z", "zeta")):
        w = np.concatenate([s.cells[j] for s in steps])
        bad = np.flatnonzero(np.asarray(a[key]) != w)
        if bad.size:
            k = int(np.searchsorted(off, bad[0], side="right")) - 1
            return "%sCell differs first at iteration %d, cell %d" % (key, steps[k].iter, int(bad[0] - off[k]))
    if a["ptS"] is None:
        return "the history holds no ptS"
    bad = np.flatnonzero((np.asarray(a["ptS"]) != np.stack([s.ptS for s in steps])).any(axis=1))
    if bad.size:
        return "ptS differs first at iteration %d" % steps[int(bad[0])].iter
    return None


def steps_diff(got, want, with_ptS=True):
    """What differs between two runs of oracle.chain_ref.run (==: iter, action, accept, outcome, nCells, phi, ptS
    and the four cell arrays of every step, then accepted and proposed, and the starting model's phi and ptS),
    or None.  Without `with_ptS` no ptS is compared (debug_prior = 1: evaluate computes none)."""
    a, b = got["steps"], want["steps"]
    if len(a) != len(b):
        return "%d steps, %d wanted" % (len(a), len(b))
    for s, w in zip(a, b):
        for key in ("iter", "action", "accept", "outcome", "ncells", "phi"):
            if getattr(s, key) != getattr(w, key):
                return "%s differs first at iteration %d (action %d): %r, wanted %r" % (
                    key, w.iter, w.action, getattr(s, key), getattr(w, key))
        if with_ptS and not (s.ptS is not None and np.array_equal(s.ptS, w.ptS)):
            return "ptS differs first at iteration %d (action %d)" % (w.iter, w.action)
        for j, key in enumerate(("x", "y", "z", "zeta")):
            if not np.array_equal(s.cells[j], w.cells[j]):
                return "%sCell differs first at iteration %d (action %d)" % (key, w.iter, w.action)
    for key in ("accepted", "proposed"):
        if list(got[key]) != list(want[key]):
            return "%s is %r, wanted %r" % (key, got[key], want[key])
    if got["start"][0] != want["start"][0]:
        return "the starting model's phi is %r, wanted %r" % (got["start"][0], want["start"][0])
    if with_ptS and not (got["start"][1] is not None and np.array_equal(got["start"][1], want["start"][1])):
        return "the starting model's ptS differs"
    return None


def window(steps, first, n):
    """What a run resumed after steps[first - 1] (the model after iteration `first` of a run from iteration 1)
    must give for n iterations, in the shape of oracle.chain_ref.run's result."""
    part = steps[first:first + n]
    acc, prop = counts(part)
    return dict(steps=part, start=(steps[first - 1].phi, steps[first - 1].ptS), accepted=acc, proposed=prop)


def counts(steps):
    """(accepted, proposed) per action 1..4 over the steps: td_chain_stats' counters after them."""
    from oracle import chain_ref

    acc, prop = [0] * 4, [0] * 4
    for s in steps:
        acc[s.action - 1] += s.accept
        prop[s.action - 1] += s.outcome != chain_ref.SKIPPED
    return acc, prop


def end_diff(stats, cells, phi, ptS, steps, iterations=None):
    """What differs between a chain's stats() and model after the steps and the restatement, or None."""
    acc, prop = counts(steps)
    s = steps[-1]
    want = dict(accepted=acc, proposed=prop, phi=s.phi, ncells=s.ncells, last_action=s.action, last_accept=s.accept,
                iterations=len(steps) if iterations is None else iterations)
    for key, w in want.items():
        if stats[key] != w:
            return "stats %s is %r, restatement %r" % (key, stats[key], w)
    if phi != s.phi:
        return "the model's phi is %r, restatement %r" % (phi, s.phi)
    for j, key in enumerate(("x", "y", "z", "zeta")):
        if not np.array_equal(np.asarray(cells[j]), s.cells[j]):
            return "%sCell of the end model differs" % key
    if not np.array_equal(np.asarray(ptS), s.ptS):
        return "ptS of the end model differs"
    return None


def tally(ref):
    """What the conditions count: per action 1..4 [accepted, rejected after evaluation, skipped, invalid], and
    the smallest margin of an evaluated proposal."""
    from oracle import chain_ref

    t = {a: [0, 0, 0, 0] for a in (1, 2, 3, 4)}
    margin = np.inf
    for s in ref["steps"]:
        if s.outcome == chain_ref.EVALUATED:
            t[s.action][0 if s.accept else 1] += 1
            margin = min(margin, s.margin)
        else:
            assert s.accept == 0
            t[s.action][2 if s.outcome == chain_ref.SKIPPED else 3] += 1
    return t, float(margin)
