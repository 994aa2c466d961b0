"""The restatement of the reference's loop (oracle/chain_ref.py, TD_inversion_function.jl:69-288) by itself:
no GPU.  tests/test_gpu_chain_reference.py holds every chain engine to its runs with ==; that says something
only if those runs visit every branch of the loop and no decision in them hangs on the last bits of alpha.
So, for every case of tests/chain_cases.py:

  * every evaluated proposal has |ln u - ln alpha_raw| >= 1e-6.  A condition, not a tolerance: the build decides
    ln u < ln alpha with det_log (within 4e-16 relative of libm, test_deterministic_math), the restatement u <
    min(1, alpha) with libm's exp, and the two forms differ by rounding of order 1e-12 at |phi| <= 1e3 -- six
    decades below.  No decision is excused as a near tie;
  * each of the four actions is accepted >= 10 times and rejected after its evaluation >= 10 times;
  * in each 8-cell case (A) a birth is skipped at max_cells and a death at min_cells;
  * under priors 1 and 3 a birth's zeta and a change's zeta fall outside the prior's support;
  * a move leaves the box.

Seeds passed over (the conditions stay, the seed moves on; seeds are tried in the order 1, 2, 3, ...):
  A-p2-T1    seeds 1-4: no death skipped at min_cells (the chain stays above 5 cells); 5: no birth skipped
             at max_cells -> seed 6;
  A-p3-T2.5  seeds 1-5: no birth skipped at max_cells (the chain stays below 12 cells) -> seed 6.
"""
import ctypes

import numpy as np
import pytest

import chain_cases as cc

MARGIN = 1e-6


@pytest.mark.parametrize("name", list(cc.CASES))
def test_restatement_visits_every_branch(tt, orc, name):
    ref = cc.reference(tt, name)
    prior = cc.CASES[name][5]
    assert len(ref["steps"]) == cc.CASES[name][4]
    t, margin = cc.tally(ref)
    print(name, t, "smallest margin %.3g" % margin)
    assert margin >= MARGIN
    for a in (1, 2, 3, 4):
        accepted, rejected, skipped, invalid = t[a]
        assert accepted >= 10 and rejected >= 10, (a, t[a])
        assert ref["accepted"][a - 1] == accepted and ref["proposed"][a - 1] == accepted + rejected + invalid
    if name.startswith("A"):
        assert t[1][2] >= 1 and t[2][2] >= 1, t  # skipped at max_cells (:77) and at min_cells (:127)
    if prior in (1, 3):
        assert t[1][3] >= 1 and t[3][3] >= 1, t  # :103 / :117 and :199 / :211
    else:
        assert t[1][3] == 0 and t[3][3] == 0  # the normal prior has no support to leave
    assert t[2][3] == 0 or prior == 3  # only the exponential death can be invalid (:171)
    assert t[4][3] >= 1, t  # :244
    assert t[3][2] == 0 and t[4][2] == 0  # a change is never skipped; a move only without cells


def test_restatement_of_the_other_runs(tt, orc):
    """The runs of tests/test_gpu_chain_reference.py beyond the ten cases: case A prior 1 from iteration 2^32 -
    100 on, and the driver's 300 iterations with their thinning (:275-288).  The margin holds there too, the
    iterations are the absolute ones, and burn_in 100, keep_each 20 save 119, 139, ..., 299 -- ten models, the
    first at model_num = 20 (iteration 100 counts: iter >= burn_in, :276), not at iteration 120."""
    hi = cc.reference(tt, "A-p1-T1", cc.HIGH_ITERS, cc.HIGH_START)
    assert [s.iter for s in hi["steps"]] == list(range(2 ** 32 - 100, 2 ** 32 + 100))
    assert cc.tally(hi)[1] >= MARGIN
    assert sum(hi["accepted"]) >= 10
    # the actions at 2^32 + 1 .. 2^32 + 99 (a function of the draws alone) are not those of iterations 1 .. 99
    lo = cc.reference(tt, "A-p1-T1")["steps"]
    assert [s.action for s in hi["steps"][101:]] != [s.action for s in lo[:99]]
    drv = cc.driver_reference(tt)
    assert drv["saved"] == list(range(119, 300, 20))
    assert cc.tally(drv)[1] >= MARGIN


class ScriptedDraws:
    """What oracle/chain_np.py's loop asks of its generator, answered from the build's uniforms of one chain
    in the order that loop asks (one chain: K = 1): per iteration integers -> the action, random(K) -> u_accept,
    then u_index for kill, change and move, random((K, 3)) -> the birth site's uniforms, standard_normal(K) ->
    z(u_zeta) for birth and change, standard_normal((K, 3)) -> the move's normals."""

    def __init__(self, tt, seed, chain):
        self.draws, self.q = cc.draws_of(tt, seed, chain), tt.lib().tdt_normal_quantile
        self.it, self.u, self.scalars = 0, None, 0

    def integers(self, lo, hi, K):
        assert (lo, hi, K) == (1, 5, 1)
        self.it += 1
        self.u, self.scalars = self.draws(self.it), 0
        return np.array([1 + int(4 * self.u[0])])

    def random(self, shape):
        if shape == 1:
            self.scalars += 1
            return np.array([self.u[1] if self.scalars == 1 else self.u[6]])
        assert shape == (1, 3)
        return np.array([[self.u[2], self.u[3], self.u[4]]])

    def standard_normal(self, shape):
        if shape == 1:
            return np.array([self.q(self.u[5])])
        assert shape == (1, 3)
        return np.array([[self.q(self.u[2]), self.q(self.u[3]), self.q(self.u[4])]])


@pytest.mark.parametrize("prior", [1, 2, 3])
def test_restatement_agrees_with_chain_np_on_the_prior(tt, orc, prior):
    """With phi_n - phi forced to 0 (debug_prior = 1: evaluate returns phi = 1, MCsub.jl:134-136) the restatement
    and oracle/chain_np.py -- two restatements of the same lines, the second vectorised and written for another
    purpose -- must make the same chain out of the same numbers: which branches are legal (skipped at the cell
    bounds, the prior's support, the box), which model's value enters czeta and a death's zetanew, N - 1, N and
    N + 1 in the model-size factor, the order of deleteat! and append!.  600 iterations from 8 cells between 5
    and 12; every cell of the final model, and the cell count after every prefix of 100."""
    from oracle import chain_np

    name = "A-p%d-T1" % prior
    seed = cc.CASES[name][7]
    p = cc.chain_params(tt, name)
    start = cc.start_model(tt, 8, prior, seed)
    ds = cc.rays(tt, "syn24")
    ref = cc.restate(tt, ds, p, start, 600, debug_prior=1)
    assert all(s.phi == 1.0 for s in ref["steps"])
    assert cc.tally(ref)[1] >= MARGIN
    assert min(ref["accepted"]) >= 10
    box = (p.xmin, p.xmax, p.ymin, p.ymax, p.zmin, p.zmax)
    for iters in (100, 200, 300, 400, 500, 600):
        N, zetas, xs = chain_np.run(1, iters, box, prior=prior, sig=p.sig, zeta_scale=p.zeta_scale,
                                    max_cells=p.max_cells, min_cells=p.min_cells,
                                    rng=ScriptedDraws(tt, p.seed, p.chain), start=start.cells())
        s = ref["steps"][iters - 1]
        assert N[0] == s.ncells, iters
        assert np.array_equal(xs[0], s.cells[0]) and np.array_equal(zetas[0], s.cells[3]), iters


def test_comparison_with_a_history_can_fail(tt, orc):
    """The whole judgement of tests/test_gpu_chain_reference.py (chain_cases.history_diff, end_diff) on a
    history made up from the restatement's own steps: nothing to report; then with one thing changed at a
    time, by one unit in the last place where it is a float: each is reported."""
    steps = cc.reference(tt, "A-p1-T1")["steps"][:300]

    def faithful():
        return dict(off=np.concatenate([[0], np.cumsum([s.ncells for s in steps])]),
                    x=np.concatenate([s.cells[0] for s in steps]), y=np.concatenate([s.cells[1] for s in steps]),
                    z=np.concatenate([s.cells[2] for s in steps]), zeta=np.concatenate([s.cells[3] for s in steps]),
                    phi=np.array([s.phi for s in steps]), iter=np.array([s.iter for s in steps]),
                    action=np.array([s.action for s in steps]), accept=np.array([s.accept for s in steps]),
                    ptS=np.stack([s.ptS for s in steps]))

    assert cc.history_diff(faithful(), steps) is None
    for key, word in (("phi", "phi"), ("x", "xCell"), ("y", "yCell"), ("z", "zCell"), ("zeta", "zetaCell"),
                      ("ptS", "ptS"), ("iter", "iter"), ("action", "action"), ("accept", "accept")):
        a = faithful()
        flat = a[key].reshape(-1)
        k = (7 * len(flat)) // 11
        flat[k] = np.nextafter(flat[k], np.inf) if flat.dtype == np.float64 else flat[k] + 1
        bad = cc.history_diff(a, steps)
        assert bad is not None and word in bad, (key, bad)
    a = faithful()
    a["off"] = a["off"].copy()
    a["off"][100] += 1
    assert "nCells" in cc.history_diff(a, steps)
    assert "samples" in cc.history_diff(faithful(), steps[:-1])
    a = faithful()
    a["ptS"] = None
    assert "no ptS" in cc.history_diff(a, steps)
    # the end state: stats and model after the steps
    acc, prop = cc.counts(steps)
    s = steps[-1]
    stats = dict(accepted=acc, proposed=prop, phi=s.phi, ncells=s.ncells, last_action=s.action, last_accept=s.accept,
                 iterations=len(steps))
    assert cc.end_diff(stats, s.cells, s.phi, s.ptS, steps) is None
    assert sum(acc) > 0 and acc != prop
    for key, other in (("accepted", prop), ("proposed", acc), ("phi", np.nextafter(s.phi, 0.0)),
                       ("ncells", s.ncells + 1), ("last_action", s.action % 4 + 1), ("last_accept", 1 - s.accept),
                       ("iterations", len(steps) + 1)):
        assert key in cc.end_diff(dict(stats, **{key: other}), s.cells, s.phi, s.ptS, steps)
    assert "phi" in cc.end_diff(stats, s.cells, np.nextafter(s.phi, 0.0), s.ptS, steps)
    moved = [c.copy() for c in s.cells]
    moved[3][0] = np.nextafter(moved[3][0], np.inf)
    assert "zetaCell" in cc.end_diff(stats, moved, s.phi, s.ptS, steps)
    ptS = s.ptS.copy()
    ptS[-1] = np.nextafter(ptS[-1], np.inf)
    assert "ptS" in cc.end_diff(stats, s.cells, s.phi, ptS, steps)


def test_draws_use_the_iteration_counters_high_word(tt):
    """tdt_draws at iteration 2^32 + k is not iteration k's (k = 1..64): the Philox counter's second word
    (chain_logic.h draw_iteration i1) carries the iteration's high half."""
    L = tt.lib()
    a, b = (ctypes.c_double * 7)(), (ctypes.c_double * 7)()
    for k in range(1, 65):
        L.tdt_draws(99, 1, k, a)
        L.tdt_draws(99, 1, 2 ** 32 + k, b)
        assert all(0.0 < v < 1.0 for v in b)
        assert all(x != y for x, y in zip(a, b)), k  # (seven 52-bit values each: equal only if the word is dropped)
    L.tdt_draws(99, 1, 2 ** 33 + 1, a)
    L.tdt_draws(99, 1, 2 ** 32 + 1, b)
    assert list(a) != list(b)


def test_draws_launch_counter_hook(tt):
    """tdt_chain_draws_launches (the count of k_draws launches, beside tdt_chain_launch_counts) checks its
    argument before anything else; what it counts needs a GPU (tests/test_gpu_chain_reference.py)."""
    L = tt.lib()
    n = ctypes.c_int64(-1)
    assert L.tdt_chain_draws_launches(None) == 1  # TD_ERR_ARG
    assert L.tdt_chain_draws_launches(ctypes.byref(n)) == 0 and n.value >= 0
