"""Literal Python restatement of the rj-MCMC loop WITH the data in play --
TEST INFRASTRUCTURE ONLY (tests/test_chain_reference.py, tests/test_gpu_chain_reference.py,
tests/test_gpu_shim_replay.py).

One chain of TD_inversion_function.jl:69-288, statement by statement, so that every chain engine of
the build (the HOST engine's host_iteration, the fourteen k_chain_run instances, the drop-in path,
the driver's thinning) can be followed decision for decision by something that was not written from
the build's reading of the Julia.  Every number that reaches the chain's state goes through IEEE
+ - * / only, `evaluate` and `Interpolation` are the C oracle's (oracle.evaluate,
oracle.interpolation), so phi, ptS and every cell compare with ==.

Restated lines (TD_inversion_function.jl unless MCsub.jl is named):
  constants   :22 sig_zeta = zeta_scale * sig / 100; :30-32 xr, yr, zr = (sig / 100) * (max - min)
  alpha       :69 alpha = 0 BEFORE the loop: it lives across iterations and is overwritten only where
              the reference overwrites it (a branch that sets valid = 0 leaves the last one standing)
  valid       evaluate returns 1 (MCsub.jl:128,184); :103, :117, :171, :199, :244 set 0; the
              exponential change at :211 sets alpha = 0 instead and leaves valid alone
  action      :72 rand(1:4); :73-74 model.action = action, model.accept = 0 -- on every iteration,
              also when the branch is then skipped (:77, :127, :221) or invalid
  birth       :77-124 (czeta from the CURRENT model :81; append! :85-88; alpha per prior :96-97,
              :107-108, :113-114 with model.nCells / (model.nCells + 1))
  death       :127-180 (deleteat! :132-135; evaluate :141; zetanew = Interpolation of the REDUCED
              model at the killed site :146; alpha per prior :151-152, :160-162 -- after a second
              evaluate, :159 -- and :166-168, with model.nCells / (model.nCells - 1))
  change      :184-218 (evaluated at :191 BEFORE the validity check of :195 / :206)
  move        :221-250 (box check :230-232, evaluate only inside)
  decision    rand(1)[1] < alpha && valid == 1 (:121, :176, :214, :247), alpha = min(1, alpha) in the
              reference's own product-and-exp form -- not the build's log-domain comparison
  thinning    :275-288 (iter >= burn_in: model_num += 1; saved when mod(model_num, keep_each) == 0)

What is NOT the reference's and comes from the caller, because only the build defines it:
  * the seven uniforms of an iteration, `draws(iter)` -> (u_action, u_accept, u_a, u_b, u_c, u_zeta,
    u_index) -- the reference seeds from the wall clock (:13) -- and the standard-normal quantile
    `normal_quantile(p)`: rand(Normal(m, s)) is m + s * normal_quantile(u);
  * how the uniforms map to the reference's rand calls (csrc/chain_logic.h's comments, restated
    here, not called): action = 1 + floor(4 u_action) (:72); a birth site is u * (max - min) + min
    from u_a, u_b, u_c (:78-80) and zetanew = czeta + sig_zeta * z(u_zeta) (:82); kill / change /
    move = floor(u_index * nCells), 0-based (:128, :184, :222); a change is zeta + sig_zeta *
    z(u_zeta) (:188); a move is site + (xr, yr, zr) * z(u_a, u_b, u_c) (:226-228); the decision's
    rand(1)[1] is u_accept;
  * the temperature T, the build's one extension: (modeln.phi - model.phi) / 2 is divided by T.

Not restated: action 5 (unreachable, :72), the checkpoint files (:41-67, :282-294; `resume=` restates what
a loaded checkpoint means for the loop, no evaluate of a starting model, not the files) and the aliasing
of :280 (push!(model_hist, model) pushes a reference whose action / accept fields later iterations
overwrite at :73-74 until an acceptance rebinds `model`): `saved` holds the model of the saved
iteration itself, as the build's copies do.
"""
import math

import numpy as np

from . import evaluate, interpolation

SKIPPED, INVALID, EVALUATED = "skipped", "invalid", "evaluated"


class Step:
    """One iteration's outcome: the model AFTER it (cells = (x, y, z, zeta) arrays in Julia order,
    never modified afterwards: steps share them), what the iteration did and, for a proposal whose
    alpha the decision consulted, margin = |ln u - ln alpha_raw| (alpha_raw: before min(1, .))."""
    __slots__ = ("iter", "action", "accept", "outcome", "margin", "ncells", "phi", "ptS", "cells")


class Params:
    """What the loop reads of TD_parameters and dataStruct (define_TDstructure.jl:5-27; xVec, yVec,
    zVec enter only through their min and max, :30-32, :78-80, :230-232)."""

    def __init__(self, box, prior=1, sig=10, zeta_scale=50, max_cells=100, min_cells=5, debug_prior=0,
                 temperature=1.0, burn_in=None, keep_each=None):
        self.box = tuple(float(b) for b in box)
        self.prior, self.sig, self.zeta_scale = int(prior), sig, zeta_scale
        self.max_cells, self.min_cells, self.debug_prior = max_cells, min_cells, int(debug_prior)
        self.temperature = float(temperature)
        self.burn_in, self.keep_each = burn_in, keep_each


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:  # Julia's exp gives Inf; min(1, Inf) = 1
        return math.inf


def _margin(u, alpha_raw):
    if alpha_raw <= 0.0 or math.isinf(alpha_raw):
        return math.inf
    return abs(math.log(u) - math.log(alpha_raw))


def run(ds, prm, cells, iters, draws, normal_quantile, start_iter=1, forward=None, resume=None):
    """`iters` iterations start_iter, start_iter + 1, ... of one chain from the model `cells` on the
    rays of `ds` (rayX, rayY, rayZ, rayL, rayU, tS, allSig as DataStruct holds them).
    `forward` = (ev, interp) puts the caller's forward calls in the place of the C oracle's: ev(cells) ->
    (phi, ptS, valid), interp(cells, x, y, z) -> float (tests/shim_replay.py: the loop drives the library as
    the Julia host would); the evaluations are still counted here.  `resume` = (phi, ptS) of the model that
    `cells` holds: a chain loaded from its checkpoint (:41-67) evaluates no starting model, and `start` is
    `resume`.
    -> dict(steps = [Step], start = (phi, ptS) of the starting model (build_starting's evaluate,
    MCsub.jl:118), saved = the iterations pushed to model_hist (:275-288; [] without burn_in /
    keep_each), accepted / proposed = per action 1..4 (proposed: the branch was entered, i.e. not
    skipped at :77, :127, :221), evaluations)."""
    xmin, xmax, ymin, ymax, zmin, zmax = prm.box
    zeta_scale = prm.zeta_scale
    sig_zeta = prm.zeta_scale * prm.sig / 100  # :22
    xr = (prm.sig / 100) * (xmax - xmin)  # :30-32
    yr = (prm.sig / 100) * (ymax - ymin)
    zr = (prm.sig / 100) * (zmax - zmin)
    T = prm.temperature
    prior = prm.prior
    pi = math.pi
    nev = [0]

    def ev(c):
        """evaluate (MCsub.jl:123-185) -> (phi, ptS, valid = 1)"""
        nev[0] += 1
        r = evaluate(ds.rayX, ds.rayY, ds.rayZ, ds.rayL, ds.rayU, ds.tS, ds.allSig, c, prm.debug_prior)
        return r["phi"], r["ptS"], 1

    def interp(c, x, y, z):
        """Interpolation(TD_parameters, model, [x], [y], [z])[1] (MCsub.jl:306-327)"""
        return float(interpolation(c, [x], [y], [z])[0][0])

    if forward is not None:
        forward_ev, interp = forward

        def ev(c):
            nev[0] += 1
            return forward_ev(c)

    x, y, z, zeta = (np.array(a, dtype=np.float64) for a in cells)
    if resume is None:
        phi, ptS, valid = ev((x, y, z, zeta))
    else:
        phi, ptS = resume  # :41-67: the checkpoint's model as it was saved, no evaluate
    start = (phi, ptS)
    steps, saved = [], []
    accepted, proposed = [0] * 5, [0] * 5
    model_num = 0
    alpha = 0  # :69
    for it in range(start_iter, start_iter + iters):
        u_action, u_accept, u_a, u_b, u_c, u_zeta, u_index = draws(it)
        n = len(x)  # model.nCells
        action = 1 + int(math.floor(4 * u_action))  # :72
        accept = 0  # :73-74
        outcome, margin = SKIPPED, None
        modeln = None
        if action == 1:  # birth
            if n < prm.max_cells:  # :77
                proposed[1] += 1
                xn = u_a * (xmax - xmin) + xmin  # :78-80
                yn = u_b * (ymax - ymin) + ymin
                zn = u_c * (zmax - zmin) + zmin
                czeta = interp((x, y, z, zeta), xn, yn, zn)  # :81, the current model
                zetanew = czeta + sig_zeta * normal_quantile(u_zeta)  # :82
                cn = (np.append(x, xn), np.append(y, yn), np.append(z, zn), np.append(zeta, zetanew))  # :84-89
                outcome = INVALID
                if prior == 1:
                    if zetanew > 0 and zetanew < zeta_scale:  # :92
                        phin, ptSn, valid = ev(cn)
                        alpha = (n / (n + 1)) * ((sig_zeta * math.sqrt(2 * pi)) / zeta_scale) * \
                            _exp(((czeta - zetanew) ** 2) / (2 * sig_zeta ** 2) - (phin - phi) / 2 / T)  # :96-97
                        outcome, margin = EVALUATED, _margin(u_accept, alpha)
                        alpha = min(1, alpha)
                    else:
                        valid = 0  # :103
                elif prior == 2:
                    phin, ptSn, valid = ev(cn)  # :106
                    alpha = (n / (n + 1)) * (sig_zeta / zeta_scale) * \
                        _exp(-(zetanew) ** 2 / (zeta_scale ** 2) + (czeta - zetanew) ** 2 / (2 * sig_zeta ** 2) -
                             (phin - phi) / 2 / T)  # :107-108
                    outcome, margin = EVALUATED, _margin(u_accept, alpha)
                    alpha = min(1, alpha)
                elif prior == 3:
                    if zetanew > 0:  # :111
                        phin, ptSn, valid = ev(cn)
                        alpha = (n / (n + 1)) * (math.sqrt(2 * pi) * sig_zeta / zeta_scale) * \
                            _exp(-zetanew / zeta_scale + (czeta - zetanew) ** 2 / (2 * sig_zeta ** 2) -
                                 (phin - phi) / 2 / T)  # :113-114
                        outcome, margin = EVALUATED, _margin(u_accept, alpha)
                        alpha = min(1, alpha)
                    else:
                        valid = 0  # :117
                if u_accept < alpha and valid == 1:  # :121
                    modeln = (cn, phin, ptSn)
        elif action == 2:  # death
            if n > prm.min_cells:  # :127
                proposed[2] += 1
                kill = int(math.floor(u_index * n))  # :128 (0-based)
                cn = tuple(np.delete(a, kill) for a in (x, y, z, zeta))  # :130-136
                phin, ptSn, valid = ev(cn)  # :141
                zetanew = interp(cn, x[kill], y[kill], z[kill])  # :146, the reduced model at the killed site
                outcome = INVALID
                if prior == 1:
                    alpha = (n / (n - 1)) * (zeta_scale / (sig_zeta * math.sqrt(2 * pi))) * \
                        _exp(-((zeta[kill] - zetanew) ** 2) / (2 * sig_zeta ** 2) - (phin - phi) / 2 / T)  # :151-152
                    outcome, margin = EVALUATED, _margin(u_accept, alpha)
                    alpha = min(1, alpha)
                elif prior == 2:
                    phin, ptSn, valid = ev(cn)  # :159
                    alpha = (n / (n - 1)) * (zeta_scale / sig_zeta) * \
                        _exp((zeta[kill] ** 2) / (2 * zeta_scale ** 2) -
                             (zeta[kill] - zetanew) ** 2 / (2 * sig_zeta ** 2) - (phin - phi) / 2 / T)  # :160-162
                    outcome, margin = EVALUATED, _margin(u_accept, alpha)
                    alpha = min(1, alpha)
                elif prior == 3:
                    if zetanew > 0:  # :165
                        alpha = (n / (n - 1)) * (zeta_scale / (math.sqrt(2 * pi) * sig_zeta)) * \
                            _exp(zeta[kill] / zeta_scale - (zeta[kill] - zetanew) ** 2 / (2 * sig_zeta ** 2) -
                                 (phin - phi) / 2 / T)  # :166-168
                        outcome, margin = EVALUATED, _margin(u_accept, alpha)
                        alpha = min(1, alpha)
                    else:
                        valid = 0  # :171
                if u_accept < alpha and valid == 1:  # :176
                    modeln = (cn, phin, ptSn)
        elif action == 3:  # change
            proposed[3] += 1
            change = int(math.floor(u_index * n))  # :184
            zetan = zeta[change] + sig_zeta * normal_quantile(u_zeta)  # :188
            zn_ = zeta.copy()
            zn_[change] = zetan  # :189
            cn = (x, y, z, zn_)
            phin, ptSn, valid = ev(cn)  # :191, before the validity check
            outcome = INVALID
            if prior == 1:
                if zetan > 0 and zetan < zeta_scale:  # :195
                    alpha = _exp(-(phin - phi) / 2 / T)  # :196
                    outcome, margin = EVALUATED, _margin(u_accept, alpha)
                    alpha = min(1, alpha)
                else:
                    valid = 0  # :199
            elif prior == 2:
                alpha = _exp((zeta[change] ** 2 - zetan ** 2) / (2 * zeta_scale ** 2) - (phin - phi) / 2 / T)  # :202-203
                outcome, margin = EVALUATED, _margin(u_accept, alpha)
                alpha = min(1, alpha)
            elif prior == 3:
                if zetan > 0:  # :206
                    alpha = _exp((zeta[change] - zetan) / zeta_scale - (phin - phi) / 2 / T)  # :207-208
                    outcome, margin = EVALUATED, _margin(u_accept, alpha)
                    alpha = min(1, alpha)
                else:
                    alpha = 0  # :211 (valid stays 1)
            if u_accept < alpha and valid == 1:  # :214
                modeln = (cn, phin, ptSn)
        elif action == 4:  # move
            if n > 0:  # :221
                proposed[4] += 1
                move = int(math.floor(u_index * n))  # :222
                xn = x[move] + xr * normal_quantile(u_a)  # :226-228
                yn = y[move] + yr * normal_quantile(u_b)
                zn = z[move] + zr * normal_quantile(u_c)
                outcome = INVALID
                if xmin <= xn <= xmax and ymin <= yn <= ymax and zmin <= zn <= zmax:  # :230-232
                    cn = (x.copy(), y.copy(), z.copy(), zeta)
                    cn[0][move], cn[1][move], cn[2][move] = xn, yn, zn  # :234-236
                    phin, ptSn, valid = ev(cn)  # :238
                    alpha = _exp(-(phin - phi) / 2 / T)  # :241
                    outcome, margin = EVALUATED, _margin(u_accept, alpha)
                    alpha = min(1, alpha)
                else:
                    valid = 0  # :244
                if u_accept < alpha and valid == 1:  # :247
                    modeln = (cn, phin, ptSn)
        if modeln is not None:  # model = deepcopy(modeln); model.accept = 1
            (x, y, z, zeta), phi, ptS = modeln
            accept = 1
            accepted[action] += 1
        s = Step()
        s.iter, s.action, s.accept, s.outcome, s.margin = it, action, accept, outcome, margin
        s.ncells, s.phi, s.ptS, s.cells = len(x), phi, ptS, (x, y, z, zeta)
        steps.append(s)
        if prm.burn_in is not None and prm.keep_each and it >= prm.burn_in:  # :276-281
            model_num += 1
            if model_num % int(prm.keep_each) == 0:
                saved.append(it)
    return dict(steps=steps, start=start, saved=saved, accepted=accepted[1:], proposed=proposed[1:],
                evaluations=nev[0])
