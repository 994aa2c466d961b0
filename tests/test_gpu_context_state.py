"""GPU: an answer does not depend on what its context did before.

A caller keeps one context and calls evaluate, then plot_model_hist, then posterior_volume, then evaluate
again; the context carries grow-only workspaces carved up by the current call's shape, bucket counts zeroed
by one search for the next, a staged-cells flag, memcmp'd misfit inputs, a resident shadow chain and sticky
kernel attributes from call to call ("cross-call state").  Here every operation of
tests/context_ops.py runs after every other on one context -- ordered pairs, size ladders, seeded walks, two
contexts in turn, refused calls in between -- and every answer must equal, bit for bit, the operation's
answer on a fresh context that did nothing else, which in turn equals the CPU oracle's where there is one.
The resident-kernel contract of include/tdstar.h (the library stops this thread's resident kernels before
any call that launches other work) is held through tdt_resident_count."""
import ctypes

import numpy as np
import pytest

import context_ops as co

pytestmark = pytest.mark.gpu

REFS = co.References()  # computed once per (operation, sigma, edited model), shared by every test, never modified


@pytest.fixture
def session():
    s = co.Session()
    yield s
    s.close()


# ---------------------------------------------------------------- the references are not circular
@pytest.mark.parametrize("name", [o.name for o in co.OPS if o.oracle])
def test_fresh_context_reference_equals_the_cpu_oracle(name, orc):
    o = co.BY_NAME[name]
    for scale in (1.0, co.SIGMA_SCALE) if o.sigma else (1.0,):
        ref = REFS.get(o, scale)
        exp = o.oracle(np.asarray(co.rays().allSig, dtype=np.float64) * scale) if o.sigma else o.oracle()
        for k, v in exp.items():
            assert co.same(ref[k], v), "%s output %d at sigma x %g: %s" % (name, k, scale,
                                                                          co.first_difference((ref[k],), (v,)))


def test_edit_reference_equals_the_cpu_oracle(orc):
    """The reference of evaluate_edit_* (a full evaluate of the edited model, the incremental path off)."""
    ds = co.rays()
    for kind in ("move", "birth", "death"):
        prop = co.edited(co.cells(*co.EDIT_BASE), kind)
        ref = REFS.get(co.BY_NAME["evaluate_edit_" + kind], 1.0, prop)
        r = orc.evaluate(ds.rayX, ds.rayY, ds.rayZ, ds.rayL, ds.rayU, ds.tS, ds.allSig, prop)
        assert co.same(ref, (r["ptS"], r["phi"], r["likelihood"]))


# ---------------------------------------------------------------- pairs
PAIRS = co.pair_list()


@pytest.mark.parametrize("a", [o.name for o in co.OPS])
def test_pairs_a_then_b_then_a(a, session):
    """A, B, A on one context shared by every B of this A: each answer equals its reference."""
    A = co.BY_NAME[a]
    bs = [co.BY_NAME[y] for x, y in PAIRS if x == a]
    assert len(bs) >= len(co.FAMILIES)
    for B in bs:
        try:
            co.run_checked(A, session, REFS)
            co.run_checked(B, session, REFS)
            co.run_checked(A, session, REFS)
        except AssertionError as e:
            raise AssertionError("pair (%s, %s): %s" % (a, B.name, e)) from None


# ---------------------------------------------------------------- size ladders
LADDERS = [  # (large, small)
    ("evaluate_2500", "evaluate_63"), ("evaluate_2500_nearest", "evaluate_63_nearest"), ("evaluate_2500", "evaluate_300"),
    ("interpolate_700pt_1200cells", "interpolate_1pt_40cells"), ("interpolate_700pt_40cells", "interpolate_1pt_1200cells"),
    ("misfit_381_A", "misfit_100_A"), ("misfit_381_B", "misfit_100_A"),
    ("rasterize_per_model", "rasterize_one_model"), ("rasterize_batched", "rasterize_one_model"),
    ("rasterize_per_model", "rasterize_batched"),
    ("marginals_hist50", "marginals_3probs_nobins_resident"), ("marginals_3probs_8bins_streaming", "marginals_3probs_nobins_streaming"),
    ("convergence_2x40_lag0", "convergence_4x9_lag0"), ("convergence_2x40_lag5", "convergence_4x9_lag5"),
    ("convergence_models_2x40_lag0", "convergence_models_4x9_lag0"),
    ("volume_16_auto", "volume_8_auto"), ("volume_16_forced", "volume_8_forced"),
    ("predict_16_auto", "predict_8_auto"), ("predict_16_forced", "predict_8_forced"),
    ("covariance_16_auto", "covariance_8_auto"), ("covariance_16_forced", "covariance_8_forced"),
    ("chain_batch_5", "chain_batch_1"), ("chain_batch_5", "chain_batch_2"),
    ("trilinear_40x33x60_5000pts", "trilinear_2x2x2_50pts"), ("trilinear_4100x2x2_5000pts", "trilinear_4100x2x2_50pts"),
    ("trilinear_4100x2x2_5000pts", "trilinear_40x33x60_50pts"),
] + [("history_%s_2h" % n, "history_%s_1h" % n)
     for n in ("read", "rasterize", "marginals", "zeta_hist", "convergence", "volume", "predict", "covariance")]


@pytest.mark.parametrize("large,small", LADDERS)
def test_size_ladder(large, small, session):
    """large, small, large, small, then small, large, small, large on one context."""
    L, S = co.BY_NAME[large], co.BY_NAME[small]
    for o in (L, S, L, S, S, L, S, L):
        co.run_checked(o, session, REFS)


def test_every_operation_with_several_sizes_has_a_ladder():
    laddered = {co.BY_NAME[n].family for pair in LADDERS for n in pair}
    assert laddered >= set(co.FAMILIES) - {"evaluate_edit", "evaluate_batch", "set_sigma", "modifier"}


# ---------------------------------------------------------------- evaluate edits between everything
def test_evaluate_edits_between_everything(session):
    """evaluate(model), then 40 x (one random operation, one edit of the walk's model): every edit's answer
    equals a full evaluate on a second context with the incremental path off."""
    ref_ctx = co.Session()
    ref_ctx.ctx.set_incremental(0)
    rng = np.random.default_rng(2024)
    names = [o.name for o in co.LIGHT if not o.name.startswith(("set_sigma", "set_incremental"))]
    cur = co.cells(400, 11)
    incremental = 0
    try:
        a, b = session.ctx.evaluate(cur), ref_ctx.ctx.evaluate(cur)
        assert co.same(a[:3], b[:3])
        for step in range(40):
            o = co.BY_NAME[names[int(rng.integers(len(names)))]]
            co.run_checked(o, session, REFS)
            kind = ("move", "birth", "death")[int(rng.integers(3))]
            prop = co.edited(cur, kind)
            a = session.ctx.evaluate(prop)
            incremental += session.resident_count()
            b = ref_ctx.ctx.evaluate(prop)
            assert co.same(a[:3], b[:3]), (step, o.name, kind, co.first_difference(a[:3], b[:3]))
            if rng.random() < 0.6:
                cur = prop
    finally:
        ref_ctx.close()
    assert incremental > 0  # some edits were answered by the resident shadow


# ---------------------------------------------------------------- seeded walks
def walk(sessions, seed, steps, names):
    rng = np.random.default_rng(seed)
    done = []
    for step in range(steps):
        k = step % len(sessions)
        o = co.BY_NAME[names[int(rng.integers(len(names)))]]
        done.append("%s%s" % (o.name, "@%d" % k if len(sessions) > 1 else ""))
        try:
            co.run_checked(o, sessions[k], REFS)
        except AssertionError as e:
            print("seed %d, step %d, last three operations: %s" % (seed, step, done[-3:]))
            raise AssertionError("seed %d step %d after %s: %s" % (seed, step, done[-3:], e)) from None


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_seeded_walk(seed, session):
    """150 calls drawn from the whole catalogue, modifiers and heavy entries included."""
    walk([session], seed, 150, [o.name for o in co.OPS])


def test_two_contexts_alternating(session):
    """Two contexts on one thread, one operation each in turn (they share the thread's resident launches and
    td_trilinear's thread-local buffer)."""
    other = co.Session()
    try:
        walk([session, other], 77, 60, [o.name for o in co.LIGHT])
    finally:
        other.close()


# ---------------------------------------------------------------- refused calls change nothing
def refused(call, ctx_h=None):
    """The error code of a call the host refuses."""
    try:
        rc = call()
    except co.tt().TdError as e:
        return e.code
    return rc


def test_refused_calls_change_nothing(session):
    """Between two valid calls of an entry point, a call refused by an argument check that returns before
    any kernel or copy is issued (each read in the source: the check stands before the entry point's
    hipSetDevice): TD_ERR_ARG, and the next valid answer equals its reference."""
    t = co.tt()
    lib, P = t.lib(), t._lib.ptr
    s, ctx = session, session.ctx
    ARG = t._lib.TD_ERR_ARG
    other = co.Session()
    foreign = co.record(other, 71)
    empty = t.History(ctx, 2, 2 * co.HISTORY["max_cells"])
    models, q = co.marg_models(), co.queries(co.MARG_NODES, 32)
    nq = len(q[0])
    bad_off = np.array([0, 8, 5], dtype=np.int64)  # not monotone, at the second model
    c5 = [np.ascontiguousarray(a) for a in co.cells(10, 1)]
    mean, std = np.empty(nq), np.empty(nq)
    vol = t._lib.TdVolume(P(q[0]), P(q[1]), P(q[2]), nq, P(mean), P(std), None, None, None)
    phi = np.zeros(2)
    pred = t._lib.TdPredict(None, P(phi), None, None, None, None)
    covo = np.empty((1, nq))
    tgt = np.array([1.0])
    cov = t._lib.TdCovariance(P(q[0]), P(q[1]), P(q[2]), nq, P(tgt), P(tgt), P(tgt), 1, None, 0, P(covo), None,
                              None, None, None, None)
    hs = (ctypes.c_void_p * 1)(foreign.h)
    hist3 = np.zeros(23, dtype=np.int64)
    tiny = [tuple(np.array([float(k)]) for _ in range(4)) for k in range(ctx.marginals_resident_max() + 1)]

    def capacity():
        ch = co.chain_of(s, 300, 400, 71)
        h = t.History(ctx, 3, 3 * 400)
        try:
            return refused(lambda: ch.run_recorded(120, 10, 10, h)), len(h), ch.stats()["iterations"]
        finally:
            h.close()
            ch.close()

    def unsorted_knots():
        axes, values, pts = co.tri_inputs((40, 33, 60), 50)
        axes[1][[3, 4]] = axes[1][[4, 3]]
        out, n = np.empty(50), ctypes.c_int64()
        return lib.td_trilinear(ctx.device, P(axes[0]), 40, P(axes[1]), 33, P(axes[2]), 60,
                                P(np.ascontiguousarray(values.ravel(order="F"))), P(pts[0]), P(pts[1]), P(pts[2]), 50,
                                P(out), ctypes.byref(n))

    def too_many_for_the_resident_regime(call):
        def refusal():
            ctx.set_marginals_method(1)
            try:
                return refused(call)
            finally:
                ctx.set_marginals_method(0)
        return refusal

    q4 = tuple(a[:4] for a in q)

    cases = [  # (the valid operation around it, the refused call)
        ("marginals_3probs_8bins_resident", lambda: refused(lambda: ctx.marginals(models, *q, probs=(0.5, 1.5)))),
        ("marginals_3probs_8bins_streaming", lambda: refused(lambda: ctx.marginals(models, *q, probs=(np.nan,)))),
        ("marginals_hist50", lambda: refused(lambda: ctx.marginals(models, *q, bins=(co.MARG_MAX_BINS + 1, 0.0, 50.0)))),
        ("marginals_3probs_nobins_resident",
         too_many_for_the_resident_regime(lambda: ctx.marginals(tiny, *q4, probs=co.MARG_PROBS))),
        ("volume_8_forced", too_many_for_the_resident_regime(lambda: ctx.volume(tiny, *q4, bins=(8, 0.0, 50.0)))),
        ("predict_8_forced", too_many_for_the_resident_regime(lambda: ctx.predict(tiny, probs=co.MARG_PROBS))),
        ("history_marginals_1h", lambda: refused(lambda: ctx.marginals_history([foreign], *q, probs=(0.5,)))),
        ("rasterize_batched", lambda: lib.td_rasterize(ctx.h, 2, P(bad_off), *(P(a) for a in c5), P(q[0]), P(q[1]), P(q[2]),
                                                       nq, P(mean), P(std), None)),
        ("evaluate_batch", lambda: lib.td_evaluate_batch(ctx.h, 2, P(bad_off), *(P(a) for a in c5), None, P(phi), None)),
        ("volume_8_auto", lambda: lib.td_rasterize_volume(ctx.h, 2, P(bad_off), *(P(a) for a in c5), 0, None,
                                                          ctypes.byref(vol))),
        ("predict_8_auto", lambda: lib.td_rasterize_predict(ctx.h, 2, P(bad_off), *(P(a) for a in c5), 0, None,
                                                            ctypes.byref(pred))),
        ("covariance_8_auto", lambda: lib.td_rasterize_covariance(ctx.h, 2, P(bad_off), *(P(a) for a in c5),
                                                                  ctypes.byref(cov))),
        ("history_rasterize_1h", lambda: lib.td_history_rasterize(ctx.h, hs, 1, P(q[0]), P(q[1]), P(q[2]), nq, P(mean),
                                                                  P(std), None)),
        ("history_zeta_hist_1h", lambda: lib.td_history_zeta_hist(ctx.h, hs, 1, 20, 0.0, 50.0, P(hist3), None)),
        ("history_volume_1h", lambda: lib.td_history_volume(ctx.h, hs, 1, ctypes.byref(vol))),
        ("history_convergence_1h", lambda: refused(lambda: ctx.convergence_history([foreign], *q, max_lag=-1))),
        # only histories without a sample
        ("history_rasterize_1h", lambda: refused(lambda: ctx.rasterize_history([empty, empty], *q))),
        ("history_volume_1h", lambda: refused(lambda: ctx.volume_history([empty], *q))),
        ("history_predict_1h", lambda: refused(lambda: ctx.predict_history([empty]))),
        ("history_covariance_1h", lambda: refused(lambda: ctx.covariance_history([empty, empty], *q, targets=co.COV_TARGETS))),
        ("convergence_2x40_lag0", lambda: refused(lambda: ctx.convergence(co.conv_values((40, 40)), (40, 39)))),
        ("convergence_models_4x9_lag0", lambda: refused(lambda: ctx.convergence_models(co.conv_models((9,) * 4), (9, 9, 9, 3),
                                                                                         *co.queries(co.CONV_NODES, 61)))),
        ("history_record", lambda: capacity()[0]),
        ("trilinear_40x33x60_50pts", unsorted_knots),
        ("misfit_381_A", lambda: lib.td_misfit(ctx.h, -1, None, None, None, None, None)),
        ("evaluate_300", lambda: lib.td_evaluate(ctx.h, None, None, None, None, 5, 0, None, None, None, None)),
        ("interpolate_700pt_40cells", lambda: lib.td_interpolate(ctx.h, None, None, None, None, 0, P(q[0]), nq, P(q[1]),
                                                                 nq - 1, P(q[2]), nq, P(mean), None, None)),
    ]
    try:
        assert capacity() == (ARG, 0, 0)  # nothing ran: the history is empty, the chain has not moved
        for name, call in cases:
            o = co.BY_NAME[name]
            co.run_checked(o, s, REFS)
            rc = call()
            want = t._lib.TD_ERR_BOUNDS if name.startswith("interpolate") else ARG
            assert rc == want, (name, rc)
            co.run_checked(o, s, REFS)
        # a history without a sample between the two of the session: skipped, the two histories' answer
        h2 = co.session_histories(s, 2)
        between, hq = [h2[0], empty, h2[1]], co.queries(co.H_NODES, 75)
        routes = {
            "rasterize": lambda: ctx.rasterize_history(between, *hq, want_values=True),
            "volume": lambda: co.flat(ctx.volume_history(between, *hq, probs=co.MARG_PROBS, bins=(8, 0.0, 50.0),
                                                         convergence=True, want_values=True),
                                      ("mean", "std", "values", "quantiles", "hist", "rhat", "ess", "lags")),
            "predict": lambda: co.flat(ctx.predict_history(between, probs=co.MARG_PROBS, convergence=True, want_values=True),
                                       ("phi", "mean", "std", "ptS", "quantiles", "rhat", "ess", "lags")),
            "covariance": lambda: co.flat(ctx.covariance_history(between, *hq, targets=co.COV_TARGETS),
                                          ("cov", "corr", "mean", "std", "target_mean", "target_std")),
        }
        for name, route in routes.items():
            ref = REFS.get(co.BY_NAME["history_%s_2h" % name], s.sigma_scale)
            out = route()
            assert co.same(out, ref), (name, co.first_difference(out, ref))
    finally:
        empty.close()
        foreign.close()
        other.close()


# ---------------------------------------------------------------- the resident-kernel contract
def start_server(s):
    """evaluate, then one edit: td_evaluate's resident server answers the edit and stays."""
    base = co.cells(*co.EDIT_BASE)
    s.ctx.evaluate(base)
    s.last_cells = base
    assert co.run_checked(co.BY_NAME["evaluate_edit_move"], s, REFS, counted=True) == 1, \
        "td_evaluate's incremental path keeps its server"


GPU_OPS = [o.name for o in co.OPS if o.gpu]


@pytest.mark.parametrize("name", GPU_OPS)
def test_no_resident_kernel_survives_a_call_that_launches_other_work(name, session):
    """include/tdstar.h, td_set_incremental: "The library stops this thread's resident kernels before any
    call that launches other work".  With the shadow server up (and again with a tempering round's launch
    resident) every operation that issues GPU work returns with none registered -- except the calls
    documented to keep td_evaluate's server, which must keep it."""
    o = co.BY_NAME[name]
    for prelude in ("server", "ladder"):
        if prelude == "server":
            start_server(session)
        else:
            assert co.run_checked(co.BY_NAME["ladder_step"], session, REFS, counted=True) == 1, \
                "a tempering round leaves its launch resident"
        n = co.run_checked(o, session, REFS, counted=True)
        if name == "ladder_step" or (o.family == "evaluate_edit" and prelude == "server") or name == "chain_dropin":
            assert n == 1, (name, prelude, n)  # its own launch / the server it is documented to keep
        elif o.keeps:
            assert n <= 1, (name, prelude, n)  # td_evaluate: a full evaluate stops the server, an edit keeps it
        else:
            assert n == 0, "%s after a resident %s: %d resident launches registered on return" % (name, prelude, n)


def test_documented_keepers_keep_the_server(session):
    """td_evaluate's incremental path, the one-point td_interpolate on the shadow's model and a DROPIN chain's
    run keep the server (include/tdstar.h; csrc/chain.cpp td_chain_run)."""
    s = session
    start_server(s)
    prop = s.edit_prop
    v, _ = s.ctx.interpolate(prop, [prop[0][3]], [prop[1][3]], [prop[2][3]])
    assert v[0] == prop[3][3] and s.resident_count() == 1
    assert co.run_checked(co.BY_NAME["evaluate_edit_birth"], s, REFS, counted=True) == 1
    assert co.run_checked(co.BY_NAME["chain_dropin"], s, REFS, counted=True) == 1
    s.ctx.evaluate(co.cells(63, 103), want_nearest=True)  # the full path: other work
    assert s.resident_count() == 0
    s.ctx.set_incremental(1)  # a launch per call: nothing stays
    start = co.cells(*co.EDIT_BASE)
    s.ctx.evaluate(start)
    s.ctx.evaluate(co.edited(start, "move"))
    assert s.resident_count() == 0
