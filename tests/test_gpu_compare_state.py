"""GPU: the posterior comparison calls do not depend on what their context did before, and leave the context as the
next call expects it -- they share the volume workspace, the raster workspace and its pinned staging, and the
marginals' workspace with the volume, predictive, covariance, regions, support and recovery calls.  The entry points
of include/tdstar_compare.h are declared in a header of their own and are not in the catalogue of
tests/context_ops.py; here they run before and after a catalogue operation of every kind that shares their workspaces,
before and after a recovery call, large - small - large on one context, after a resident server and after refused
calls: every answer equals a fresh context's, which equals the numpy restatement (tests/compare_ref.py) on the two
sides' volumes, and every catalogue answer still equals its own reference."""
import numpy as np
import pytest

import compare_ref as cr
import context_ops as co
import recovery_ref as rref

pytestmark = pytest.mark.gpu

REFS = co.References()
PROBS, BINS = (0.1, 0.5, 0.9), (8, 0.0, 60.0)
FIELDS = cr.FIELDS + tuple(f + s for s in "ab" for f in ("mean_", "std_", "quantiles_", "hist_"))
# (models of A, of B, cells per model, nodes): the small one is swept by k_raster_brute in one slab, the large one by
# the bucket grids in slabs of 128 nodes
SHAPES = {"small": (5, 9, 40, 70), "large": (12, 20, 300, 300)}


def inputs(which):
    na, nb, nc, nq = SHAPES[which]
    A = [co.cells(nc, 8500 + 10 * na + k) for k in range(na)]
    B = [co.cells(nc, 8700 + 10 * nb + k) for k in range(nb - 2)] + A[:2]
    return (A, B) + co.queries(nq, 210 + na)


def call(s, which):
    A, B, qx, qy, qz = inputs(which)
    s.ctx.set_volume_slab_nodes(co.FORCED_SLAB_NODES if which == "large" else 0)
    try:
        r = s.ctx.compare(A, B, qx, qy, qz, cr.EXCEED, PROBS, BINS)
    finally:
        s.ctx.set_volume_slab_nodes(0)
    return tuple(r[f] for f in FIELDS)


def values_call(s):
    A, B = cr.inputs("ties", 257, 1000, 7)
    r = s.ctx.compare_values(A, B, cr.EXCEED, want=("counts", "ks"))
    assert cr.differences(r, cr.reference("ties", 257, 1000, 7)) == []


_fresh = {}


def fresh(which):
    """The call's answer on a context that did nothing else, held to the numpy restatement; made once."""
    if which not in _fresh:
        f = co.Session()
        try:
            out = call(f, which)
            A, B, qx, qy, qz = inputs(which)
            va, vb = (f.ctx.volume(m, qx, qy, qz, PROBS, BINS, want_values=True) for m in (A, B))
        finally:
            f.close()
        want = cr.brute(va["values"], vb["values"])
        assert want["equal"].min() > 0 and np.any(want["less"] > 0) and np.any(want["greater"] > 0)
        want.update({f + "_" + side: v[f] for side, v in (("a", va), ("b", vb)) for f in ("mean", "std", "quantiles", "hist")})
        got = dict(zip(FIELDS, out))
        assert cr.differences(got, want, FIELDS) == []
        _fresh[which] = out
    return _fresh[which]


def checked(s, which):
    out = call(s, which)
    n = s.resident_count()
    ref = fresh(which)
    assert co.same(out, ref), "compare (%s) differs from a fresh context's: %s" % (which, co.first_difference(out, ref))
    return n


@pytest.fixture
def session():
    s = co.Session()
    yield s
    s.close()


NEIGHBOURS = ["evaluate_300", "volume_16_forced", "covariance_16_auto", "history_volume_2h"]


@pytest.mark.parametrize("name", NEIGHBOURS)
def test_before_and_after_a_catalogue_operation(name, session):
    o = co.BY_NAME[name]
    for which in ("large", "small"):
        assert checked(session, which) == 0
        co.run_checked(o, session, REFS)
        assert checked(session, which) == 0
        values_call(session)
        co.run_checked(o, session, REFS)


def test_before_and_after_a_recovery_call(session):
    """Not in the catalogue: held to its own restatement here.  It overwrites the value matrix's place in the raster
    workspace with the error D; the comparison sorts into the same workspace."""
    s = session
    models = [co.cells(40, 7100 + k) for k in range(6)]
    px, py, pz = co.queries(90, 55)
    truth = np.random.default_rng(3).uniform(5.0, 45.0, 90)
    off = np.array([0, 1, 30, 90])
    ref = rref.recovery(models, px, py, pz, truth, off, None, True)
    for which in ("large", "small"):
        assert checked(s, which) == 0
        r = s.ctx.recovery(models, px, py, pz, truth, off, None, True)
        assert co.same(tuple(r[f] for f in rref.FIELDS), tuple(ref[f] for f in rref.FIELDS))
        assert checked(s, which) == 0
        values_call(s)


def test_large_small_large_on_one_context(session):
    for which in ("large", "small", "large", "small", "small", "large"):
        assert checked(session, which) == 0
    values_call(session)
    assert checked(session, "large") == 0


def test_around_an_incremental_evaluate(session):
    """After evaluate_edit_* td_evaluate's server is resident; the call launches other work, so none is on return
    (include/tdstar.h, td_set_incremental), and the next edit is still answered right."""
    s = session
    base = co.cells(*co.EDIT_BASE)
    s.ctx.evaluate(base)
    s.last_cells = base
    assert co.run_checked(co.BY_NAME["evaluate_edit_move"], s, REFS, counted=True) == 1
    assert checked(s, "small") == 0 and s.resident_count() == 0
    assert co.run_checked(co.BY_NAME["evaluate_edit_birth"], s, REFS, counted=True) == 1
    values_call(s)
    assert s.resident_count() == 0
    co.run_checked(co.BY_NAME["evaluate_edit_death"], s, REFS)
    assert checked(s, "large") == 0 and s.resident_count() == 0


def test_a_refused_call_leaves_the_next_answers_unchanged(session):
    s = session
    tt = co.tt()
    A, B, qx, qy, qz = inputs("small")
    assert checked(s, "small") == 0
    for bad in (lambda: s.ctx.compare(A, B, qx, qy, qz, exceed=((0.0, 1.0),)),
                lambda: s.ctx.compare(A, B, qx, qy, qz, exceed=((1.0, np.nan),)),
                lambda: s.ctx.compare(A, B, qx, qy, qz, probs=(1.5,)),
                lambda: s.ctx.compare(A, B, qx, qy, qz, exceed=[(1.0, 0.0)] * 17),
                lambda: s.ctx.compare(A, B, qx, qy, qz, want=()),
                lambda: s.ctx.compare([], B, qx, qy, qz),
                lambda: s.ctx.compare(A, [], qx, qy, qz),
                lambda: s.ctx.compare_history([], [], qx, qy, qz),
                lambda: s.ctx.compare_values(np.zeros((16385, 1)), np.zeros((3, 1)))):
        with pytest.raises(tt.TdError):
            bad()
        assert checked(s, "small") == 0
        co.run_checked(co.BY_NAME["volume_16_forced"], s, REFS)
    assert checked(s, "large") == 0
