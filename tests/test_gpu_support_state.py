"""GPU: the posterior support call does not depend on what its context did before, and leaves the context as the
next call expects it -- it overwrites the fourth component of the volume workspace's cell block, which the volume,
predictive, covariance, interfaces and regions calls read.  td_rasterize_support / td_history_support are declared
in a header of their own and are not in the catalogue of tests/context_ops.py; here they run before and after one
catalogue operation of every kind that shares their workspaces (an evaluate, a chain run, predict, volume, an
incremental td_evaluate), before and after a regions call, large - small - large on one context, after a resident
server and after a refused call: every answer equals a fresh context's, which equals the numpy restatement
(tests/support_ref.py), and every catalogue answer still equals its own reference."""
import numpy as np
import pytest

import context_ops as co
import regions_ref as rref
import support_ref as sref

pytestmark = pytest.mark.gpu

REFS = co.References()
FIELDS = ("cell", "count", "barren", "orphans", "values", "mean", "std", "exceed", "quantiles", "hist")
PROBS, BINS, THR = (0.1, 0.5, 0.9), (8, 0.0, 2.0), (0.0, 0.3)
# (models, cells per model, nodes): the small one is swept by k_raster_brute in one slab, the large one by the bucket
# grids in slabs of 128 ray points (132 of them) and nodes
SHAPES = {"small": (6, 40, 70), "large": (16, 300, 300)}


@pytest.fixture(scope="module")
def points():
    """The valid points of the session's rays and their t* weights."""
    ds = co.rays()
    _, px, py, pz = sref.csr_points(np.asarray(ds.rayX), np.asarray(ds.rayY), np.asarray(ds.rayZ))
    return px, py, pz, co.tt().support_weights(ds, "tstar")


def inputs(which):
    nm, nc, nq = SHAPES[which]
    models = [co.cells(nc, 6000 + 10 * nm + k)[:3] for k in range(nm)]
    return models, co.queries(nq, 90 + nm)


def call(s, which, w):
    models, q = inputs(which)
    s.ctx.set_volume_slab_nodes(co.FORCED_SLAB_NODES if which == "large" else 0)
    try:
        r = s.ctx.support(models, w, *q, thresholds=THR, probs=PROBS, bins=BINS, want_values=True)
    finally:
        s.ctx.set_volume_slab_nodes(0)
    return tuple(r[f] for f in FIELDS)


_fresh = {}


def fresh(which, points):
    """The call's answer on a context that did nothing else, held to the numpy restatement; made once."""
    if which not in _fresh:
        px, py, pz, w = points
        f = co.Session()
        try:
            out = call(f, which, w)
        finally:
            f.close()
        models, q = inputs(which)
        ref = sref.support(models, px, py, pz, w, *q, thr=THR)
        # barren cells in every model, a cell one wave collides on, and at half the nodes the models disagree (a node
        # whose cell is barren in every model has sigma 0)
        assert np.all(ref["barren"] > 0) and ref["count"].max() >= 64 and np.mean(ref["std"] > 0) > 0.5
        assert all(np.any((x > 0) & (x < len(models))) for x in ref["exceed"])
        want = tuple(ref[f] for f in FIELDS[:8])
        assert co.same(out[:8], want), co.first_difference(out[:8], want)
        assert np.allclose(out[8], np.quantile(ref["values"], PROBS, axis=0), rtol=1e-12, atol=0)
        assert np.all(out[9].sum(axis=1) == len(models))
        _fresh[which] = out
    return _fresh[which]


def checked(s, which, points):
    out = call(s, which, points[3])
    n = s.resident_count()
    ref = fresh(which, points)
    assert co.same(out, ref), "support (%s) differs from a fresh context's: %s" % (which, co.first_difference(out, ref))
    return n


@pytest.fixture
def session():
    s = co.Session()
    yield s
    s.close()


NEIGHBOURS = ["evaluate_300", "chain_device_lds0", "predict_16_forced", "volume_16_forced", "history_volume_2h"]


@pytest.mark.parametrize("name", NEIGHBOURS)
def test_before_and_after_a_catalogue_operation(name, session, points):
    o = co.BY_NAME[name]
    for which in ("large", "small"):
        assert checked(session, which, points) == 0
        co.run_checked(o, session, REFS)
        assert checked(session, which, points) == 0
        co.run_checked(o, session, REFS)


def test_before_and_after_a_regions_call(session, points):
    """The regions call is not in the catalogue either: it is held to its own restatement here.  It reads the cells'
    fourth component, which the support call before it has overwritten in the workspace."""
    s = session
    models = [co.cells(40, 7100 + k) for k in range(6)]
    px, py, pz = co.queries(90, 55)
    off = np.array([0, 1, 30, 90])
    ref = rref.regions(models, px, py, pz, off, None, True)
    want = tuple(ref[f] for f in ("series", "weight", "mean", "std", "greater"))
    for which in ("large", "small"):
        assert checked(s, which, points) == 0
        r = s.ctx.regions(models, px, py, pz, off)
        assert co.same(tuple(r[f] for f in ("series", "weight", "mean", "std", "greater")), want)
        assert checked(s, which, points) == 0


def test_large_small_large_on_one_context(session, points):
    for which in ("large", "small", "large", "small", "small", "large"):
        assert checked(session, which, points) == 0


def test_around_an_incremental_evaluate(session, points):
    """After evaluate_edit_* td_evaluate's server is resident; the call launches other work, so none is on return
    (include/tdstar.h, td_set_incremental), and the next edit is still answered right."""
    s = session
    base = co.cells(*co.EDIT_BASE)
    s.ctx.evaluate(base)
    s.last_cells = base
    assert co.run_checked(co.BY_NAME["evaluate_edit_move"], s, REFS, counted=True) == 1
    assert checked(s, "small", points) == 0 and s.resident_count() == 0
    assert co.run_checked(co.BY_NAME["evaluate_edit_birth"], s, REFS, counted=True) == 1
    assert checked(s, "large", points) == 0
    co.run_checked(co.BY_NAME["evaluate_edit_death"], s, REFS)


def test_histories_on_a_used_context(session, points):
    """The history entry point on the session's recorded histories, between catalogue history operations, equals
    the array entry point on the samples read back."""
    s = session
    px, py, pz, w = points
    hs = co.session_histories(s, 2)
    flat = [m.cells() for h in hs for m in h.read()]
    _, q = inputs("small")
    kw = dict(thresholds=THR, probs=PROBS, bins=BINS, want_values=True)
    want = s.ctx.support(flat, w, *q, **kw)
    ref = sref.support(flat, px, py, pz, w, *q, thr=THR)
    assert co.same(tuple(want[f] for f in FIELDS[:8]), tuple(ref[f] for f in FIELDS[:8]))
    for name in ("history_covariance_2h", "history_rasterize_1h"):
        co.run_checked(co.BY_NAME[name], s, REFS)
        got = s.ctx.support_history(hs, w, *q, **kw)
        assert co.same(tuple(got[f] for f in FIELDS), tuple(want[f] for f in FIELDS)), name
        assert s.resident_count() == 0


def test_a_refused_call_leaves_the_next_answers_unchanged(session, points):
    s = session
    tt = co.tt()
    w = points[3]
    models, q = inputs("small")
    assert checked(s, "small", points) == 0
    for bad in (lambda: s.ctx.support(models, np.where(np.arange(len(w)) == 3, np.nan, w)),
                lambda: s.ctx.support(models, w, *q, probs=(1.5,)),
                lambda: s.ctx.support(models, w, q[0], q[1], np.full(len(q[0]), np.inf)),
                lambda: s.ctx.support([], w),
                lambda: s.ctx.support_history([], w)):
        with pytest.raises(tt.TdError):
            bad()
        assert checked(s, "small", points) == 0
        co.run_checked(co.BY_NAME["volume_16_forced"], s, REFS)
    assert checked(s, "large", points) == 0
