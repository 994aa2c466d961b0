"""GPU: the ensemble Gram and distance calls do not depend on what their context did before, and leave the context
as the next call expects it -- they share the volume workspace and the raster workspace with its pinned staging
with the volume, covariance, regions and comparison calls, and keep their M x M accumulators in the raster
workspace, which nothing zeroes between calls.  td_rasterize_gram / td_history_gram are declared in a header of
their own and are not in the catalogue of tests/context_ops.py; here they run before and after one catalogue
operation of every kind that shares their workspaces, before and after a comparison call, large - small - large on
one context, after a resident server and after refused calls: every answer equals a fresh context's, which equals
the numpy restatement (tests/gram_ref.py), and every catalogue answer still equals its own reference."""
import numpy as np
import pytest

import compare_ref as cr
import context_ops as co
import gram_ref as gref

pytestmark = pytest.mark.gpu

REFS = co.References()
FIELDS = ("gram", "dist2", "mean", "std", "wsum")
# (models, cells per model, points): the small one is swept by k_raster_brute in one slab and fills a corner of one
# tile, the large one by the bucket grids in slabs of 128 points (the accumulators go through the workspace three
# times) and fills two tiles of 64 rows
SHAPES = {"small": (6, 40, 70), "large": (70, 300, 300)}


def inputs(which):
    nm, nc, n = SHAPES[which]
    models = [co.cells(nc, 9100 + 10 * nm + k) for k in range(nm)]
    px, py, pz = co.queries(n, 70 + nm)
    w = np.random.default_rng(80 + nm).uniform(0.5, 2.0, n)
    return models, px, py, pz, w


def call(s, which):
    models, px, py, pz, w = inputs(which)
    s.ctx.set_volume_slab_nodes(co.FORCED_SLAB_NODES if which == "large" else 0)
    try:
        r = s.ctx.gram(models, px, py, pz, w)
    finally:
        s.ctx.set_volume_slab_nodes(0)
    return tuple(r[f] for f in FIELDS)


_fresh = {}


def fresh(which):
    """The call's answer on a context that did nothing else, held to the numpy restatement; made once."""
    if which not in _fresh:
        f = co.Session()
        try:
            out = call(f, which)
        finally:
            f.close()
        ref = gref.gram(*inputs(which))
        M = SHAPES[which][0]
        assert np.all(ref["dist2"][~np.eye(M, dtype=bool)] > 0) and np.all(np.diag(ref["gram"]) > 0)
        assert all(gref.same_bits(a, ref[f]) for a, f in zip(out, FIELDS)), co.first_difference(out, tuple(ref[f] for f in FIELDS))
        _fresh[which] = out
    return _fresh[which]


def checked(s, which):
    out = call(s, which)
    n = s.resident_count()
    ref = fresh(which)
    assert co.same(out, ref), "gram (%s) differs from a fresh context's: %s" % (which, co.first_difference(out, ref))
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
        co.run_checked(o, session, REFS)


def test_before_and_after_a_compare_call(session):
    """Not in the catalogue: held to its own restatement here.  It sorts into the raster workspace where the
    matrices' accumulators lie."""
    s = session
    A, B = cr.inputs("ties", 257, 1000, 7)
    want = cr.reference("ties", 257, 1000, 7)
    for which in ("large", "small"):
        assert checked(s, which) == 0
        r = s.ctx.compare_values(A, B, cr.EXCEED, want=("counts", "ks"))
        assert cr.differences(r, want) == []
        assert checked(s, which) == 0


def test_large_small_large_on_one_context(session):
    """The small call's matrices lie where the large call's queries and slab lay, and the other way round: the first
    slab starts its accumulators itself, so stale workspace never shows."""
    for which in ("large", "small", "large", "small", "small", "large"):
        assert checked(session, which) == 0
    for form in (2, 1, 0):
        co.tt().TdContext.set_gram_form(form)
        try:
            assert checked(session, "large") == 0 and checked(session, "small") == 0
        finally:
            co.tt().TdContext.set_gram_form(0)


def test_it_stops_a_resident_server(session):
    """After evaluate_edit_* td_evaluate's server is resident; the call launches other work, so none is on return
    (include/tdstar.h, td_set_incremental), and the next edit is still answered right."""
    s = session
    base = co.cells(*co.EDIT_BASE)
    s.ctx.evaluate(base)
    s.last_cells = base
    assert co.run_checked(co.BY_NAME["evaluate_edit_move"], s, REFS, counted=True) == 1
    assert checked(s, "small") == 0 and s.resident_count() == 0
    assert co.run_checked(co.BY_NAME["evaluate_edit_birth"], s, REFS, counted=True) == 1
    assert checked(s, "large") == 0


def test_histories_on_a_used_context(session):
    """The history entry point on the session's recorded histories, between catalogue history operations, equals
    the array entry point on the samples read back."""
    s = session
    hs = co.session_histories(s, 2)
    flat = [m.cells() for h in hs for m in h.read()]
    _, px, py, pz, w = inputs("small")
    want = s.ctx.gram(flat, px, py, pz, w)
    ref = gref.gram(flat, px, py, pz, w)
    assert all(gref.same_bits(want[f], ref[f]) for f in FIELDS)
    for name in ("history_covariance_2h", "history_rasterize_1h"):
        co.run_checked(co.BY_NAME[name], s, REFS)
        got = s.ctx.gram_history(hs, px, py, pz, w)
        assert co.same(tuple(got[f] for f in FIELDS), tuple(want[f] for f in FIELDS)), name
        assert s.resident_count() == 0


def test_a_refused_call_leaves_the_next_answers_unchanged(session):
    s = session
    tt = co.tt()
    models, px, py, pz, w = inputs("small")
    assert checked(s, "small") == 0
    for bad in (lambda: s.ctx.gram(models, px, py, pz, -w),
                lambda: s.ctx.gram(models, px, py, pz, np.where(np.arange(len(w)) == 3, np.nan, w)),
                lambda: s.ctx.gram(models, np.where(np.arange(len(px)) == 5, np.inf, px), py, pz, w),
                lambda: s.ctx.gram([], px, py, pz, w),
                lambda: s.ctx.gram_history([], px, py, pz, w),
                lambda: s.ctx.gram([(np.zeros(1),) * 4] * 11586, px, py, pz, w, want=("dist2",))):
        with pytest.raises(tt.TdError):
            bad()
        assert checked(s, "small") == 0
        co.run_checked(co.BY_NAME["volume_16_forced"], s, REFS)
    assert checked(s, "large") == 0
