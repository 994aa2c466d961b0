"""GPU: the posterior recovery call does not depend on what its context did before, and leaves the context as the next
call expects it -- it shares the volume workspace and the raster workspace (whose value matrix it overwrites with the
error D in place) with the volume, predictive, covariance, interfaces, regions and support calls.
td_rasterize_recovery / td_history_recovery are declared in a header of their own and are not in the catalogue of
tests/context_ops.py; here they run before and after one catalogue operation of every kind that shares their
workspaces (an evaluate, a chain run, predict, volume, an incremental td_evaluate), before and after a regions call
and a support call, large - small - large on one context and after a refused call: every answer equals a fresh
context's, which equals the numpy restatement (tests/recovery_ref.py), and every catalogue answer still equals its own
reference."""
import numpy as np
import pytest

import context_ops as co
import recovery_ref as cref
import regions_ref as rref
import support_ref as sref

pytestmark = pytest.mark.gpu

REFS = co.References()
FIELDS = cref.FIELDS + ("quantiles", "hist")
PROBS, BINS = (0.1, 0.5, 0.9), (8, 0.0, 1500.0)
# (models, cells per model, points, region sizes): the small one is swept by k_raster_brute in one slab, the large one
# by the bucket grids in slabs of 128 points, which cut the leaves of the region of 1100 points
SHAPES = {"small": (6, 40, (1, 20, 49)), "large": (16, 300, (1, 7, 70, 1100, 122))}


def inputs(which):
    nm, nc, sizes = SHAPES[which]
    models = [co.cells(nc, 8000 + 10 * nm + k) for k in range(nm)]
    px, py, pz = co.queries(sum(sizes), 190 + nm)
    rng = np.random.default_rng(300 + nm)
    return models, px, py, pz, rng.uniform(5.0, 45.0, len(px)), np.concatenate(([0], np.cumsum(sizes))), rng.uniform(0.5, 2.0, len(px))


def call(s, which):
    models, px, py, pz, truth, off, w = inputs(which)
    s.ctx.set_volume_slab_nodes(co.FORCED_SLAB_NODES if which == "large" else 0)
    try:
        r = s.ctx.recovery(models, px, py, pz, truth, off, w, True, PROBS, BINS)
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
        models, px, py, pz, truth, off, w = inputs(which)
        ref = cref.recovery(models, px, py, pz, truth, off, w, True)
        M = len(models)
        assert np.any((ref["below"] > 0) & (ref["above"] > 0)) and np.mean(ref["dstd"] > 0) > 0.5
        assert all(len(set(ref["series"][:, r].tolist())) > M // 2 for r in range(len(off) - 1))
        n = len(cref.FIELDS)
        want = tuple(ref[f] for f in cref.FIELDS)
        assert co.same(out[:n], want), co.first_difference(out[:n], want)
        assert np.allclose(out[n], np.quantile(ref["series"], PROBS, axis=0), rtol=1e-12, atol=0)
        assert np.all(out[n + 1].sum(axis=1) == M)
        _fresh[which] = out
    return _fresh[which]


def checked(s, which):
    out = call(s, which)
    n = s.resident_count()
    ref = fresh(which)
    assert co.same(out, ref), "recovery (%s) differs from a fresh context's: %s" % (which, co.first_difference(out, ref))
    return n


@pytest.fixture
def session():
    s = co.Session()
    yield s
    s.close()


NEIGHBOURS = ["evaluate_300", "chain_device_lds0", "predict_16_forced", "volume_16_forced", "history_volume_2h"]


@pytest.mark.parametrize("name", NEIGHBOURS)
def test_before_and_after_a_catalogue_operation(name, session):
    o = co.BY_NAME[name]
    for which in ("large", "small"):
        assert checked(session, which) == 0
        co.run_checked(o, session, REFS)
        assert checked(session, which) == 0
        co.run_checked(o, session, REFS)


def test_before_and_after_a_regions_call_and_a_support_call(session):
    """Neither is in the catalogue: each is held to its own restatement here.  The regions call reads the value matrix's
    place in the workspace, where the recovery call has left D; the support call overwrites the cells' fourth
    component in the volume workspace, which the recovery call's sweep reads."""
    s = session
    models = [co.cells(40, 7100 + k) for k in range(6)]
    px, py, pz = co.queries(90, 55)
    off = np.array([0, 1, 30, 90])
    ref = rref.regions(models, px, py, pz, off, None, True)
    want = tuple(ref[f] for f in ("series", "weight", "mean", "std", "greater"))
    ds = co.rays()
    _, rx, ry, rz = sref.csr_points(np.asarray(ds.rayX), np.asarray(ds.rayY), np.asarray(ds.rayZ))
    sup_models = [m[:3] for m in models]
    sup_ref = sref.support(sup_models, rx, ry, rz, None, px, py, pz, thr=(0.0,))
    sup_fields = ("cell", "count", "barren", "orphans", "mean", "std", "exceed")
    for which in ("large", "small"):
        assert checked(s, which) == 0
        r = s.ctx.regions(models, px, py, pz, off)
        assert co.same(tuple(r[f] for f in ("series", "weight", "mean", "std", "greater")), want)
        assert checked(s, which) == 0
        u = s.ctx.support(sup_models, None, px, py, pz, thresholds=(0.0,))
        assert co.same(tuple(u[f] for f in sup_fields), tuple(sup_ref[f] for f in sup_fields))
        assert checked(s, which) == 0


def test_large_small_large_on_one_context(session):
    for which in ("large", "small", "large", "small", "small", "large"):
        assert checked(session, which) == 0


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
    assert checked(s, "large") == 0
    co.run_checked(co.BY_NAME["evaluate_edit_death"], s, REFS)


def test_histories_on_a_used_context(session):
    """The history entry point on the session's recorded histories, between catalogue history operations, equals
    the array entry point on the samples read back."""
    s = session
    hs = co.session_histories(s, 2)
    flat = [m.cells() for h in hs for m in h.read()]
    _, px, py, pz, truth, off, w = inputs("small")
    want = s.ctx.recovery(flat, px, py, pz, truth, off, w, True, PROBS, BINS)
    ref = cref.recovery(flat, px, py, pz, truth, off, w, True)
    assert co.same(tuple(want[f] for f in cref.FIELDS), tuple(ref[f] for f in cref.FIELDS))
    for name in ("history_covariance_2h", "history_rasterize_1h"):
        co.run_checked(co.BY_NAME[name], s, REFS)
        got = s.ctx.recovery_history(hs, px, py, pz, truth, off, w, True, PROBS, BINS)
        assert co.same(tuple(got[f] for f in FIELDS), tuple(want[f] for f in FIELDS)), name
        assert s.resident_count() == 0


def test_a_refused_call_leaves_the_next_answers_unchanged(session):
    s = session
    tt = co.tt()
    models, px, py, pz, truth, off, w = inputs("small")
    assert checked(s, "small") == 0
    for bad in (lambda: s.ctx.recovery(models, px, py, pz, np.where(np.arange(len(px)) == 3, np.nan, truth), off, w),
                lambda: s.ctx.recovery(models, px, py, pz, truth, off, w, probs=(1.5,)),
                lambda: s.ctx.recovery(models, px, py, np.full(len(px), np.inf), truth, off, w),
                lambda: s.ctx.recovery(models, px, py, pz, truth, [0, 5, 5, len(px)], w),
                lambda: s.ctx.recovery([], px, py, pz, truth, off, w),
                lambda: s.ctx.recovery_history([], px, py, pz, truth, off, w)):
        with pytest.raises(tt.TdError):
            bad()
        assert checked(s, "small") == 0
        co.run_checked(co.BY_NAME["volume_16_forced"], s, REFS)
    assert checked(s, "large") == 0
