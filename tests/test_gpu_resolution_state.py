"""GPU: the posterior resolution call does not depend on what its context did before, and leaves the context as the next
call expects it -- its ring of blocks, its rows and its tables lie in the raster workspace and its search structure in
the volume workspace, which the volume, predictive, covariance, interfaces, regions, support and recovery calls use too.
td_rasterize_resolution / td_history_resolution are declared in a header of their own and are not in the catalogue of
tests/context_ops.py; here they run before and after one catalogue operation of every kind that shares their workspaces
(volume, predict, covariance, an evaluate, a chain run), before and after an interfaces, a regions, a support and a
recovery call, large - small - large on one context and after a refused call: every answer equals a fresh context's,
which equals the numpy restatement (tests/resolution_ref.py), and every other answer still equals its own reference."""
import numpy as np
import pytest

import context_ops as co
import interfaces_ref as iref
import recovery_ref as cref
import regions_ref as rref
import resolution_ref as sref
import support_ref as uref

pytestmark = pytest.mark.gpu

REFS = co.References()
# (models, cells per model, lattice, its box, lags): the small one is swept by k_raster_brute in one block, the large one
# by the bucket grids in blocks of 128 nodes, three of them resident (its cells are about 125 km wide: nodes 60 km apart)
SHAPES = {"small": (6, 40, (5, 4, 3), ((0.0, 1000.0), (-200.0, 400.0), (0.0, 660.0)), (2, 1, 1)),
          "large": (16, 300, (9, 8, 6), ((200.0, 700.0), (-50.0, 300.0), (150.0, 500.0)), (2, 2, 2))}


def inputs(which):
    nm, nc, shape, box, lags = SHAPES[which]
    models = [co.cells(nc, 8100 + 10 * nm + k) for k in range(nm)]
    lat = tuple(np.linspace(lo, hi, n) for (lo, hi), n in zip(box, shape))
    w = np.random.default_rng(400 + nm).uniform(0.5, 2.0, shape[0] * shape[1] * shape[2])
    return models, lat, co.tt().resolution_offsets(lags), w


def call(s, which):
    models, lat, off, w = inputs(which)
    s.ctx.set_volume_slab_nodes(co.FORCED_SLAB_NODES if which == "large" else 0)
    try:
        r = s.ctx.resolution(models, *lat, off, 0.5, w, want=co.tt().TdContext.RES_ALL)
    finally:
        s.ctx.set_volume_slab_nodes(0)
    return tuple(r[f] for f in sref.FIELDS)


_fresh = {}


def fresh(which):
    """The call's answer on a context that did nothing else, held to the numpy restatement; made once."""
    if which not in _fresh:
        f = co.Session()
        try:
            out = call(f, which)
        finally:
            f.close()
        models, lat, off, w = inputs(which)
        ref = sref.resolution(models, *lat, off, 0.5, w)
        share, ended, censored = sref.vacuity(ref, off, *(len(v) for v in lat))
        assert 0.05 < share < 0.95 and ended > 0 and censored > 0, (share, ended, censored)
        want = tuple(ref[f] for f in sref.FIELDS)
        assert co.same(out, want), co.first_difference(out, want)
        _fresh[which] = out
    return _fresh[which]


def checked(s, which):
    out = call(s, which)
    n = s.resident_count()
    ref = fresh(which)
    assert co.same(out, ref), "resolution (%s) differs from a fresh context's: %s" % (which, co.first_difference(out, ref))
    return n


@pytest.fixture
def session():
    s = co.Session()
    yield s
    s.close()


NEIGHBOURS = ["volume_16_forced", "predict_16_forced", "covariance_16_forced", "evaluate_300", "chain_device_lds0",
              "history_volume_2h"]


@pytest.mark.parametrize("name", NEIGHBOURS)
def test_before_and_after_a_catalogue_operation(name, session):
    o = co.BY_NAME[name]
    for which in ("large", "small"):
        assert checked(session, which) == 0
        co.run_checked(o, session, REFS)
        assert checked(session, which) == 0
        co.run_checked(o, session, REFS)


def test_before_and_after_the_calls_with_headers_of_their_own(session):
    """Interfaces, regions, support and recovery are not in the catalogue: each is held to its own restatement here,
    after a resolution call, and the resolution call after each of them to its fresh answer."""
    s = session
    models = [co.cells(40, 7200 + k) for k in range(6)]
    px, py, pz = co.queries(90, 56)
    off = np.array([0, 1, 30, 90])
    lat = (np.linspace(0.0, 1000.0, 5), np.linspace(-200.0, 400.0, 4), np.linspace(0.0, 660.0, 3))
    truth = np.random.default_rng(57).uniform(5.0, 45.0, len(px))
    iface = iref.interfaces(models, *lat, (5.0,))
    reg = rref.regions(models, px, py, pz, off, None, True)
    reg_fields = ("series", "weight", "mean", "std", "greater")
    ds = co.rays()
    _, rx, ry, rz = uref.csr_points(np.asarray(ds.rayX), np.asarray(ds.rayY), np.asarray(ds.rayZ))
    sup_models = [m[:3] for m in models]
    sup = uref.support(sup_models, rx, ry, rz, None, px, py, pz, thr=(0.0,))
    sup_fields = ("cell", "count", "barren", "orphans", "mean", "std", "exceed")
    rec = cref.recovery(models, px, py, pz, truth, off, None, True)
    for which in ("large", "small"):
        assert checked(s, which) == 0
        r = s.ctx.interfaces(models, *lat, (5.0,))
        assert co.same(tuple(r[f] for f in iref.FIELDS), tuple(iface[f] for f in iref.FIELDS))
        assert checked(s, which) == 0
        r = s.ctx.regions(models, px, py, pz, off)
        assert co.same(tuple(r[f] for f in reg_fields), tuple(reg[f] for f in reg_fields))
        assert checked(s, which) == 0
        r = s.ctx.support(sup_models, None, px, py, pz, thresholds=(0.0,))
        assert co.same(tuple(r[f] for f in sup_fields), tuple(sup[f] for f in sup_fields))
        assert checked(s, which) == 0
        r = s.ctx.recovery(models, px, py, pz, truth, off)
        assert co.same(tuple(r[f] for f in cref.FIELDS), tuple(rec[f] for f in cref.FIELDS))
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
    T = co.tt().TdContext
    hs = co.session_histories(s, 2)
    flat = [m.cells() for h in hs for m in h.read()]
    _, lat, off, w = inputs("small")
    want = s.ctx.resolution(flat, *lat, off, 0.5, w, want=T.RES_ALL)
    ref = sref.resolution(flat, *lat, off, 0.5, w)
    assert co.same(tuple(want[f] for f in sref.FIELDS), tuple(ref[f] for f in sref.FIELDS))
    for name in ("history_covariance_2h", "history_rasterize_1h"):
        co.run_checked(co.BY_NAME[name], s, REFS)
        got = s.ctx.resolution_history(hs, *lat, off, 0.5, w, want=T.RES_ALL)
        assert co.same(tuple(got[f] for f in sref.FIELDS), tuple(want[f] for f in sref.FIELDS)), name
        assert s.resident_count() == 0


def test_a_refused_call_leaves_the_next_answers_unchanged(session):
    s = session
    tt = co.tt()
    models, lat, off, w = inputs("small")
    assert checked(s, "small") == 0
    for bad in (lambda: s.ctx.resolution(models, *lat, [(1, 0, 0), (-1, 0, 0)], 0.5, w),
                lambda: s.ctx.resolution(models, *lat, off, np.nan, w),
                lambda: s.ctx.resolution(models, *lat, off, 0.5, np.where(np.arange(len(w)) == 3, np.inf, w)),
                lambda: s.ctx.resolution(models, lat[0][::-1], lat[1], lat[2], off, 0.5, w),
                lambda: s.ctx.resolution(models, *lat, off, 0.5, w, want=()),
                lambda: s.ctx.resolution([], *lat, off, 0.5, w),
                lambda: s.ctx.resolution_history([], *lat, off, 0.5, w)):
        with pytest.raises(tt.TdError):
            bad()
        assert checked(s, "small") == 0
        co.run_checked(co.BY_NAME["volume_16_forced"], s, REFS)
    assert checked(s, "large") == 0
