"""GPU: the posterior interfaces call does not depend on what its context did before, and leaves the context as
the next call expects it.  td_rasterize_interfaces / td_history_interfaces are declared in a header of their
own and are not in the catalogue of tests/context_ops.py; here they run before and after one catalogue
operation of every kind that shares their workspaces (ctx->raster, ctx->h_raster, ctx->vol, ctx->vol_grid), large
- small - large on one context, and after a resident server: every answer equals a fresh context's, which equals
the numpy restatement (tests/interfaces_ref.py), and every catalogue answer still equals its own reference."""
import numpy as np
import pytest

import context_ops as co
import interfaces_ref as iref

pytestmark = pytest.mark.gpu

REFS = co.References()
THR = (5.0, 20.0)
FIELDS = ("count", "any", "exceed", "jump", "mean", "std", "density", "skipped")
# (models, cells per model, lattice): the small one is swept by k_raster_brute in one slab, the large one by the
# bucket grids in slabs of 128 nodes with two column ranges (a plane of 180 nodes)
SHAPES = {"small": (6, 40, (5, 4, 3)), "large": (16, 300, (20, 9, 6))}


def inputs(which):
    nm, nc, (nx, ny, nz) = SHAPES[which]
    models = [co.cells(nc, 3000 + 10 * nm + k) for k in range(nm)]
    return models, np.linspace(-50.0, 1050.0, nx), np.linspace(-150.0, 450.0, ny), np.linspace(0.0, 660.0, nz)


def call(s, which):
    models, xs, ys, zs = inputs(which)
    s.ctx.set_volume_slab_nodes(co.FORCED_SLAB_NODES if which == "large" else 0)
    try:
        r = s.ctx.interfaces(models, xs, ys, zs, THR)
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
        models, xs, ys, zs = inputs(which)
        ref = iref.interfaces(models, xs, ys, zs, THR)
        nf, mid, _ = iref.contested(ref, len(models))
        assert mid > nf // 2
        assert co.same(out, tuple(ref[f] for f in FIELDS)), co.first_difference(out, tuple(ref[f] for f in FIELDS))
        _fresh[which] = out
    return _fresh[which]


def checked(s, which):
    out = call(s, which)
    n = s.resident_count()
    ref = fresh(which)
    assert co.same(out, ref), "interfaces (%s) differs from a fresh context's: %s" % (which, co.first_difference(out, ref))
    return n


@pytest.fixture
def session():
    s = co.Session()
    yield s
    s.close()


NEIGHBOURS = ["evaluate_300", "volume_16_forced", "covariance_16_auto", "predict_16_forced", "marginals_3probs_8bins_resident",
              "history_volume_2h"]


@pytest.mark.parametrize("name", NEIGHBOURS)
def test_before_and_after_a_catalogue_operation(name, session):
    o = co.BY_NAME[name]
    for which in ("large", "small"):
        assert checked(session, which) == 0
        co.run_checked(o, session, REFS)
        assert checked(session, which) == 0
        co.run_checked(o, session, REFS)


def test_large_small_large_on_one_context(session):
    for which in ("large", "small", "large", "small", "small", "large"):
        assert checked(session, which) == 0


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
    _, xs, ys, zs = inputs("small")
    want = s.ctx.interfaces(flat, xs, ys, zs, THR)
    ref = iref.interfaces(flat, xs, ys, zs, THR)
    assert co.same(tuple(want[f] for f in FIELDS), tuple(ref[f] for f in FIELDS))
    for name in ("history_covariance_2h", "history_rasterize_1h"):
        co.run_checked(co.BY_NAME[name], s, REFS)
        got = s.ctx.interfaces_history(hs, xs, ys, zs, THR)
        assert co.same(tuple(got[f] for f in FIELDS), tuple(want[f] for f in FIELDS)), name
        assert s.resident_count() == 0


def test_a_refused_call_leaves_the_next_answers_unchanged(session):
    s = session
    tt = co.tt()
    models, xs, ys, zs = inputs("small")
    assert checked(s, "small") == 0
    for bad in (lambda: s.ctx.interfaces(models, xs[::-1], ys, zs, THR),
                lambda: s.ctx.interfaces(models, xs, ys, zs, (np.nan,)),
                lambda: s.ctx.interfaces(models, xs, ys, zs, THR, want=()),
                lambda: s.ctx.interfaces([], xs, ys, zs, THR),
                lambda: s.ctx.interfaces_history([], xs, ys, zs, THR)):
        with pytest.raises(tt.TdError):
            bad()
        assert checked(s, "small") == 0
        co.run_checked(co.BY_NAME["volume_16_forced"], s, REFS)
    assert checked(s, "large") == 0
