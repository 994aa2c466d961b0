"""GPU: the posterior regions call does not depend on what its context did before, and leaves the context as the
next call expects it.  td_rasterize_regions / td_history_regions are declared in a header of their own and are not
in the catalogue of tests/context_ops.py; here they run before and after one catalogue operation of every kind
that shares their workspaces (ctx->raster, ctx->h_raster, ctx->vol, ctx->vol_grid, ctx->marg, ctx->conv), before and
after an interfaces call, large - small - large on one context, after a resident server and after a refused call:
every answer equals a fresh context's, which equals the numpy restatement (tests/regions_ref.py), and every
catalogue answer still equals its own reference."""
import numpy as np
import pytest

import context_ops as co
import interfaces_ref as iref
import regions_ref as rref

pytestmark = pytest.mark.gpu

REFS = co.References()
FIELDS = ("series", "weight", "mean", "std", "greater", "quantiles", "hist")
PROBS, BINS = (0.1, 0.5, 0.9), (8, 0.0, 40.0)
# (models, cells per model, region sizes): the small one is swept by k_raster_brute in one slab, the large one by
# the bucket grids in slabs of 128 columns, which cut its leaves (1500 = 750 + 750)
SHAPES = {"small": (6, 40, (1, 20, 3)), "large": (16, 300, (70, 1500, 2, 300))}


def inputs(which):
    nm, nc, sizes = SHAPES[which]
    models = [co.cells(nc, 5000 + 10 * nm + k) for k in range(nm)]
    n = sum(sizes)
    px, py, pz = co.queries(n, 50 + nm)
    w = np.random.default_rng(60 + nm).uniform(0.5, 2.0, n)
    return models, px, py, pz, np.concatenate(([0], np.cumsum(sizes))), w


def call(s, which):
    models, px, py, pz, off, w = inputs(which)
    s.ctx.set_volume_slab_nodes(co.FORCED_SLAB_NODES if which == "large" else 0)
    try:
        r = s.ctx.regions(models, px, py, pz, off, w, True, PROBS, BINS)
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
        models, px, py, pz, off, w = inputs(which)
        ref = rref.regions(models, px, py, pz, off, w, True)
        assert all(len(set(ref["series"][:, r].tolist())) == len(models) for r in range(len(off) - 1))
        assert co.same(out[:5], tuple(ref[f] for f in FIELDS[:5])), co.first_difference(out[:5], tuple(ref[f] for f in FIELDS[:5]))
        assert np.allclose(out[5], np.quantile(ref["series"], PROBS, axis=0), rtol=1e-12, atol=0)
        assert np.all(out[6].sum(axis=1) == len(models))
        _fresh[which] = out
    return _fresh[which]


def checked(s, which):
    out = call(s, which)
    n = s.resident_count()
    ref = fresh(which)
    assert co.same(out, ref), "regions (%s) differs from a fresh context's: %s" % (which, co.first_difference(out, ref))
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


def test_before_and_after_an_interfaces_call(session):
    """The interfaces call is not in the catalogue either: it is held to its own restatement here."""
    s = session
    models = [co.cells(40, 7000 + k) for k in range(6)]
    xs, ys, zs = np.linspace(-50.0, 1050.0, 5), np.linspace(-150.0, 450.0, 4), np.linspace(0.0, 660.0, 3)
    ref = iref.interfaces(models, xs, ys, zs, (5.0,))
    want = tuple(ref[f] for f in iref.FIELDS)
    for which in ("large", "small"):
        assert checked(s, which) == 0
        r = s.ctx.interfaces(models, xs, ys, zs, (5.0,))
        assert co.same(tuple(r[f] for f in iref.FIELDS), want)
        assert checked(s, which) == 0


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
    _, px, py, pz, off, w = inputs("small")
    want = s.ctx.regions(flat, px, py, pz, off, w, True, PROBS, BINS)
    ref = rref.regions(flat, px, py, pz, off, w, True)
    assert co.same(tuple(want[f] for f in FIELDS[:5]), tuple(ref[f] for f in FIELDS[:5]))
    for name in ("history_covariance_2h", "history_rasterize_1h"):
        co.run_checked(co.BY_NAME[name], s, REFS)
        got = s.ctx.regions_history(hs, px, py, pz, off, w, True, PROBS, BINS)
        assert co.same(tuple(got[f] for f in FIELDS), tuple(want[f] for f in FIELDS)), name
        assert s.resident_count() == 0


def test_a_refused_call_leaves_the_next_answers_unchanged(session):
    s = session
    tt = co.tt()
    models, px, py, pz, off, w = inputs("small")
    assert checked(s, "small") == 0
    bad_off = off.copy()
    bad_off[1] = bad_off[2]
    for bad in (lambda: s.ctx.regions(models, px, py, pz, bad_off, w),
                lambda: s.ctx.regions(models, px, py, pz, off, np.where(np.arange(len(w)) == 3, np.nan, w)),
                lambda: s.ctx.regions(models, px, py, pz, off, w, probs=(1.5,)),
                lambda: s.ctx.regions([], px, py, pz, off, w),
                lambda: s.ctx.regions_history([], px, py, pz, off, w)):
        with pytest.raises(tt.TdError):
            bad()
        assert checked(s, "small") == 0
        co.run_checked(co.BY_NAME["volume_16_forced"], s, REFS)
    assert checked(s, "large") == 0
