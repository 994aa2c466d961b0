"""GPU: the posterior comparison (include/tdstar_compare.h) against its numpy restatements (tests/compare_ref.py).
Every output is compared for equality: integers as integers, ks_at bit for bit.  td_compare_values on the shapes and
inputs of compare_ref (one model a side, non-powers of two, the wave and tile edges, the 1024 and 4096 edges; ties,
distinct values, NaN / inf / zeros of both signs / denormals, identical samples, disjoint samples), at the limit of
16384 models a side, and with the sides swapped; td_rasterize_compare on ensembles swept by the brute-force kernel and
by the bucket grids, in one slab and in three, against the restatement on the two sides' value matrices and against
the volume of each side alone; td_history_compare on recorded histories against the array entry point."""
import numpy as np
import pytest

import compare_ref as cr
import context_ops as co

pytestmark = pytest.mark.gpu

RANKS = ("counts", "ks")
PROBS, BINS = (0.1, 0.5, 0.9), (8, 0.0, 60.0)


@pytest.fixture(scope="module")
def session():
    s = co.Session()
    yield s
    s.close()


@pytest.mark.parametrize("shape", cr.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("kind", cr.KINDS)
def test_values_against_the_restatement(session, kind, shape):
    A, B = cr.inputs(kind, *shape)
    want = cr.reference(kind, *shape)
    got = session.ctx.compare_values(A, B, cr.EXCEED, want=RANKS)
    assert cr.differences(got, want) == []
    assert np.array_equal(got["exceed"][0], got["greater"])  # the pair (1, 0)
    if kind == "ties":
        assert got["equal"].sum() > 0
    if kind == "identical":
        assert not got["ks_plus"].any() and not got["ks_minus"].any() and np.isnan(got["ks_at"]).all()
    if kind == "hostile" and shape[2] >= 4:
        na, nb = np.isnan(A), np.isnan(B)
        assert np.any(na.all(axis=0) & nb.all(axis=0)) and np.any(na.any(axis=0) & ~nb.any(axis=0))
    if kind == "hostile" and A.size + B.size >= 200:
        zeros = np.concatenate((A[A == 0], B[B == 0]))
        assert np.any(np.signbit(zeros)) and np.any(~np.signbit(zeros))


@pytest.mark.parametrize("shape", [(1, 5, 3), (63, 65, 65), (257, 1000, 7)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("kind", ["ties", "hostile"])
def test_swapping_the_sides(session, kind, shape):
    A, B = cr.inputs(kind, *shape)
    ab, ba = session.ctx.compare_values(A, B, want=RANKS), session.ctx.compare_values(B, A, want=RANKS)
    sw = cr.swapped(ab)
    assert cr.differences(ba, sw, tuple(sw)) == []


def test_single_outputs_and_the_sides_statistics_of_values(session):
    """Each group of outputs alone gives what it gives with the others; the sides' statistics of a host matrix are
    the volume kernels' (held here to numpy within rounding; bit for bit against ``volume`` below)."""
    A, B = cr.inputs("distinct", 63, 65, 65)
    want = cr.reference("distinct", 63, 65, 65)
    ctx = session.ctx
    r = ctx.compare_values(A, B, want="counts")
    assert cr.differences(r, want, ("less", "equal", "greater")) == [] and r["ks_plus"] is None and r["mean_a"] is None
    r = ctx.compare_values(A, B, want="ks")
    assert cr.differences(r, want, ("ks_plus", "ks_minus", "ks_at")) == [] and r["less"] is None
    r = ctx.compare_values(A, B, cr.EXCEED, want=())
    assert cr.same(r["exceed"], want["exceed"]) and r["less"] is None and r["ks_at"] is None
    r = ctx.compare_values(A, B, probs=(0.5,), bins=(4, -1.0, 1.0), want="stats")
    for side, V in (("a", A), ("b", B)):
        assert np.allclose(r["mean_" + side], V.mean(axis=0), rtol=1e-13, atol=1e-15)
        assert np.allclose(r["std_" + side], V.std(axis=0, ddof=1), rtol=1e-12)
        assert np.allclose(r["quantiles_" + side][0], np.median(V, axis=0), rtol=1e-14)
        assert np.all(r["hist_" + side].sum(axis=1) == V.shape[0])


@pytest.mark.parametrize("form", [(1, 64, 64), (0, 1024, 1024), (1, 256, 128)], ids=str)
def test_the_forms_of_the_kernels_agree(session, form):
    """Either placement of the sort kernel's columns and any number of threads: the same answer."""
    tt = co.tt()
    try:
        tt.TdContext.set_compare_form(*form)
        for kind, shape in (("hostile", (1025, 130, 66)), ("ties", (64, 64, 130)), ("distinct", (1, 5, 3))):
            got = session.ctx.compare_values(*cr.inputs(kind, *shape), cr.EXCEED, want=RANKS)
            assert cr.differences(got, cr.reference(kind, *shape)) == [], (kind, shape)
    finally:
        tt.TdContext.set_compare_form()


def test_the_limit_of_a_side(session):
    rng = np.random.default_rng(16384)
    A = np.round(rng.standard_normal((16384, 2)), 2)
    B = np.round(rng.standard_normal((16384, 2)) * 1.2 + 0.1, 2)
    A[5, 0], B[7, 1], A[9, 1] = np.nan, np.inf, -0.0
    got = session.ctx.compare_values(A, B, cr.EXCEED, want=RANKS)
    want = cr.by_sorting(A, B)
    assert cr.differences(got, want) == []
    assert want["equal"].min() > 0 and want["less"].sum() > 2 ** 27
    tt = co.tt()
    for a, b in ((np.zeros((16385, 1)), B[:, :1]), (A[:, :1], np.zeros((16385, 1)))):
        with pytest.raises(tt.TdError, match="holds 16385 models"):
            session.ctx.compare_values(a, b)
    again = session.ctx.compare_values(A, B, cr.EXCEED, want=RANKS)  # a refused call changed nothing
    assert cr.differences(again, want) == []


def test_no_column_is_in_order(session):
    r = session.ctx.compare_values(np.zeros((3, 0)), np.zeros((2, 0)))
    assert r["less"].shape == (0,)


def ensembles(ncells):
    """37 and 150 models; B holds five of A's."""
    rng = np.random.default_rng(ncells or 60)
    size = (lambda: int(rng.integers(5, 61))) if ncells is None else (lambda: ncells)
    A = [co.cells(size(), 9100 + k) for k in range(37)]
    B = [co.cells(size(), 9300 + k) for k in range(145)] + A[3:8]
    return A, B


@pytest.mark.parametrize("ncells", [None, 300], ids=["brute", "grids"])
def test_ensembles_in_one_slab_and_in_three(session, ncells):
    ctx = session.ctx
    A, B = ensembles(ncells)
    qx, qy, qz = co.queries(130, 77)
    auto = ctx.compare(A, B, qx, qy, qz, cr.EXCEED, PROBS, BINS)
    counters = ctx.volume_counters()
    assert (counters[3] == 187 * 130) == (ncells is None)  # the brute-force kernel took every pair, or none
    ctx.set_volume_slab_nodes(64)
    try:
        forced = ctx.compare(A, B, qx, qy, qz, cr.EXCEED, PROBS, BINS)
    finally:
        ctx.set_volume_slab_nodes(0)
    fields = cr.FIELDS + tuple(f + s for s in "ab" for f in ("mean_", "std_", "quantiles_", "hist_"))
    assert cr.differences(forced, auto, fields) == []
    va, vb = (ctx.volume(m, qx, qy, qz, PROBS, BINS, want_values=True) for m in (A, B))
    want = cr.brute(va["values"], vb["values"])
    assert cr.differences(auto, want) == []
    assert want["equal"].min() > 0 and np.any(want["less"] > 0) and np.any(want["greater"] > 0)
    assert np.any(want["ks_plus"] > 0) and np.any(want["ks_minus"] > 0)
    for side, v in (("a", va), ("b", vb)):  # each side's numbers are the volume's of that side alone, bit for bit
        for f in ("mean", "std", "quantiles", "hist"):
            assert cr.same(auto[f + "_" + side], v[f]), (side, f)


def test_posterior_compare_on_a_small_lattice():
    """The public function: lattice-shaped outputs in ``posterior_volume``'s node order, and the derived quantities."""
    tt = co.tt()
    ds, prm = co.rays(), tt.define_TDstructrure()
    A = [tt.random_model(40, 500 + k) for k in range(6)]
    B = [tt.random_model(40, 600 + k) for k in range(9)] + A[:2]
    xs, ys, zs = np.linspace(0.0, 1000.0, 5), np.linspace(-100.0, 400.0, 4), np.linspace(0.0, 600.0, 3)
    pairs, bins = ((1.0, 0.0), (2.0, 0.0)), (4, 0.0, 50.0)
    out = tt.posterior_compare(A, [B[:5], B[5:]], ds, prm, exceed=pairs, probs=(0.5,), bins=bins, xs=xs, ys=ys, zs=zs)
    qx, qy, qz = np.tile(xs, 12), np.tile(np.repeat(ys, 5), 3), np.repeat(zs, 20)  # x fastest
    r = tt.context_for(ds).compare([m.cells() for m in A], [m.cells() for m in B], qx, qy, qz, pairs, (0.5,), bins)
    assert (out["MA"], out["MB"]) == (6, 11) and out["equal"].min() >= 2
    for f in cr.FIELDS[:3] + cr.FIELDS[4:] + ("mean_a", "std_b"):
        assert out[f].shape == (5, 4, 3) and cr.same(out[f].transpose(2, 1, 0).ravel(), r[f]), f
    assert out["exceed"].shape == (2, 5, 4, 3) and cr.same(out["exceed"][1].transpose(2, 1, 0).ravel(), r["exceed"][1])
    assert out["hist_a"].shape == (5, 4, 3, 7) and cr.same(out["hist_b"].transpose(2, 1, 0, 3).reshape(60, 7), r["hist_b"])
    assert out["quantiles_a"].shape == (1, 5, 4, 3)
    assert np.array_equal(out["prob_greater"], (out["greater"] + 0.5 * out["equal"]) / 66.0)
    assert np.array_equal(out["prob_exceed"][0], out["greater"] / 66.0)
    assert np.array_equal(out["ks"], np.maximum(out["ks_plus"], out["ks_minus"]) / 66.0)
    assert np.array_equal(out["ks_sign"], np.sign(out["ks_plus"] - out["ks_minus"]))
    assert np.array_equal(out["mean_diff"], out["mean_a"] - out["mean_b"])
    assert out["info_gain_bits"].shape == (5, 4, 3) and np.all(out["info_gain_bits"] >= 0)


def test_histories_against_the_models_read_back(session):
    """Side A: three histories of short recorded chains, one of them empty; side B: a debug_prior = 1 history recorded
    on another context of the device."""
    tt = co.tt()
    s = session
    other = co.Session()
    hs = []
    try:
        hs = [co.record(s, 81), tt.History(s.ctx, 4, 4 * 400), co.record(s, 82)]
        prm = tt.define_TDstructrure().replace(debug_prior=1, max_cells=100)
        ch = tt.Chain(other.ctx, tt.chain_params(prm, None, seed=83, chain=1, engine=tt.TD_ENGINE_DEVICE))
        prior = tt.History(other.ctx, 20, 20 * 100)
        hs.append(prior)
        try:
            ch.run_recorded(400, 20, 20, prior)
        finally:
            ch.close()
        assert len(hs[1]) == 0 and len(prior) == 20
        A = [m.cells() for h in hs[:3] for m in h.read()]
        B = [m.cells() for m in prior.read()]
        qx, qy, qz = co.queries(130, 78)
        want = s.ctx.compare(A, B, qx, qy, qz, cr.EXCEED, PROBS, BINS)
        got = s.ctx.compare_history(hs[:3], [prior], qx, qy, qz, cr.EXCEED, PROBS, BINS)
        fields = cr.FIELDS + tuple(f + side for side in "ab" for f in ("mean_", "std_", "quantiles_", "hist_"))
        assert cr.differences(got, want, fields) == []
        assert np.any(want["less"] > 0) and np.any(want["greater"] > 0) and len(A) == 24
        assert s.resident_count() == 0
    finally:
        for h in hs:
            h.close()
        other.close()
