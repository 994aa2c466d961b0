"""GPU: the ensemble Gram and distance matrices (td_rasterize_gram, td_history_gram) against the numpy restatement of
their definition (tests/gram_ref.py), bit for bit, NaN positions included: the inputs on which the association shows
in the bits (tests/test_gram_host.py) under every slab size, sweep, kernel form, weighting and choice of outputs, the
tails of the pair kernel's tiles in models and of its blocks in points, awkward models and weights, the history
form, the statistics against the volume's, and the size limit."""
import numpy as np
import pytest

import gram_ref as gref

pytestmark = pytest.mark.gpu

FIELDS = ("gram", "dist2", "mean", "std")
FORMS = (1, 2)


@pytest.fixture(scope="module")
def sds(tt):
    return tt.synthetic_rays(24, seed=1)


@pytest.fixture(scope="module")
def ctx(tt, sds):
    c = tt.TdContext.from_datastruct(sds)
    yield c
    c.set_volume_slab_nodes(0)
    c.set_volume_method(tt.TdContext.VOL_AUTO)
    tt.TdContext.set_gram_form(0)
    c.close()


def same(r, ref, fields=FIELDS):
    for f in fields:
        a, b = r[f], ref[f]
        assert a.shape == b.shape and a.dtype == b.dtype, (f, a.shape, b.shape, a.dtype, b.dtype)
        bad = ~((a == b) & (np.signbit(a) == np.signbit(b)) | ((a != a) & (b != b)))
        assert not bad.any(), "%s: %d of %d differ, first at %s: %r against %r" % (
            f, bad.sum(), a.size, np.argwhere(bad)[0], a[bad][0], b[bad][0])
    assert r["wsum"] == ref["wsum"]


def settings(tt, ctx, slabs=(64, 128, 0), methods=None, forms=FORMS):
    """Every (slab, method, form), the context set accordingly and put back at the end."""
    methods = (tt.TdContext.VOL_GRID, tt.TdContext.VOL_BRUTE) if methods is None else methods
    try:
        for slab in slabs:
            for method in methods:
                for form in forms:
                    ctx.set_volume_slab_nodes(slab)
                    ctx.set_volume_method(method)
                    tt.TdContext.set_gram_form(form)
                    yield slab, method, form
    finally:
        ctx.set_volume_slab_nodes(0)
        ctx.set_volume_method(tt.TdContext.VOL_AUTO)
        tt.TdContext.set_gram_form(0)


# ---------------------------------------------------------------- the base case

@pytest.fixture(scope="module")
def base():
    models, px, py, pz, w = gref.base_case()
    ref = {wt: gref.gram(models, px, py, pz, w if wt else None) for wt in (True, False)}
    return dict(models=models, px=px, py=py, pz=pz, w=w, ref=ref)


@pytest.mark.parametrize("weighted", [True, False])
def test_base_case_whatever_the_slab_the_sweep_and_the_form(tt, ctx, base, weighted):
    """1301 points (20 blocks of 64 and one of 21), 70 models (two tiles of 64, one of 128): slabs of 64 and 128 points
    cut the list 21 and 11 times, the last slab holding the partial block.  The association test of
    test_gram_host.py holds for these very inputs, so another order of summation cannot pass."""
    ref = base["ref"][weighted]
    M, npts = len(base["models"]), len(base["px"])
    args = (base["models"], base["px"], base["py"], base["pz"], base["w"] if weighted else None)
    runs = []
    for slab, method, form in settings(tt, ctx):
        ctx.timing(enable=True, reset=True)
        try:
            r = ctx.gram(*args)
            nslabs = tt.TdContext.gram_plan(M, npts, 0, slab)[1]
            assert nslabs == (-(-npts // slab) if slab else 1)
            assert ctx.timing(kernel="gram_pairs")[0] == nslabs and ctx.timing(kernel="gram_centre")[0] == nslabs
            assert ctx.timing(kernel="gram_mirror")[0] == 1 and ctx.timing(kernel="raster_stats")[0] == nslabs
        finally:
            ctx.timing(enable=False)
        c = ctx.volume_counters()
        assert (c[3] == M * npts and sum(c[:3]) == 0) if method == tt.TdContext.VOL_BRUTE else (c[3] == 0), c
        runs.append(r)
    runs.append(ctx.gram(*args))  # automatic in all three, and a repeated call
    for r in runs:
        same(r, ref)
    # each output alone equals the two together
    for form in FORMS:
        tt.TdContext.set_gram_form(form)
        try:
            for slab in (128, 0):
                ctx.set_volume_slab_nodes(slab)
                for want in ("gram", "dist2"):
                    r = ctx.gram(*args, want=(want,))
                    other = "dist2" if want == "gram" else "gram"
                    assert r[other] is None
                    same(r, ref, (want, "mean", "std"))
        finally:
            tt.TdContext.set_gram_form(0)
            ctx.set_volume_slab_nodes(0)
    none = ctx.gram(*args, want=())
    same(none, ref, ("mean", "std"))
    if not weighted:  # NULL weights are an array of ones, bit for bit
        ones = ctx.gram(base["models"], base["px"], base["py"], base["pz"], np.ones(npts))
        same(ones, runs[0])
        assert ones["wsum"] == float(npts)


# ---------------------------------------------------------------- the tails of the tiles and of the blocks

def case(seed, M, npts, lo=40, hi=300):
    rng = np.random.default_rng(seed)
    models = gref.make_models(rng, M, lo, hi)
    return (models,) + gref.make_points(rng, npts)


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 127, 128, 129, 130])
def test_model_count_tails(tt, ctx, M):
    """One below, at and above the edge of both forms' tiles (64 and 128 rows), two tiles and two, and the smallest
    ensembles; 200 points: three blocks and one of 8, in slabs of 64 and in one.  M = 1 gives NaN sigma, as
    k_raster_stats does, and a matrix of one +0.0."""
    assert {tt.TdContext.gram_tile(f) for f in FORMS} == {64, 128}
    models, px, py, pz, w = case(900 + M, M, 200)
    ref = gref.gram(models, px, py, pz, w)
    if M > 1:
        assert np.all(np.isfinite(ref["std"])) and np.all(ref["dist2"][~np.eye(M, dtype=bool)] > 0)
    else:
        assert np.isnan(ref["std"]).all() and ref["gram"].tolist() == [[0.0]] and ref["dist2"].tolist() == [[0.0]]
    for slab, method, form in settings(tt, ctx, slabs=(64, 0), methods=(tt.TdContext.VOL_AUTO,)):
        same(ctx.gram(models, px, py, pz, w), ref)


@pytest.mark.parametrize("npts", [1, 63, 64, 65, 129])
def test_point_count_tails(tt, ctx, npts):
    """A single point, one short of a block, a block, a block and one, two blocks and one (a slab of 64 then holds a
    single point); 67 models: a tile and three rows."""
    models, px, py, pz, w = case(950 + npts, 67, npts)
    ref = gref.gram(models, px, py, pz, w)
    for slab, method, form in settings(tt, ctx, slabs=(64, 0), methods=(tt.TdContext.VOL_AUTO,)):
        same(ctx.gram(models, px, py, pz, w), ref)


# ---------------------------------------------------------------- awkward models, points and weights

def test_special_cases(tt, ctx):
    """A model without cells (0.0 everywhere), duplicate models (distance exactly +0.0 off the diagonal, equal rows
    of gram), zero weights (their points contribute +0.0, their mean and std are still the volume's) and, in a
    second ensemble, a NaN zeta that wins somewhere: the mean there is NaN, so every model's X and every entry."""
    rng = np.random.default_rng(78)
    models = gref.make_models(rng, 20, 5, 30)
    models[3] = (np.zeros(0),) * 4
    models[11] = tuple(a.copy() for a in models[4])
    px, py, pz, w = gref.make_points(rng, 150)
    w[[0, 17, 63, 64, 149]] = 0.0
    ref = gref.gram(models, px, py, pz, w)
    assert not ref["values"][3].any() and ref["X"][3].any()
    assert ref["dist2"][4][11] == 0.0 and not np.signbit(ref["dist2"][4][11]) and np.array_equal(ref["gram"][4], ref["gram"][11])
    assert np.count_nonzero(ref["dist2"] == 0.0) == 20 + 2 and not ref["X"][:, 17].any() and ref["std"][17] > 0
    for slab, method, form in settings(tt, ctx, slabs=(64, 0)):
        same(ctx.gram(models, px, py, pz, w), ref)
    nan_models = [tuple(a.copy() for a in m) for m in models]
    nan_models[5][3][2] = np.nan
    qx, qy, qz = px.copy(), py.copy(), pz.copy()
    qx[70], qy[70], qz[70] = (nan_models[5][k][2] for k in range(3))  # the NaN cell itself, so that it wins there
    ref = gref.gram(nan_models, qx, qy, qz, w)
    assert np.isnan(ref["values"][5][70]) and np.isnan(ref["mean"][70]) and np.isnan(ref["gram"]).all() and np.isnan(ref["dist2"]).all()
    for slab, method, form in settings(tt, ctx, slabs=(64, 0), methods=(tt.TdContext.VOL_AUTO,)):
        same(ctx.gram(nan_models, qx, qy, qz, w), ref)
    # ... unless its point weighs nothing?  No: 0 * NaN is NaN.  The NaN stays out only where its cell owns no point.
    far = gref.gram(nan_models, px, py, pz, w)
    if not np.isnan(far["values"]).any():
        assert np.isfinite(far["gram"]).all()
        same(ctx.gram(nan_models, px, py, pz, w), far)


def test_refusals_that_need_a_context(tt, ctx):
    models = [(np.zeros(1),) * 4] * 3
    p = np.zeros(4)
    before = ctx.gram(models, p, p, p)
    with pytest.raises(tt.TdError, match="td_rasterize_gram: every weight must be finite and >= 0"):
        ctx.gram(models, p, p, p, [1.0, -1.0, 1.0, 1.0])
    with pytest.raises(tt.TdError, match="td_rasterize_gram: a coordinate is not finite"):
        ctx.gram(models, p, [0.0, np.inf, 0.0, 0.0], p)
    with pytest.raises(tt.TdError, match="td_rasterize_gram: need nmodels >= 1"):
        ctx.gram([], p, p, p)
    with pytest.raises(tt.TdError, match="td_history_gram: the histories hold no sample"):
        ctx.gram_history([], p, p, p)
    # the size limit: refused with a message, never attempted (no kernel of the call is launched)
    many = [(np.zeros(1),) * 4] * (tt.TdContext.GRAM_MAX_MODELS + 1)
    ctx.timing(enable=True, reset=True)
    try:
        for want in (("gram",), ("dist2",), ("gram", "dist2")):
            with pytest.raises(tt.TdError, match="td_rasterize_gram: 11586 models: a matrix \\[M\\]\\[M\\] exceeds 1 GiB"):
                ctx.gram(many, p, p, p, want=want)
        for k in ("gram_pairs", "gram_centre", "gram_mirror", "raster_stats", "raster_brute", "vol_search", "vol_boxes"):
            assert ctx.timing(kernel=k)[0] == 0, k
    finally:
        ctx.timing(enable=False)
    same(ctx.gram(models, p, p, p), before)
    assert before["gram"].tolist() == [[0.0] * 3] * 3 and before["wsum"] == 4.0


# ---------------------------------------------------------------- histories and the statistics

@pytest.fixture(scope="module")
def recorded(tt, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=400)
    hists = []
    for k in range(2):
        c = tt.Chain(ctx, tt.chain_params(prm, None, seed=370 + k, chain=k + 1), tt.random_model(30, 370 + k))
        h = tt.History(ctx, 40, 40 * 400, with_ptS=False)
        c.run_recorded(400, 10, 10, h)
        assert len(h) == 40
        hists.append(h)
        c.close()
    empty = tt.History(ctx, 4, 4 * 400, with_ptS=False)
    yield [hists[0], empty, hists[1]]
    for h in hists + [empty]:
        h.close()


def box_points(tt, n, seed):
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    rng = np.random.default_rng(seed)
    return rng.uniform(xmin, xmax, n), rng.uniform(ymin, ymax, n), rng.uniform(zmin, zmax, n)


def test_histories_equal_their_models_read_back_and_the_statistics_the_volumes(tt, ctx, recorded):
    hists = recorded
    flat = [m.cells() for h in hists if len(h) for m in h.read()]
    assert len(flat) == 80
    px, py, pz = box_points(tt, 700, 19)
    w = np.random.default_rng(20).uniform(0.5, 2.0, len(px))
    ref = gref.gram(flat, px, py, pz, w)
    assert np.count_nonzero(ref["dist2"]) > 80 * 40
    arrays = ctx.gram(flat, px, py, pz, w)
    same(arrays, ref)
    for slab, method, form in settings(tt, ctx, slabs=(64, 0), methods=(tt.TdContext.VOL_AUTO,)):
        same(ctx.gram_history(hists, px, py, pz, w), arrays)
    vol = ctx.volume(flat, px, py, pz)
    assert np.array_equal(arrays["mean"], vol["mean"]) and np.array_equal(arrays["std"], vol["std"])
    with pytest.raises(tt.TdError, match="td_history_gram: the histories hold no sample"):
        ctx.gram_history([hists[1]], px, py, pz)
