"""GPU: posterior regions (td_rasterize_regions, td_history_regions, posterior_regions) against the numpy
restatement of their definition (tests/regions_ref.py), bit for bit, NaN positions included: the inputs on which the
association matters (tests/test_regions_host.py) under every slab size, sweep, weighting and normalisation, the
tails of the 64-model tile, models and points that are awkward, the history form, and the statistics against the
calls they are taken from."""
import numpy as np
import pytest

import regions_ref as rref

pytestmark = pytest.mark.gpu

FIELDS = ("series", "weight", "mean", "std", "greater")


@pytest.fixture(scope="module")
def sds(tt):
    return tt.synthetic_rays(24, seed=1)


@pytest.fixture(scope="module")
def ctx(tt, sds):
    c = tt.TdContext.from_datastruct(sds)
    yield c
    c.set_volume_counting(False)
    c.set_volume_slab_nodes(0)
    c.set_volume_method(tt.TdContext.VOL_AUTO)
    c.close()


def same(r, ref, fields=FIELDS):
    for f in fields:
        a, b = r[f], ref[f]
        assert a.shape == b.shape and a.dtype == b.dtype, (f, a.shape, b.shape, a.dtype, b.dtype)
        bad = ~((a == b) | ((a != a) & (b != b)))
        assert not bad.any(), "%s: %d of %d differ, first at %s: %r against %r" % (
            f, bad.sum(), a.size, np.argwhere(bad)[0], a[bad][0], b[bad][0])


def settings(tt, ctx, slabs=(64, 128, 0), methods=None):
    """Every (slab, method), the context set accordingly and put back at the end."""
    methods = (tt.TdContext.VOL_GRID, tt.TdContext.VOL_BRUTE) if methods is None else methods
    try:
        for slab in slabs:
            for method in methods:
                ctx.set_volume_slab_nodes(slab)
                ctx.set_volume_method(method)
                yield slab, method
    finally:
        ctx.set_volume_slab_nodes(0)
        ctx.set_volume_method(tt.TdContext.VOL_AUTO)


# ---------------------------------------------------------------- the base case

@pytest.fixture(scope="module")
def base():
    models, px, py, pz, w, off = rref.base_case()
    ref = {(wt, nz): rref.regions(models, px, py, pz, off, w if wt else None, nz) for wt in (True, False) for nz in (True, False)}
    return dict(models=models, px=px, py=py, pz=pz, w=w, off=off, ref=ref)


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
def test_base_case_whatever_the_slab_and_the_sweep(tt, ctx, base, weighted, normalize):
    """8347 points, 65 models (two tiles of models, the second with one), regions of 1 .. 3000 points: leaves of
    1025 = 513 + 512, 2049 = 513 + 512 + 512 + 512 and 3000 = 4 x 750 points that slabs of 64 and 128 columns cut many
    times, regions that share a slab and a tile.  The association test of test_regions_host.py holds for these very
    inputs, so another order of summation cannot pass."""
    ref = base["ref"][(weighted, normalize)]
    M, npts = len(base["models"]), len(base["px"])
    runs = []
    for slab, method in settings(tt, ctx):
        ctx.timing(enable=True, reset=True)
        try:
            r = ctx.regions(base["models"], base["px"], base["py"], base["pz"], base["off"], base["w"] if weighted else None,
                            normalize)
            nslabs = tt.TdContext.regions_plan(M, npts, 0, slab)[1]
            assert nslabs == (-(-npts // slab) if slab else 1)
            assert ctx.timing(kernel="region_sums")[0] == nslabs and ctx.timing(kernel="region_combine")[0] == 1
            assert ctx.timing(kernel="region_greater")[0] == 1 and ctx.timing(kernel="raster_stats")[0] == 1
        finally:
            ctx.timing(enable=False)
        c = ctx.volume_counters()
        assert (c[3] == M * npts and sum(c[:3]) == 0) if method == tt.TdContext.VOL_BRUTE else (c[3] == 0), c
        runs.append(r)
    runs.append(ctx.regions(base["models"], base["px"], base["py"], base["pz"], base["off"], base["w"] if weighted else None,
                            normalize))  # automatic in both, and a repeated call
    for r in runs:
        same(r, ref)
        same(r, runs[0])
    if not weighted:  # NULL weights are an array of ones, bit for bit
        ones = ctx.regions(base["models"], base["px"], base["py"], base["pz"], base["off"], np.ones(npts), normalize)
        same(ones, runs[0])
        assert np.array_equal(ones["weight"], np.diff(base["off"]).astype(np.float64))


# ---------------------------------------------------------------- the tails of the model tile

TAIL_SIZES = (1, 7, 70, 1100)


@pytest.mark.parametrize("M", [1, 3, 63, 64, 65, 130])
def test_model_count_tails(tt, ctx, M):
    """One lane, a few, one short of a tile, a tile, a tile and one, two tiles and two; models of 40 .. 300 cells,
    which the bucket grids take as well as the brute-force sweep.  M = 1 gives NaN sigma, as k_raster_stats does."""
    rng = np.random.default_rng(500 + M)
    models = []
    for _ in range(M):
        n = int(rng.integers(40, 301))
        models.append((rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(0, 200, n), rng.uniform(0, 50, n)))
    npts = sum(TAIL_SIZES)
    px, py, pz = rng.uniform(-100, 100, npts), rng.uniform(-100, 100, npts), rng.uniform(0, 200, npts)
    w = rng.uniform(0.5, 2.0, npts)
    off = np.concatenate(([0], np.cumsum(TAIL_SIZES)))
    ref = rref.regions(models, px, py, pz, off, w, True)
    if M > 1:
        assert all(len(set(ref["series"][:, r].tolist())) == M for r in range(4))
        assert np.all(np.isfinite(ref["std"])) and np.all(ref["std"] > 0)
    else:
        assert np.isnan(ref["std"]).all() and ref["greater"].max() == 1  # (one model still orders the regions)
    for slab, method in settings(tt, ctx, slabs=(64, 0)):
        same(ctx.regions(models, px, py, pz, off, w, True), ref)


# ---------------------------------------------------------------- awkward models, points and weights

def test_special_cases(tt, ctx):
    """A model without cells (0.0 everywhere), a NaN zeta that wins somewhere (NaN sums, and NaN is greater than
    nothing), a metre frame whose far points lie beyond the 1e9 sentinel of every cell (0.0), a point listed in two
    regions, and a contrast of +-1 weights with W = 0 (the division gives +-inf or NaN)."""
    rng = np.random.default_rng(77)
    models = []
    for k in range(20):
        n = int(rng.integers(5, 30))
        models.append([rng.uniform(-2e4, 2e4, n), rng.uniform(-2e4, 2e4, n), rng.uniform(0, 4e4, n), rng.uniform(0, 50, n)])
    models[3] = [np.zeros(0)] * 4
    models[5][3][2] = np.nan
    models = [tuple(m) for m in models]
    near = 40
    px = np.concatenate((rng.uniform(-2e4, 2e4, near), rng.uniform(4e5, 6e5, 10)))
    py = np.concatenate((rng.uniform(-2e4, 2e4, near), rng.uniform(4e5, 6e5, 10)))
    pz = np.concatenate((rng.uniform(0, 4e4, near), rng.uniform(0, 4e4, 10)))
    # a point of model 5's NaN cell itself, so that the cell wins there
    px[7], py[7], pz[7] = models[5][0][2], models[5][1][2], models[5][2][2]
    # regions: the near points | the far points | near and far | point 7 and point 0 again | a contrast of +-1
    idx = np.concatenate((np.arange(near), np.arange(near, near + 10), np.arange(30, near + 10), [7, 0], np.arange(10, 20)))
    off = np.array([0, near, near + 10, near + 30, near + 32, near + 42])
    qx, qy, qz = px[idx], py[idx], pz[idx]
    w = rng.uniform(0.5, 2.0, len(idx))
    w[off[4]:] = [1.0, -1.0] * 5
    for normalize in (True, False):
        ref = rref.regions(models, qx, qy, qz, off, w, normalize)
        V = ref["values"]
        assert not V[3].any() and np.isnan(V[5][7]) and np.isnan(V[5]).sum() >= 2  # (point 7 is listed twice)
        # beyond the sentinel (31.6 km): 0.0 for every model; within the models' box most points have an answer
        assert not V[:, off[1]:off[2]].any() and np.mean(V[[0, 1, 2, 4], :near] != 0) > 0.5
        assert ref["weight"][4] == 0.0 and np.isnan(ref["series"][5][0]) and np.isnan(ref["series"][5][3])
        if normalize:
            assert np.isinf(ref["series"][:, 4]).any()
        assert not np.isnan(ref["series"][:, 1]).any() and np.isnan(ref["mean"][0])
        for slab, method in settings(tt, ctx, slabs=(64, 0)):
            same(ctx.regions(models, qx, qy, qz, off, w, normalize), ref)
    sign = ctx.regions(models, qx[:1], qy[:1], qz[:1], [0, 1], [-1.0], False)["series"]
    assert np.signbit(sign[3][0]) and sign[3][0] == 0.0  # -1 * 0.0: the sum starts with its first term


def test_refusals_that_need_a_context(tt, ctx):
    models = [(np.zeros(1),) * 4] * 3
    p = np.zeros(4)
    before = ctx.regions(models, p, p, p, [0, 1, 4])
    with pytest.raises(tt.TdError, match="td_rasterize_regions: a region without points"):
        ctx.regions(models, p, p, p, [0, 1, 1, 4])
    with pytest.raises(tt.TdError, match="td_rasterize_regions: w is not finite"):
        ctx.regions(models, p, p, p, [0, 1, 4], [1.0, np.nan, 1.0, 1.0])
    with pytest.raises(tt.TdError, match="td_rasterize_regions: nchains must be >= 1"):
        ctx.regions(models, p, p, p, [0, 1, 4], chain_len=[])
    # the size limits: refused with a message, never attempted
    many = np.zeros(11586)
    with pytest.raises(tt.TdError, match="td_rasterize_regions: greater_out of more than 2\\^27 counters"):
        ctx.regions(models, many, many, many, np.arange(11587))
    big = np.zeros((1 << 18) + 1)
    with pytest.raises(tt.TdError, match="td_rasterize_regions: more than 2\\^18 regions"):
        ctx.regions(models, big, big, big, np.arange((1 << 18) + 2), greater=False)
    with pytest.raises(tt.TdError, match="td_rasterize_regions: the series \\[nmodels\\]\\[nreg\\] exceed 1 GiB"):
        ctx.regions([(np.zeros(1),) * 4] * 600, big[:-1], big[:-1], big[:-1], np.arange((1 << 18) + 1), greater=False)
    same(ctx.regions(models, p, p, p, [0, 1, 4]), before)


# ---------------------------------------------------------------- histories and the statistics

@pytest.fixture(scope="module")
def recorded(tt, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=400)
    hists = []
    for k in range(2):
        c = tt.Chain(ctx, tt.chain_params(prm, None, seed=270 + k, chain=k + 1), tt.random_model(30, 270 + k))
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


def test_histories_equal_their_models_read_back_and_the_statistics_their_own_calls(tt, ctx, recorded):
    hists = recorded
    flat = [m.cells() for h in hists if len(h) for m in h.read()]
    assert len(flat) == 80
    sizes = (1, 30, 1500)
    px, py, pz = box_points(tt, sum(sizes), 9)
    w = np.random.default_rng(10).uniform(0.5, 2.0, len(px))
    off = np.concatenate(([0], np.cumsum(sizes)))
    probs, bins = (0.05, 0.5, 0.95), (8, 0.0, 40.0)
    ref = rref.regions(flat, px, py, pz, off, w, True)
    # (a point keeps its value over many samples of a chain; an average over 30 points does not)
    assert len(set(ref["series"][:, 0].tolist())) > 1 and all(len(set(ref["series"][:, r].tolist())) > 40 for r in (1, 2))
    arrays = ctx.regions(flat, px, py, pz, off, w, True, probs, bins, chain_len=[40, 40])
    same(arrays, ref)
    for slab, method in settings(tt, ctx, slabs=(64, 0)):
        h = ctx.regions_history(hists, px, py, pz, off, w, True, probs, bins, convergence=True)
        same(h, arrays, FIELDS + ("quantiles", "hist", "rhat", "ess", "lags"))
    # R-hat and ESS are td_convergence_values' of the series, the quantiles and histograms td_marginals' of it
    conv = ctx.convergence(arrays["series"], [40, 40])
    same(arrays, conv, ("rhat", "ess", "lags"))
    assert np.all(np.isfinite(arrays["rhat"][1:])) and np.all(arrays["ess"][1:] > 1)
    q = np.quantile(arrays["series"], probs, axis=0)
    assert np.allclose(arrays["quantiles"], q, rtol=1e-12, atol=0)
    assert arrays["hist"].shape == (3, 11) and np.all(arrays["hist"].sum(axis=1) == 80)
    with pytest.raises(tt.TdError, match="td_history_regions: the histories hold no sample"):
        ctx.regions_history([hists[1]], px, py, pz, off)


def test_one_point_regions_are_the_volume(tt, ctx, recorded):
    """A region of one point with w = NULL: F is V, so every statistic is TdContext.volume's at that point."""
    flat = [m.cells() for h in recorded if len(h) for m in h.read()]
    px, py, pz = box_points(tt, 70, 11)
    probs, bins = (0.1, 0.5, 0.9), (6, 0.0, 30.0)
    vol = ctx.volume(flat, px, py, pz, probs, bins, chain_len=[40, 40], want_values=True)
    assert len(np.unique(vol["values"])) > 70
    for normalize in (True, False):
        r = ctx.regions(flat, px, py, pz, np.arange(71), None, normalize, probs, bins, chain_len=[40, 40])
        assert np.array_equal(r["series"], vol["values"])
        same(r, vol, ("mean", "std", "quantiles", "hist", "rhat", "ess", "lags"))
        assert np.array_equal(r["greater"], rref.greater(vol["values"])) and np.all(r["weight"] == 1.0)


def test_series_compose_with_the_covariance(tt, ctx, sds, recorded):
    """posterior_covariance(series=posterior_regions(...)["series"]): a one-point region's row equals the point
    target's (a series that is a target's values gives the target's row)."""
    hists = recorded
    prm = tt.define_TDstructrure()
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    xs, ys, zs = np.linspace(xmin, xmax, 6), np.linspace(ymin, ymax, 5), np.linspace(zmin, zmax, 4)
    tx, ty, tz = box_points(tt, 2, 12)
    pr = tt.posterior_regions(hists, sds, prm, {"a": ([tx[0]], [ty[0]], [tz[0]]), "b": ([tx[1]], [ty[1]], [tz[1]])},
                              probs=(), xs=xs, ys=ys, zs=zs)
    assert pr["series"].shape == (80, 2) and all(len(set(pr["series"][:, r].tolist())) > 1 for r in (0, 1))
    by_series = tt.posterior_covariance(hists, sds, prm, None, series=pr["series"], xs=xs, ys=ys, zs=zs)
    by_target = tt.posterior_covariance(hists, sds, prm, np.stack((tx, ty, tz), axis=1), xs=xs, ys=ys, zs=zs)
    for f in ("cov", "corr", "target_mean", "target_std"):
        assert np.array_equal(by_series[f], by_target[f], equal_nan=True), f
    assert np.isfinite(by_series["cov"]).all() and (by_series["cov"] != 0).any()


def test_posterior_regions_on_the_lattice(tt, ctx, sds, recorded):
    """posterior_regions against numpy on the route there was before: volume_history(want_values=True) and the
    restatement's tree.  Masks (depth layers, a box) with volume weights and without, free points, sums; Models and
    nested lists give what the histories give."""
    hists = recorded
    prm = tt.define_TDstructrure()
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    xs, ys, zs = np.linspace(xmin, xmax, 9), np.linspace(ymin, ymax, 7), np.linspace(zmin, zmax, 6)
    regs = dict(tt.depth_layers(zs, [zmin, 0.5 * (zmin + zmax), zmax + 1.0]))
    regs["box"] = tt.box_region(xs, ys, zs, (xs[2], ys[1], zs[1]), (xs[6], ys[5], zs[4]))
    path = box_points(tt, 25, 13)
    regs["path"] = path + (np.linspace(1.0, 2.0, 25),)
    M = 80
    for weights, normalize in (("volume", True), (None, True), ("volume", False)):
        out = tt.posterior_regions(hists, sds, prm, regs, weights, normalize, bins=(8, 0.0, 40.0), convergence=True,
                                   xs=xs, ys=ys, zs=zs)
        names, px, py, pz, w, off = tt.region_points(regs, xs, ys, zs, weights)
        assert out["names"] == names == list(regs) and len(names) == 4
        V = ctx.volume_history(hists, px, py, pz, want_values=True)["values"]
        F, W = rref.series(V, off, w, normalize)
        mean, std = rref.statistics(F)
        g = rref.greater(F)
        same(out, dict(series=F, weight=W, mean=mean, std=std, greater=g))
        assert np.array_equal(out["prob_greater"], g / 80.0)
        assert out["quantiles"].shape == (3, 4) and out["hist"].shape == (4, 11) and out["rhat"].shape == (4,)
        assert ((g > 0) & (g < M)).any()
    vol = tt.voxel_weights(xs, ys, zs)
    lo = np.broadcast_to(regs[names[0]], vol.shape)
    assert np.isclose(out["weight"][0], vol[lo].sum(), rtol=1e-13)
    flat_models = [m for h in hists if len(h) for m in h.read()]
    nested = [[m for m in h.read()] for h in hists if len(h)]
    for form in (flat_models, nested):  # (a flat list is one chain: its R-hat is another)
        conv = form is nested
        o2 = tt.posterior_regions(form, sds, prm, regs, "volume", False, bins=(8, 0.0, 40.0), convergence=conv,
                                  xs=xs, ys=ys, zs=zs)
        for f in ("series", "weight", "mean", "std", "greater", "prob_greater", "quantiles", "hist") + (("rhat", "ess", "lags") if conv else ()):
            assert np.array_equal(o2[f], out[f], equal_nan=True), f
    assert M == len(flat_models)
