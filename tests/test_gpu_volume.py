"""GPU: posterior volumes (td_rasterize_volume, td_history_volume, posterior_volume) against the section
entry points they must equal bit for bit (rasterize, marginals, convergence and their history forms) and
against oracle_np.rasterize, at the smallest shapes that can still go wrong: models of 0 .. 600 cells in
layouts that tie, duplicate, degenerate and leave blocks of the bucket grid empty; nodes that are no
multiple of a slab, lie far outside every model or are NaN; slabs of 64 and 128 nodes and automatic."""
import copy

import numpy as np
import pytest

from oracle import oracle_np

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
BINS = (20, 0.0, 50.0)


@pytest.fixture(scope="module")
def ctx(tt, ds):
    c = tt.TdContext.from_datastruct(ds)
    c.set_volume_counting(True)  # (the product's instance, which does not count, is compared in each test)
    yield c
    c.set_volume_counting(False)
    c.set_volume_slab_nodes(0)
    c.set_volume_method(tt.TdContext.VOL_AUTO)


def lattice(xs, ys, zs):
    """x fastest"""
    xs, ys, zs = (np.asarray(v, dtype=np.float64) for v in (xs, ys, zs))
    return (np.tile(xs, len(ys) * len(zs)), np.tile(np.repeat(ys, len(xs)), len(zs)), np.repeat(zs, len(xs) * len(ys)))


def same(a, b, fields):
    for f in fields:
        assert a[f].shape == b[f].shape and a[f].dtype == b[f].dtype, f
        assert np.array_equal(a[f], b[f], equal_nan=a[f].dtype.kind == "f"), f


def adversarial():
    """13 models (not a multiple of 8) of 0, 1, 2, 255, 256, 257 and 600 cells; 9 x 7 x 5 nodes on
    multiples of 100 plus three nodes far outside every box and one with a NaN coordinate."""
    rng = np.random.default_rng(5)
    hi = np.array([800.0, 600.0, 400.0])

    def uniform(n):
        return tuple((rng.random((n, 3)) * hi).T) + (rng.uniform(0, 50, n),)

    # cells on the even multiples of 100: a node on an odd multiple is exactly as far from 2, 4 or 8 of them
    # (every distance is an integer), and each carries its own zeta -- the lowest index must win
    gx, gy, gz = np.meshgrid(np.arange(10) * 200.0 - 400, np.arange(10) * 200.0 - 600, np.arange(6) * 200.0 - 200,
                             indexing="ij")
    perm = rng.permutation(600)
    on_lattice = (gx.ravel()[perm], gy.ravel()[perm], gz.ravel()[perm], np.arange(600) * 0.0625 + 1.0)
    x, y, z, _ = uniform(128)
    dup = rng.permutation(256) % 128
    duplicates = (x[dup], y[dup], z[dup], np.arange(256) * 0.125)  # every cell twice, zeta by index
    x, y, z, ze = uniform(255)
    coplanar = (x, y, np.full(255, 137.5), ze)  # a degenerate axis
    c = rng.random((256, 3)) * 3.0  # a tight cluster in one corner and one far cell: empty blocks around most nodes
    cluster = (np.append(c[:, 0], 800.0), np.append(c[:, 1], 600.0), np.append(c[:, 2], 400.0), rng.uniform(0, 50, 257))
    x, y, z, ze = uniform(600)
    x = x.copy()
    x[311] = np.nan  # never wins
    with_nan = (x, y, z, ze)
    beyond = (np.array([1e5]), np.array([1e5]), np.array([1e5]), np.array([7.0]))  # farther than sqrt(1e9): 0.0
    empty = (np.zeros(0),) * 4
    two = uniform(2)
    models = [uniform(600), empty, on_lattice, beyond, duplicates, two, coplanar, uniform(600), cluster, with_nan,
              uniform(600), uniform(600), uniform(600)]
    assert sorted(len(m[0]) for m in models) == [0, 1, 2, 255, 256, 257] + [600] * 7
    qx, qy, qz = lattice(np.arange(9) * 100.0, np.arange(7) * 100.0, np.arange(5) * 100.0)
    far = np.array([[5e3, -4e3, 2e3], [-1e4, 1e4, -1e4], [3e4, 3e4, 3e4], [np.nan, 100.0, 100.0]])
    qx, qy, qz = (np.concatenate([q, far[:, k]]) for k, q in enumerate((qx, qy, qz)))
    assert len(qx) == 319
    return models, qx, qy, qz


def test_adversarial_models_host_arrays(tt, ctx):
    models, qx, qy, qz = adversarial()
    T = tt.TdContext
    mean, std, V = oracle_np.rasterize(models, qx, qy, qz)
    m2, s2, V2 = ctx.rasterize(models, qx, qy, qz, want_values=True)
    assert np.array_equal(V, V2) and np.array_equal(mean, m2) and np.array_equal(std, s2, equal_nan=True)
    assert np.all(V[1] == 0.0) and np.all(V[3] == 0.0) and np.all(V[:, -1] == 0.0) and np.all(V[:, -2] == 0.0)
    x, y, z, ze = models[2]  # an all-odd node: eight cells tie, the one of the lowest index answers
    d = (x - 300.0) ** 2 + (y - 100.0) ** 2 + (z - 300.0) ** 2
    assert np.sum(d == d.min()) == 8 and V[2][3 + 9 * (1 + 7 * 3)] == ze[np.flatnonzero(d == d.min())[0]]
    pairs = len(models) * len(qx)
    runs = []
    try:
        for method in (T.VOL_GRID, T.VOL_AUTO, T.VOL_BRUTE):
            ctx.set_volume_method(method)
            for slab in (64, 128, 0, 0):  # the seams between slabs; the scatter's order differs from run to run
                ctx.set_volume_slab_nodes(slab)
                r = ctx.volume(models, qx, qy, qz, want_values=True)
                c = ctx.volume_counters()
                print("method %d slab %d counters %s" % (method, slab, c))
                assert sum(c) == pairs
                if method == T.VOL_GRID:  # each of the three grid paths is taken
                    assert c[0] > 0 and c[1] > 0 and c[2] > 0 and c[3] == 0, c
                if method == T.VOL_BRUTE:
                    assert c == (0, 0, 0, pairs)
                runs.append(r)
        ctx.set_volume_method(T.VOL_GRID)  # the product's instance of the search, which counts nothing
        ctx.set_volume_counting(False)
        for slab in (64, 0):
            ctx.set_volume_slab_nodes(slab)
            runs.append(ctx.volume(models, qx, qy, qz, want_values=True))
            assert ctx.volume_counters() == (-1, -1, -1, 0)
    finally:
        ctx.set_volume_counting(True)
        ctx.set_volume_method(T.VOL_AUTO)
        ctx.set_volume_slab_nodes(0)
    ref = dict(mean=mean, std=std, values=V)
    for r in runs:
        assert r["quantiles"] is None and r["hist"] is None and "rhat" not in r
        same(r, ref, ("values", "mean", "std"))


def test_the_grid_path_is_the_one_tested(tt, ctx):
    """2000 cells uniform in the shipped lattice's box, nodes inside it: full scans <= 1 % of the pairs and
    the 3x3x3 block >= 95 % (a numpy restatement of make_cell_grid and grid_block_lb gave 0 and 99.1-99.8 %
    for 64 to 5000 uniform cells)."""
    models = [tt.random_model(2000, 40 + k).cells() for k in range(8)]
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    qx, qy, qz = lattice(xmin + (xmax - xmin) * (np.arange(20) + 0.5) / 20, ymin + (ymax - ymin) * (np.arange(12) + 0.5) / 12,
                         zmin + (zmax - zmin) * (np.arange(12) + 0.5) / 12)
    mean, std, V = oracle_np.rasterize(models, qx, qy, qz)
    m2, s2, V2 = ctx.rasterize(models, qx, qy, qz, want_values=True)
    assert np.array_equal(V, V2)
    ctx.timing(enable=True, reset=True)
    try:
        r = ctx.volume(models, qx, qy, qz, want_values=True)
        launches = {k: ctx.timing(kernel=k)[0] for k in ("vol_boxes", "vol_grid_build", "vol_search", "raster_brute")}
    finally:
        ctx.timing(enable=False)
    same(r, dict(values=V, mean=mean, std=std), ("values", "mean", "std"))
    assert np.array_equal(r["mean"], m2) and np.array_equal(r["std"], s2)
    assert launches == dict(vol_boxes=1, vol_grid_build=1, vol_search=1, raster_brute=0), launches
    c = ctx.volume_counters()
    pairs = 8 * len(qx)
    print("counters", c, "of", pairs)
    assert sum(c) == pairs and c[3] == 0
    assert c[2] <= 0.01 * pairs and c[0] >= 0.95 * pairs, c
    ctx.set_volume_counting(False)  # the product's instance: the same values
    try:
        same(ctx.volume(models, qx, qy, qz, want_values=True), r, ("values", "mean", "std"))
        assert ctx.volume_counters() == (-1, -1, -1, 0)
    finally:
        ctx.set_volume_counting(True)


def test_histories(tt, ds, ctx):
    T = tt.TdContext
    prm = tt.define_TDstructrure().replace(max_cells=400)
    hists = []
    for k in range(2):
        c = tt.Chain(ctx, tt.chain_params(prm, None, seed=90 + k, chain=k + 1), tt.random_model(300, 90 + k))
        h = tt.History(ctx, 40, 40 * 400, with_ptS=False)
        c.run_recorded(400, 10, 10, h)
        assert len(h) == 40
        hists.append(h)
    empty = tt.History(ctx, 4, 4 * 400, with_ptS=False)
    hists = [hists[0], empty, hists[1]]
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    qx, qy, qz = lattice(np.linspace(xmin - 30, xmax + 30, 9), np.linspace(ymin, ymax, 7), np.linspace(zmin, zmax + 50, 5))
    assert len(qx) == 315
    m1, s1, V = ctx.rasterize_history(hists, qx, qy, qz, want_values=True)
    marg = ctx.marginals_history(hists, qx, qy, qz, PROBS, BINS)
    conv = ctx.convergence_history(hists, qx, qy, qz)
    ref = dict(mean=m1, std=s1, values=V, quantiles=marg["quantiles"], hist=marg["hist"], rhat=conv["rhat"],
               ess=conv["ess"], lags=conv["lags"])
    assert np.array_equal(marg["mean"], m1) and np.array_equal(conv["mean"], m1)
    assert np.isfinite(conv["rhat"]).any()
    try:
        for method in (T.VOL_GRID, T.VOL_BRUTE):
            ctx.set_volume_method(method)
            for slab in (64, 0):
                ctx.set_volume_slab_nodes(slab)
                r = ctx.volume_history(hists, qx, qy, qz, PROBS, BINS, convergence=True, want_values=True)
                same(r, ref, ("values", "mean", "std", "quantiles", "hist", "rhat", "ess", "lags"))
                assert sum(ctx.volume_counters()) == 80 * 315
        ctx.set_volume_method(T.VOL_GRID)
        ctx.set_volume_counting(False)  # the product's instance
        r = ctx.volume_history(hists, qx, qy, qz, PROBS, BINS, convergence=True, want_values=True)
        same(r, ref, ("values", "mean", "std", "quantiles", "hist", "rhat", "ess", "lags"))
        ctx.set_volume_counting(True)
        ctx.set_volume_method(T.VOL_AUTO)
        ctx.set_volume_slab_nodes(128)  # the models read back: the host-array entry point, same numbers
        flat = [m.cells() for h in hists if len(h) for m in h.read()]
        r = ctx.volume(flat, qx, qy, qz, PROBS, BINS, chain_len=[40, 40], max_lag=7)
        same(r, ref, ("mean", "std", "quantiles", "hist", "rhat"))
        lag7 = ctx.convergence_history(hists, qx, qy, qz, max_lag=7)
        same(r, lag7, ("ess", "lags"))
        with pytest.raises(tt.TdError, match="td_history_volume"):
            ctx.volume_history([empty], qx, qy, qz)
        with pytest.raises(tt.TdError, match="td_rasterize_volume"):
            ctx.volume(flat, qx, qy, qz, chain_len=[40, 39])
    finally:
        ctx.set_volume_counting(True)
        ctx.set_volume_method(T.VOL_AUTO)
        ctx.set_volume_slab_nodes(0)
    z = ctx.volume(flat, [], [], [])  # nq == 0: TD_OK
    assert z["mean"].shape == (0,)


def test_orientation(tt, ds):
    """posterior_volume's [nx, ny, nz] arrays against the sections of plot_model_hist, credible_maps and
    convergence_maps on the shipped lattice thinned to every 4th node."""
    hist = [[tt.random_model(80 + 10 * j, 10 * c + j) for j in range(6)] for c in range(2)]
    tt.context_for(ds)
    thin = copy.copy(ds)  # (shares the context)
    thin.xVec, thin.yVec, thin.zVec = (np.asarray(v, dtype=np.float64)[::4] for v in (ds.xVec, ds.yVec, ds.zVec))
    xv, yv, zv = thin.xVec, thin.yVec, thin.zVec
    js, ks = (0, 3, len(yv) - 1), (1, len(zv) - 1)
    prm = tt.define_TDstructrure().replace(xzMap=True, ySlice=[float(yv[j]) for j in js], xyMap=True,
                                           zSlice=[float(zv[k]) for k in ks])
    vol = tt.posterior_volume(hist, thin, prm, probs=PROBS, bins=BINS, convergence=True)
    assert vol["mean"].shape == vol["std"].shape == vol["masked"].shape == vol["rhat"].shape == (len(xv), len(yv), len(zv))
    assert vol["quantiles"].shape == (3, len(xv), len(yv), len(zv)) and vol["hist"].shape == vol["mean"].shape + (23,)
    assert np.array_equal(vol["width"], vol["quantiles"][-1] - vol["quantiles"][0])
    assert np.array_equal(vol["x"], xv) and np.array_equal(vol["y"], yv) and np.array_equal(vol["z"], zv)
    sections = tt.plot_model_hist(hist, thin, prm)
    cred = tt.credible_maps(hist, thin, prm, probs=PROBS, bins=BINS)
    conv = tt.convergence_maps(hist, thin, prm)
    cut = [(("xz", float(yv[j])), (slice(None), j, slice(None))) for j in js]
    cut += [(("xy", float(zv[k])), (slice(None), slice(None), k)) for k in ks]
    for key, ix in cut:
        for f in ("mean", "std", "masked"):
            assert np.array_equal(vol[f][ix], sections[key][f], equal_nan=True), (key, f)
        assert np.array_equal(vol["quantiles"][(slice(None),) + ix], cred[key]["quantiles"]), key
        assert np.array_equal(vol["width"][ix], cred[key]["width"]) and np.array_equal(vol["hist"][ix], cred[key]["hist"])
        for f in ("rhat", "ess", "lags"):
            assert np.array_equal(vol[f][ix], conv[key][f], equal_nan=True), (key, f)
        assert vol["summary"]["n"] == conv[key]["summary"]["n"] and vol["summary"]["m"] == conv[key]["summary"]["m"]
    # a sub-lattice by argument, without convergence or histograms
    sub = tt.posterior_volume(hist, ds, prm, probs=(0.5,), xs=xv, ys=yv[:2], zs=zv[1:3])
    assert "hist" not in sub and "rhat" not in sub and sub["mean"].shape == (len(xv), 2, 2)
    assert np.array_equal(sub["mean"], vol["mean"][:, :2, 1:3]) and np.array_equal(sub["quantiles"][0], vol["quantiles"][1][:, :2, 1:3])
