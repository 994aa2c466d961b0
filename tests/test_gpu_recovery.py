"""GPU: posterior recovery (td_rasterize_recovery, td_history_recovery, posterior_recovery) against the numpy
restatement of its definition (tests/recovery_ref.py), bit for bit, NaN positions included: the inputs on which the
association and the rounding matter (tests/test_recovery_host.py) under every slab size, sweep, weighting and
normalisation, the tails of the 64-model tile, models and points that are awkward, the history form, the statistics
against the calls they are taken from, and one recovery from exact synthetic data end to end."""
import time

import numpy as np
import pytest

import recovery_ref as cref

pytestmark = pytest.mark.gpu

FIELDS = cref.FIELDS


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
        if a.dtype.kind == "f":  # (the sign of a zero counts, the sign of a NaN does not)
            bad |= (np.signbit(a) != np.signbit(b)) & (a == a)
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
def base(tt):
    models, px, py, pz, w, off, truths, board = cref.base_case(tt.checkerboard_model)
    _, _, V = cref.oracle_np.rasterize(models, px, py, pz)
    ref = {(name, wt, nz): cref.from_values(V, truths[name], off, w if wt else None, nz)
           for name in truths for wt in (True, False) for nz in (True, False)}
    return dict(models=models, px=px, py=py, pz=pz, w=w, off=off, truths=truths, board=board, ref=ref)


@pytest.mark.parametrize("truth", ["model", "board"])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
def test_base_case_whatever_the_slab_and_the_sweep(tt, ctx, base, truth, weighted, normalize):
    """7147 points, 65 models (two tiles of models, the second with one), regions of 1 .. 3000 points: leaves of
    1025 = 513 + 512, 2049 = 513 + 512 + 512 + 512 and 3000 = 4 x 750 points that slabs of 64 and 128 columns cut many
    times.  The association and rounding tests of test_recovery_host.py hold for these very inputs."""
    ref = base["ref"][(truth, weighted, normalize)]
    M, npts = len(base["models"]), len(base["px"])
    args = (base["models"], base["px"], base["py"], base["pz"], base["truths"][truth], base["off"])
    wv = base["w"] if weighted else None
    runs = []
    for slab, method in settings(tt, ctx):
        ctx.timing(enable=True, reset=True)
        try:
            r = ctx.recovery(*args, wv, normalize)
            nslabs = tt.TdContext.regions_plan(M, npts, 0, slab)[1]
            assert nslabs == (-(-npts // slab) if slab else 1)
            for kernel in ("recovery_counts", "recovery_dstats", "recovery_sums"):  # one launch per slab
                assert ctx.timing(kernel=kernel)[0] == nslabs, kernel
            assert ctx.timing(kernel="recovery_combine")[0] == 1 and ctx.timing(kernel="raster_stats")[0] == 1
            assert ctx.timing(kernel="region_sums")[0] == 0
        finally:
            ctx.timing(enable=False)
        c = ctx.volume_counters()
        assert (c[3] == M * npts and sum(c[:3]) == 0) if method == tt.TdContext.VOL_BRUTE else (c[3] == 0), c
        runs.append(r)
    runs.append(ctx.recovery(*args, wv, normalize))  # automatic in both, and a repeated call
    for r in runs:
        same(r, ref)
        same(r, runs[0])
    if not weighted:  # NULL weights are an array of ones, bit for bit
        ones = ctx.recovery(*args, np.ones(npts), normalize)
        same(ones, runs[0])
        assert np.array_equal(ones["weight"], np.diff(base["off"]).astype(np.float64))
    if truth == "board":  # the truth as a Model, rasterised by the device's own search, is the restatement's
        t = ctx.rasterize([base["board"].cells()], base["px"], base["py"], base["pz"], want_values=True)[2][0]
        far = np.array(cref.BASE_FAR)
        assert not t[far].any() and np.array_equal(np.delete(t, far), np.delete(base["truths"]["board"], far))


# ---------------------------------------------------------------- the tails of the model tile

TAIL_SIZES = (1, 7, 70, 1100)


@pytest.mark.parametrize("M", [1, 3, 63, 64, 65, 130])
def test_model_count_tails(tt, ctx, M):
    """One lane, a few, one short of a tile, a tile, a tile and one, two tiles and two; models of 40 .. 300 cells,
    which the bucket grids take as well as the brute-force sweep; the counting kernel's batches of eight rows end
    in tails of 1, 3, 7, 0, 1 and 2.  M = 1 gives NaN sigma, as k_raster_stats does."""
    rng = np.random.default_rng(800 + M)
    models = []
    for _ in range(M):
        n = int(rng.integers(40, 301))
        models.append((rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(0, 200, n), rng.uniform(0, 50, n)))
    npts = sum(TAIL_SIZES)
    px, py, pz = rng.uniform(-100, 100, npts), rng.uniform(-100, 100, npts), rng.uniform(0, 200, npts)
    w = rng.uniform(0.5, 2.0, npts)
    off = np.concatenate(([0], np.cumsum(TAIL_SIZES)))
    _, _, V = cref.oracle_np.rasterize(models, px, py, pz)
    truth = np.where(np.arange(npts) % 3 == 0, V[np.arange(npts) % M, np.arange(npts)], rng.uniform(0, 50, npts))
    ref = cref.from_values(V, truth, off, w, True)
    assert np.all(ref["below"] + ref["equal"] + ref["above"] == M) and ref["equal"].max() >= 1
    if M > 1:
        assert all(len(set(ref["series"][:, r].tolist())) == M for r in range(4))
        assert np.all(np.isfinite(ref["std"])) and np.all(ref["std"] > 0) and np.mean(ref["dstd"] > 0) > 0.9
    else:
        assert np.isnan(ref["std"]).all() and np.isnan(ref["dstd"]).all()
    for slab, method in settings(tt, ctx, slabs=(64, 0)):
        same(ctx.recovery(models, px, py, pz, truth, off, w, True), ref)
    one = ctx.recovery(models, px, py, pz, truth)  # reg_off=None: all points are one region
    same(one, cref.from_values(V, truth, [0, npts], None, True))


# ---------------------------------------------------------------- awkward models, points and weights

def test_special_cases(tt, ctx):
    """A model without cells (0.0 everywhere), a model of one cell, a NaN zeta that wins somewhere (it counts neither
    below, equal nor above, and its sums are NaN), a metre frame whose far points lie beyond the 1e9 sentinel of every
    cell (0.0, against truths of -0.0 and 0.0), a point listed in two regions, and a contrast of +-1 weights with
    W = 0 (the division gives +-inf or NaN)."""
    rng = np.random.default_rng(78)
    models = []
    for k in range(20):
        n = int(rng.integers(5, 30))
        models.append([rng.uniform(-2e4, 2e4, n), rng.uniform(-2e4, 2e4, n), rng.uniform(0, 4e4, n), rng.uniform(0, 50, n)])
    models[3] = [np.zeros(0)] * 4
    models[4] = [np.array([100.0]), np.array([-200.0]), np.array([2e4]), np.array([33.0])]
    models[5][3][2] = np.nan
    models = [tuple(m) for m in models]
    near = 40
    px = np.concatenate((rng.uniform(-2e4, 2e4, near), rng.uniform(4e5, 6e5, 10)))
    py = np.concatenate((rng.uniform(-2e4, 2e4, near), rng.uniform(4e5, 6e5, 10)))
    pz = np.concatenate((rng.uniform(0, 4e4, near), rng.uniform(0, 4e4, 10)))
    px[7], py[7], pz[7] = models[5][0][2], models[5][1][2], models[5][2][2]  # model 5's NaN cell wins at its nucleus
    # regions: the near points | the far points | near and far | point 7 and point 0 again | a contrast of +-1
    idx = np.concatenate((np.arange(near), np.arange(near, near + 10), np.arange(30, near + 10), [7, 0], np.arange(10, 20)))
    off = np.array([0, near, near + 10, near + 30, near + 32, near + 42])
    qx, qy, qz = px[idx], py[idx], pz[idx]
    w = rng.uniform(0.5, 2.0, len(idx))
    w[off[4]:] = [1.0, -1.0] * 5
    truth = rng.uniform(0, 50, len(idx))
    truth[idx >= near] = np.where(np.arange(np.sum(idx >= near)) % 2 == 0, -0.0, 0.0)
    _, _, V = cref.oracle_np.rasterize(models, qx, qy, qz)
    truth[idx == 0] = V[4][0]  # the one-cell model's value at point 0, wherever the point is listed
    for normalize in (True, False):
        ref = cref.from_values(V, truth, off, w, normalize)
        assert not V[3].any() and np.isnan(V[5][7]) and np.isnan(V[5]).sum() >= 2  # (point 7 is listed twice)
        assert set(V[4].tolist()) == {0.0, 33.0} and not V[:, off[1]:off[2]].any()
        total = ref["below"] + ref["equal"] + ref["above"]
        assert total[7] == 19 and total[off[3]] == 19 and np.array_equal(total, 20 - np.isnan(V).sum(axis=0))
        assert np.all(ref["equal"][off[1]:off[2]] == 20) and np.all(ref["equal"][idx == 0] >= 1)
        assert ref["weight"][4] == 0.0 and np.isnan(ref["series"][5][0]) and np.isnan(ref["series"][5][3])
        assert np.isnan(ref["dmean"][7]) and not ref["series"][:, 1].any()
        if normalize:
            assert not np.isfinite(ref["series"][:, 4]).all()
        for slab, method in settings(tt, ctx, slabs=(64, 0)):
            same(ctx.recovery(models, qx, qy, qz, truth, off, w, normalize), ref)


def test_refusals_that_need_a_context(tt, ctx):
    models = [(np.zeros(1),) * 4] * 3
    p = np.zeros(4)
    before = ctx.recovery(models, p, p, p, p, [0, 1, 4])
    with pytest.raises(tt.TdError, match="td_rasterize_recovery: a region without points"):
        ctx.recovery(models, p, p, p, p, [0, 1, 1, 4])
    with pytest.raises(tt.TdError, match="td_rasterize_recovery: truth is not finite"):
        ctx.recovery(models, p, p, p, [1.0, np.nan, 1.0, 1.0], [0, 1, 4])
    with pytest.raises(tt.TdError, match="td_rasterize_recovery: nchains must be >= 1"):
        ctx.recovery(models, p, p, p, p, [0, 1, 4], chain_len=[])
    # the size limits: refused with a message, never attempted
    big = np.zeros((1 << 18) + 1)
    with pytest.raises(tt.TdError, match="td_rasterize_recovery: more than 2\\^18 regions"):
        ctx.recovery(models, big, big, big, big, np.arange((1 << 18) + 2))
    with pytest.raises(tt.TdError, match="td_rasterize_recovery: the series \\[nmodels\\]\\[nreg\\] exceed 1 GiB"):
        ctx.recovery([(np.zeros(1),) * 4] * 600, big[:-1], big[:-1], big[:-1], big[:-1], np.arange((1 << 18) + 1))
    same(ctx.recovery(models, p, p, p, p, [0, 1, 4]), before)


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


def test_histories_equal_their_models_read_back_and_the_statistics_their_own_calls(tt, ctx, recorded):
    hists = recorded
    flat = [m.cells() for h in hists if len(h) for m in h.read()]
    assert len(flat) == 80
    sizes = (1, 30, 1500)
    px, py, pz = box_points(tt, sum(sizes), 19)
    w = np.random.default_rng(20).uniform(0.5, 2.0, len(px))
    truth = np.random.default_rng(21).uniform(5.0, 45.0, len(px))
    off = np.concatenate(([0], np.cumsum(sizes)))
    probs, bins = (0.05, 0.5, 0.95), (8, 0.0, 800.0)
    ref = cref.recovery(flat, px, py, pz, truth, off, w, True)
    assert all(len(set(ref["series"][:, r].tolist())) > 40 for r in (1, 2))
    arrays = ctx.recovery(flat, px, py, pz, truth, off, w, True, probs, bins, chain_len=[40, 40])
    same(arrays, ref)
    every = FIELDS + ("quantiles", "hist", "rhat", "ess", "lags")
    for slab, method in settings(tt, ctx, slabs=(64, 0)):
        same(ctx.recovery_history(hists, px, py, pz, truth, off, w, True, probs, bins, convergence=True), arrays, every)
    # R-hat and ESS are td_convergence_values' of the series, the quantiles and histograms td_marginals' of it
    conv = ctx.convergence(arrays["series"], [40, 40])
    same(arrays, conv, ("rhat", "ess", "lags"))
    assert np.all(np.isfinite(arrays["rhat"][1:])) and np.all(arrays["ess"][1:] > 1)
    assert np.allclose(arrays["quantiles"], np.quantile(arrays["series"], probs, axis=0), rtol=1e-12, atol=0)
    assert arrays["hist"].shape == (3, 11) and np.all(arrays["hist"].sum(axis=1) == 80)
    assert (arrays["hist"][:, 1:9] > 0).sum() >= 4  # (the bins were chosen to hold the series)
    with pytest.raises(tt.TdError, match="td_history_recovery: the histories hold no sample"):
        ctx.recovery_history([hists[1]], px, py, pz, truth, off)


def test_posterior_recovery_on_a_small_lattice(tt, ctx, sds, recorded):
    """pit, inside, coverage and mean_model_rms against numpy from the restatement's counts and bias; the truth as a
    Model and as the array of its node values; named regions and the default; Models give what the histories give."""
    hists = recorded
    prm = tt.define_TDstructrure()
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    xs, ys, zs = np.linspace(xmin, xmax, 9), np.linspace(ymin, ymax, 7), np.linspace(zmin, zmax, 6)
    board = tt.checkerboard_model(xs, ys, zs, blocks=(2, 1, 2), lo=5.0, hi=15.0)
    flat = [m for h in hists if len(h) for m in h.read()]
    M, nq = 80, 9 * 7 * 6
    qx, qy, qz = (g.transpose(2, 1, 0).ravel() for g in np.meshgrid(xs, ys, zs, indexing="ij"))
    vol = tt.voxel_weights(xs, ys, zs).transpose(2, 1, 0).ravel()
    tnode = cref.oracle_np.rasterize([board.cells()], qx, qy, qz)[2][0]
    assert set(tnode.tolist()) == {5.0, 15.0}
    ref = cref.recovery([m.cells() for m in flat], qx, qy, qz, tnode, None, vol, True)
    pit = (ref["below"] + 0.5 * ref["equal"]) / M
    inside = (0.05 <= pit) & (pit <= 0.95)

    def grid(a):
        return a.reshape(6, 7, 9).transpose(2, 1, 0)

    out = tt.posterior_recovery(hists, sds, prm, board, bins=(8, 0.0, 800.0), convergence=True, xs=xs, ys=ys, zs=zs)
    assert out["names"] == ["all"] and out["msd"].shape == (M, 1)
    for f, want in (("truth", tnode), ("bias", ref["dmean"]), ("std", ref["dstd"]), ("below", ref["below"]),
                    ("equal", ref["equal"]), ("above", ref["above"]), ("pit", pit), ("inside", inside)):
        assert np.array_equal(out[f], grid(want), equal_nan=f in ("bias", "std")), f
    assert np.array_equal(out["msd"][:, 0], ref["series"][:, 0]) and np.array_equal(out["rms"], np.sqrt(out["msd"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(out["zscore"], grid(ref["dmean"] / ref["dstd"]), equal_nan=True)
    assert np.array_equal(out["msd_mean"], ref["mean"]) and np.array_equal(out["msd_std"], ref["std"])
    assert np.isclose(out["coverage"][0], np.sum(vol * inside) / np.sum(vol), rtol=1e-13)
    assert np.isclose(out["mean_model_rms"][0], np.sqrt(np.sum(vol * ref["dmean"] ** 2) / np.sum(vol)), rtol=1e-13)
    assert out["pit_hist"].sum() == nq and np.array_equal(out["pit_hist"], np.histogram(pit, bins=10, range=(0, 1))[0])
    # the mean model is closer to the truth than the samples are on average (Jensen, the weights being positive)
    assert out["mean_model_rms"][0] ** 2 < out["msd_mean"][0]
    assert out["msd_quantiles"].shape == (3, 1) and out["msd_hist"].shape == (1, 11) and out["rhat"].shape == (1,)
    assert out["summary"]["m"] == 4 and np.isclose(out["rms_mean"][0], out["rms"].mean())
    # the truth as node values [nx, ny, nz]; named regions; Models in nested lists
    regs = dict(tt.depth_layers(zs, [zmin, 0.5 * (zmin + zmax), zmax + 1.0]))
    nested = [[m for m in h.read()] for h in hists if len(h)]
    o2 = tt.posterior_recovery(nested, sds, prm, grid(tnode), regs, bins=(8, 0.0, 800.0), convergence=True, xs=xs, ys=ys, zs=zs)
    for f in ("truth", "bias", "std", "zscore", "below", "equal", "above", "pit", "inside", "pit_hist"):
        assert np.array_equal(o2[f], out[f], equal_nan=True), f
    names, px, py, pz, w, off = tt.region_points(regs, xs, ys, zs, "volume")
    assert o2["names"] == names and len(names) == 2 and o2["msd"].shape == (M, 2) and o2["rhat"].shape == (2,)
    tp = cref.oracle_np.rasterize([board.cells()], px, py, pz)[2][0]
    r2 = cref.recovery([m.cells() for m in flat], px, py, pz, tp, off, w, True)
    assert np.array_equal(o2["msd"], r2["series"]) and np.array_equal(o2["weight"], r2["weight"])
    assert np.array_equal(o2["msd_mean"], r2["mean"]) and o2["msd_quantiles"].shape == (3, 2)
    pit2 = (r2["below"] + 0.5 * r2["equal"]) / M
    in2 = (0.05 <= pit2) & (pit2 <= 0.95)
    for r in range(2):
        a, b = off[r], off[r + 1]
        assert np.isclose(o2["coverage"][r], np.sum(w[a:b] * in2[a:b]) / np.sum(w[a:b]), rtol=1e-13)
        assert np.isclose(o2["mean_model_rms"][r], np.sqrt(np.sum(w[a:b] * r2["dmean"][a:b] ** 2) / np.sum(w[a:b])), rtol=1e-13)
    with pytest.raises(ValueError, match="free points need a Model"):
        tt.posterior_recovery(hists, sds, prm, grid(tnode), dict(path=([0.0], [0.0], [1.0])), xs=xs, ys=ys, zs=zs)


# ---------------------------------------------------------------- end to end

E2E_PROPOSALS, E2E_FIRST, E2E_EVERY = 16000, 4000, 100


def test_exact_synthetic_data_pull_the_chain_towards_the_truth(tt, ds):
    """The shipped 381 rays, truth = a checkerboard of 2 x 1 x 2 blocks with zeta 5 and 15 (both far from the prior's
    mean of 25), exact synthetic data.  Two recorded chains from random_model(200, seed) with the same seed, length
    and thinning, one on the data and one with debug_prior = 1: over the nodes that rays pass (ray_density > 0) the
    data chain's median RMS distance to the truth lies below the prior chain's.  The length is short because the
    data chain is not cheap here: it sheds cells until few are left (7 of the 200 after 10^5 proposals), each owning
    thousands of the 16 845 ray points, and a proposal then costs 0.46 ms (10^5 proposals: 36.5 s, against 0.36 s for
    the prior chain).  Measured medians: 3.06 against 19.71 at 10^5 proposals, 3.97 against 19.32 at
    4 x 10^4, and 7.90 against 19.94 at the 16 000 used here (0.7 s for the whole test)."""
    t0 = time.time()
    prm = tt.define_TDstructrure().replace(max_cells=400)
    board = tt.checkerboard_model(ds.xVec, ds.yVec, ds.zVec, blocks=(2, 1, 2), lo=5.0, hi=15.0)
    syn = tt.synthetic_data(ds, board, prm, noise=0)
    exact, _, valid = tt.evaluate(board.copy(), ds, prm)
    assert valid == 1 and np.array_equal(np.ravel(syn.tS), np.ravel(exact.ptS)) and syn is not ds
    assert not np.array_equal(np.ravel(syn.tS), np.ravel(ds.tS))
    mask = tt.ray_density(ds)["density"] > 0
    assert 0 < mask.sum() < mask.size
    nsamp = (E2E_PROPOSALS - E2E_FIRST) // E2E_EVERY + 1
    medians = {}
    for name, p in (("data", prm), ("prior", prm.replace(debug_prior=1))):
        c = tt.context_for(syn)
        chain = tt.Chain(c, tt.chain_params(p, syn, seed=41, chain=1), tt.random_model(200, 41))
        h = tt.History(c, nsamp, nsamp * 400, with_ptS=False)
        chain.run_recorded(E2E_PROPOSALS, E2E_FIRST, E2E_EVERY, h)
        assert len(h) == nsamp
        out = tt.posterior_recovery([h], syn, prm, board, {"rays": mask}, probs=())
        medians[name] = float(np.median(out["rms"][:, 0]))
        h.close()
        chain.close()
    tt.context_for(syn).close()
    print("median rms over the nodes with rays: data %.4f, prior %.4f (%d samples each, %.1f s)" % (
        medians["data"], medians["prior"], nsamp, time.time() - t0))
    assert medians["data"] < medians["prior"], medians
