"""GPU: posterior predictive data (td_rasterize_predict, td_history_predict, posterior_predictive).  Every
model's row of ptS and its phi must equal td_evaluate's -- the C oracle's -- bit for bit, whatever the
sweep, the slab of ray points and the chunk of models; the statistics must equal what the section calls'
kernels give for the matrix ptS as a value matrix.  Every assertion is equality."""
import numpy as np
import pytest

import convergence_ref as cref
from oracle import oracle_np
from test_gpu_marginals import ref_hist, ref_quantiles

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
BINS = (50, 0.0, 2.0)


def ref_eval(orc, ds, cells):
    r = orc.evaluate(ds.rayX, ds.rayY, ds.rayZ, ds.rayL, ds.rayU, ds.tS, ds.allSig, cells, 0)
    assert r["rc"] == 0
    return r


@pytest.fixture(scope="module")
def ctx(tt, ds):
    c = tt.TdContext.from_datastruct(ds)
    yield c
    c.close()


def reset(c):
    c.set_predict_plan(0, 0)
    c.set_predict_placement(False)
    c.set_volume_method(c.VOL_AUTO)
    c.set_volume_slab_nodes(0)
    c.set_volume_counting(False)


def hostile_models(tt, ds):
    """The cases of test_gpu_evaluate.py::test_ties_duplicates_and_sentinel and the sizes around them."""
    base = tt.random_model(300, 11)
    x, y, z, zeta = (np.concatenate([a, a[::3]]) for a in base.cells())
    zeta[300:] += 1.0  # every third cell again later, with another zeta: the first index must win
    dup = (x, y, z, zeta)
    px, py, pz = (a[~np.isnan(a)] for a in (ds.rayX, ds.rayY, ds.rayZ))
    sel = np.arange(0, len(px), 97)  # cells exactly on ray points, and mirrored pairs equidistant to them
    on_points = (np.concatenate([px[sel], px[sel] + 3.0, px[sel] - 3.0]), np.concatenate([py[sel]] * 3),
                 np.concatenate([pz[sel]] * 3), np.arange(3 * len(sel), dtype=np.float64) % 50)
    far = (np.full(4, 1e5), np.zeros(4), np.zeros(4), np.ones(4))  # beyond the sentinel distance: zeta 0
    x, y, z, zeta = (a.copy() for a in tt.random_model(600, 8).cells())
    x[311] = np.nan  # never wins
    z[7::60] = np.nan
    models = [(np.zeros(0),) * 4, tt.random_model(1, 7).cells(), tt.random_model(63, 5).cells(), dup, on_points, far,
              (x, y, z, zeta), tt.random_model(700, 3).cells(), tt.random_model(2000, 100).cells()]
    assert [len(m[0]) for m in models][:4] == [0, 1, 63, 400] and len(models) == 9
    return models


@pytest.fixture(scope="module")
def hostile(tt, orc, ds, ctx):
    models = hostile_models(tt, ds)
    refs = [ref_eval(orc, ds, m) for m in models]
    ptS = np.array([r["ptS"] for r in refs])
    phi = np.array([r["phi"] for r in refs])
    b_ptS, b_phi, _ = ctx.evaluate_batch(models)
    assert np.array_equal(b_ptS, ptS) and np.array_equal(b_phi, phi)
    assert np.all(ptS[0] == 0.0) and np.all(ptS[5] == 0.0) and phi[0] == phi[5]
    ptS.setflags(write=False)
    phi.setflags(write=False)
    return models, ptS, phi


@pytest.mark.parametrize("method", [0, 1, 2])
def test_hostile_models_on_the_shipped_rays(tt, ctx, hostile, method):
    models, ptS, phi = hostile
    longest = int(np.max(np.sum(~np.isnan(ctx._arrays[0]), axis=1)))
    assert 64 < longest  # slab points 64 are raised to the longest ray
    try:
        ctx.set_volume_method(method)
        for slab in (64, 4096, 0):
            for chunk in (1, 4, 0):
                ctx.set_predict_plan(slab, chunk)
                for rep in range(2):  # (the order inside a bucket differs from run to run)
                    r = ctx.predict(models, want_values=True)
                    assert r["ptS"].shape == ptS.shape and r["phi"].shape == phi.shape
                    bad = np.flatnonzero((r["ptS"] != ptS).any(axis=1))
                    assert np.array_equal(r["ptS"], ptS), (method, slab, chunk, rep, bad)
                    assert np.array_equal(r["phi"], phi), (method, slab, chunk, rep)
                    assert r["quantiles"] is None and r["hist"] is None and "rhat" not in r
        # every (model, point) pair is searched exactly once, by the sweep asked for
        ctx.set_volume_counting(True)
        for plan in ((64, 4), (0, 0)):
            ctx.set_predict_plan(*plan)
            r = ctx.predict(models, want_values=True)
            c = ctx.volume_counters()
            print("method %d plan %s counters %s" % (method, plan, c))
            assert sum(c) == len(models) * ctx.P
            assert (c[3] == sum(c)) if method == 2 else (c[3] == 0 and c[0] > 0)
            assert np.array_equal(r["ptS"], ptS) and np.array_equal(r["phi"], phi)
        ctx.set_volume_counting(False)
        ctx.set_predict_placement(True)  # the ray sums of model m on XCD m % 8
        for plan in ((64, 4), (4096, 1), (0, 0)):
            ctx.set_predict_plan(*plan)
            r = ctx.predict(models, want_values=True)
            assert np.array_equal(r["ptS"], ptS) and np.array_equal(r["phi"], phi)
        # phi alone, ptS alone (no statistics): the same numbers
        assert np.array_equal(ctx.predict(models)["phi"], phi)
    finally:
        reset(ctx)


def edge_datastruct(tt):
    """Rays of every class of wave_ray_sum and the boundaries between them: 0, 1 and 2 points; 15 and 16 (the
    sequential sums end at 15 segments); 17, 34, 35 (the first accumulator step takes 34 segments); 1025 (the
    last single block) and 1026, 2100, 4200 (Julia's pairwise split, one, two and three levels deep); a NaN
    inside a valid point."""
    def line(a, d, m):
        return np.asarray(a, dtype=np.float64) + np.linspace(0, 1, m)[:, None] * np.asarray(d, dtype=np.float64)

    rays = [np.zeros((0, 3)), np.array([[1.0, 2.0, 3.0]]), np.array([[0, 0, 0], [10, 0, 5.0]]),
            line([20.0, -100.0, 600.0], [800.0, 300.0, -600.0], 2100),
            np.array([[100.0, 10.0, 50.0], [110.0, np.nan, 60.0], [120.0, 12.0, 70.0]]),
            line([300.0, 50.0, 100.0], [50.0, 20.0, 30.0], 9), line([500.0, -50.0, 200.0], [-80.0, 40.0, 60.0], 17),
            line([900.0, 300.0, 10.0], [-700.0, -400.0, 500.0], 1025), line([50.0, 0.0, 30.0], [90.0, 60.0, 80.0], 15),
            line([100.0, 350.0, 620.0], [850.0, -500.0, -600.0], 1026), line([700.0, 200.0, 400.0], [-60.0, 90.0, 100.0], 16),
            line([400.0, -200.0, 50.0], [200.0, 300.0, 250.0], 34), line([250.0, 100.0, 500.0], [300.0, -150.0, -400.0], 35),
            line([0.0, -240.0, 0.0], [1000.0, 600.0, 640.0], 4200), np.array([[640.0, 20.0, 300.0], [660.0, 30.0, 280.0]])]
    m, n = 4200, len(rays)
    X, Y, Z = (np.full((m, n), np.nan) for _ in range(3))
    for i, r in enumerate(rays):
        X[:len(r), i], Y[:len(r), i], Z[:len(r), i] = r[:, 0], r[:, 1], r[:, 2]
    U = np.where(np.isnan(X), np.nan, 0.1 + 0.001 * np.nan_to_num(Z))
    L, Uu = tt.segments(X, Y, Z, U)
    L[0:2, 4] = [3.0, 4.0]  # (the NaN in Y makes two lengths NaN: kept finite so that the layout is valid)
    tS = np.linspace(0.1, 0.5, n)
    sig = np.linspace(0.05, 0.3, n)
    return tt.DataStruct(tS, tS, tS, tS, sig, tS, tS, tS, tS, tS, tS, tS, tS, tS, tS, tS, tS, X, Y, Z, L, Uu, U), \
        [len(r) for r in rays]


def test_edge_rays(tt, orc):
    ds2, lens = edge_datastruct(tt)
    c2 = tt.TdContext.from_datastruct(ds2)
    try:
        models = [tt.random_model(nc, seed).cells() for nc, seed in ((1, 1), (37, 2), (300, 4), (2000, 5))]
        refs = [ref_eval(orc, ds2, m) for m in models]
        ptS, phi = np.array([r["ptS"] for r in refs]), np.array([r["phi"] for r in refs])
        assert np.all(ptS[:, :2] == 0.0)
        # forced 64 points are raised to the longest ray: three slabs, one of them the 4200-point ray's
        assert tt.TdContext.predict_plan(4, lens, forced_points=64)[2] == [0, 11, 13, 15]
        assert tt.TdContext.predict_plan(4, lens)[2] == [0, 15]
        for method in (c2.VOL_AUTO, c2.VOL_BRUTE):
            c2.set_volume_method(method)
            for plan in ((64, 0), (64, 1), (64, 3), (8192, 2), (0, 0)):
                c2.set_predict_plan(*plan)
                for placement in (False, True):
                    c2.set_predict_placement(placement)
                    r = c2.predict(models, want_values=True)
                    bad = np.argwhere(r["ptS"] != ptS)
                    assert np.array_equal(r["ptS"], ptS), (method, plan, placement, bad[:8])
                    assert np.array_equal(r["phi"], phi), (method, plan, placement)
    finally:
        c2.close()


def julia_mean_std(V):
    """Statistics.mean / std over the rows of V in Julia's association (oracle_np.rasterize's)."""
    rows = [V[k] for k in range(len(V))]
    mean = oracle_np.julia_mapreduce_arrays(rows) / float(len(rows))
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(oracle_np.julia_mapreduce_arrays([(v - mean) * (v - mean) for v in rows]) / float(len(rows) - 1))
    return mean, std


@pytest.fixture(scope="module")
def recorded(tt, ds, ctx):
    """Two DEVICE chains of 200 cells on the shipped rays, 200 proposals, every 5th recorded with its ptS."""
    prm = tt.define_TDstructrure().replace(max_cells=300)
    hists = []
    for k in range(2):
        c = tt.Chain(ctx, tt.chain_params(prm, None, seed=70 + k, chain=k + 1), tt.random_model(200, 70 + k))
        h = tt.History(ctx, 40, 40 * 300, with_ptS=True)
        c.run_recorded(200, 5, 5, h)
        assert len(h) == 40
        hists.append(h)
        c.close()
    arrays = [h.read_arrays() for h in hists]
    V = np.concatenate([a["ptS"] for a in arrays])
    phi = np.concatenate([a["phi"] for a in arrays])
    V.setflags(write=False)
    phi.setflags(write=False)
    return hists, V, phi


def test_a_recorded_ensemble_pins_itself(tt, ds, ctx, recorded):
    hists, V, phi = recorded
    assert V.shape == (80, ctx.n) and len(np.unique(phi)) > 10
    want = dict(ptS=V, phi=phi)
    want["mean"], want["std"] = julia_mean_std(V)
    want["quantiles"], want["hist"] = ref_quantiles(V, PROBS), ref_hist(V, BINS)
    want.update(cref.convergence(V, [40, 40]))
    dev = ctx.convergence(V, [40, 40])  # td_convergence_values on the matrix read back
    for f in ("rhat", "ess", "lags"):
        assert np.array_equal(dev[f], want[f], equal_nan=True), f
    assert np.isfinite(want["rhat"]).any() and (want["hist"].sum(axis=1) == 80).all()
    empty = tt.History(ctx, 4, 4 * 300, with_ptS=True)
    fields = ("ptS", "phi", "mean", "std", "quantiles", "hist", "rhat", "ess", "lags")

    def same(r):
        for f in fields:
            assert r[f].shape == want[f].shape and r[f].dtype == want[f].dtype, f
            assert np.array_equal(r[f], want[f], equal_nan=r[f].dtype.kind == "f"), f

    try:
        ctx.timing(enable=True, reset=True)
        same(ctx.predict_history(hists, PROBS, BINS, convergence=True, want_values=True))
        launches = {k: ctx.timing(kernel=k)[0] for k in ("vol_boxes", "vol_grid_build", "vol_search", "pred_ray_sums",
                                                         "pred_chi2", "raster_brute")}
        ctx.timing(enable=False)
        assert launches == dict(vol_boxes=1, vol_grid_build=1, vol_search=1, pred_ray_sums=1, pred_chi2=1,
                                raster_brute=0), launches
        same(ctx.predict_history([hists[0], empty, hists[1]], PROBS, BINS, convergence=True, want_values=True))
        ctx.set_predict_plan(64, 7)
        ctx.set_volume_slab_nodes(64)  # the statistics in six slabs of rays gathered from the matrix
        same(ctx.predict_history([empty, hists[0], hists[1]], PROBS, BINS, convergence=True, want_values=True))
        ctx.set_volume_method(ctx.VOL_BRUTE)
        same(ctx.predict_history(hists, PROBS, BINS, convergence=True, want_values=True))
        reset(ctx)
        # the models read back: the host-array entry point, same numbers; a lag cap is the section call's
        flat = [m.cells() for h in hists for m in h.read()]
        same(ctx.predict(flat, PROBS, BINS, chain_len=[40, 40], want_values=True))
        r7 = ctx.predict(flat, chain_len=[40, 40], max_lag=7)
        c7 = ctx.convergence(V, [40, 40], max_lag=7)
        for f in ("rhat", "ess", "lags"):
            assert np.array_equal(r7[f], c7[f], equal_nan=True), f
        with pytest.raises(tt.TdError, match="td_history_predict: the histories hold no sample"):
            ctx.predict_history([empty])
        with pytest.raises(tt.TdError, match="td_rasterize_predict"):
            ctx.predict(flat, chain_len=[40, 39])
    finally:
        ctx.timing(enable=False)
        reset(ctx)
        empty.close()


def test_held_out_rays(tt, orc, ds, ctx, recorded):
    hists, V, phi = recorded
    held = tt.synthetic_rays(50)
    c50 = tt.TdContext.from_datastruct(held)
    try:
        models = [m.cells() for h in hists for m in h.read()]
        b_ptS, b_phi, _ = c50.evaluate_batch(models)
        r = c50.predict_history(hists, PROBS, convergence=True, want_values=True)
        assert r["ptS"].shape == (80, 50)
        assert np.array_equal(r["ptS"], b_ptS) and np.array_equal(r["phi"], b_phi)
        assert not np.array_equal(b_phi, phi)  # (other rays, other data)
        mean, std = julia_mean_std(b_ptS)
        assert np.array_equal(r["mean"], mean) and np.array_equal(r["std"], std, equal_nan=True)
        assert np.array_equal(r["quantiles"], ref_quantiles(b_ptS, PROBS), equal_nan=True)
        want = cref.convergence(b_ptS, [40, 40])
        for f in ("rhat", "ess", "lags"):
            assert np.array_equal(r[f], want[f], equal_nan=True), f
        # the histories and their own context are as they were
        again = [h.read_arrays() for h in hists]
        assert np.array_equal(np.concatenate([a["ptS"] for a in again]), V)
        cells = tt.random_model(300, 21).cells()
        ptS1, phi1, _, _ = ctx.evaluate(cells)
        ref = ref_eval(orc, ds, cells)
        assert np.array_equal(ptS1, ref["ptS"]) and phi1 == ref["phi"]
        # another allSig on the predicting context: phi is td_misfit's for it, ptS is untouched
        sig = np.linspace(0.07, 0.9, 50)
        c50.set_sigma(sig)
        r2 = c50.predict_history(hists, want_values=True)
        assert np.array_equal(r2["ptS"], b_ptS)
        mis = np.array([c50.misfit(b_ptS[k], held.tS, sig)[0] for k in range(80)])
        assert np.array_equal(r2["phi"], mis) and not np.array_equal(r2["phi"], b_phi)
        # a history of another device would be refused; one of this device's other context is not
        assert c50.device == ctx.device
    finally:
        c50.close()


def test_posterior_predictive_end_to_end(tt, ds, recorded):
    hists, V, phi = recorded
    prm = tt.define_TDstructrure()
    nested = [h.read() for h in hists]
    kw = dict(probs=PROBS, bins=BINS, convergence=True, values=True)
    a = tt.posterior_predictive(hists, ds, prm, **kw)      # (ds's own cached context: not the histories')
    b = tt.posterior_predictive(nested, ds, prm, **kw)
    one_h = tt.posterior_predictive(hists[0], ds, prm, **kw)
    one_m = tt.posterior_predictive(nested[0], ds, prm, **kw)
    for x, y in ((a, b), (one_h, one_m)):
        assert sorted(x) == sorted(y) == sorted(["phi", "mean", "std", "residual", "quantiles", "coverage", "hist", "ptS",
                                                  "rhat", "ess", "lags", "summary"])
        for f in x:
            if f == "summary":
                assert x[f].keys() == y[f].keys()
                assert all(np.array_equal(x[f][k], y[f][k], equal_nan=True) for k in x[f]), (f, x[f], y[f])
            else:
                assert np.array_equal(x[f], y[f], equal_nan=True), f
    assert np.array_equal(a["ptS"], V) and np.array_equal(a["phi"], phi)
    assert np.array_equal(one_h["ptS"], V[:40]) and one_h["summary"]["m"] == 2 and a["summary"]["m"] == 4
    tS, sig = np.asarray(ds.tS, dtype=np.float64), np.asarray(ds.allSig, dtype=np.float64)
    assert np.array_equal(a["residual"], (a["mean"] - tS) / sig)
    q = a["quantiles"]
    assert q.shape == (3, len(tS)) and np.all(q[0] <= q[1]) and np.all(q[1] <= q[2])
    assert a["coverage"] == float(np.mean((tS >= q[0]) & (tS <= q[2])))
    # fewer outputs: one probability gives no coverage, no bins no histogram, and nothing is computed for them
    few = tt.posterior_predictive(hists, ds, prm, probs=(0.5,))
    assert sorted(few) == ["mean", "phi", "quantiles", "residual", "std"]
    assert np.array_equal(few["quantiles"][0], q[1]) and np.array_equal(few["mean"], a["mean"])
