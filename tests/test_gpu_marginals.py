"""GPU: posterior marginals (td_rasterize_marginals, td_history_marginals, td_history_zeta_hist) against
numpy, bit for bit: the value matrix of oracle_np.rasterize, per column np.sort and Julia's quantile
formula restated (np.quantile rounds differently), and floor((v - lo) / w) for the bins."""
import numpy as np
import pytest

from marginals_ref import rank, ref_hist, ref_quantiles, ref_slots  # noqa: F401 (test_gpu_predict imports them here)
from oracle import oracle_np

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.025, 0.05, 1 / 3, 0.5, 0.95, 1.0)


@pytest.fixture(scope="module")
def ctx(tt, ds):
    return tt.TdContext.from_datastruct(ds)


def check(ctx, models, qx, qy, qz, probs=PROBS, bins=(25, 0.0, 50.0), ref=None):
    """-> (the device result, (mean, std, V) of the oracle)"""
    r = ctx.marginals(models, qx, qy, qz, probs, bins)
    m2, s2, V = oracle_np.rasterize(models, qx, qy, qz) if ref is None else ref
    assert np.array_equal(r["mean"], m2, equal_nan=True) and np.array_equal(r["std"], s2, equal_nan=True)
    assert r["quantiles"].shape == (len(probs), len(qx))
    assert np.array_equal(r["quantiles"], ref_quantiles(V, probs), equal_nan=True)
    assert r["hist"].shape == (len(qx), bins[0] + 3) and r["hist"].dtype == np.int64
    assert np.array_equal(r["hist"], ref_hist(V, bins))
    assert np.all(r["hist"].sum(axis=1) == len(models))
    return r, (m2, s2, V)


def tiny_models(rng, M):
    return [tuple(rng.uniform([0, -200, 0, 0], [1000, 400, 600, 50], (6, 4)).T) for _ in range(M)]


def test_mixed_sizes(tt, ctx):
    rng = np.random.default_rng(0)
    qx, qy, qz = rng.uniform(-100, 1100, 700), rng.uniform(-200, 500, 700), rng.uniform(-10, 700, 700)
    models = [tt.random_model(n, 100 + k).cells() for k, n in enumerate([5, 40, 300, 1200, 7, 2000, 90, 600, 12, 100])]
    r, _ = check(ctx, models, qx, qy, qz)
    mean, std, _ = ctx.rasterize(models, qx, qy, qz)
    assert np.array_equal(r["mean"], mean) and np.array_equal(r["std"], std, equal_nan=True)
    # mean / std only; quantiles only; histogram only
    r0 = ctx.marginals(models, qx, qy, qz)
    assert r0["quantiles"] is None and r0["hist"] is None and np.array_equal(r0["mean"], mean)
    r1 = ctx.marginals(models, qx, qy, qz, probs=(0.5,))
    assert r1["hist"] is None and np.array_equal(r1["quantiles"][0], r["quantiles"][4])
    r2 = ctx.marginals(models, qx, qy, qz, bins=(25, 0.0, 50.0))
    assert r2["quantiles"] is None and np.array_equal(r2["hist"], r["hist"])


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 127, 128, 129])
def test_column_lengths(ctx, M):
    """130 nodes: neither a multiple of 64 nor of 128, so the last tile is partial."""
    rng = np.random.default_rng(M)
    qx, qy, qz = rng.uniform(0, 1000, 130), rng.uniform(-200, 400, 130), rng.uniform(0, 600, 130)
    check(ctx, tiny_models(rng, M), qx, qy, qz)


def test_ties_and_empties(ctx):
    """zeta of three values only: columns of ties.  Bins of width 10 on [-10, 30): -10 == lo, 10 on an
    edge, 30 == hi, and the largest double below hi, whose (v - lo) / w rounds to nbins (the clamp into
    the last bin); a model beyond the sentinel distance and an empty one give 0.0, on an edge too.
    Bins (2, 0, 20): -10 below lo, 0.0 == lo, 30 above hi."""
    top = np.nextafter(30.0, 0.0)
    assert top < 30.0 and (top - -10.0) / 10.0 == 4.0
    rng = np.random.default_rng(7)
    P = (500.0, 100.0, 300.0)
    regular = []
    for k in range(37):
        x, y, z, _ = rng.uniform([0, -200, 0, 0], [1000, 400, 600, 50], (6, 4)).T
        ze = rng.choice([-10.0, 10.0, 30.0], 6)
        x[2], y[2], z[2], ze[2] = P[0], P[1], P[2], 10.0  # every model's nearest cell at node 0
        regular.append((x, y, z, ze))
    below_hi = tuple(rng.uniform([0, -200, 0], [1000, 400, 600], (6, 3)).T) + (np.full(6, top),)
    far = (np.full(5, 4e4), np.full(5, 4e4), np.full(5, 4e4), np.full(5, 10.0))
    empty = (np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0))
    qx = np.concatenate([[P[0]], rng.uniform(0, 1000, 99)])
    qy = np.concatenate([[P[1]], rng.uniform(-200, 400, 99)])
    qz = np.concatenate([[P[2]], rng.uniform(0, 600, 99)])
    models = regular[:20] + [far, below_hi] + regular[20:] + [empty]
    bins = (4, -10.0, 30.0)
    r, ref = check(ctx, models, qx, qy, qz, bins=bins)
    V = ref[2]
    assert np.all(V[20] == 0.0) and np.all(V[-1] == 0.0) and np.all(V[21] == top)
    assert np.all(r["hist"][:, 0] == 0) and np.all(r["hist"][:, 6] == 0)
    assert np.all(r["hist"][:, 2] == 2)  # the far and the empty model: [0, 10)
    assert np.all(r["hist"][:, 4] == 1)  # the largest double below hi: the last bin, not slot nbins + 1
    assert r["hist"][:, 1].sum() > 0 and r["hist"][:, 3].sum() > 0 and r["hist"][:, 5].sum() > 0
    r, _ = check(ctx, models, qx, qy, qz, bins=(2, 0.0, 20.0), ref=ref)
    assert r["hist"][:, 0].sum() > 0 and np.all(r["hist"][:, 1] == 2) and np.all(r["hist"][:, 3] >= 1)
    r, (_, _, V) = check(ctx, regular, qx, qy, qz, bins=bins)
    assert np.all(V[:, 0] == 10.0) and np.all(r["quantiles"][:, 0] == 10.0)  # the all-equal column
    assert r["hist"][0, 3] == len(regular)


def test_nan_columns(tt, ctx):
    rng = np.random.default_rng(11)
    qx, qy, qz = rng.uniform(0, 1000, 300), rng.uniform(-200, 400, 300), rng.uniform(0, 600, 300)
    models = [tt.random_model(30 + k, 500 + k).cells() for k in range(21)]
    for k in (3, 17):
        x, y, z, ze = (a.copy() for a in models[k])
        ze[::4] = np.nan
        models[k] = (x, y, z, ze)
    bins = (25, 0.0, 50.0)
    r, (_, _, V) = check(ctx, models, qx, qy, qz, bins=bins)
    nanq = np.isnan(V).any(axis=0)
    assert nanq.any() and not nanq.all()
    assert np.array_equal(np.isnan(r["quantiles"]), np.broadcast_to(nanq, r["quantiles"].shape))
    assert np.array_equal(r["hist"][:, bins[0] + 2], np.isnan(V).sum(axis=0))
    assert np.all(r["hist"].sum(axis=1) == len(models))


def test_regimes_agree(tt, ctx):
    rng = np.random.default_rng(13)
    qx, qy, qz = rng.uniform(0, 1000, 130), rng.uniform(-200, 400, 130), rng.uniform(0, 600, 130)
    models = tiny_models(rng, 129)
    x, y, z, ze = (a.copy() for a in models[5])
    ze[:3] = np.nan
    models[5] = (x, y, z, ze)
    ref = oracle_np.rasterize(models, qx, qy, qz)
    got = {}
    try:
        for method in (tt.TdContext.MARG_RESIDENT, tt.TdContext.MARG_STREAMING):
            ctx.set_marginals_method(method)
            got[method], _ = check(ctx, models, qx, qy, qz, ref=ref)
            ctx.timing(enable=True, reset=True)
            ctx.marginals(models[:7], qx, qy, qz, PROBS, (25, 0.0, 50.0))
            assert ctx.timing(kernel="raster_quantile")[0] == 1 and ctx.timing(kernel="raster_node_hist")[0] == 1
            ctx.timing(enable=False)
    finally:
        ctx.timing(enable=False)
        ctx.set_marginals_method(tt.TdContext.MARG_AUTO)
    a, b = got[tt.TdContext.MARG_RESIDENT], got[tt.TdContext.MARG_STREAMING]
    assert np.array_equal(a["quantiles"], b["quantiles"], equal_nan=True) and np.array_equal(a["hist"], b["hist"])


def test_auto_at_the_resident_limit(tt, ctx):
    """M = resident_max (the largest sorted in LDS) and resident_max + 1 (the first radix select)."""
    rmax = ctx.marginals_resident_max()
    assert 1024 <= rmax <= 1 << 15
    rng = np.random.default_rng(17)
    qx, qy, qz = rng.uniform(0, 1000, 8), rng.uniform(-200, 400, 8), rng.uniform(0, 600, 8)
    models = tiny_models(rng, rmax + 1)
    V = oracle_np.rasterize(models, qx, qy, qz)[2]
    for M in (rmax, rmax + 1):
        r = ctx.marginals(models[:M], qx, qy, qz, PROBS, (25, 0.0, 50.0))
        assert np.array_equal(r["quantiles"], ref_quantiles(V[:M], PROBS))
        assert np.array_equal(r["hist"], ref_hist(V[:M], (25, 0.0, 50.0)))
    try:  # the resident regime cannot hold this column
        ctx.set_marginals_method(tt.TdContext.MARG_RESIDENT)
        with pytest.raises(tt.TdError):
            ctx.marginals(models, qx, qy, qz, PROBS)
    finally:
        ctx.set_marginals_method(tt.TdContext.MARG_AUTO)


def test_histories(tt, ds, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=300)
    hists, chains = [], []
    for k in range(2):
        c = tt.Chain(ctx, tt.chain_params(prm, None, seed=70 + k, chain=k + 1), tt.random_model(200, 70 + k))
        h = tt.History(ctx, 30, 30 * 300, with_ptS=False)
        c.run_recorded(300, 10, 10, h)
        assert len(h) == 30
        hists.append(h)
        chains.append(c)
    flat = [m.cells() for h in hists for m in h.read()]
    gx, gz = np.meshgrid(np.linspace(-50, 1050, 37), np.linspace(0, 660, 11))
    qx, qz = gx.ravel(), gz.ravel()
    qy = np.full(qx.shape, 150.0)
    bins = (25, 0.0, 50.0)
    a = ctx.marginals_history(hists, qx, qy, qz, PROBS, bins)
    b = ctx.marginals(flat, qx, qy, qz, PROBS, bins)
    for f in ("mean", "std", "quantiles", "hist"):
        assert np.array_equal(a[f], b[f], equal_nan=f != "hist"), f
    V = ctx.rasterize_history(hists, qx, qy, qz, want_values=True)[2]
    assert np.array_equal(a["quantiles"], ref_quantiles(V, PROBS)) and np.array_equal(a["hist"], ref_hist(V, bins))
    # the ensemble distributions: bins whose edges the prior's zeta range straddles
    for zb in ((50, 0.0, 50.0), (7, 3.0, 41.5), (4096, 0.0, 50.0)):
        arrs = [h.read_arrays() for h in hists]
        for h, arr in zip(hists, arrs):
            d = h.distributions(zb)
            assert np.array_equal(d["zeta_hist"], np.bincount(ref_slots(arr["zeta"], zb), minlength=zb[0] + 3))
            assert d["zeta_hist"].sum() == h.count()[1]
            assert np.array_equal(d["ncells"], np.diff(arr["off"]))
        d = tt.model_distributions(hists, zb)
        zeta = np.concatenate([arr["zeta"] for arr in arrs])
        assert np.array_equal(d["zeta_hist"], np.bincount(ref_slots(zeta, zb), minlength=zb[0] + 3))
        assert d["zeta_hist"].sum() == sum(h.count()[1] for h in hists)
        assert np.array_equal(d["ncells"], np.concatenate([np.diff(arr["off"]) for arr in arrs]))


def test_credible_maps(tt, ds):
    prm = tt.define_TDstructrure().replace(xzMap=True, ySlice=[0, 150], xyMap=True, zSlice=[100])
    hist = [[tt.random_model(80 + 10 * j, 10 * c + j) for j in range(6)] for c in range(2)]
    before = tt.plot_model_hist(hist, ds, prm)
    probs, bins = (0.05, 0.5, 0.95), (10, 0.0, 50.0)
    maps = tt.credible_maps(hist, ds, prm, bins=bins)
    after = tt.plot_model_hist(hist, ds, prm)
    assert set(maps) == set(before) == {("xz", 0), ("xz", 150), ("xy", 100)}
    xv, yv, zv = (np.asarray(v, dtype=np.float64) for v in (ds.xVec, ds.yVec, ds.zVec))
    for key, m in maps.items():
        n2 = len(zv) if key[0] == "xz" else len(yv)
        assert m["quantiles"].shape == (3, len(xv), n2) and m["hist"].shape == (len(xv), n2, bins[0] + 3)
        assert m["width"].shape == m["mean"].shape == m["std"].shape == before[key]["mean"].shape == (len(xv), n2)
        assert np.array_equal(m["width"], m["quantiles"][-1] - m["quantiles"][0])
        assert np.array_equal(m["mean"], before[key]["mean"]) and np.array_equal(m["std"], before[key]["std"])
        assert np.all(m["quantiles"][0] <= m["quantiles"][1]) and np.all(m["quantiles"][1] <= m["quantiles"][2])
        for f in ("mean", "std", "masked"):  # plot_model_hist is what it was
            assert np.array_equal(before[key][f], after[key][f], equal_nan=True)
    assert "hist" not in tt.credible_maps(hist, ds, prm.replace(xyMap=False, ySlice=[0]), probs=(0.5,))[("xz", 0)]
    ctx = tt.context_for(ds)
    flat = [m.cells() for chain in hist for m in chain]
    i, j = 7, 11
    for key, node in ((("xz", 150), ([xv[i]], [150.0], [zv[j]])), (("xy", 100), ([xv[i]], [yv[j]], [100.0]))):
        one = ctx.marginals(flat, *node, probs, bins)
        assert np.array_equal(maps[key]["quantiles"][:, i, j], one["quantiles"][:, 0])
        assert np.array_equal(maps[key]["hist"][i, j], one["hist"][0])
        V = oracle_np.rasterize(flat, *node)[2]
        assert np.array_equal(one["quantiles"], ref_quantiles(V, probs))
    # plot_model_hist against the oracle, as before
    vals = [oracle_np.rasterize([c], [xv[i]], [150.0], [zv[j]])[0][0] for c in flat]
    assert after[("xz", 150)]["mean"][i, j] == oracle_np.julia_mapreduce_arrays([np.array([v]) for v in vals])[0] / len(vals)
