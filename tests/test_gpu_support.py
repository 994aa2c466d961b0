"""GPU: posterior data support (td_rasterize_support, td_history_support, posterior_support, ray_density) against the
numpy restatement of its definition (tests/support_ref.py), bit for bit: the base case under every weighting, slab
size, sweep and scatter mode, a metre frame whose points are mostly orphans, a model above the LDS cap, the history
form on another context's histories, and the statistics against the calls they are taken from."""
import numpy as np
import pytest

import support_ref as sref

pytestmark = pytest.mark.gpu

FIELDS = ("cell", "count", "barren", "orphans", "values", "mean", "std", "exceed")
THR = {"none": (0.0, 10.0), "tstar": (0.0, 0.01), "signed": (0.0, -1.0, 1.0)}


def same(r, ref, fields=FIELDS):
    for f in fields:
        a, b = r[f], ref[f]
        assert a.shape == b.shape and a.dtype == b.dtype, (f, a.shape, b.shape, a.dtype, b.dtype)
        bad = ~((a == b) | ((a != a) & (b != b)))
        assert not bad.any(), "%s: %d of %d differ, first at %s: %r against %r" % (
            f, bad.sum(), a.size, np.argwhere(bad)[0], a[bad][0], b[bad][0])


def context(tt, rays):
    return tt.TdContext(rays.rayX, rays.rayY, rays.rayZ, rays.rayL, rays.rayU, rays.tS, rays.allSig)


def reset(tt, c):
    c.set_volume_slab_nodes(0)
    c.set_volume_method(tt.TdContext.VOL_AUTO)
    c.set_support_scatter(tt.TdContext.SUP_AUTO)


def weights(tt, rays, kind):
    if kind == "none":
        return None
    if kind == "tstar":
        return tt.support_weights(rays, "tstar")
    return np.random.default_rng(12).normal(0.0, 1.0, len(rays.px))


@pytest.fixture(scope="module")
def base(tt, ds):
    """The base case, its context, and the restatement's answer per weighting: computed once, never modified."""
    rays, models, q = sref.base_case(tt, ds)
    ref = {k: sref.support(models, rays.px, rays.py, rays.pz, weights(tt, rays, k), *q, thr=THR[k]) for k in THR}
    c = context(tt, rays)
    assert c.P == len(rays.px)
    yield dict(rays=rays, models=models, q=q, ref=ref, ctx=c)
    reset(tt, c)
    c.close()


def test_the_base_case_is_contested(base):
    """Otherwise the comparisons below prove nothing."""
    models, ref = base["models"], base["ref"]["none"]
    M, P = len(models), len(base["rays"].px)
    sizes = np.array([len(m[0]) for m in models])
    off = np.concatenate(([0], np.cumsum(sizes)))
    assert np.sum((ref["barren"] > 0) & (ref["barren"] < sizes)) >= M / 2  # barren and non-barren cells side by side
    assert ref["count"].max() >= 64  # one wave's lanes collide on one LDS word
    dup = ref["count"][off[sref.DUPLICATES]:off[sref.DUPLICATES + 1]]
    assert dup[0] > 0 and dup[1] == 0  # of two exact duplicates the lower index owns everything
    assert ref["barren"][65] == 0 and ref["orphans"][65] == P  # no cell: every point is an orphan
    assert ref["count"][off[66]] == P  # one cell owns every point
    assert np.all(ref["count"].sum() + ref["orphans"].sum() == M * P)
    assert P % 64 and P > 3 * 64 and len(base["q"][0]) == 150  # at least 3 slabs of 64 in both phases, the last partial
    for k in THR:  # the supports differ from sample to sample, and the thresholds split the samples
        r = base["ref"][k]
        assert np.all(r["std"] > 0) and any(np.any((x > 0) & (x < M)) for x in r["exceed"])
    assert np.any(base["ref"]["signed"]["cell"] < 0) and base["ref"]["tstar"]["e"] != 0


@pytest.mark.parametrize("kind", list(THR))
def test_base_case_whatever_the_slab_the_sweep_and_the_scatter(tt, base, kind):
    c, rays, models, q, ref = base["ctx"], base["rays"], base["models"], base["q"], base["ref"][kind]
    w = weights(tt, rays, kind)
    T = tt.TdContext
    M, P, nq = len(models), len(rays.px), len(q[0])
    runs = []
    try:
        for slab in (64, 0):
            for method in (T.VOL_GRID, T.VOL_BRUTE):
                for mode in (T.SUP_AUTO, T.SUP_LDS, T.SUP_GLOBAL):
                    c.set_volume_slab_nodes(slab)
                    c.set_volume_method(method)
                    c.set_support_scatter(mode)
                    c.timing(enable=True, reset=True)
                    try:
                        r = c.support(models, w, *q, thresholds=THR[kind], want_values=True)
                        ps, qs = (-(-P // slab), -(-nq // slab)) if slab else (1, 1)
                        assert c.timing(kernel="sup_index")[0] == 1 and c.timing(kernel="sup_finish")[0] == 1
                        assert c.timing(kernel="sup_scatter")[0] == ps and c.timing(kernel="sup_exceed")[0] == qs
                    finally:
                        c.timing(enable=False)
                    cnt = c.volume_counters()
                    assert (cnt[3] == M * (P + nq) and sum(cnt[:3]) == 0) if method == T.VOL_BRUTE else (cnt[3] == 0), cnt
                    runs.append(r)
    finally:
        reset(tt, c)
    runs.append(c.support(models, w, *q, thresholds=THR[kind], want_values=True))  # automatic in all, a repeated call
    for r in runs:
        same(r, ref)
    if kind == "none":  # NULL weights are an array of ones, bit for bit
        ones = c.support(models, np.ones(P), *q, thresholds=THR[kind], want_values=True)
        same(ones, runs[0])
        assert np.array_equal(ones["cell"], ones["count"].astype(np.float64))
    few = c.support(models, w)  # without nodes: the per-cell and per-model outputs alone
    same(few, ref, FIELDS[:4])
    assert few["mean"] is None and few["exceed"] is None
    fewer = c.support(models, w, want_cells=False)  # the per-model outputs alone
    same(fewer, ref, ("barren", "orphans"))
    assert fewer["cell"] is None and fewer["count"] is None


def test_metre_frame_orphans(tt, ds):
    """Everything times 1000: most ray points lie beyond the sentinel of every cell, and most nodes pick none."""
    rays, models, q = sref.base_case(tt, ds, metres=True)
    w = tt.support_weights(rays, "length")
    ref = sref.support(models, rays.px, rays.py, rays.pz, w, *q, thr=(0.0,))
    P = len(rays.px)
    assert np.all(ref["orphans"] > 0) and np.any(ref["orphans"] < P) and np.any(ref["count"] > 0)
    assert np.any(ref["values"] > 0) and np.mean(ref["values"] == 0) > 0.5
    c = context(tt, rays)
    try:
        for slab in (64, 0):
            c.set_volume_slab_nodes(slab)
            same(c.support(models, w, *q, thresholds=(0.0,), want_values=True), ref)
    finally:
        reset(tt, c)
        c.close()


def test_a_model_above_the_lds_cap(tt, base):
    """One model of tdt_support_lds_cells() + 1 cells between small ones: under auto its sums go to the global arrays
    while its neighbours' stay in LDS, in one launch."""
    c, rays, q = base["ctx"], base["rays"], base["q"]
    cap = tt.TdContext.support_lds_cells()
    assert cap == 5120
    rng = np.random.default_rng(13)
    lo = [float(np.min(v)) for v in (rays.px, rays.py, rays.pz)]
    hi = [float(np.max(v)) for v in (rays.px, rays.py, rays.pz)]
    models = [tuple(rng.uniform(lo[d], hi[d], n) for d in range(3)) for n in (30, cap + 1, cap, 7)]
    w = weights(tt, rays, "signed")
    ref = sref.support(models, rays.px, rays.py, rays.pz, w, *q, thr=(0.0,))
    assert np.all(ref["barren"][:3] > 0) and ref["barren"][1] < cap + 1 and ref["count"][30:30 + cap + 1].max() > 1
    try:
        for mode in (tt.TdContext.SUP_AUTO, tt.TdContext.SUP_LDS, tt.TdContext.SUP_GLOBAL):
            c.set_support_scatter(mode)
            same(c.support(models, w, *q, thresholds=(0.0,), want_values=True), ref)
    finally:
        reset(tt, c)


@pytest.fixture(scope="module")
def recorded(tt):
    """Two histories of 40 samples and an empty one, recorded on a context of other rays."""
    other = tt.TdContext.from_datastruct(tt.synthetic_rays(24, seed=1))
    prm = tt.define_TDstructrure().replace(max_cells=400)
    hists = []
    for k in range(2):
        ch = tt.Chain(other, tt.chain_params(prm, None, seed=370 + k, chain=k + 1), tt.random_model(30, 370 + k))
        h = tt.History(other, 40, 40 * 400, with_ptS=False)
        ch.run_recorded(400, 10, 10, h)
        assert len(h) == 40
        hists.append(h)
        ch.close()
    empty = tt.History(other, 4, 4 * 400, with_ptS=False)
    yield [hists[0], empty, hists[1]]
    for h in hists + [empty]:
        h.close()
    other.close()


def test_histories_of_another_context_equal_their_models_read_back(tt, base, recorded):
    c, rays, q = base["ctx"], base["rays"], base["q"]
    hists = recorded
    flat = [m.cells() for h in hists if len(h) for m in h.read()]
    assert len(flat) == 80
    w = weights(tt, rays, "tstar")
    probs, bins, thr = (0.05, 0.5, 0.95), (8, 0.0, 0.5), (0.0, 0.05)
    ref = sref.support(flat, rays.px, rays.py, rays.pz, w, *q, thr=thr)
    assert np.all(ref["barren"] > 0) and len(np.unique(ref["values"])) > 80
    arrays = c.support(flat, w, *q, thresholds=thr, probs=probs, bins=bins, chain_len=[40, 40], want_values=True)
    same(arrays, ref)
    every = FIELDS + ("quantiles", "hist", "rhat", "ess", "lags")
    try:
        for slab in (64, 0):
            c.set_volume_slab_nodes(slab)
            h = c.support_history(hists, w, *q, thresholds=thr, probs=probs, bins=bins, convergence=True, want_values=True)
            same(h, arrays, every)
    finally:
        reset(tt, c)
    # R-hat and ESS are td_convergence_values' of the node matrix, the quantiles and histograms td_marginals' of it
    conv = c.convergence(arrays["values"], [40, 40])
    same(arrays, conv, ("rhat", "ess", "lags"))
    assert np.allclose(arrays["quantiles"], np.quantile(arrays["values"], probs, axis=0), rtol=1e-12, atol=0)
    assert arrays["hist"].shape == (150, 11) and np.all(arrays["hist"].sum(axis=1) == 80)
    with pytest.raises(tt.TdError, match="td_history_support: the histories hold no sample"):
        c.support_history([hists[1]], w)


def test_posterior_support_and_ray_density(tt, base, recorded):
    """The two public functions against the restatement: Models, nested lists and histories give the same maps."""
    rays, hists = base["rays"], recorded
    prm = tt.define_TDstructrure()
    rays._td_ctx = base["ctx"]  # (context_for: the context the fixture closes)
    try:
        xs, ys, zs = (np.linspace(v.min(), v.max(), n) for v, n in ((rays.px, 7), (rays.py, 5), (rays.pz, 4)))
        qx, qy, qz = np.tile(xs, 20), np.tile(np.repeat(ys, 7), 4), np.repeat(zs, 35)
        nested = [[m for m in h.read()] for h in hists if len(h)]
        flat = [m.cells() for chain in nested for m in chain]
        w = tt.support_weights(rays, "tstar")
        ref = sref.support(flat, rays.px, rays.py, rays.pz, w, qx, qy, qz, thr=(0.0, 0.05))
        grid = lambda a: a.reshape(a.shape[:-1] + (4, 5, 7)).swapaxes(-1, -3)  # noqa: E731
        for form in (hists, nested):
            out = tt.posterior_support(form, rays, prm, "tstar", (0.0, 0.05), probs=(0.5,), convergence=True, xs=xs, ys=ys,
                                       zs=zs)
            for f in ("mean", "std", "exceed"):
                assert np.array_equal(out[f], grid(ref[f])), f
            assert np.array_equal(out["share"], grid(ref["exceed"]) / 80.0)
            assert np.array_equal(out["barren"], ref["barren"]) and np.array_equal(out["orphans"], ref["orphans"])
            assert np.array_equal(out["cells"], [len(m[0]) for m in flat])
            assert np.array_equal(out["barren_share"], ref["barren"] / out["cells"])
            assert out["quantiles"].shape == (1, 7, 5, 4) and out["rhat"].shape == (7, 5, 4)
        assert np.all(out["barren_share"] > 0) and np.all(out["barren_share"] < 1)
        for kind in ("length", "count"):
            dens = tt.ray_density(rays, xs, ys, zs, kind)
            one = sref.support([(qx, qy, qz)], rays.px, rays.py, rays.pz, tt.support_weights(rays, kind))
            assert np.array_equal(dens["density"], grid(one["cell"])) and np.array_equal(dens["count"], grid(one["count"]))
            assert dens["orphans"] == 0 and dens["count"].sum() == len(rays.px) and (dens["count"] == 0).any()
    finally:
        rays._td_ctx = None


def test_refusals_that_need_a_context(tt, base):
    c, rays = base["ctx"], base["rays"]
    models = base["models"][:3]
    P = len(rays.px)
    before = c.support(models, None)
    bad = np.ones(P)
    bad[5] = np.nan
    with pytest.raises(tt.TdError, match="td_rasterize_support: w is not finite"):
        c.support(models, bad)
    with pytest.raises(tt.TdError, match="td_rasterize_support: the sum of \\|w\\| is not finite"):
        c.support(models, np.full(P, 1e308))
    with pytest.raises(tt.TdError, match="td_rasterize_support: qy is not finite"):
        c.support(models, None, [0.0], [np.inf], [0.0])
    with pytest.raises(tt.TdError, match="td_rasterize_support: nchains must be >= 1"):
        c.support(models, None, [0.0], [0.0], [0.0], chain_len=[])
    with pytest.raises(ValueError):
        c.support(models, np.ones(P + 1))
    same(c.support(models, None), before, FIELDS[:4])
