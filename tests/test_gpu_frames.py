"""Every search and chain path in coordinate frames beyond the Tonga ray frame (tests/frames.py): metres far
from their origin (where the 1e9 sentinel of v_nearest binds for most points), offsets of 2^33 against an
extent of 10^3, a box of 10^-3 units, negative coordinates and a flat prior axis.  Each search here is exact
because a floating-point bound lets it stop early (the bucket-face allowance and grid_lb_close, the chain's
grid pad, the FP32 tile and super-tile filters, the host one-point grid's tolerance), and every bound's size
depends on |coordinate| / extent, which the rest of the suite holds at about 1.  Bounded searches may only
cost time, never change an answer: everything below is compared bit for bit with the C oracle, oracle_np
or the HOST engine, on the 381 shipped rays (16 845 points) and models of 300 cells, just above the
evaluate's grid threshold.

Out of scope: covariance, marginals and convergence consume the value matrix that the volume sweep
produces and have no frame-dependent arithmetic of their own."""
import numpy as np
import pytest

import frames
from oracle import oracle_np
from test_gpu_chain import same_models
from tile_filter_ref import boundary_case, filter_hits, tile_boxes

pytestmark = pytest.mark.gpu

# chain seeds: with them the HOST engine accepts at least one proposal of each action within the run
CHAIN_SEED = dict(identity=1, metres=1, far=1, small_far=1, tiny=1, negative=1, flat=1)
DROPIN_SEED = dict(metres=2, far=2, small_far=2, flat=2)
ENSEMBLE_SEED = 30


@pytest.fixture(scope="module")
def fds(ds):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = frames.in_frame(ds, name)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def fctx(tt, fds):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = tt.TdContext.from_datastruct(fds(name))
        return cache[name]

    yield get
    for c in cache.values():
        c.close()


def ref_eval(orc, f, cells):
    r = orc.evaluate(f.rayX, f.rayY, f.rayZ, f.rayL, f.rayU, f.tS, f.allSig, cells)
    assert r["rc"] == 0
    return r


@pytest.mark.parametrize("name", frames.ALL)
def test_evaluate(orc, fds, fctx, name):
    f, ctx = fds(name), fctx(name)
    for n in (frames.GPU_CELLS, 2500) if name in ("metres", "far") else (frames.GPU_CELLS,):
        cells = frames.frame_model(name, n, frames.MODEL_SEED, hostile=True).cells()
        ref = ref_eval(orc, f, cells)
        none = float(np.mean(ref["nearest"] < 0))
        print(name, n, "points with no cell in reach: %.3f" % none)
        if (name, n) == ("metres", frames.GPU_CELLS):  # (test_frames_host.py: the sentinel binds, not everywhere)
            assert 0.5 <= none <= 0.97
        try:
            for m in (ctx.NN_AUTO, ctx.NN_GRID, ctx.NN_BRUTE, ctx.NN_BRUTE_SPLIT):
                ctx.set_nn_method(m)
                ptS, phi, lk, near = ctx.evaluate(cells, want_nearest=True)
                assert np.array_equal(near, ref["nearest"]), (m, n, np.flatnonzero(near != ref["nearest"])[:5])
                assert np.array_equal(ptS, ref["ptS"]), (m, n)
                assert phi == ref["phi"] and lk == ref["likelihood"], (m, n)
        finally:
            ctx.set_nn_method(ctx.NN_AUTO)


@pytest.mark.parametrize("name", ["metres", "far", "tiny", "flat"])
def test_interpolate_large_query_set(orc, fctx, name):
    """66 000 queries (k_nn_grid4 and its fallbacks): inside the box, on cells, out to 3 extents outside (off
    the plane too in `flat`), NaN-terminated."""
    ctx = fctx(name)
    rng = np.random.default_rng(31)
    cells = frames.frame_model(name, frames.GPU_CELLS, frames.MODEL_SEED, hostile=True).cells()
    b = np.array(frames.frame_box(name))
    lo, ext = b[0::2], b[1::2] - b[0::2]
    scale = ext.max()
    inside = lo + ext * rng.random((60000, 3))
    on = np.stack(cells[:3], 1)
    on = on[~np.isnan(on).any(axis=1)]
    outside = lo - 3 * scale + (ext + 6 * scale) * rng.random((66000 - 60000 - len(on), 3))
    Q = np.concatenate([inside, on, outside, [[np.nan, lo[1], lo[2]], lo]])
    X, Y, Z = (np.ascontiguousarray(Q[:, a]) for a in range(3))
    zr, ir = orc.interpolation(cells, X, Y, Z)
    assert len(zr) == 66000  # (Interpolation stops at the NaN, MCsub.jl:306-327)
    print(name, "queries with no cell in reach: %.3f" % np.mean(ir < 0))
    if name == "metres":
        assert 0.03 <= np.mean(ir < 0) <= 0.97
    try:
        for m in (ctx.NN_GRID, ctx.NN_BRUTE):
            ctx.set_nn_method(m)
            z, near = ctx.interpolate(cells, X, Y, Z, want_nearest=True)
            assert np.array_equal(near, ir), (m, np.flatnonzero(near != ir)[:5])
            assert np.array_equal(z, zr), m
    finally:
        ctx.set_nn_method(ctx.NN_AUTO)


def chain_pair(tt, ctxs, name, seed, engines, lds_mode=0):
    prm = tt.define_TDstructrure().replace(max_cells=400)
    model = frames.frame_model(name, frames.GPU_CELLS, seed)
    out = []
    for c, e in zip(ctxs, engines):
        ch = tt.Chain(c, tt.chain_params(prm, None, seed=seed, chain=1, engine=e, extent=frames.frame_box(name)), model)
        if e == tt.TD_ENGINE_DEVICE and lds_mode:
            assert tt.lib().tdt_chain_set_lds_mode(ch.h, lds_mode) == 0
        out.append(ch)
    return out


def assert_chains_agree(tt, orc, f, name, chains, iters, rounds, every_action):
    for _ in range(rounds):
        for ch in chains:
            ch.run(iters // rounds)
        st = [ch.stats() for ch in chains]
        for s in st[1:]:
            assert s["phi"] == st[0]["phi"], st
            assert s["accepted"] == st[0]["accepted"] and s["proposed"] == st[0]["proposed"], st
            assert s["ncells"] == st[0]["ncells"]
    ms = [ch.model() for ch in chains]
    for m in ms[1:]:
        assert same_models(ms[0], m) and np.array_equal(ms[0].ptS, m.ptS)
    ref = ref_eval(orc, f, ms[0].cells())  # the chain's state is the full evaluate of its cells
    assert np.array_equal(ms[0].ptS, ref["ptS"]) and ms[0].phi == ref["phi"]
    print(name, "accepted", st[0]["accepted"], "of", st[0]["proposed"], "cells", st[0]["ncells"])
    assert st[0]["iterations"] == iters and sum(st[0]["accepted"]) > 0
    if every_action:
        assert min(st[0]["accepted"]) >= 1, st[0]  # births, deaths, changes and moves all committed
    if name == "flat":
        assert np.all(ms[0].yCell == frames.FLAT_Y)  # (the move's y range is 0)
    if name == "metres":
        none = float(np.mean(ref["nearest"] < 0))
        print(name, "points with no cell in reach after the chain: %.3f" % none)
        assert 0.03 <= none <= 0.97
    for ch in chains:
        ch.close()


@pytest.mark.parametrize("name,lds_mode", [(n, 0) for n in frames.ALL] + [(n, 1) for n in ("metres", "far", "flat")]
                         + [("metres", 2)])
def test_device_chain_follows_host_engine(tt, orc, fds, fctx, name, lds_mode):
    """lds_mode 0: the LDS layout; 1: the HBM layout with its FP32 super-tiles; 2: the 256-thread kernel."""
    ctx = fctx(name)
    chains = chain_pair(tt, (ctx, ctx), name, CHAIN_SEED[name], (tt.TD_ENGINE_HOST, tt.TD_ENGINE_DEVICE), lds_mode)
    assert_chains_agree(tt, orc, fds(name), name, chains, 300, 3, True)


@pytest.mark.parametrize("name", ["metres", "far", "small_far", "flat"])
def test_dropin_engine_follows_host(tt, orc, fds, name):
    """As test_gpu_incremental.py::test_dropin_engine_follows_host_and_device: the live host_nn answers the
    births' and deaths' one-point queries."""
    ctxs = [tt.TdContext.from_datastruct(fds(name)) for _ in range(3)]
    try:
        chains = chain_pair(tt, ctxs, name, DROPIN_SEED[name],
                            (tt.TD_ENGINE_HOST, tt.TD_ENGINE_DROPIN, tt.TD_ENGINE_DEVICE))
        assert_chains_agree(tt, orc, fds(name), name, chains, 200, 4, False)
        t = np.zeros(18, dtype=np.int64)  # (the shadow chain needs |coordinate| <= 1e6: elsewhere, full evaluates)
        assert tt.lib().tdt_dropin_timing(ctxs[1].h, 0, t.ctypes.data) == 0
        print(name, "td_evaluate calls %d, full evaluates %d, one-point queries %d" % (t[6], t[8], t[7]))
        assert t[7] > 0  # births and deaths asked for their one-point Interpolation
        if name == "flat":  # sane coordinates: the shadow chain and its live host_nn answered, not full evaluates
            assert 10 * t[8] <= t[6]
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("name", ["identity", "metres", "far", "flat"])
def test_recorded_ensemble(tt, orc, fds, fctx, name):
    """Two DEVICE chains x 20 samples in a History: the volume sweep on a lattice (grid and brute), the
    predictive sweep on the rays, and td_rasterize (k_raster_brute) against the references."""
    f, ctx = fds(name), fctx(name)
    prm = tt.define_TDstructrure().replace(max_cells=400)
    hists = []
    for k in range(2):
        p = tt.chain_params(prm, None, seed=ENSEMBLE_SEED + k, chain=k + 1, extent=frames.frame_box(name))
        c = tt.Chain(ctx, p, frames.frame_model(name, frames.GPU_CELLS, ENSEMBLE_SEED + k))
        h = tt.History(ctx, 20, 20 * 400, with_ptS=True)
        c.run_recorded(200, 10, 10, h)
        assert len(h) == 20
        hists.append(h)
        c.close()
    models = [m.cells() for h in hists for m in h.read()]
    assert len({len(m[0]) for m in models}) > 1  # (the samples differ)
    qx, qy, qz = frames.frame_lattice(name)
    mean, std, V = oracle_np.rasterize(models, qx, qy, qz)
    assert np.all(V[:, -4:] == 0.0)  # beyond the sentinel, and the NaN node
    print(name, "nodes with no cell in reach: %.3f" % np.mean(V[:, :315] == 0.0))
    try:
        for method in (ctx.VOL_GRID, ctx.VOL_BRUTE):
            ctx.set_volume_method(method)
            r = ctx.volume_history(hists, qx, qy, qz, want_values=True)
            assert np.array_equal(r["values"], V), (method, np.argwhere(r["values"] != V)[:5])
            assert np.array_equal(r["mean"], mean) and np.array_equal(r["std"], std, equal_nan=True), method
        m2, s2, V2 = ctx.rasterize(models, qx, qy, qz, want_values=True)
        assert np.array_equal(V2, V) and np.array_equal(m2, mean) and np.array_equal(s2, std, equal_nan=True)
        refs = [ref_eval(orc, f, m) for m in models]
        for method in (ctx.VOL_GRID, ctx.VOL_BRUTE):
            ctx.set_volume_method(method)
            r = ctx.predict_history(hists, want_values=True)
            assert np.array_equal(r["ptS"], np.array([x["ptS"] for x in refs])), method
            assert np.array_equal(r["phi"], np.array([x["phi"] for x in refs])), method
    finally:
        ctx.set_volume_method(ctx.VOL_AUTO)
    rec = np.concatenate([h.read_arrays()["ptS"] for h in hists])
    assert np.array_equal(rec, np.array([x["ptS"] for x in refs]))  # what the chains recorded, too
    for h in hists:
        h.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", [n for n in frames.ALL if n != "flat"])
def test_tile_filter_never_drops_a_tile_in_reach(tt, fds, name, mode):
    """test_gpu_tile_filter.py on tiles of 16 consecutive ray points of the frame.  FP32 cannot resolve `far`
    (its ulp there is 1024 units) or `small_far`, and in `metres` it is not asked to prune either: the claim
    in every frame is only that no tile in reach is dropped."""
    rng = np.random.default_rng(17 + mode)
    nt = 400
    pts, qs, md, owner, maxd = boundary_case(rng, frames.ray_points(fds(name)), unit=frames.FRAMES[name][0],
                                             large=False, nt=nt)
    lo, hi = tile_boxes(pts)
    hit = filter_hits(tt, lo, hi, maxd, qs, mode)
    must = md <= maxd[None, :]
    missed = np.argwhere(must & ~hit)
    assert missed.size == 0, (missed[:5], [(md[q, t], maxd[t]) for q, t in missed[:5]])
    exact = np.setdiff1d(np.arange(nt), np.arange(0, nt, 7))
    assert must[owner[exact], exact].all()  # (the boundary pairs, maximum == the distance, are in the set)
    print(name, "tiles passed: %.3f" % hit.mean())
    if name in ("identity", "tiny", "negative"):
        assert hit.mean() < 0.6  # (and it does prune)
