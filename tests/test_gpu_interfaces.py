"""GPU: posterior interfaces (td_rasterize_interfaces, td_history_interfaces, posterior_interfaces) against the
numpy restatement of their definition (tests/interfaces_ref.py), bit for bit, at the smallest shapes that can
still go wrong: every branch of the sum's association and of the leaf split (1 .. 2500 models), both sweeps, a
halo of one range and of two with slabs of 64, 128 and automatic size, degenerate lattices, and models that are
empty, hold NaN, duplicate cells or put cells on a voxel's edge and outside the lattice's hull."""
import copy

import numpy as np
import pytest

import interfaces_ref as iref

pytestmark = pytest.mark.gpu

BOX_LO, BOX_HI = np.array([0.0, -200.0, 0.0]), np.array([1000.0, 400.0, 660.0])
THR = (0.0, 5.0, 25.0)


@pytest.fixture(scope="module")
def ctx(tt, ds):
    c = tt.TdContext.from_datastruct(ds)
    yield c
    c.set_volume_counting(False)
    c.set_volume_slab_nodes(0)
    c.set_volume_method(tt.TdContext.VOL_AUTO)


def same(r, ref, fields=iref.FIELDS):
    for f in fields:
        a, b = r[f], ref[f]
        if a is None or b is None:
            assert a is None and b is None, f
        elif f == "skipped":
            assert a == b, (f, a, b)
        else:
            assert a.shape == b.shape and a.dtype == b.dtype, (f, a.shape, b.shape, a.dtype, b.dtype)
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f


def uniform_models(M, seed, lo=3, hi=12):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(M):
        n = int(rng.integers(lo, hi + 1))
        p = BOX_LO + rng.random((n, 3)) * (BOX_HI - BOX_LO)
        out.append((p[:, 0], p[:, 1], p[:, 2], rng.uniform(0, 50, n)))
    return out


def axes(nx, ny, nz):
    return np.linspace(0.0, 1000.0, nx), np.linspace(-200.0, 400.0, ny), np.linspace(0.0, 660.0, nz)


def contested(ref, M):
    """More than half of the faces have 0 < count < M: the case cannot pass on all-equal or all-different values."""
    nfaces, mid, zero = iref.contested(ref, M)
    print("M = %d: %d faces, %d with 0 < count < M, %d with count == 0" % (M, nfaces, mid, zero))
    assert mid > nfaces // 2, (nfaces, mid, zero)


# ---------------------------------------------------------------- the association and the leaves

@pytest.mark.parametrize("M", [1, 2, 15, 16, 17, 1024, 1025, 2500])
def test_every_branch_of_the_association_and_of_the_leaf_split(ctx, M):
    """M = 1; < 16: left to right; 16 .. 1024: one block, one leaf; 1025: two leaves of 513 + 512; 2500: a tree of
    three levels, four leaves of 625.  Every output, with three thresholds and with none.  (One model has no count
    strictly between 0 and M, and two models, whose faces differ with a probability p each, have one on 2 p (1 - p)
    <= half of the faces at best: there the restatement must hold every possible count, 0 .. M, on more than a
    tenth of the faces each, which all-equal or all-different values cannot give either.)"""
    nx, ny, nz = 5, 4, 3
    models = uniform_models(M, 3000 + M)
    xs, ys, zs = axes(nx, ny, nz)
    ref = iref.interfaces(models, xs, ys, zs, THR)
    if M > 2:
        contested(ref, M)
    else:
        c = ref["count"][ref["count"] >= 0]
        assert len(c) == 133 and min(np.sum(c == v) for v in range(M + 1)) > len(c) // 10
    assert ref["density"].sum() + ref["skipped"] == sum(len(m[0]) for m in models) and ref["skipped"] == 0
    ctx.timing(enable=True, reset=True)
    try:
        r = ctx.interfaces(models, xs, ys, zs, THR)
        assert ctx.timing(kernel="iface_faces")[0] == 1 and ctx.timing(kernel="iface_density")[0] == 1
    finally:
        ctx.timing(enable=False)
    same(r, ref)
    none = ctx.interfaces(models, xs, ys, zs)
    assert none["exceed"] is None
    same(none, dict(ref, exceed=None))
    for t, thr in enumerate(THR):  # one threshold at a time: the kernel's other instances
        one = ctx.interfaces(models, xs, ys, zs, (thr,), want=("exceed", "jump"))
        assert one["count"] is None and one["density"] is None and one["mean"] is None and one["skipped"] is None
        assert np.array_equal(one["exceed"][0], ref["exceed"][t]) and np.array_equal(one["jump"], ref["jump"], equal_nan=True)
    five = ctx.interfaces(models, xs, ys, zs, THR + (1.0, 50.0), want=("exceed",))  # (five thresholds: the widest)
    assert np.array_equal(five["exceed"][:3], ref["exceed"]) and np.all(five["exceed"][4] <= ref["exceed"][2])


# ---------------------------------------------------------------- both sweeps, both halos, every slab size

@pytest.fixture(scope="module")
def sweeps():
    """(models, lattice, reference) of the three ensembles below, each made once."""
    out = {}
    for name, M, lo, hi, shape in (("grid", 16, 300, 300, (7, 6, 5)), ("brute", 16, 40, 40, (7, 6, 5)),
                                   ("two_ranges", 40, 3, 12, (20, 9, 3))):
        models = uniform_models(M, 4000 + len(name), lo, hi)
        lat = axes(*shape)
        if name == "grid":  # cells of about 110 km: nodes 40 km apart, or every face would differ in every model
            lat = (np.linspace(300.0, 550.0, 7), np.linspace(0.0, 200.0, 6), np.linspace(200.0, 400.0, 5))
        ref = iref.interfaces(models, *lat, THR)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[name] = (models, lat, ref)
    return out


@pytest.mark.parametrize("name", ["grid", "brute", "two_ranges"])
def test_both_sweeps_both_halos_every_slab_size(tt, ctx, sweeps, name):
    """7 x 6 x 5: a plane of 42 nodes < 64, so a slab's two column ranges meet; 20 x 9 x 3: a plane of 180 > 128, so
    they do not.  300 cells per model: the bucket grids; 40 and fewer: k_raster_brute."""
    models, lat, ref = sweeps[name]
    M, (nx, ny, nz) = len(models), (len(v) for v in lat)
    contested(ref, M)
    nq = nx * ny * nz
    runs = []
    try:
        for slab in (64, 128, 0):
            ctx.set_volume_slab_nodes(slab)
            nodes, nslabs, maxcols = tt.TdContext.interfaces_plan(M, nx, ny, nz, 0, slab)
            assert nslabs == (-(-nq // slab) if slab else 1)
            if slab:  # the halo's shape: one range when the plane is smaller than the slab
                assert maxcols == (slab + nx * ny if nx * ny <= slab + nx else 2 * slab + nx)
            runs.append(ctx.interfaces(models, *lat, THR))
            c = ctx.volume_counters()
            assert (c[3] == 0 and c[:3] == (-1, -1, -1)) if name == "grid" else (c[3] > 0 and sum(c[:3]) == 0), c
        runs.append(ctx.interfaces(models, *lat, THR))  # a repeated call
    finally:
        ctx.set_volume_slab_nodes(0)
    for r in runs:
        same(r, ref)


@pytest.mark.parametrize("shape", [(1, 1, 1), (6, 1, 4), (1, 5, 1)])
def test_degenerate_lattices(ctx, shape):
    nx, ny, nz = shape
    models = uniform_models(17, 5000 + nx)
    xs, ys, zs = axes(6, 5, 4)
    xs, ys, zs = xs[:nx] + 100.0, ys[:ny] + 50.0, zs[:nz] + 30.0
    ref = iref.interfaces(models, xs, ys, zs, THR)
    r = ctx.interfaces(models, xs, ys, zs, THR)
    same(r, ref)
    total = sum(len(m[0]) for m in models)
    assert r["density"].sum() + r["skipped"] == total
    for a, n in enumerate(shape):
        if n == 1:
            assert np.all(r["count"][a] == -1) and np.all(r["exceed"][:, a] == -1) and np.isnan(r["jump"][a]).all()
        else:
            assert np.sum(r["count"][a] >= 0) == (n - 1) * (nx * ny * nz // n)
    if shape == (1, 1, 1):
        assert r["any"].tolist() == [-1] and r["density"].tolist() == [total] and np.isfinite(r["mean"]).all()
    else:
        contested(ref, 17)
        try:
            ctx.set_volume_slab_nodes(64)
            same(ctx.interfaces(models, xs, ys, zs, THR), ref)
        finally:
            ctx.set_volume_slab_nodes(0)


# ---------------------------------------------------------------- awkward models

def awkward():
    """19 models on an 8 x 4 x 3 lattice whose third and fourth x nodes are 1e-7 apart: an empty model, one whose
    cells hold NaN coordinates (never win, counted in `skipped`) and NaN zeta (a NaN value differs from everything,
    itself included), one of duplicated cells, one with cells exactly on voxel midpoints and far outside the
    hull, and 15 ordinary ones."""
    rng = np.random.default_rng(77)
    xs = np.array([0.0, 150.0, 300.0, 300.0000001, 450.0, 600.0, 800.0, 1000.0])
    ys, zs = np.linspace(-200.0, 400.0, 4), np.array([0.0, 300.0, 660.0])
    models = uniform_models(15, 78)
    x, y, z, ze = (a.copy() for a in uniform_models(1, 79, 30, 30)[0])
    x[::5] = np.nan
    y[7] = np.nan
    z[8] = np.nan
    ze[1::3] = np.nan
    with_nan = (x, y, z, ze)
    x, y, z, ze = uniform_models(1, 80, 10, 10)[0]
    dup = rng.permutation(20) % 10
    duplicates = (x[dup], y[dup], z[dup], np.arange(20) * 0.5)
    mx, my, mz = 0.5 * (xs[:-1] + xs[1:]), 0.5 * (ys[:-1] + ys[1:]), 0.5 * (zs[:-1] + zs[1:])
    edge = (np.array([mx[0], mx[4], mx[6], -1e4, 2e4, 500.0, np.inf, -np.inf]),
            np.array([my[0], 100.0, my[2], 100.0, -1e4, 1e4, 0.0, 0.0]),
            np.array([mz[0], mz[1], 100.0, 1e4, 100.0, -1e4, 0.0, 0.0]), np.arange(8) * 3.0 + 1.0)
    empty = (np.zeros(0),) * 4
    return models[:7] + [empty, with_nan] + models[7:11] + [duplicates, edge] + models[11:], xs, ys, zs


def test_awkward_models_whatever_the_slab_and_the_sweep(tt, ctx):
    models, xs, ys, zs = awkward()
    M = len(models)
    ref = iref.interfaces(models, xs, ys, zs, THR)
    contested(ref, M)
    assert ref["skipped"] == 8 and ref["density"].sum() + ref["skipped"] == sum(len(m[0]) for m in models)
    assert np.isnan(ref["mean"]).any() and np.isnan(ref["jump"][ref["count"] >= 0]).any()  # (the NaN zeta is seen)
    T = tt.TdContext
    try:
        for method in (T.VOL_AUTO, T.VOL_GRID, T.VOL_BRUTE):
            ctx.set_volume_method(method)
            for slab in (64, 0):
                ctx.set_volume_slab_nodes(slab)
                same(ctx.interfaces(models, xs, ys, zs, THR), ref)
    finally:
        ctx.set_volume_method(T.VOL_AUTO)
        ctx.set_volume_slab_nodes(0)
    d = ctx.interfaces(models, xs, ys, zs, want="density")
    assert np.array_equal(d["density"], ref["density"]) and d["skipped"] == 8 and d["count"] is None


def test_two_nodes_equal_in_every_model(ctx):
    """The lattice's third and fourth x nodes are 1e-7 apart and no cell boundary runs between them: count 0,
    exceed 0 and a jump of exactly 0.0 on those faces."""
    _, xs, ys, zs = awkward()
    models = uniform_models(15, 78)
    ref = iref.interfaces(models, xs, ys, zs, THR)
    contested(ref, 15)
    close = 2 + len(xs) * np.arange(len(ys) * len(zs))  # the nodes whose +x neighbour is 1e-7 away
    assert np.all(ref["count"][0][close] == 0) and np.all(ref["jump"][0][close] == 0.0)
    assert np.all(ref["exceed"][:, 0][:, close] == 0)
    r = ctx.interfaces(models, xs, ys, zs, THR)
    same(r, ref)
    assert np.all(r["count"][0][close] == 0) and np.all(r["jump"][0][close] == 0.0) and not np.signbit(r["jump"][0][close]).any()


def test_refusals_that_need_a_context(tt, ctx):
    models = uniform_models(3, 1)
    xs, ys, zs = axes(3, 2, 2)
    before = ctx.interfaces(models, xs, ys, zs, THR)
    with pytest.raises(tt.TdError, match="td_rasterize_interfaces: xs is not strictly increasing"):
        ctx.interfaces(models, xs[::-1], ys, zs)
    with pytest.raises(tt.TdError, match="td_rasterize_interfaces: every threshold must be finite and >= 0"):
        ctx.interfaces(models, xs, ys, zs, (1.0, -1.0))
    with pytest.raises(tt.TdError, match="td_rasterize_interfaces: nthr must be 0 .. 8"):
        ctx.interfaces(models, xs, ys, zs, tuple(range(9)))
    with pytest.raises(tt.TdError, match="td_rasterize_interfaces: no output asked for"):
        ctx.interfaces(models, xs, ys, zs, want=())
    same(ctx.interfaces(models, xs, ys, zs, THR), before)


# ---------------------------------------------------------------- histories and the lattice form

@pytest.fixture(scope="module")
def recorded(tt, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=400)
    hists = []
    for k in range(2):
        c = tt.Chain(ctx, tt.chain_params(prm, None, seed=170 + k, chain=k + 1), tt.random_model(30, 170 + k))
        h = tt.History(ctx, 40, 40 * 400, with_ptS=False)
        c.run_recorded(400, 10, 10, h)
        assert len(h) == 40
        hists.append(h)
    empty = tt.History(ctx, 4, 4 * 400, with_ptS=False)
    return [hists[0], empty, hists[1]]


def test_histories_equal_their_models_read_back(tt, ctx, recorded):
    hists = recorded
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    xs, ys, zs = np.linspace(xmin - 30, xmax + 30, 9), np.linspace(ymin, ymax, 7), np.linspace(zmin, zmax + 50, 5)
    flat = [m.cells() for h in hists if len(h) for m in h.read()]
    assert len(flat) == 80
    ref = iref.interfaces(flat, xs, ys, zs, (5.0,))
    contested(ref, 80)
    same(ctx.interfaces(flat, xs, ys, zs, (5.0,)), ref)
    try:
        for slab in (64, 0):
            ctx.set_volume_slab_nodes(slab)
            same(ctx.interfaces_history(hists, xs, ys, zs, (5.0,)), ref)
    finally:
        ctx.set_volume_slab_nodes(0)
    same(ctx.interfaces_history(hists, xs, ys, zs, (5.0,)), ref)  # a repeated call
    with pytest.raises(tt.TdError, match="td_history_interfaces: the histories hold no sample"):
        ctx.interfaces_history([hists[1]], xs, ys, zs)


def test_posterior_interfaces_on_the_lattice(tt, ctx, ds, recorded):
    """posterior_interfaces against numpy on the route there was before: volume_history(want_values=True) for the
    faces, History.read() for the density.  ds's own cached context is not the one that recorded the histories: a
    history of another context on the same device is accepted."""
    hists = recorded
    own = tt.context_for(ds)
    assert own is not ctx
    thin = copy.copy(ds)
    thin.xVec, thin.yVec, thin.zVec = (np.asarray(v, dtype=np.float64)[::6] for v in (ds.xVec, ds.yVec, ds.zVec))
    xv, yv, zv = thin.xVec, thin.yVec, thin.zVec
    nx, ny, nz = len(xv), len(yv), len(zv)
    prm = tt.define_TDstructrure()
    thr = (2.0, 5.0)
    out = tt.posterior_interfaces(hists, thin, prm, thr)
    vol = ctx.volume_history(hists, *iref.lattice(xv, yv, zv), want_values=True)
    V, M = vol["values"], 80
    assert V.shape == (M, nx * ny * nz)
    count, anyc, exceed, jump = iref.face_statistics(V, nx, ny, nz, thr)
    flat_models = [m for h in hists if len(h) for m in h.read()]
    dens, skipped = iref.density([m.cells() for m in flat_models], xv, yv, zv)
    nf, mid, _ = iref.contested(dict(count=count), M)
    assert mid > nf // 2

    def grid(a):
        return a.reshape(a.shape[:-1] + (nz, ny, nx)).swapaxes(-1, -3)

    assert out["count"].shape == out["prob"].shape == out["jump"].shape == (3, nx, ny, nz)
    assert out["exceed"].shape == (2, 3, nx, ny, nz) and out["density"].shape == out["mean"].shape == (nx, ny, nz)
    assert np.array_equal(out["count"], grid(count)) and np.array_equal(out["any"], grid(anyc))
    assert np.array_equal(out["jump"], grid(jump), equal_nan=True)
    assert np.array_equal(out["prob"], np.where(grid(count) < 0, np.nan, grid(count) / 80.0), equal_nan=True)
    assert np.array_equal(out["prob_any"], np.where(grid(anyc) < 0, np.nan, grid(anyc) / 80.0), equal_nan=True)
    assert np.array_equal(out["exceed"], np.where(grid(exceed) < 0, np.nan, grid(exceed) / 80.0), equal_nan=True)
    assert np.array_equal(out["mean"], grid(vol["mean"])) and np.array_equal(out["std"], grid(vol["std"]))
    assert np.array_equal(out["density"], grid(dens)) and out["skipped"] == skipped == 0
    assert np.array_equal(out["density_per_model"], grid(dens) / 80.0)
    assert out["density"].sum() == sum(len(m.cells()[0]) for m in flat_models)
    assert out["count"][0, 3, 2, 1] == count[0][3 + nx * (2 + ny * 1)]  # [a, i, j, k] is node i + nx (j + ny k)
    assert np.isnan(out["prob"][0, nx - 1]).all() and np.isnan(out["jump"][2, :, :, nz - 1]).all()
    assert np.array_equal(out["thresholds"], thr) and np.array_equal(out["x"], xv)
    # Models and nested lists give what the histories give
    nested = [[m for m in h.read()] for h in hists if len(h)]
    for form in (flat_models, nested):
        o2 = tt.posterior_interfaces(form, thin, prm, thr)
        for f in ("prob", "prob_any", "exceed", "jump", "count", "any", "density", "mean", "std"):
            assert np.array_equal(o2[f], out[f], equal_nan=True), f
