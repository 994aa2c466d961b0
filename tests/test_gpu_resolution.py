"""GPU: posterior resolution (td_rasterize_resolution, td_history_resolution, posterior_resolution) against the numpy
restatement of its definition (tests/resolution_ref.py), bit for bit, at the smallest shapes that can still go wrong:
every branch of the sum's association and of the leaf split (1 .. 2500 models), a ring of several blocks with forced
blocks of 64, 128 and the automatic one under both sweeps and both forms of the pair kernel, each block swept exactly
once, the window budget, recorded histories, the existing covariance call at point targets, degenerate lattices and
windows, zero sigma, empty and NaN models, and the thresholds at both infinities."""
import copy

import numpy as np
import pytest

import resolution_ref as rref
from test_gpu_interfaces import axes, uniform_models

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(tt, ds):
    c = tt.TdContext.from_datastruct(ds)
    yield c
    c.set_volume_counting(False)
    c.set_volume_slab_nodes(0)
    c.set_volume_method(tt.TdContext.VOL_AUTO)
    c.set_resolution(0, tt.TdContext.RES_FORM_KEPT)


def same(r, ref, fields=rref.FIELDS):
    for f in fields:
        a, b = r[f], ref[f]
        if a is None or b is None:
            assert a is None and b is None, f
        else:
            assert a.shape == b.shape and a.dtype == b.dtype, (f, a.shape, b.shape, a.dtype, b.dtype)
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (f, int(np.sum(~((a == b) | ((a != a) & (b != b))))))


def not_vacuous(ref, off, shape, M):
    """Between 5 % and 95 % of the pairs on the lattice have corr >= 0.5, some x run ends on a failing correlation and
    some is censored: the case cannot pass on correlations that all pass or all fail."""
    share, ended, censored = rref.vacuity(ref, off, *shape)
    print("%s, M = %d: %.1f %% of the pairs with corr >= 0.5, %d x runs ended by correlation, %d censored"
          % (shape, M, 100 * share, ended, censored))
    assert 0.05 < share < 0.95 and ended > 0 and censored > 0, (share, ended, censored)
    assert not np.any(ref["std"] == 0)


def frozen(ref):
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def weights_of(shape, seed=9):
    return np.random.default_rng(seed).uniform(0.5, 2.0, shape[0] * shape[1] * shape[2])


# ---------------------------------------------------------------- the association and the leaves

@pytest.mark.parametrize("M", [1, 2, 15, 16, 17, 1024, 1025, 2500])
def test_every_branch_of_the_association_and_of_the_leaf_split(tt, ctx, M):
    """M = 1: NaN rows, runs of 0, the edge bits alone; < 16: left to right; 16 .. 1024: one block, one leaf; 1025: two
    leaves of 513 + 512; 2500: a tree of three levels, four leaves of 625.  The box window of lags (2, 1, 1), 22
    offsets: three groups of eight in k_res_pairs, the last one short.  Every output."""
    shape = (5, 4, 3)
    models = uniform_models(M, 3000 + M, 3, 12)
    lat = axes(*shape)
    off = tt.resolution_offsets((2, 1, 1))
    assert len(off) == 22
    w = weights_of(shape)
    ref = rref.resolution(models, *lat, off, 0.5, w)
    if M > 2:
        not_vacuous(ref, off, shape, M)
    ctx.timing(enable=True, reset=True)
    try:
        r = ctx.resolution(models, *lat, off, 0.5, w, want=tt.TdContext.RES_ALL)
        assert ctx.timing(kernel="res_pairs")[0] == 1 and ctx.timing(kernel="res_combine")[0] == 1
        assert ctx.timing(kernel="res_summary")[0] == 1 and ctx.timing(kernel="raster_stats")[0] == 1
    finally:
        ctx.timing(enable=False)
    same(r, ref)
    if M == 1:
        assert np.isnan(r["corr"]).all() and not r["run"].any() and np.array_equal(r["footprint"], w)
        idx = rref.indices(*shape)
        edge = sum(((idx[a] == shape[a] - 1).astype(np.int32) << (2 * a)) | ((idx[a] == 0).astype(np.int32) << (2 * a + 1))
                   for a in range(3))
        assert np.array_equal(r["censored"], edge)
    part = ctx.resolution(models, *lat, off, 0.5, w, want=("corr", "run"))  # what is not asked for is None
    assert all(part[f] is None for f in ("cov", "footprint", "extent", "censored", "mean", "std"))
    same(part, ref, ("corr", "run"))
    default = ctx.resolution(models, *lat, off, 0.5, w)
    assert default["cov"] is None and default["corr"] is None
    same(default, ref, ("footprint", "run", "extent", "censored", "mean", "std"))
    try:  # both forms of the pair kernel: runs of five offsets and of two, and groups of eight
        for form in (tt.TdContext.RES_FORM_PLAIN, tt.TdContext.RES_FORM_XRUNS):
            ctx.set_resolution(0, form)
            same(ctx.resolution(models, *lat, off, 0.5, w, want=tt.TdContext.RES_ALL), ref)
    finally:
        ctx.set_resolution(0, tt.TdContext.RES_FORM_KEPT)


# ---------------------------------------------------------------- the ring of blocks, both sweeps

RING = {"ring": (40, 3, 12, (20, 9, 3), (3, 2, 1)), "brute40": (16, 40, 40, (7, 6, 5), (2, 2, 2)),
        "grid": (16, 300, 300, (7, 6, 5), (2, 2, 2))}


@pytest.fixture(scope="module")
def rings(tt):
    """(models, lattice, offsets, weights, reference) of the ensembles below, each made once."""
    out = {}
    for name, (M, lo, hi, shape, lags) in RING.items():
        models = uniform_models(M, 4000 + len(name), lo, hi)
        lat = axes(*shape)
        if name == "grid":  # cells of about 110 km: nodes 40 km apart, or no pair of nodes would be tied
            lat = (np.linspace(300.0, 550.0, 7), np.linspace(0.0, 200.0, 6), np.linspace(200.0, 400.0, 5))
        off = tt.resolution_offsets(lags)
        w = tt.voxel_weights(*lat).transpose(2, 1, 0).ravel()
        out[name] = (models, lat, off, w, frozen(rref.resolution(models, *lat, off, 0.5, w)))
    return out


@pytest.mark.parametrize("name", sorted(RING))
def test_the_ring_of_blocks_every_block_size_both_sweeps(tt, ctx, rings, name):
    """20 x 9 x 3 with lags (3, 2, 1): the largest flat offset is 3 + 20 (2 + 9) = 223 nodes, so blocks of 64 keep
    five resident and blocks of 128 three, and a tile's partners lie in two slots; 7 x 6 x 5 with lags (2, 2, 2): 100 of
    210 nodes.  Forced blocks of 64 and 128 and the automatic single block give the same bits, under the bucket grids
    and under k_raster_brute, with the plain and the x-run form of the pair kernel (lags of 3: runs of seven offsets, the
    instance of eight; a tile's staged segment lies in two slots); the sweep is launched once per block: no node is swept
    twice."""
    models, lat, off, w, ref = rings[name]
    M, shape = len(models), tuple(len(v) for v in lat)
    nq = shape[0] * shape[1] * shape[2]
    not_vacuous(ref, off, shape, M)
    reach = max(int(o[0]) + shape[0] * (int(o[1]) + shape[1] * int(o[2])) for o in off)
    assert reach == {"ring": 223}.get(name, 100)
    T = tt.TdContext
    runs = []
    try:
        for method in (T.VOL_GRID, T.VOL_BRUTE, T.VOL_AUTO):
            ctx.set_volume_method(method)
            for block in (64, 128, 0):
                ctx.set_volume_slab_nodes(block)
                ns, R, nblocks = T.resolution_plan(M, nq, reach, 0, block)
                assert nblocks == (-(-nq // block) if block else 1) and R == (-(-reach // ns) + 1)
                ctx.timing(enable=True, reset=True)
                runs.append(ctx.resolution(models, *lat, off, 0.5, w, want=T.RES_ALL))
                swept = ctx.timing(kernel="vol_search")[0], ctx.timing(kernel="raster_brute")[0]
                ctx.timing(enable=False)
                ctx.set_resolution(0, T.RES_FORM_PLAIN)
                runs.append(ctx.resolution(models, *lat, off, 0.5, w, want=T.RES_ALL))
                ctx.set_resolution(0, T.RES_FORM_KEPT)
                grid = method == T.VOL_GRID or (method == T.VOL_AUTO and name == "grid")
                assert swept == ((nblocks, 0) if grid else (0, nblocks)), (swept, nblocks, method)
                c = ctx.volume_counters()
                assert (c[3] == 0) if grid else (c[3] == M * ns * nblocks), c
    finally:
        ctx.timing(enable=False)
        ctx.set_volume_method(T.VOL_AUTO)
        ctx.set_volume_slab_nodes(0)
        ctx.set_resolution(0, T.RES_FORM_KEPT)
    for r in runs:
        same(r, ref)


def test_the_window_budget_decides_the_blocks_and_nothing_else(tt, ctx, rings):
    """A budget of 8 M 64 R bytes with R = 5 leaves room for blocks of 64 nodes alone, one of 8 M 576 2 for the single
    block; the same bits.  A budget below every ring is refused with M and the reach in the message; 13 offsets along
    x alone are one run of twelve and one of one (the widest instance of the x-run kernel)."""
    models, lat, off, w, ref = rings["ring"]
    M, T = len(models), tt.TdContext
    try:
        for budget, plan in ((8 * M * 64 * 5, (64, 5, 9)), (8 * M * 128 * 3 + 8 * M * 64, (128, 3, 5)), (8 * M * 576 * 2, (576, 2, 1))):
            assert T.resolution_plan(M, 540, 223, budget) == plan
            ctx.set_resolution(budget, T.RES_FORM_KEPT)
            ctx.timing(enable=True, reset=True)
            r = ctx.resolution(models, *lat, off, 0.5, w, want=T.RES_ALL)
            assert ctx.timing(kernel="raster_brute")[0] == plan[2]
            ctx.timing(enable=False)
            same(r, ref)
        ctx.set_resolution(8 * M * 64 * 5 - 1, T.RES_FORM_KEPT)
        with pytest.raises(tt.TdError, match=r"no block of 64 nodes fits the window budget.*M = 40 models, reach = 223 nodes"):
            ctx.resolution(models, *lat, off, 0.5, w)
        ctx.set_resolution(0, T.RES_FORM_KEPT)
        x13 = tt.resolution_offsets((13, 0, 0), "axes")
        want = rref.resolution(models, *lat, x13, 0.5, w)
        assert want["run"][0].max() > 4
        for form in (T.RES_FORM_XRUNS, T.RES_FORM_PLAIN):
            ctx.set_resolution(0, form)
            same(ctx.resolution(models, *lat, x13, 0.5, w, want=T.RES_ALL), want)
    finally:
        ctx.timing(enable=False)
        ctx.set_resolution(0, T.RES_FORM_KEPT)


def test_histories_equal_the_arrays_call(tt, ctx, ds):
    """Two short recorded histories: the history entry point equals the arrays entry point on the samples read back,
    which equals the restatement; posterior_resolution (on the data's own context, not the one that recorded) shapes
    the same numbers as [.., nx, ny, nz]."""
    prm = tt.define_TDstructrure().replace(max_cells=400)
    hs = []
    try:
        for k in range(2):
            ch = tt.Chain(ctx, tt.chain_params(prm, None, seed=270 + k, chain=k + 1), tt.random_model(30, 270 + k))
            h = tt.History(ctx, 8, 8 * 400, with_ptS=False)
            ch.run_recorded(80, 10, 10, h)
            hs.append(h)
        flat = [m.cells() for h in hs for m in h.read()]
        assert len(flat) == 16
        xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
        lat = (np.linspace(xmin, xmax, 6), np.linspace(ymin, ymax, 5), np.linspace(zmin, zmax, 4))
        off = tt.resolution_offsets((2, 1, 1))
        w = weights_of((6, 5, 4))
        want = ctx.resolution(flat, *lat, off, 0.3, w, want=tt.TdContext.RES_ALL)
        same(want, rref.resolution(flat, *lat, off, 0.3, w))
        for block in (64, 0):
            ctx.set_volume_slab_nodes(block)
            same(ctx.resolution_history(hs, *lat, off, 0.3, w, want=tt.TdContext.RES_ALL), want)
        p = tt.posterior_resolution(hs, ds, prm, lags=(2, 1, 1), threshold=0.3, weights=w.reshape(4, 5, 6).transpose(2, 1, 0),
                                    xs=lat[0], ys=lat[1], zs=lat[2], want=tt.TdContext.RES_ALL)
        for f in rref.FIELDS:
            lead = want[f].shape[:-1]
            k = len(lead)
            assert np.array_equal(p[f], want[f].reshape(lead + (4, 5, 6)).transpose(tuple(range(k)) + (k + 2, k + 1, k)),
                                  equal_nan=True), f
        assert np.array_equal(p["offsets"], off) and p["threshold"] == 0.3
    finally:
        ctx.set_volume_slab_nodes(0)
        for h in hs:
            h.close()


# ---------------------------------------------------------------- against the existing call

def test_the_covariance_call_at_point_targets_gives_the_same_numbers(tt, ctx, rings):
    """For an interior node, a corner and a node of the last plane: td_rasterize_covariance with point targets at n
    and at n + f reproduces corr[o][n] and cov[o][n], both ways round."""
    models, lat, off, w, ref = rings["ring"]
    nx, ny, nz = (len(v) for v in lat)
    qx, qy, qz = rref.lattice(*lat)
    r = ctx.resolution(models, *lat, off, want=("cov", "corr"))
    checked = 0
    for n in (7 + nx * (4 + ny * 1), 0, 3 + nx * (2 + ny * (nz - 1))):
        for t, o in enumerate(off):
            on, f = rref.on_lattice(nx, ny, nz, o)
            if not on[n]:
                assert np.isnan(r["corr"][t, n]) and np.isnan(r["cov"][t, n])
                continue
            c = ctx.covariance(models, qx, qy, qz, targets=[[qx[n], qy[n], qz[n]], [qx[n + f], qy[n + f], qz[n + f]]])
            for f_ in ("cov", "corr"):
                assert c[f_][0, n + f] == r[f_][t, n] and c[f_][1, n] == r[f_][t, n], (n, t, f_)
            checked += 1
    assert checked > 52  # the interior node has every pair, the corner and the last plane a part of them


# ---------------------------------------------------------------- degenerate cases

@pytest.mark.parametrize("shape", [(6, 1, 5), (1, 4, 5), (1, 1, 1), (7, 3, 1), (13, 5, 2)])
def test_degenerate_lattices(tt, ctx, shape):
    """ny = 1, nx = 1, a single node, nz = 1, and 130 nodes (no multiple of 64); the box window of lags (2, 1, 2) holds
    offsets larger than each of them."""
    models = uniform_models(20, 77 + shape[0], 3, 12)
    lat = tuple(np.linspace(0.0, 100.0 * n, n) + 50.0 for n in shape)
    off = tt.resolution_offsets((2, 1, 2))
    ref = rref.resolution(models, *lat, off, 0.5, None)
    out_of_bounds = [t for t, o in enumerate(off) if not rref.on_lattice(*shape, o)[0].any()]
    assert out_of_bounds and np.isnan(ref["corr"][out_of_bounds]).all()
    for block in (64, 0):
        ctx.set_volume_slab_nodes(block)
        try:
            same(ctx.resolution(models, *lat, off, 0.5, None, want=tt.TdContext.RES_ALL), ref)
        finally:
            ctx.set_volume_slab_nodes(0)


def test_an_offset_larger_than_the_lattice_and_an_axes_only_list(tt, ctx):
    shape = (5, 4, 3)
    models = uniform_models(24, 81, 3, 12)
    lat = axes(*shape)
    off = np.array([(1, 0, 0), (2, 0, 0), (0, 1, 0), (9, 0, 0), (0, 0, 40), (-4, 1, 0), (-5, 1, 0), (3, 0, 0)], dtype=np.int32)
    ref = rref.resolution(models, *lat, off)
    assert np.isnan(ref["corr"][[3, 4, 6]]).all() and not np.isnan(ref["corr"][[0, 1, 2, 5, 7]]).all()
    assert np.all(ref["censored"] & 48 == 48) and not ref["run"][2].any()  # no z offset on the lattice's list: both bits
    same(ctx.resolution(models, *lat, off, want=tt.TdContext.RES_ALL), ref)
    x_only = tt.resolution_offsets((3, 0, 0), "axes")
    ref = rref.resolution(models, *lat, x_only, 0.2)
    assert np.all(ref["censored"] & 60 == 60) and not ref["run"][1:].any() and ref["run"][0].any()
    same(ctx.resolution(models, *lat, x_only, 0.2, want=tt.TdContext.RES_ALL), ref)
    z_only = tt.resolution_offsets((0, 0, 2), "axes")
    ref = rref.resolution(models, *lat, z_only, 0.2)
    assert np.all(ref["censored"] & 15 == 15) and ref["run"][2].any()
    same(ctx.resolution(models, *lat, z_only, 0.2, want=tt.TdContext.RES_ALL), ref)


def test_a_node_with_the_same_value_in_every_sample(tt, ctx):
    """Every model has one cell of zeta 7.5 next to node 0 and none nearer: sigma there is 0, and its rows hold what
    the division gives (0 / 0 = NaN), as the restatement's do."""
    shape = (5, 4, 3)
    lat = axes(*shape)
    models = []
    for m in uniform_models(18, 90, 3, 12):
        x, y, z, ze = (np.array(a) for a in m)
        far = (x - lat[0][0]) ** 2 + (y - lat[1][0]) ** 2 + (z - lat[2][0]) ** 2 > 150.0 ** 2
        models.append((np.append(x[far], lat[0][0] + 1.0), np.append(y[far], lat[1][0] + 1.0), np.append(z[far], lat[2][0] + 1.0),
                       np.append(ze[far], 7.5)))
    off = tt.resolution_offsets((2, 1, 1))
    ref = rref.resolution(models, *lat, off)
    assert ref["std"][0] == 0.0 and np.count_nonzero(ref["std"] == 0) == 1 and ref["mean"][0] == 7.5
    assert np.isnan(ref["corr"][:, 0][~np.isnan(ref["cov"][:, 0])]).all() and not np.isnan(ref["cov"][0, 0])
    same(ctx.resolution(models, *lat, off, want=tt.TdContext.RES_ALL), ref)


def test_an_empty_model_and_a_nan_zeta(tt, ctx):
    shape = (5, 4, 3)
    lat = axes(*shape)
    models = uniform_models(20, 91, 3, 12)
    models[3] = tuple(np.zeros(0) for _ in range(4))
    bad = copy.deepcopy(models[11])
    bad[3][1] = np.nan
    models[11] = bad
    off = tt.resolution_offsets((2, 1, 1))
    ref = rref.resolution(models, *lat, off)
    assert np.isnan(ref["mean"]).any() and not np.isnan(ref["mean"]).all()
    T = tt.TdContext
    try:
        for method in (T.VOL_AUTO, T.VOL_GRID, T.VOL_BRUTE):
            ctx.set_volume_method(method)
            same(ctx.resolution(models, *lat, off, want=T.RES_ALL), ref)
    finally:
        ctx.set_volume_method(T.VOL_AUTO)


def test_thresholds_at_both_infinities_and_counting_weights(tt, ctx, rings):
    models, lat, off, w, _ = rings["brute40"]
    shape = tuple(len(v) for v in lat)
    low = rref.resolution(models, *lat, off, -np.inf, None)
    on = np.array([rref.on_lattice(*shape, o)[0] for o in off])
    assert not np.isnan(low["corr"][on]).any()
    # everything that is not NaN passes: a node counts itself and every pair it is part of
    assert np.array_equal(low["footprint"], 1.0 + on.sum(axis=0) + np.array(
        [np.bincount(np.flatnonzero(m) + rref.on_lattice(*shape, o)[1], minlength=on.shape[1]) for m, o in zip(on, off)]).sum(axis=0))
    assert np.all(low["censored"] == 63) and low["run"].max() == 2
    same(ctx.resolution(models, *lat, off, -np.inf, None, want=tt.TdContext.RES_ALL), low)
    high = rref.resolution(models, *lat, off, np.inf, None)
    assert np.all(high["footprint"] == 1.0) and not high["run"].any() and not high["extent"].any()
    same(ctx.resolution(models, *lat, off, np.inf, None, want=tt.TdContext.RES_ALL), high)
    counted = rref.resolution(models, *lat, off, 0.5, None)
    assert np.array_equal(counted["footprint"], np.round(counted["footprint"])) and counted["footprint"].max() > 1.0
    same(ctx.resolution(models, *lat, off, 0.5, want=tt.TdContext.RES_ALL), counted)


def test_refusals_with_a_context(tt, ctx):
    """The limits that follow the context: more rows than 1 GiB, and a ring that does not fit the budget."""
    models = uniform_models(4, 1, 3, 5)
    off = tt.resolution_offsets((5, 3, 5))
    big = (np.arange(600.0), np.arange(600.0), np.arange(10.0))
    with pytest.raises(tt.TdError, match="rows .noff..nq. of more than 1 GiB"):
        ctx.resolution(models, *big, off)
    with pytest.raises(tt.TdError, match="an offset appears twice"):
        ctx.resolution(models, *axes(5, 4, 3), [(1, 0, 0), (1, 0, 0)])
    r = ctx.resolution(models, *axes(5, 4, 3), [(1, 0, 0)], want="stats")  # a call after the refusals
    assert np.array_equal(r["mean"], rref.resolution(models, *axes(5, 4, 3), [(1, 0, 0)])["mean"])
