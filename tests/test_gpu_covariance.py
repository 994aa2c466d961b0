"""GPU: posterior covariance (td_rasterize_covariance, td_history_covariance, posterior_covariance) against the
numpy restatement of its definition (tests/covariance_ref.py), bit for bit, at the smallest shapes that can
still go wrong: every branch of the sum's association (1 .. 2500 models), target counts around the kernel's
register group, 70 nodes in slabs of 64, and an ensemble of models that tie, duplicate, degenerate, answer
nothing or hold NaN, with targets on a node, off the lattice, out of reach and at a NaN coordinate."""
import copy

import numpy as np
import pytest

import covariance_ref as cref

pytestmark = pytest.mark.gpu

FIELDS = ("cov", "corr", "mean", "std", "target_mean", "target_std")
ONE_ULPS = 4.5e-16  # how far the correlation of a node with itself may be from 1: 4 roundings of 2^-53 (see its use)


@pytest.fixture(scope="module")
def ctx(tt, ds):
    c = tt.TdContext.from_datastruct(ds)
    yield c
    c.set_volume_counting(False)
    c.set_volume_slab_nodes(0)
    c.set_volume_method(tt.TdContext.VOL_AUTO)


def same(a, b, fields=FIELDS):
    for f in fields:
        assert a[f].shape == b[f].shape and a[f].dtype == b[f].dtype, f
        assert np.array_equal(a[f], b[f], equal_nan=True), f


def rows(ref, idx):
    """The reference restricted to the target rows idx."""
    idx = np.asarray(idx, dtype=np.int64)
    return dict(cov=ref["cov"][idx], corr=ref["corr"][idx], mean=ref["mean"], std=ref["std"],
                target_mean=ref["target_mean"][idx], target_std=ref["target_std"][idx])


def lattice(xs, ys, zs):
    """x fastest"""
    xs, ys, zs = (np.asarray(v, dtype=np.float64) for v in (xs, ys, zs))
    return (np.tile(xs, len(ys) * len(zs)), np.tile(np.repeat(ys, len(xs)), len(zs)), np.repeat(zs, len(xs) * len(ys)))


# ---------------------------------------------------------------- the association, the groups, the slabs

HI = np.array([800.0, 600.0, 400.0])
NPTS = 9  # target points of the widest request; its series follow


def small_ensemble(M):
    """M models of 1 - 4 uniform cells, 70 nodes (a forced slab of 64 leaves a tail of 6), 9 target points and
    M x 8 series, one of them constant (a zero sigma) -- and the reference for all 17 targets, made once."""
    rng = np.random.default_rng(1000 + M)
    models = []
    for _ in range(M):
        n = int(rng.integers(1, 5))
        models.append(tuple((rng.random((n, 3)) * HI).T) + (rng.uniform(0, 50, n),))
    q = rng.uniform(-0.1, 1.1, (70, 3)) * HI
    t = rng.uniform(0, 1, (NPTS, 3)) * HI
    t[1] = q[3]  # (a target that is a node)
    series = rng.normal(size=(M, 8)) * rng.uniform(0.1, 30, 8) + rng.uniform(-5, 5, 8)
    series[:, 2] = 2.0
    ref = cref.covariance(models, q[:, 0], q[:, 1], q[:, 2], t[:, 0], t[:, 1], t[:, 2], series)
    return models, q, t, series, ref


@pytest.mark.parametrize("M", [1, 2, 15, 16, 17, 1024, 1025, 2500])
def test_every_branch_of_the_association_and_every_group_shape(tt, ctx, M):
    """M = 1: NaN; < 16: left to right; 16 .. 1024: one block; 1025: 513 + 512; 2500: two levels.  T = 1, G,
    G + 1, 2 G + 1 targets (points and series mixed), slabs of 64 + 6 nodes."""
    G = tt.TdContext.covariance_group()
    assert G == 8  # (the widest request below is 2 G + 1 = 9 points + 8 series)
    models, q, t, series, ref = small_ensemble(M)
    if M == 1:
        assert np.isnan(ref["cov"]).all() and np.isnan(ref["std"]).all()
    else:
        assert np.isfinite(ref["cov"]).all() and np.isnan(ref["corr"][NPTS + 2]).all()  # (the constant series)
        assert np.isfinite(np.delete(ref["corr"], NPTS + 2, axis=0)).all()
    ctx.set_volume_slab_nodes(64)
    ctx.timing(enable=True, reset=True)
    try:
        for T in (1, G, G + 1, 2 * G + 1):
            npts = (T + 1) // 2
            nser = T - npts
            r = ctx.covariance(models, q[:, 0], q[:, 1], q[:, 2], t[:npts], series[:, :nser] if nser else None)
            same(r, rows(ref, list(range(npts)) + [NPTS + j for j in range(nser)]))
        assert ctx.timing(kernel="cov_targets")[0] == 4 * 2  # (one launch group per slab)
        only_series = ctx.covariance(models, q[:, 0], q[:, 1], q[:, 2], None, series, want="corr")
        assert only_series["cov"] is None
        same(only_series, rows(ref, [NPTS + j for j in range(8)]), ("corr", "mean", "std", "target_mean", "target_std"))
        only_cov = ctx.covariance(models, q[:, 0], q[:, 1], q[:, 2], t[:3], want=("cov",))
        assert only_cov["corr"] is None
        same(only_cov, rows(ref, [0, 1, 2]), ("cov", "mean", "std", "target_mean", "target_std"))
    finally:
        ctx.timing(enable=False)
        ctx.set_volume_slab_nodes(0)


def test_no_nodes_still_gives_the_target_statistics(ctx):
    models, q, t, series, ref = small_ensemble(17)
    r = ctx.covariance(models, [], [], [], t[:2], series[:, :1])
    assert r["cov"].shape == r["corr"].shape == (3, 0) and r["mean"].shape == (0,)
    want = rows(ref, [0, 1, NPTS])
    same(r, want, ("target_mean", "target_std"))


def test_more_models_than_the_combine_stack_holds_are_refused(tt, ctx):
    """2^25 + 1 models would need a 16th level of waiting left halves (more than 64 KiB of LDS): TD_ERR_ARG
    before any device work (models of no cells: only their offsets exist)."""
    import ctypes
    from importlib import import_module

    _lib = import_module("mcmc_in_tonga_amd._lib")
    L = tt.lib()
    nm = (1 << 25) + 1
    off = np.zeros(nm + 1, dtype=np.int64)
    q, t, out = np.zeros(1), np.zeros(1), np.zeros(1)
    p = _lib.ptr
    req = _lib.TdCovariance(p(q), p(q), p(q), 1, p(t), p(t), p(t), 1, None, 0, p(out), None, None, None, None, None)
    assert L.td_rasterize_covariance(ctx.h, nm, p(off), None, None, None, None, ctypes.byref(req)) == 1
    assert L.td_last_error(ctx.h) == b"td_rasterize_covariance: more than 2^25 models"


# ---------------------------------------------------------------- the adversarial ensemble

def adversarial():
    """13 models (not a multiple of 8) of 0, 1, 2, 255, 256, 257 and 600 cells -- an empty one, one whose only
    cell lies beyond the sentinel, cells that tie, cells that are duplicated, a degenerate axis, a far
    outlier, a NaN cell -- and 9 x 7 x 5 nodes on multiples of 100 plus three nodes far outside every box and
    one with a NaN coordinate."""
    rng = np.random.default_rng(5)
    hi = np.array([800.0, 600.0, 400.0])

    def uniform(n):
        return tuple((rng.random((n, 3)) * hi).T) + (rng.uniform(0, 50, n),)

    # cells on the even multiples of 100: a node on an odd multiple is exactly as far from 2, 4 or 8 of them
    gx, gy, gz = np.meshgrid(np.arange(10) * 200.0 - 400, np.arange(10) * 200.0 - 600, np.arange(6) * 200.0 - 200,
                             indexing="ij")
    perm = rng.permutation(600)
    on_lattice = (gx.ravel()[perm], gy.ravel()[perm], gz.ravel()[perm], np.arange(600) * 0.0625 + 1.0)
    x, y, z, _ = uniform(128)
    dup = rng.permutation(256) % 128
    duplicates = (x[dup], y[dup], z[dup], np.arange(256) * 0.125)  # every cell twice, zeta by index
    x, y, z, ze = uniform(255)
    coplanar = (x, y, np.full(255, 137.5), ze)
    c = rng.random((256, 3)) * 3.0  # a tight cluster in one corner and one far cell
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


NODE_A, NODE_B = 3 + 9 * (1 + 7 * 3), 5 + 9 * (4 + 7 * 2)  # (300, 100, 300): eight cells of model 2 tie; (500, 400, 200)
# a lattice node, a second one, an off-lattice point, a point out of every model's reach, a NaN coordinate
ADV_TARGETS = np.array([[300.0, 100.0, 300.0], [500.0, 400.0, 200.0], [123.4, 234.5, 56.7], [-1e5, -1e5, -1e5],
                        [200.0, np.nan, 100.0]])


@pytest.fixture(scope="module")
def adv():
    models, qx, qy, qz = adversarial()
    assert (qx[NODE_A], qy[NODE_A], qz[NODE_A]) == (300.0, 100.0, 300.0)
    assert (qx[NODE_B], qy[NODE_B], qz[NODE_B]) == (500.0, 400.0, 200.0)
    ref = cref.covariance(models, qx, qy, qz, *ADV_TARGETS.T)
    for a in ref.values():
        a.setflags(write=False)
    return models, qx, qy, qz, ref


def test_adversarial_ensemble_whatever_the_slab_the_sweep_and_the_instance(tt, ctx, adv):
    models, qx, qy, qz, ref = adv
    T = tt.TdContext
    A = ref["targets"]
    assert np.all(A[:, 3] == 0.0) and np.all(A[:, 4] == 0.0) and np.all(A[1] == 0.0) and np.all(A[3] == 0.0)
    for t in (3, 4):  # a series of zeros: cov is exactly 0, corr is 0 / 0
        assert np.all(ref["cov"][t] == 0.0) and np.isnan(ref["corr"][t]).all()
    assert np.isfinite(ref["cov"]).all() and np.isfinite(ref["corr"][:3, :317]).all()
    assert np.isnan(ref["corr"][:, 317:]).all()  # (the two nodes nothing reaches: sigma 0)
    runs = []
    try:
        for method in (T.VOL_AUTO, T.VOL_GRID, T.VOL_BRUTE):
            ctx.set_volume_method(method)
            for slab in (64, 128, 0):
                ctx.set_volume_slab_nodes(slab)
                for counting in (False, True):
                    ctx.set_volume_counting(counting)
                    runs.append(ctx.covariance(models, qx, qy, qz, ADV_TARGETS))
                    c = ctx.volume_counters()
                    if counting or method == T.VOL_BRUTE:  # the nodes' and the targets' sweeps
                        assert sum(c) == len(models) * (len(qx) + len(ADV_TARGETS)), c
                    else:
                        assert c == (-1, -1, -1, 0)
        runs.append(ctx.covariance(models, qx, qy, qz, ADV_TARGETS))  # a repeated call
    finally:
        ctx.set_volume_counting(False)
        ctx.set_volume_method(T.VOL_AUTO)
        ctx.set_volume_slab_nodes(0)
    for r in runs:
        same(r, ref)
        assert np.all(r["cov"][3] == 0.0) and np.isnan(r["corr"][3]).all()


def test_invariants_that_need_no_reference(tt, ctx, adv):
    models, qx, qy, qz, _ = adv
    r = ctx.covariance(models, qx, qy, qz, ADV_TARGETS[:3])
    # a target that is a node: its own variance, and the two nodes' cross terms agree
    assert np.sqrt(r["cov"][0][NODE_A]) == r["std"][NODE_A] and np.sqrt(r["cov"][1][NODE_B]) == r["std"][NODE_B]
    assert r["target_mean"][0] == r["mean"][NODE_A] and r["target_std"][1] == r["std"][NODE_B]
    assert r["cov"][0][NODE_B] == r["cov"][1][NODE_A] and r["cov"][0][NODE_B] != 0.0
    assert r["corr"][0][NODE_B] == r["corr"][1][NODE_A]
    # corr = c / (sqrt(c) * sqrt(c)): four roundings (two roots, the product, the quotient) of at most 2^-53 each
    assert abs(r["corr"][0][NODE_A] - 1.0) <= ONE_ULPS
    # mean and std are the volume's
    vol = ctx.volume(models, qx, qy, qz, want_values=True)
    assert np.array_equal(r["mean"], vol["mean"]) and np.array_equal(r["std"], vol["std"], equal_nan=True)
    # the same series handed in by the caller: the same rows, wherever they stand
    V = vol["values"]
    ser = np.ascontiguousarray(V[:, [NODE_B, NODE_A]])
    s = ctx.covariance(models, qx, qy, qz, ADV_TARGETS[2:3], ser)
    for f in ("cov", "corr"):
        assert np.array_equal(s[f][0], r[f][2], equal_nan=True), f
        assert np.array_equal(s[f][1], r[f][1], equal_nan=True) and np.array_equal(s[f][2], r[f][0], equal_nan=True), f
    only = ctx.covariance(models, qx, qy, qz, None, ser[:, 1])  # (one series, as a vector)
    assert np.array_equal(only["cov"][0], r["cov"][0], equal_nan=True)
    # one NaN in a series: a NaN row, the others untouched
    bad = ser.copy()
    bad[7, 0] = np.nan
    b = ctx.covariance(models, qx, qy, qz, ADV_TARGETS[2:3], bad)
    assert np.isnan(b["cov"][1]).all() and np.isnan(b["corr"][1]).all()
    assert np.isnan(b["target_mean"][1]) and np.isnan(b["target_std"][1])
    for f in FIELDS:
        assert np.array_equal(np.delete(b[f], 1, axis=0) if f.startswith(("c", "t")) else b[f],
                              np.delete(s[f], 1, axis=0) if f.startswith(("c", "t")) else s[f], equal_nan=True), f


# ---------------------------------------------------------------- histories and the lattice form

@pytest.fixture(scope="module")
def recorded(tt, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=400)
    hists = []
    for k in range(2):
        c = tt.Chain(ctx, tt.chain_params(prm, None, seed=70 + k, chain=k + 1), tt.random_model(30, 70 + k))
        h = tt.History(ctx, 40, 40 * 400, with_ptS=False)
        c.run_recorded(400, 10, 10, h)
        assert len(h) == 40
        hists.append(h)
    empty = tt.History(ctx, 4, 4 * 400, with_ptS=False)
    return [hists[0], empty, hists[1]]


def test_histories_equal_their_models_read_back(tt, ctx, recorded):
    hists = recorded
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    qx, qy, qz = lattice(np.linspace(xmin - 30, xmax + 30, 9), np.linspace(ymin, ymax, 7), np.linspace(zmin, zmax + 50, 5))
    targets = np.array([[qx[100], qy[100], qz[100]], [0.5 * (xmin + xmax), 0.5 * (ymin + ymax), 0.3 * (zmin + zmax)]])
    flat = [m.cells() for h in hists if len(h) for m in h.read()]
    assert len(flat) == 80
    series = np.array([[len(m[0]), float(np.mean(m[3]))] for m in flat])  # the nCells trace, the mean zeta
    ref = cref.covariance(flat, qx, qy, qz, *targets.T, series)
    assert np.isfinite(ref["corr"]).any()
    a = ctx.covariance(flat, qx, qy, qz, targets, series)
    same(a, ref)
    try:
        for slab in (64, 0):
            ctx.set_volume_slab_nodes(slab)
            same(ctx.covariance_history(hists, qx, qy, qz, targets, series), ref)
    finally:
        ctx.set_volume_slab_nodes(0)
    with pytest.raises(tt.TdError, match="td_history_covariance: the histories hold no sample"):
        ctx.covariance_history([hists[1]], qx, qy, qz, targets)
    with pytest.raises(ValueError, match="series must be"):
        ctx.covariance_history(hists, qx, qy, qz, targets, series[:79])


def test_posterior_covariance_on_the_lattice(tt, ds, recorded):
    hists = recorded
    own = tt.context_for(ds)  # (ds's own cached context: not the one that recorded the histories)
    thin = copy.copy(ds)
    thin.xVec, thin.yVec, thin.zVec = (np.asarray(v, dtype=np.float64)[::6] for v in (ds.xVec, ds.yVec, ds.zVec))
    xv, yv, zv = thin.xVec, thin.yVec, thin.zVec
    nx, ny, nz = len(xv), len(yv), len(zv)
    prm = tt.define_TDstructrure()
    targets = np.array([[xv[nx // 2], yv[ny // 2], zv[1]], [xv[1] + 3.0, yv[2] - 2.0, zv[nz // 2] + 1.0]])
    flat_models = [m for h in hists if len(h) for m in h.read()]
    series = np.array([[float(len(m.cells()[0]))] for m in flat_models])
    out = tt.posterior_covariance(hists, thin, prm, targets, series)
    qx, qy, qz = lattice(xv, yv, zv)
    r = own.covariance_history(hists, qx, qy, qz, targets, series)
    T = 3
    assert out["cov"].shape == out["corr"].shape == (T, nx, ny, nz) and out["mean"].shape == out["std"].shape == (nx, ny, nz)
    for f in ("cov", "corr"):
        for t in range(T):
            assert np.array_equal(out[f][t], r[f][t].reshape(nz, ny, nx).transpose(2, 1, 0), equal_nan=True), (f, t)
            assert out[f][t][3, 2, 1] == r[f][t][3 + nx * (2 + ny * 1)] or np.isnan(out[f][t][3, 2, 1])
    for f in ("mean", "std"):
        assert np.array_equal(out[f], r[f].reshape(nz, ny, nx).transpose(2, 1, 0), equal_nan=True), f
    assert np.array_equal(out["target_mean"], r["target_mean"]) and np.array_equal(out["target_std"], r["target_std"])
    # the target on a node correlates fully with that node
    assert abs(out["corr"][0][nx // 2, ny // 2, 1] - 1.0) <= ONE_ULPS
    # the footprint, recounted
    vol = (xv[-1] - xv[0]) / (nx - 1) * (yv[-1] - yv[0]) / (ny - 1) * (zv[-1] - zv[0]) / (nz - 1)
    assert np.isclose(out["node_volume"], vol, rtol=1e-15, atol=0) and out["footprint"].shape == (T,)
    for t in range(T):
        count = sum(1 for v in out["corr"][t].ravel() if v >= 0.5)
        assert out["footprint"][t] == count * out["node_volume"]
    assert out["footprint"][0] >= out["node_volume"]  # (at least the target's own node)
    # Models and nested lists give what the histories give
    nested = [[m for m in h.read()] for h in hists if len(h)]
    for form in (flat_models, nested):
        o2 = tt.posterior_covariance(form, thin, prm, targets, series)
        for f in ("cov", "corr", "mean", "std", "footprint"):
            assert np.array_equal(o2[f], out[f], equal_nan=True), f
