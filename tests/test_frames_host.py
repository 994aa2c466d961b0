"""Coordinate frames on the CPU (tests/frames.py): the helper itself, the C oracle in every frame, the host
one-point grid (csrc/host_nn.h) in every frame, and the bucket grid's lower bound (csrc/internal.h
grid_block_lb through the tdt_grid_lb hook) -- the claim the evaluate grid, the chain's grid query and the
volume sweep all rest on: every cell whose bucket lies outside a point's (2R+1)^3 block is strictly
farther, in the reference's FP64 squared distance, than the bound.  No GPU."""
import ctypes

import numpy as np
import pytest

import frames
from test_host_nn import check
from tile_filter_ref import dist2


@pytest.fixture(scope="module")
def identity_ref(orc, ds):
    cells = frames.frame_model("identity", frames.GPU_CELLS, frames.MODEL_SEED).cells()
    r = orc.evaluate(ds.rayX, ds.rayY, ds.rayZ, ds.rayL, ds.rayU, ds.tS, ds.allSig, cells)
    assert r["rc"] == 0 and np.all(r["nearest"] >= 0)
    r["ptS"].setflags(write=False)
    return r


def test_identity_reproduces_the_shipped_data(ds):
    f = frames.in_frame(ds, "identity")
    for name in ("rayX", "rayY", "rayZ", "U", "rayL", "rayU", "xVec", "yVec", "zVec"):
        a, b = getattr(f, name), getattr(ds, name)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), name
    assert f.tS is ds.tS and f.allSig is ds.allSig
    assert frames.frame_box("identity") == tuple(frames.tonga.load().box())


@pytest.mark.parametrize("name", frames.ALL)
def test_frame_is_legal_for_the_oracle(orc, ds, identity_ref, name):
    f = frames.in_frame(ds, name)
    assert np.array_equal(np.isnan(f.rayX), np.isnan(ds.rayX)) and np.array_equal(np.isnan(f.rayY), np.isnan(ds.rayX))
    b = frames.frame_box(name)
    m = frames.frame_model(name, frames.GPU_CELLS, frames.MODEL_SEED)
    for a, v in enumerate(m.cells()[:3]):
        assert np.all((v >= b[2 * a]) & (v <= b[2 * a + 1]))
    r = orc.evaluate(f.rayX, f.rayY, f.rayZ, f.rayL, f.rayU, f.tS, f.allSig, m.cells())
    assert r["rc"] == 0
    if name not in frames.SENTINEL_BINDS:
        # lengths scale by s and slowness by 1 / s: ptS is the identity frame's up to the rounding of the
        # coordinates (2.1e-8 in `far`, whose ulp is 2e-6 against segments of about 10); a forgotten 1 / s
        # would be off by at least 1e3
        assert np.all(r["nearest"] >= 0)
        rel = np.max(np.abs(r["ptS"] - identity_ref["ptS"]) / np.abs(identity_ref["ptS"]))
        print(name, "max relative difference of ptS %.2e" % rel)
        assert rel <= 1e-5
    if name == "flat":
        assert np.all(f.rayY[~np.isnan(f.rayY)] == frames.FLAT_Y) and b[2] == b[3] == frames.FLAT_Y
        assert np.all(m.yCell == frames.FLAT_Y)


def test_the_sentinel_binds_in_metres(orc, ds):
    """In a metre frame the 1e9 sentinel is (31.6 km)^2: with the cells the GPU tests use, most ray points
    have no cell in reach (the oracle's nearest = -1, zeta 0) and some have one."""
    f = frames.in_frame(ds, "metres")
    cells = frames.frame_model("metres", frames.GPU_CELLS, frames.MODEL_SEED, hostile=True).cells()
    r = orc.evaluate(f.rayX, f.rayY, f.rayZ, f.rayL, f.rayU, f.tS, f.allSig, cells)
    share = float(np.mean(r["nearest"] >= 0))
    print("share of ray points with a cell in reach: %.3f" % share)
    assert r["rc"] == 0 and 0.03 <= share <= 0.5


def frame_points(rng, name, k, pad=0.0):
    """k points uniform in the frame's box widened by `pad` extents on every side (flat axes stay flat)."""
    b = np.array(frames.frame_box(name))
    lo, hi = b[0::2], b[1::2]
    ext = hi - lo
    return lo - pad * ext + (ext + 2 * pad * ext) * rng.random((k, 3))


@pytest.mark.parametrize("n", [1, 2, 50, 700])
@pytest.mark.parametrize("name", frames.ALL)
def test_host_grid_in_every_frame(tt, orc, name, n):
    """test_host_nn.py::test_random_models_and_edits with the cells, the committed edits, the pending edit
    and the queries in the frame."""
    rng = np.random.default_rng(n)
    c = frame_points(rng, name, n)
    cells = [c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy(), rng.normal(size=n)]
    edits, m = [], n
    for _ in range(40):
        a = int(rng.integers(1, 5)) if m > 1 else 1
        k = int(rng.integers(0, m)) if a != 1 else m
        p = frame_points(rng, name, 1)[0]
        edits.append([a, k, p[0], p[1], p[2], rng.normal()])
        m += 1 if a == 1 else -1 if a == 2 else 0
    Q = np.concatenate([frame_points(rng, name, 40, 0.1),  # inside and just around the box
                        frame_points(rng, name, 8, 10.0),  # far outside
                        c[:5]])  # on cells (distance 0)
    for a in (None, 1, 2, 3, 4):
        if a is None:
            pend = None
        elif a == 1:
            pend = [1, m] + list(frame_points(rng, name, 1)[0]) + [0.5]
        else:
            pend = [a, int(rng.integers(0, m))] + list(frame_points(rng, name, 1)[0]) + [rng.normal()]
        if a == 2 and m < 2:
            continue
        check(tt, orc, cells, edits, pend, Q)


def grid_lb(tt, lo, hi, target, max_dim, max_buckets, P, R):
    """tdt_grid_lb -> (ijk [n, 3], lb [n], dims [3], h [3], e [3])"""
    pd = ctypes.POINTER(ctypes.c_double)
    pi = ctypes.POINTER(ctypes.c_int32)
    lo, hi = (np.ascontiguousarray(v, dtype=np.float64) for v in (lo, hi))
    px, py, pz = (np.ascontiguousarray(P[:, a], dtype=np.float64) for a in range(3))
    ijk = np.full((len(P), 3), -1, dtype=np.int32)
    lb = np.full(len(P), np.nan)
    dims = np.zeros(3, dtype=np.int32)
    h, e = np.zeros(3), np.zeros(3)
    rc = tt.lib().tdt_grid_lb(lo.ctypes.data_as(pd), hi.ctypes.data_as(pd), float(target), int(max_dim),
                              int(max_buckets), px.ctypes.data_as(pd), py.ctypes.data_as(pd), pz.ctypes.data_as(pd),
                              len(P), int(R), ijk.ctypes.data_as(pi), lb.ctypes.data_as(pd), dims.ctypes.data_as(pi),
                              h.ctypes.data_as(pd), e.ctypes.data_as(pd))
    assert rc == 0
    return ijk, lb, dims, h, e


def bound_queries(rng, name, lo, hi, dims, h):
    """About 2000 points: inside the frame's box; on the computed faces v0 + i h of the grid over [lo, hi]
    and one ulp to either side; just outside and far outside; NaN.  -> (Q, number of inside ones first)."""
    inside = frame_points(rng, name, 800)
    on = []
    for a in range(3):
        g = int(dims[a])
        idx = np.arange(g + 1) if g <= 24 else np.unique(np.concatenate([np.arange(4), rng.integers(0, g + 1, 16),
                                                                          np.arange(g - 3, g + 1)]))
        for i in idx:
            f = lo[a] + float(i) * h[a]  # the face as grid_block_lb computes it
            for v in (f, np.nextafter(f, np.inf), np.nextafter(f, -np.inf)):
                q = frame_points(rng, name, 1)[0]
                q[a] = v
                on.append(q)
    ext = hi - lo
    near = frame_points(rng, name, 240)
    for k, q in enumerate(near):  # one axis just past a side of the grid's box: 1 ulp, 4 ulps, 1e-9 extents
        a, side = k % 3, (k // 3) % 2
        edge = hi[a] if side else lo[a]
        step = [np.nextafter(edge, np.inf if side else -np.inf) - edge, 4 * abs(np.spacing(edge)) * (1 if side else -1),
                1e-9 * ext[a] * (1 if side else -1), 0.0][(k // 6) % 4]
        q[a] = edge + step
    far = np.concatenate([frame_points(rng, name, 150, 3.0), frame_points(rng, name, 50, 1e6)])
    nan = frame_points(rng, name, 20)
    for k in range(20):
        nan[k, k % 3] = np.nan
    nan[-1] = np.nan
    return np.concatenate([inside, np.array(on), near, far, nan]), len(inside)


def aligned_pairs(rng, name, lo, hi, dims, h):
    """The pairs that hold the bound tight.  A random cell is off a query in all three axes, so its distance
    exceeds any face gap by far; these cells sit on the interior faces v0 + i h and one ulp to either side
    (where the rounding of floor((v - v0) inv) decides the bucket), and two queries per cell share its
    other two coordinates: dist2 is the squared gap along one axis alone.  -> (cells, queries)"""
    cells, qs = [], []
    for a in range(3):
        g = int(dims[a])
        for i in (np.arange(1, g) if g <= 24 else np.unique(rng.integers(1, g, 20))):
            f = lo[a] + float(i) * h[a]
            for v in (f, np.nextafter(f, np.inf), np.nextafter(f, -np.inf)):
                c = frame_points(rng, name, 1)[0]
                c[a] = min(max(v, lo[a]), hi[a])
                cells.append(c)
                q = c.copy()
                q[a] = lo[a] + (hi[a] - lo[a]) * rng.random()  # anywhere along the axis
                fk = lo[a] + float(rng.integers(0, g + 1)) * h[a]
                q2 = c.copy()
                q2[a] = np.nextafter(fk, rng.choice([-np.inf, np.inf]))  # beside another face
                qs += [q, q2]
    return np.array(cells).reshape(-1, 3), np.array(qs).reshape(-1, 3)


def assert_bound(tt, name, lo, hi, cells, max_dim, max_buckets, seed):
    rng = np.random.default_rng(seed)
    target = len(cells) / 2.0  # (the grid of the random cells alone, as the product would size it)
    _, _, dims, h, e = grid_lb(tt, lo, hi, target, max_dim, max_buckets, cells, 0)
    on_faces, aligned = aligned_pairs(rng, name, lo, hi, dims, h)
    cells = np.concatenate([cells, on_faces])
    cijk, _, _, _, _ = grid_lb(tt, lo, hi, target, max_dim, max_buckets, cells, 0)
    assert np.all(cijk >= 0) and np.all(cijk < dims[None, :])
    assert np.all((cells >= lo) & (cells <= hi))  # sealed: what make_cell_grid's callers promise
    Q, n_in = bound_queries(rng, name, lo, hi, dims, h)
    Q = np.concatenate([Q, aligned])
    finite = ~np.isnan(Q).any(axis=1)
    d2 = dist2(cells[None, :, 0], cells[None, :, 1], cells[None, :, 2], Q[:, 0, None], Q[:, 1, None], Q[:, 2, None])
    assert np.all(np.isnan(d2[~finite]))  # (a NaN point is no nearer to anything: nothing to prove for it)
    for R in (0, 1, 2):
        qijk, lb, _, _, _ = grid_lb(tt, lo, hi, target, max_dim, max_buckets, Q, R)
        assert not np.isnan(lb).any() and np.all(lb >= 0)
        outside = (np.abs(qijk[:, None, :] - cijk[None, :, :]) > R).any(axis=2) & finite[:, None]
        bad = np.argwhere(outside & ~(d2 > lb[:, None]))
        assert bad.size == 0, (name, R, dims, [(Q[q], cells[c], d2[q, c], lb[q]) for q, c in bad[:3]])
        share = outside.sum() / float(finite.sum() * len(cells))
        print(name, "grid", dims, "R", R, "pairs outside the block %.3f" % share,
              "inside points with a bound > 0: %.3f" % np.mean(lb[:n_in] > 0))
        assert share >= 0.1  # (the claim is about many pairs)
        if R == 1:
            assert np.mean(lb[:n_in] > 0) >= 0.5  # (and the bound says something)


@pytest.mark.parametrize("n,max_dim,max_buckets", [(300, 256, 1 << 24), (3000, 4096, 1 << 16)])
@pytest.mark.parametrize("name", frames.ALL)
def test_grid_bound_in_every_frame(tt, name, n, max_dim, max_buckets):
    """The grid over the frame's box (the chain's grid, and its limits, at 300 cells; the evaluate's at
    3000), the cells inside it."""
    b = np.array(frames.frame_box(name))
    m = frames.frame_model(name, n, 3 + n)
    assert_bound(tt, name, b[0::2], b[1::2], np.stack(m.cells()[:3], 1), max_dim, max_buckets, n)


@pytest.mark.parametrize("name", ["identity", "far"])
def test_grid_bound_over_the_cells_own_box(tt, name):
    """As the evaluate builds it: 30 of the cells lie outside the frame's box and the grid spans the cells'
    own extent, so the outermost cells sit exactly on its sides (bucket g clamped to g - 1)."""
    rng = np.random.default_rng(5)
    m = frames.frame_model(name, 300, 11)
    cells = np.concatenate([np.stack(m.cells()[:3], 1), frame_points(rng, name, 30, 0.5)])
    assert_bound(tt, name, cells.min(axis=0), cells.max(axis=0), cells, 4096, 1 << 16, 6)
