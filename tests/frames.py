"""Coordinate frames for the tests: the shipped geometry under X' = s X + o, U' = U / s.

Every search in the library is exact because a floating-point error bound lets a cheaper search stop
early, and each bound's size depends on how large the coordinates are against the extent of the box.  The
Tonga ray frame has |coordinate| about equal to the extent; these frames do not (metres far from their
origin, offsets of 2^33 against an extent of 10^3, a box of 10^-3, a flat prior axis).  A plain module that
the tests import, as they import covariance_ref; it touches neither the library nor the GPU.

t* is invariant under the transform (lengths scale by s, slowness by 1 / s) -- except through the 1e9
sentinel of v_nearest (MCsub.jl:250), which is in squared coordinate units: in `metres` a point farther
than 31.6 km from every cell has no cell at all, in the reference as here."""
import dataclasses

import numpy as np

import tonga

FLAT_Y = 150.0  # inside the Tonga y range (-164.4 .. 495.6)

# name -> (scale, offset); `flat` is the identity frame with y = FLAT_Y everywhere (a 2-D section)
FRAMES = {
    "identity": (1.0, (0.0, 0.0, 0.0)),
    "metres": (1000.0, (5e5, 7.4e6, 0.0)),
    "far": (1.0, (2.0 ** 33 + 0.3, -2.0 ** 33, 2.0 ** 32)),
    "small_far": (1e-3, (1e6, -2e6, 3e6)),
    "tiny": (1e-6, (0.0, 0.0, 0.0)),
    "negative": (1.0, (-5e4, -6e4, -7e4)),
    "flat": (1.0, (0.0, 0.0, 0.0)),
}
ALL = tuple(FRAMES)
SENTINEL_BINDS = ("metres", "flat")  # frames whose ptS need not equal the identity frame's

# what the GPU tests run, and the CPU tests assert the preconditions of
GPU_CELLS = 300  # just above the evaluate's grid threshold (kGridMinCells = 256)
MODEL_SEED = 7


def to_frame(name, x, y, z):
    """The three coordinate arrays in the frame (NaN stays NaN)."""
    s, o = FRAMES[name]
    x, y, z = (s * np.asarray(v, dtype=np.float64) + c for v, c in zip((x, y, z), o))
    if name == "flat":
        y = np.where(np.isnan(y), y, FLAT_Y)
    return x, y, z


def in_frame(ds, name):
    """`ds` in the frame: rays and xVec / yVec / zVec transformed, U / s, rayL and rayU from data.segments of
    those; tS and allSig untouched."""
    tt = tonga.load()
    s, _ = FRAMES[name]
    X, Y, Z = to_frame(name, ds.rayX, ds.rayY, ds.rayZ)
    U = ds.U / s
    L, RU = tt.segments(X, Y, Z, U)
    xv, yv, zv = to_frame(name, ds.xVec, ds.yVec, ds.zVec)
    return dataclasses.replace(ds, rayX=X, rayY=Y, rayZ=Z, U=U, rayL=L, rayU=RU, xVec=xv, yVec=yv, zVec=zv,
                               _td_ctx=None)


def frame_box(name):
    """(xmin, xmax, ymin, ymax, zmin, zmax) of the prior box in the frame, for chain_params(extent=...)."""
    b = tonga.load().box()
    lo, hi = to_frame(name, *b[0::2]), to_frame(name, *b[1::2])
    return tuple(float(v) for a in range(3) for v in (lo[a], hi[a]))


def frame_model(name, n, seed, hostile=False):
    """A Model of n cells uniform in the frame's box (the same n points of the unit cube in every frame),
    zeta U(0, 50).  hostile: the first n // 10 sites again at the end with zeta + 1 (exact ties: the lower
    index must win), and three x set to NaN (cells that never win)."""
    tt = tonga.load()
    rng = np.random.default_rng(seed)
    b = tt.box()
    u = rng.random((3, n))
    c = to_frame(name, *(b[2 * a] + (b[2 * a + 1] - b[2 * a]) * u[a] for a in range(3)))
    fb = frame_box(name)
    x, y, z = (np.clip(c[a], fb[2 * a], fb[2 * a + 1]) for a in range(3))
    zeta = rng.random(n) * 50.0
    if hostile:
        k = n // 10
        x, y, z = (np.concatenate([v, v[:k]]) for v in (x, y, z))
        zeta = np.concatenate([zeta, zeta[:k] + 1.0])
        x[[k + 1, n // 2, n - 1]] = np.nan
    return tt.Model(float(len(x)), x, y, z, zeta)


def lattice(xs, ys, zs):
    """x fastest"""
    xs, ys, zs = (np.asarray(v, dtype=np.float64) for v in (xs, ys, zs))
    return (np.tile(xs, len(ys) * len(zs)), np.tile(np.repeat(ys, len(xs)), len(zs)), np.repeat(zs, len(xs) * len(ys)))


def frame_lattice(name):
    """9 x 7 x 5 nodes over the frame's box, three nodes farther than the sentinel distance (31 623 units)
    from the box and one node with a NaN coordinate: 319 nodes."""
    b = frame_box(name)
    qx, qy, qz = lattice(np.linspace(b[0], b[1], 9), np.linspace(b[2], b[3], 7), np.linspace(b[4], b[5], 5))
    far = np.array([[b[1] + 1e5, b[2], b[4]], [b[0], b[2] - 2e5, b[5]], [b[0] - 4e4, b[3] + 4e4, b[5] + 4e4]])
    qx = np.concatenate([qx, far[:, 0], [np.nan]])
    qy = np.concatenate([qy, far[:, 1], [b[2]]])
    qz = np.concatenate([qz, far[:, 2], [b[4]]])
    return qx, qy, qz


def ray_points(ds):
    """The finite ray points of `ds` in the library's order (ray after ray), [P, 3]."""
    X, Y, Z = (np.asarray(a, dtype=np.float64).T.ravel() for a in (ds.rayX, ds.rayY, ds.rayZ))
    ok = ~np.isnan(X)
    return np.stack([X[ok], Y[ok], Z[ok]], 1)
