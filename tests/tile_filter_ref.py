"""Helpers shared by the tile-filter tests (test_gpu_tile_filter.py, test_gpu_frames.py): the reference's
FP64 squared distance, FP32 tile boxes rounded outward, and the call of the tdt_tile_filter hook.  A plain
module, not a conftest."""
import ctypes

import numpy as np


def dist2(px, py, pz, qx, qy, qz):
    dx, dy, dz = px - qx, py - qy, pz - qz  # (mx-x)^2 + (my-y)^2 + (mz-z)^2 left to right, no FMA
    return (dx * dx + dy * dy) + dz * dz


def outward_box(v):
    lo, hi = np.float32(v.min()), np.float32(v.max())
    if float(lo) > v.min():
        lo = np.nextafter(lo, np.float32(-np.inf))
    if float(hi) < v.max():
        hi = np.nextafter(hi, np.float32(np.inf))
    return lo, hi


def tile_boxes(pts):
    """FP32 boxes (SoA [3, nt]) of the tiles pts[t] = [k, 3], rounded outward."""
    nt = len(pts)
    lo = np.zeros((3, nt), dtype=np.float32)
    hi = np.zeros((3, nt), dtype=np.float32)
    for t, p in enumerate(pts):
        for a in range(3):
            lo[a, t], hi[a, t] = outward_box(p[:, a])
    return lo, hi


def min_dist(pts, qs):
    """[nq, nt]: each query's FP64 minimum squared distance to each tile's points."""
    return np.array([[dist2(p[:, 0], p[:, 1], p[:, 2], *q).min() for p in pts] for q in qs])


def filter_hits(tt, lo, hi, maxd, qs, mode):
    """tdt_tile_filter -> bool [nq, nt]: tile t passes for query q."""
    nt, nq = lo.shape[1], len(qs)
    hit = np.zeros(nq * nt, dtype=np.uint8)
    f32 = ctypes.POINTER(ctypes.c_float)
    L = tt.lib()
    lo_c, hi_c = np.ascontiguousarray(lo), np.ascontiguousarray(hi)
    qs_c = np.ascontiguousarray(qs)
    maxd = np.ascontiguousarray(maxd, dtype=np.float64)
    rc = L.tdt_tile_filter(lo_c.ctypes.data_as(f32), hi_c.ctypes.data_as(f32),
                           maxd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nt,
                           qs_c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nq, mode,
                           hit.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    assert rc == 0
    return hit.reshape(nq, nt).astype(bool)


def boundary_case(rng, P, unit=1.0, large=True, nt=400, nq=300):
    """Tiles of 16 consecutive points of P [n, 3], queries on, near and far from them (distances in `unit`s),
    and tile maxima set EXACTLY to some query's FP64 minimum distance (six of seven) or near it.
    -> (pts, qs, md [nq, nt], owner [nt], maxd [nt])."""
    starts = rng.integers(0, len(P) - 16, nt)
    pts = [P[s:s + 16].copy() for s in starts]
    if large:
        pts[:50] = [p * 37.0 + 1000.0 * rng.standard_normal(3) for p in pts[:50]]  # large coordinates too
    qs = np.empty((nq, 3))
    for k in range(nq):  # on a point, near a box, or anywhere in the cloud
        t = rng.integers(nt)
        kind = k % 3
        if kind == 0:
            qs[k] = pts[t][rng.integers(16)]
        elif kind == 1:
            qs[k] = pts[t][rng.integers(16)] + rng.standard_normal(3) * rng.choice([1e-9, 1e-4, 1.0, 30.0]) * unit
        else:
            qs[k] = pts[rng.integers(nt)].mean(0) + rng.standard_normal(3) * 200.0 * unit
    md = min_dist(pts, qs)
    # each tile's maximum: exactly some query's minimum distance to it (the boundary), or a random one
    owner = rng.integers(0, nq, nt)
    maxd = md[owner, np.arange(nt)].copy()
    maxd[::7] *= rng.uniform(0.5, 2.0, len(maxd[::7]))
    return pts, qs, md, owner, maxd
