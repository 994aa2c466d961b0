"""The posterior data support's definition (include/tdstar_support.h), restated in numpy on oracle_np.nearest_index
(the owner of a ray point and the cell a node picks; -1, or any index outside the model, is "none") and
regions_ref.statistics (the mean and sigma of the node matrix).  With k the quantised weights and e their exponent:
    K[c]       = sum over the points c owns of k[p]            (int64, np.add.at)
    count[c]   = the points c owns
    sup[c]     = np.ldexp(float64(K[c]), -e)
    barren[m]  = #{c of m : count[c] == 0},  orphans[m] = #{p : no owner}
    U[m][q]    = sup[the cell of m that node q picks], 0.0 where none
    exceed[t][q] = #{m : U[m][q] > thr[t]}"""
import math
from types import SimpleNamespace

import numpy as np

import regions_ref as rref
from oracle import oracle_np


def quantise(w, P):
    """-> (k int64 [P], e): A = the sum of |w| left to right, A = f 2^E (frexp), e = 61 - E (0 when A == 0),
    k = rint(ldexp(w, e)), to nearest even.  w None: ones and 0."""
    if w is None:
        return np.ones(P, dtype=np.int64), 0
    w = np.asarray(w, dtype=np.float64)
    assert w.shape == (P,)
    A = 0.0
    for v in w.tolist():
        A = A + abs(v)
    e = 0 if A == 0.0 else 61 - math.frexp(A)[1]
    return np.rint(np.ldexp(w, e)).astype(np.int64), e


def owners(cells, px, py, pz):
    """The owning cell of every point, -1: none."""
    nc = len(cells[0])
    idx = np.asarray(oracle_np.nearest_index(px, py, pz, cells[0], cells[1], cells[2]), dtype=np.int64)
    return np.where((idx >= 0) & (idx < nc), idx, -1)


def support(models, px, py, pz, w=None, qx=None, qy=None, qz=None, thr=()):
    """models: (x, y, z[, zeta]) per model; (px, py, pz): the context's valid ray points, ray-major.
    -> dict(cell, count [total], barren, orphans [M], k, e and with nodes values [M][nq], mean, std [nq],
    exceed [nthr][nq])."""
    px, py, pz = (np.asarray(v, dtype=np.float64).ravel() for v in (px, py, pz))
    k, e = quantise(w, len(px))
    cell, count, barren, orphans, U = [], [], [], [], []
    for cells in models:
        nc = len(cells[0])
        own = owners(cells, px, py, pz)
        has = own >= 0
        K = np.zeros(nc, dtype=np.int64)
        np.add.at(K, own[has], k[has])
        cnt = np.bincount(own[has], minlength=nc).astype(np.int64)
        sup = np.ldexp(K.astype(np.float64), -e)
        cell.append(sup)
        count.append(cnt)
        barren.append(int(np.sum(cnt == 0)))
        orphans.append(int(np.sum(~has)))
        if qx is not None:
            pick = owners(cells, qx, qy, qz)
            U.append(np.where(pick >= 0, sup[np.maximum(pick, 0)], 0.0) if nc else np.zeros(len(pick)))
    out = dict(cell=np.concatenate(cell) if cell else np.zeros(0),
               count=np.concatenate(count) if count else np.zeros(0, dtype=np.int64),
               barren=np.array(barren, dtype=np.int64), orphans=np.array(orphans, dtype=np.int64), k=k, e=e)
    if qx is not None:
        U = np.array(U)
        mean, std = rref.statistics(U)
        thr = np.asarray(thr, dtype=np.float64).ravel()
        out.update(values=U, mean=mean, std=std,
                   exceed=np.array([np.sum(U > t, axis=0) for t in thr], dtype=np.int64).reshape(len(thr), U.shape[1]))
    return out


def csr_points(rayX, rayY, rayZ):
    """The valid points (the leading non-NaN of every column of rayX), ray-major: (npts, px, py, pz)."""
    npts = np.array([int(np.argmax(np.isnan(c))) if np.isnan(c).any() else len(c) for c in rayX.T], dtype=np.int64)
    pick = lambda a: np.concatenate([a[:c, i] for i, c in enumerate(npts)])  # noqa: E731
    return npts, pick(rayX), pick(rayY), pick(rayZ)


def cut_rays(tt, ds, rng, nrays, scale=1.0):
    """`nrays` of the shipped rays, and among them rays of 0, 1 and 2 points (columns 10, 20 and the last), the
    coordinates times `scale` (1000.0: a metre frame; the slowness stays that of the kilometre depths).
    -> a namespace with rayX, rayY, rayZ, rayL, rayU, U, tS, allSig (what TdContext takes), xVec, yVec, zVec, and
    the valid points npts, px, py, pz."""
    pick = np.sort(rng.choice(ds.rayX.shape[1], nrays, replace=False))
    cols = {f: np.asarray(getattr(ds, f), dtype=np.float64)[:, pick] for f in ("rayX", "rayY", "rayZ", "U")}
    for at, c in ((10, 0), (20, 1), (cols["rayX"].shape[1] + 2, 2)):  # (a short ray: the first c points of a neighbour)
        for f in cols:
            short = np.full(cols[f].shape[0], np.nan)
            short[:c] = cols[f][:c, at - 1]
            cols[f] = np.insert(cols[f], at, short, axis=1)
    n = cols["rayX"].shape[1]
    X, Y, Z = (cols[f] * scale for f in ("rayX", "rayY", "rayZ"))
    rayL, rayU = tt.segments(X, Y, Z, cols["U"])
    npts, px, py, pz = csr_points(X, Y, Z)
    return SimpleNamespace(rayX=X, rayY=Y, rayZ=Z, rayL=rayL, rayU=rayU, U=cols["U"], tS=rng.uniform(0.05, 1.2, n),
                           allSig=rng.uniform(0.04, 0.6, n), xVec=np.asarray(ds.xVec) * scale,
                           yVec=np.asarray(ds.yVec) * scale, zVec=np.asarray(ds.zVec) * scale, npts=npts, px=px, py=py,
                           pz=pz, _td_ctx=None)


NRAYS = 40


def base_case(tt, ds, metres=False):
    """default_rng(11): a context of NRAYS shipped rays with rays of 0, 1 and 2 points among them; 65 models of 5-40
    cells uniform in the box of the ray points; then the edge models: no cell, one cell, and a model whose cells 0
    and 1 are exact duplicates (the lower index owns everything they win); nodes: a 6 x 5 x 5 lattice over the box.
    metres: everything times 1000, so that most points lie beyond the search's sentinel (31.6 km) of every cell, and
    one more model with all its cells in one corner of the box.
    -> (rays, models, (qx, qy, qz))."""
    rng = np.random.default_rng(11)
    scale = 1000.0 if metres else 1.0
    rays = cut_rays(tt, ds, rng, NRAYS, scale)
    lo = [float(np.min(v)) for v in (rays.px, rays.py, rays.pz)]
    hi = [float(np.max(v)) for v in (rays.px, rays.py, rays.pz)]
    models = []
    for _ in range(65):
        n = int(rng.integers(5, 41))
        models.append(tuple(rng.uniform(lo[d], hi[d], n) for d in range(3)))
    models.append((np.zeros(0),) * 3)
    models.append(tuple(np.array([0.5 * (lo[d] + hi[d])]) for d in range(3)))
    dup = [rng.uniform(lo[d], hi[d], 12) for d in range(3)]
    for d, v in enumerate((rays.px, rays.py, rays.pz)):  # (both on a ray point, so that they win something)
        dup[d][0] = dup[d][1] = v[100]
    models.append(tuple(dup))
    if metres:
        models.append(tuple(rng.uniform(lo[d], lo[d] + 0.01 * (hi[d] - lo[d]), 9) for d in range(3)))
    axes = [np.linspace(lo[d], hi[d], n) for d, n in enumerate((6, 5, 5))]
    qx = np.tile(axes[0], 25)
    qy = np.tile(np.repeat(axes[1], 6), 5)
    qz = np.repeat(axes[2], 30)
    return rays, models, (qx, qy, qz)


DUPLICATES = 67  # the model of base_case whose cells 0 and 1 coincide
