"""The posterior interfaces' definition (include/tdstar_interfaces.h), restated in numpy on oracle_np.rasterize
(the value matrix, its mean and sigma) and oracle_np.julia_mapreduce_arrays (the sum of |d|).  On the lattice
xs x ys x zs, node n = i + nx (j + ny k), with d = V[m][n + s_a] - V[m][n] on the forward face of n along axis a:
    count[a][n]     = #{m : V[m][n] != V[m][n + s_a]}          (-1 without a face)
    any[n]          = #{m : the value differs across one of n's existing faces}   (-1 without any)
    exceed[t][a][n] = #{m : |d| > thr[t]}                      (-1 without a face)
    jump[a][n]      = mapreduce over m of |d|, / M             (NaN without a face)
    density[n]      = the cells whose nucleus lies in n's voxel (midpoints, searchsorted side="right"); a cell
                      with a NaN coordinate counts in `skipped` alone
numpy subtracts, compares and takes |.| element by element under IEEE rules (NaN != x, not NaN > t)."""
import numpy as np

from oracle import oracle_np


def lattice(xs, ys, zs):
    """The nodes' coordinates, x fastest."""
    xs, ys, zs = (np.asarray(v, dtype=np.float64) for v in (xs, ys, zs))
    return (np.tile(xs, len(ys) * len(zs)), np.tile(np.repeat(ys, len(xs)), len(zs)), np.repeat(zs, len(xs) * len(ys)))


def faces(nx, ny, nz):
    """has[a][n]: node n has a forward face along a; stride[a]."""
    n = np.arange(nx * ny * nz)
    idx = (n % nx, (n // nx) % ny, n // (nx * ny))
    has = np.array([idx[a] < (nx, ny, nz)[a] - 1 for a in range(3)])
    return has, (1, nx, nx * ny)


def face_statistics(V, nx, ny, nz, thresholds=()):
    """count [3][nq], any [nq], exceed [nthr][3][nq] (int64), jump [3][nq] of the value matrix V[M][nq]."""
    V = np.asarray(V, dtype=np.float64)
    M, nq = V.shape
    assert nq == nx * ny * nz
    thr = np.asarray(thresholds, dtype=np.float64).ravel()
    has, stride = faces(nx, ny, nz)
    count = np.full((3, nq), -1, dtype=np.int64)
    exceed = np.full((len(thr), 3, nq), -1, dtype=np.int64)
    jump = np.full((3, nq), np.nan)
    differs_any = np.zeros((M, nq), dtype=bool)
    for a in range(3):
        n = np.flatnonzero(has[a])
        if not len(n):
            continue
        lo, hi = V[:, n], V[:, n + stride[a]]
        with np.errstate(invalid="ignore"):
            d = np.abs(hi - lo)  # one subtraction, then |.|
            count[a, n] = np.sum(lo != hi, axis=0)
            for t in range(len(thr)):
                exceed[t, a, n] = np.sum(d > thr[t], axis=0)
            jump[a, n] = oracle_np.julia_mapreduce_arrays([d[m] for m in range(M)]) / np.float64(M)
        differs_any[:, n] |= lo != hi
    anyc = np.where(has.any(axis=0), differs_any.sum(axis=0), -1).astype(np.int64)
    return count, anyc, exceed, jump


def voxel(v, x):
    """The index along an axis with nodes v of the coordinates x: the midpoints that are <= x."""
    v = np.asarray(v, dtype=np.float64)
    mid = 0.5 * (v[:-1] + v[1:])
    return np.searchsorted(mid, x, side="right")


def density(models, xs, ys, zs):
    """(density [nq] int64, skipped)."""
    nx, ny, nz = len(xs), len(ys), len(zs)
    dens = np.zeros(nx * ny * nz, dtype=np.int64)
    skipped = 0
    for m in models:
        x, y, z = (np.asarray(c, dtype=np.float64) for c in m[:3])
        bad = np.isnan(x) | np.isnan(y) | np.isnan(z)
        skipped += int(bad.sum())
        ok = ~bad
        n = voxel(xs, x[ok]) + nx * (voxel(ys, y[ok]) + ny * voxel(zs, z[ok]))
        np.add.at(dens, n, 1)
    return dens, skipped


FIELDS = ("count", "any", "exceed", "jump", "mean", "std", "density", "skipped")


def interfaces(models, xs, ys, zs, thresholds=()):
    """-> dict(count, any, exceed (None without thresholds), jump, mean, std, density, skipped, values [M][nq])."""
    xs, ys, zs = (np.asarray(v, dtype=np.float64).ravel() for v in (xs, ys, zs))
    mean, std, V = oracle_np.rasterize(models, *lattice(xs, ys, zs))
    count, anyc, exceed, jump = face_statistics(V, len(xs), len(ys), len(zs), thresholds)
    dens, skipped = density(models, xs, ys, zs)
    return dict(count=count, any=anyc, exceed=exceed if len(np.ravel(thresholds)) else None, jump=jump, mean=mean, std=std,
                density=dens, skipped=skipped, values=V)


def contested(ref, M):
    """(faces, faces with 0 < count < M, faces with count == 0): a parity case must not pass for nothing."""
    c = ref["count"][ref["count"] >= 0]
    return len(c), int(np.sum((c > 0) & (c < M))), int(np.sum(c == 0))
