"""The posterior resolution's definition (include/tdstar_resolution.h), restated in numpy on oracle_np.rasterize (the
value matrix), covariance_ref.column_stats (a column's mean and sigma) and oracle_np.julia_mapreduce_arrays (the sum S).
On the lattice xs x ys x zs, node n = i + nx (j + ny k), with the forward offsets o = (di, dj, dk), f(o) = di + nx (dj +
ny dk), the pair (n, o) on the lattice when 0 <= i + di < nx, 0 <= j + dj < ny, k + dk < nz:
    cov[o][n]  = S / (M - 1),  S = mapreduce over m of (V[m][n] - m_n) * (V[m][n + f] - m_{n + f})
    corr[o][n] = cov / (s_n * s_{n + f})                                  (NaN off the lattice)
    pass(o, n) = on the lattice and corr[o][n] >= c                       (a NaN fails)
    footprint[n]: acc = w[n]; per offset in list order: + w[n + f] if pass(o, n), then + w[n - f] if pass(o, n - f)
    run[a][0][n]: the largest r with l e_a in the list and pass(l e_a, n) for l = 1 .. r; run[a][1][n]: backwards
    extent[a][n] = coord_a[idx + run_plus] - coord_a[idx - run_minus]
    censored[n]: bit 2a (+) / 2a + 1 (-): the run ended because (r + 1) e_a is not in the list or off the lattice
numpy subtracts, multiplies and compares element by element, each rounded once (no FMA), under IEEE rules."""
import numpy as np

import covariance_ref as cref
from oracle import oracle_np

FIELDS = ("cov", "corr", "footprint", "run", "extent", "censored", "mean", "std")


def lattice(xs, ys, zs):
    """The nodes' coordinates, x fastest."""
    xs, ys, zs = (np.asarray(v, dtype=np.float64) for v in (xs, ys, zs))
    return (np.tile(xs, len(ys) * len(zs)), np.tile(np.repeat(ys, len(xs)), len(zs)), np.repeat(zs, len(xs) * len(ys)))


def indices(nx, ny, nz):
    n = np.arange(nx * ny * nz)
    return n % nx, (n // nx) % ny, n // (nx * ny)


def on_lattice(nx, ny, nz, o):
    """(the mask of the nodes n whose pair (n, o) is on the lattice, f(o))"""
    i, j, k = indices(nx, ny, nz)
    di, dj, dk = (int(v) for v in o)
    on = (i + di >= 0) & (i + di < nx) & (j + dj >= 0) & (j + dj < ny) & (k + dk < nz)
    return on, di + nx * (dj + ny * dk)


def pair_moments(V, mean, std, nx, ny, nz, offsets):
    """(cov, corr) [noff][nq] of the value matrix V[M][nq]."""
    V = np.asarray(V, dtype=np.float64)
    M, nq = V.shape
    D = V - mean  # each factor: one subtraction
    cov = np.full((len(offsets), nq), np.nan)
    corr = np.full((len(offsets), nq), np.nan)
    for t, o in enumerate(offsets):
        on, f = on_lattice(nx, ny, nz, o)
        n = np.flatnonzero(on)
        if not len(n):
            continue
        S = oracle_np.julia_mapreduce_arrays([D[m, n] * D[m, n + f] for m in range(M)])
        with np.errstate(invalid="ignore", divide="ignore"):
            cov[t, n] = S / np.float64(M - 1)
            corr[t, n] = cov[t, n] / (std[n] * std[n + f])  # the product of the sigmas first
    return cov, corr


def summaries(corr, nx, ny, nz, offsets, threshold, weights):
    """(footprint [nq], run [3][2][nq] int32, censored [nq] int32)"""
    nq = nx * ny * nz
    w = np.ones(nq) if weights is None else np.asarray(weights, dtype=np.float64).ravel()
    c = np.float64(threshold)
    with np.errstate(invalid="ignore"):
        passes = [on_lattice(nx, ny, nz, o)[0] & (corr[t] >= c) for t, o in enumerate(offsets)]
    acc = w.copy()
    for t, o in enumerate(offsets):
        f = on_lattice(nx, ny, nz, o)[1]
        n = np.flatnonzero(passes[t])  # forwards: n takes its partner's weight
        acc[n] = acc[n] + w[n + f]
        acc[n + f] = acc[n + f] + w[n]  # then backwards: the partner takes n's (every node is the partner of one n at most)
    where = {tuple(int(v) for v in o): t for t, o in enumerate(offsets)}
    idx = indices(nx, ny, nz)
    stride, length = (1, nx, nx * ny), (nx, ny, nz)
    run = np.zeros((3, 2, nq), dtype=np.int32)
    cens = np.zeros(nq, dtype=np.int32)
    for a in range(3):
        for n in range(nq):
            for d in range(2):
                r = 0
                while True:
                    l = r + 1
                    t = where.get(tuple(l if b == a else 0 for b in range(3)))
                    at = n if d == 0 else n - l * stride[a]
                    inside = idx[a][n] + l < length[a] if d == 0 else idx[a][n] - l >= 0
                    if t is None or not inside:
                        cens[n] |= 1 << (2 * a + d)
                        break
                    if not passes[t][at]:
                        break
                    r = l
                run[a, d, n] = r
    return acc, run, cens


def extents(run, xs, ys, zs):
    nx, ny, nz = len(xs), len(ys), len(zs)
    idx = indices(nx, ny, nz)
    vec = [np.asarray(v, dtype=np.float64) for v in (xs, ys, zs)]
    return np.array([vec[a][idx[a] + run[a, 0]] - vec[a][idx[a] - run[a, 1]] for a in range(3)])


def resolution_of_values(V, xs, ys, zs, offsets, threshold=0.5, weights=None):
    """The definition on a given value matrix V[M][nq] -> dict of FIELDS."""
    xs, ys, zs = (np.asarray(v, dtype=np.float64).ravel() for v in (xs, ys, zs))
    offsets = np.asarray(offsets, dtype=np.int32).reshape(-1, 3)
    nx, ny, nz = len(xs), len(ys), len(zs)
    mean, std = cref.column_stats(V)
    cov, corr = pair_moments(V, mean, std, nx, ny, nz, offsets)
    foot, run, cens = summaries(corr, nx, ny, nz, offsets, threshold, weights)
    return dict(cov=cov, corr=corr, footprint=foot, run=run, extent=extents(run, xs, ys, zs), censored=cens, mean=mean, std=std)


def resolution(models, xs, ys, zs, offsets, threshold=0.5, weights=None):
    """-> dict of FIELDS and values [M][nq]."""
    xs, ys, zs = (np.asarray(v, dtype=np.float64).ravel() for v in (xs, ys, zs))
    V = oracle_np.rasterize(models, *lattice(xs, ys, zs))[2]
    return dict(resolution_of_values(V, xs, ys, zs, offsets, threshold, weights), values=V)


def vacuity(ref, offsets, nx, ny, nz):
    """(the share of the pairs on the lattice with corr >= 0.5, the x runs -- both directions -- ended by a failing
    correlation, the x runs censored): a parity case must not pass for nothing."""
    on = np.array([on_lattice(nx, ny, nz, o)[0] for o in offsets])
    with np.errstate(invalid="ignore"):
        share = float(np.mean(ref["corr"][on] >= 0.5))
    cx = np.array([(ref["censored"] >> b) & 1 for b in (0, 1)])
    return share, int(np.sum(cx == 0)), int(np.sum(cx == 1))
