"""The posterior regions' definition (include/tdstar_regions.h), restated in numpy on oracle_np.rasterize (the value
matrix V[M][np], and the mean and sigma of the series) and oracle_np.julia_mapreduce_arrays (both sums).  Region r is
the points reg_off[r] .. reg_off[r + 1] - 1:
    t[m][p]       = w[p] * V[m][p]                     (one multiply; w None: 1.0)
    S[m][r]       = mapreduce over the region's points, in index order, of t[m][p]
    W[r]          = mapreduce over the region's points of w[p]
    F[m][r]       = S[m][r] / W[r] if normalize else S[m][r]
    greater[a][b] = #{m : F[m][a] > F[m][b]}
    mean, std     = oracle_np.rasterize's own statistics, of the columns of F
numpy multiplies, divides and compares element by element under IEEE rules (NaN > x is false)."""
import numpy as np

from oracle import oracle_np


def tree_sum(T):
    """The sum along the last axis of T[..., n] in td_rasterize's association over the index."""
    T = np.asarray(T, dtype=np.float64)
    return oracle_np.julia_mapreduce_arrays([T[..., k] for k in range(T.shape[-1])])


def statistics(F):
    """(mean, std) of the columns of F[M][R] as oracle_np.rasterize forms them."""
    F = np.asarray(F, dtype=np.float64)
    n = len(F)
    rows = [F[m] for m in range(n)]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = oracle_np.julia_mapreduce_arrays(rows) / float(n)
        dev = [(v - mean) * (v - mean) for v in rows]
        std = np.sqrt(oracle_np.julia_mapreduce_arrays(dev) / float(n - 1))
    return mean, std


def series(V, reg_off, w=None, normalize=True):
    """(F [M][R], W [R]) of the value matrix V[M][np]."""
    V = np.asarray(V, dtype=np.float64)
    reg_off = np.asarray(reg_off, dtype=np.int64)
    R = len(reg_off) - 1
    wv = np.ones(V.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    F = np.empty((len(V), R))
    W = np.empty(R)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for r in range(R):
            lo, hi = int(reg_off[r]), int(reg_off[r + 1])
            S = tree_sum(wv[lo:hi] * V[:, lo:hi])
            W[r] = tree_sum(wv[lo:hi])
            F[:, r] = S / W[r] if normalize else S
    return F, W


def greater(F):
    """greater[a][b] = #{m : F[m][a] > F[m][b]} (int64)."""
    F = np.asarray(F, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.sum(F[:, :, None] > F[:, None, :], axis=0).astype(np.int64)


def regions(models, px, py, pz, reg_off, w=None, normalize=True):
    """-> dict(series [M][R], weight [R], mean, std [R], greater [R][R], values [M][np])."""
    px, py, pz = (np.asarray(v, dtype=np.float64).ravel() for v in (px, py, pz))
    _, _, V = oracle_np.rasterize(models, px, py, pz)
    F, W = series(V, reg_off, w, normalize)
    mean, std = statistics(F)
    return dict(series=F, weight=W, mean=mean, std=std, greater=greater(F), values=V)


BASE_SIZES = (1, 2, 15, 16, 63, 64, 65, 1023, 1024, 1025, 2049, 3000)


def base_case():
    """The inputs the association was tried on: default_rng(7), 65 models of 5-40 cells uniform in +-100 x +-100 x
    [0, 200] with zeta uniform in [0, 50], 8347 uniform points with weights uniform in [0.5, 2], regions of
    BASE_SIZES points.  -> (models, px, py, pz, w, reg_off)."""
    rng = np.random.default_rng(7)
    models = []
    for _ in range(65):
        n = int(rng.integers(5, 41))
        models.append((rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(0, 200, n), rng.uniform(0, 50, n)))
    npts = sum(BASE_SIZES)
    px, py, pz = rng.uniform(-100, 100, npts), rng.uniform(-100, 100, npts), rng.uniform(0, 200, npts)
    w = rng.uniform(0.5, 2.0, npts)
    return models, px, py, pz, w, np.concatenate(([0], np.cumsum(BASE_SIZES))).astype(np.int64)
