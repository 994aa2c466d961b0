"""The posterior recovery's definition (include/tdstar_recovery.h), restated in numpy on oracle_np.rasterize (the value
matrix V[M][np]) and regions_ref (the tree sums and the statistics of a matrix's columns).  Region r is the points
reg_off[r] .. reg_off[r + 1] - 1:
    D[m][p]     = V[m][p] - truth[p]
    below[p]    = #{m : V[m][p] <  truth[p]},  equal: ==,  above: >       (IEEE: a NaN V counts in none)
    dmean, dstd = oracle_np.rasterize's own statistics, of the columns of D
    u = D * D;  t = w[p] * u                                                (two multiplies; w None: 1.0)
    S[m][r]     = mapreduce over the region's points, in index order, of t[m][p]
    W[r]        = mapreduce over the region's points of w[p]
    F[m][r]     = S[m][r] / W[r] if normalize else S[m][r]
    mean, std   = the same statistics, of the columns of F
numpy subtracts, multiplies, divides and compares element by element under IEEE rules."""
import numpy as np

import regions_ref as rref
from oracle import oracle_np

FIELDS = ("below", "equal", "above", "dmean", "dstd", "series", "weight", "mean", "std")


def terms(V, truth, w=None):
    """t[M][np] of the value matrix V."""
    V = np.asarray(V, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        D = V - np.asarray(truth, dtype=np.float64)[None, :]
        u = D * D
        return u * 1.0 if w is None else np.asarray(w, dtype=np.float64)[None, :] * u


def from_values(V, truth, reg_off, w=None, normalize=True):
    """The outputs of the value matrix V[M][np]."""
    V = np.asarray(V, dtype=np.float64)
    truth = np.asarray(truth, dtype=np.float64).ravel()
    reg_off = np.asarray(reg_off, dtype=np.int64)
    R = len(reg_off) - 1
    wv = np.ones(V.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        D = V - truth[None, :]
        below = np.sum(V < truth[None, :], axis=0).astype(np.int64)
        equal = np.sum(V == truth[None, :], axis=0).astype(np.int64)
        above = np.sum(V > truth[None, :], axis=0).astype(np.int64)
        dmean, dstd = rref.statistics(D)
        t = terms(V, truth, wv)
        F = np.empty((len(V), R))
        W = np.empty(R)
        for r in range(R):
            lo, hi = int(reg_off[r]), int(reg_off[r + 1])
            S = rref.tree_sum(t[:, lo:hi])
            W[r] = rref.tree_sum(wv[lo:hi])
            F[:, r] = S / W[r] if normalize else S
        mean, std = rref.statistics(F)
    return dict(below=below, equal=equal, above=above, dmean=dmean, dstd=dstd, series=F, weight=W, mean=mean, std=std,
                values=V)


def recovery(models, px, py, pz, truth, reg_off=None, w=None, normalize=True):
    """-> dict(below, equal, above [np] int64, dmean, dstd [np], series [M][R], weight [R], mean, std [R], values
    [M][np])."""
    px, py, pz = (np.asarray(v, dtype=np.float64).ravel() for v in (px, py, pz))
    _, _, V = oracle_np.rasterize(models, px, py, pz)
    if reg_off is None:
        reg_off = [0, len(px)]
    return from_values(V, truth, reg_off, w, normalize)


BASE_SIZES = (1, 15, 16, 17, 1024, 1025, 2049, 3000)
BASE_FAR = (16, 33, 34) + tuple(range(7127, 7147))  # beyond the sentinel: in the regions of 16, 17 and 3000 points
BASE_BLOCKS, BASE_LO, BASE_HI = (3, 2, 4), 5.0, 15.0


def base_case(checkerboard_model):
    """The inputs the association was tried on: default_rng(11), 65 models of 5-40 cells uniform in +-100 x +-100 x
    [0, 200] with zeta uniform in [0, 50], 7147 points with weights uniform in [0.5, 2], regions of BASE_SIZES points.
    The points BASE_FAR lie 4e5 away, beyond the 1e9 sentinel of every cell (V = 0.0 for every model).  Two truths:
    "model" is model (p mod 65)'s own value at point p, so equal >= 1 everywhere; "board" is a checkerboard of
    BASE_BLOCKS blocks over the box (``checkerboard_model``: the package's) at the point.  At the far points both
    truths alternate between -0.0 and 0.0.  -> (models, px, py, pz, w, reg_off, {"model": truth, "board": truth}, the
    checkerboard Model)."""
    rng = np.random.default_rng(11)
    models = []
    for _ in range(65):
        n = int(rng.integers(5, 41))
        models.append((rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(0, 200, n), rng.uniform(0, 50, n)))
    npts = sum(BASE_SIZES)
    px, py, pz = rng.uniform(-100, 100, npts), rng.uniform(-100, 100, npts), rng.uniform(0, 200, npts)
    far = np.array(BASE_FAR)
    px[far] = 4e5 + px[far]
    w = rng.uniform(0.5, 2.0, npts)
    _, _, V = oracle_np.rasterize(models, px, py, pz)
    board = checkerboard_model([-100.0, 100.0], [-100.0, 100.0], [0.0, 200.0], BASE_BLOCKS, BASE_LO, BASE_HI)
    _, _, B = oracle_np.rasterize([board.cells()], px, py, pz)
    truths = {"model": V[np.arange(npts) % 65, np.arange(npts)].copy(), "board": B[0].copy()}
    for t in truths.values():
        t[far] = np.where(np.arange(len(far)) % 2 == 0, -0.0, 0.0)
    return models, px, py, pz, w, np.concatenate(([0], np.cumsum(BASE_SIZES))).astype(np.int64), truths, board
