"""The ensemble Gram and distance matrices' definition (include/tdstar_gram.h), restated in numpy on
oracle_np.rasterize (the value matrix V[M][np]) and covariance_ref.column_stats (mean and sigma over the models):
    r[p]        = sqrt(w[p])                           (w None: 1.0)
    X[m][p]     = r[p] * (V[m][p] - mean[p])           (one subtraction, then one multiply)
    gram[a][b]  = sum_p X[a][p] * X[b][p]
    dist2[a][b] = sum_p e * e,  e = X[a][p] - X[b][p]
    W           = sum_p w[p] in td_rasterize's association (regions_ref.tree_sum)
Both sums: the points in order in blocks of 64; a block's sum runs left to right from its first term, the block sums
are added in block order to an accumulator that starts at +0.0.  The loops below run over the 64 points of a block
and over the blocks, on whole M x M arrays: numpy multiplies, subtracts and adds element by element under IEEE
rules, each operation rounded once."""
import numpy as np

import covariance_ref as cref
import regions_ref as rref
from oracle import oracle_np

BLOCK = 64


def centred(V, w=None):
    """(X [M][np], mean [np], std [np]) of the value matrix V[M][np]."""
    V = np.asarray(V, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean, std = cref.column_stats(V)
    r = np.ones(V.shape[1]) if w is None else np.sqrt(np.asarray(w, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        D = V - mean
        return r * D, mean, std


def blocked(X, block=BLOCK):
    """(gram, dist2) [M][M] of the centred matrix X[M][np] in the contract's association."""
    X = np.asarray(X, dtype=np.float64)
    M, n = X.shape
    G, D = np.zeros((M, M)), np.zeros((M, M))  # +0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for p0 in range(0, n, block):
            bg = bd = None
            for p in range(p0, min(p0 + block, n)):
                x = X[:, p]
                t = x[:, None] * x[None, :]
                e = x[:, None] - x[None, :]
                q = e * e
                bg = t if bg is None else bg + t
                bd = q if bd is None else bd + q
            G = G + bg
            D = D + bd
    return G, D


def gram(models, px, py, pz, w=None):
    """-> dict(gram, dist2 [M][M], mean, std [np], wsum, X [M][np], values [M][np])."""
    px, py, pz = (np.asarray(v, dtype=np.float64).ravel() for v in (px, py, pz))
    _, _, V = oracle_np.rasterize(models, px, py, pz)
    X, mean, std = centred(V, w)
    G, D = blocked(X)
    W = float(rref.tree_sum(np.ones(len(px)) if w is None else np.asarray(w, dtype=np.float64)))
    return dict(gram=G, dist2=D, mean=mean, std=std, wsum=W, X=X, values=V)


def same_bits(a, b):
    """Equal bit for bit, every NaN counting as one value (the payload of a NaN is not part of the contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.where(na, 0.0, a).view(np.int64), np.where(nb, 0.0, b).view(np.int64)))


BASE_POINTS = 1301  # 20 blocks of 64 and one of 21; slabs of 64 and of 128 cut it 21 and 11 times
BASE_SEED = 11


def make_models(rng, nmodels, lo=40, hi=300):
    """Models of lo .. hi cells uniform in +-100 x +-100 x [0, 200], zeta uniform in [0, 50]."""
    out = []
    for _ in range(nmodels):
        n = int(rng.integers(lo, hi + 1))
        out.append((rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(0, 200, n), rng.uniform(0, 50, n)))
    return out


def make_points(rng, n):
    return rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(0, 200, n), rng.uniform(0.5, 2.0, n)


def base_case(seed=BASE_SEED):
    """The inputs the association is tried on: default_rng(seed), 70 models of 40-300 cells, BASE_POINTS uniform
    points with weights uniform in [0.5, 2].  -> (models, px, py, pz, w).  tests/test_gram_host.py asserts that on
    this case the contract's order differs in bits from the two orders a kernel would most likely take instead."""
    rng = np.random.default_rng(seed)
    models = make_models(rng, 70)
    px, py, pz, w = make_points(rng, BASE_POINTS)
    return models, px, py, pz, w
