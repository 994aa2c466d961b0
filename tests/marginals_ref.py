"""The posterior marginals restated in numpy (no GPU): the reference of test_gpu_marginals.py and
test_gpu_marginals_values.py, itself held to scalar Python in test_marginals_host.py.

Quantiles: Statistics.quantile(v, p) with alpha = beta = 1 as include/tdstar.h writes it out -- the column
sorted in the total order of Julia's isless (-0.0 before 0.0), the two order statistics a and b and the weight
g of ``rank``, then a + g * (b - a), unfused.  Where the order statistics are not finite this is the
build's stated definition, evaluated as written: equal infinities give NaN (inf - inf), -DBL_MAX .. DBL_MAX
overflows (b - a = inf), a column that holds a NaN gives NaN at every probability.  It is not a claim about
what any Julia version returns for such columns.

The sort is on the pair (value, not signbit): a comparison of numbers, not the kernels' 64-bit keys.

Histogram slots: the four lines of the header, 0 below lo, 1 + min(floor((v - lo) / w), nbins - 1) in range,
nbins + 1 at or above hi, nbins + 2 NaN."""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)

# the double range end to end; NaN is not among them: a test places it in the columns it designates
SPECIAL = (-np.inf, -DBL_MAX, -1e300, -1.0, -DBL_MIN, -5e-324, -0.0, 0.0, 5e-324, 1e-310, DBL_MIN, 1.0,
           float(np.nextafter(1.0, 2.0)), 1e300, DBL_MAX, np.inf)


def rank(M, p):
    """Statistics.quantile's position, alpha = beta = 1: (1-based j, weight g of v[j+1])."""
    aleph = M * p + (1 - p)
    j = min(max(int(np.trunc(aleph)), 1), max(M - 1, 1))
    g = min(max(aleph - j, 0.0), 1.0)
    return j, g


def sort_columns(V):
    """Every column ascending, -0.0 before 0.0 (NaN anywhere after the numbers)."""
    V = np.asarray(V, dtype=np.float64)
    Vt = np.ascontiguousarray(V.T)
    order = np.lexsort((~np.signbit(Vt), Vt), axis=-1)  # (the last key is the primary one)
    return np.ascontiguousarray(np.take_along_axis(Vt, order, axis=-1).T)


def ref_quantiles(V, probs):
    V = np.asarray(V, dtype=np.float64)
    M = len(V)
    S = sort_columns(V)
    out = np.empty((len(probs), V.shape[1]))
    for i, p in enumerate(probs):
        j, g = rank(M, p)
        a = S[j - 1]
        b = S[0] if M == 1 else S[j]
        with np.errstate(all="ignore"):
            out[i] = a + g * (b - a)
    out[:, np.isnan(V).any(axis=0)] = np.nan
    return out


def ref_slots(v, bins):
    nbins, lo, hi = bins
    w = (hi - lo) / nbins
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        b = np.floor((v - lo) / w)
        s = 1 + np.minimum(np.where(np.isnan(b), 0, b), nbins - 1).astype(np.int64)
        s[v < lo] = 0
        s[v >= hi] = nbins + 1
    s[np.isnan(v)] = nbins + 2
    return s


def ref_hist(V, bins):
    s = ref_slots(V, bins)
    nslots = bins[0] + 3
    flat = np.bincount((s + nslots * np.arange(s.shape[1])).ravel(), minlength=nslots * s.shape[1])
    return flat.reshape(s.shape[1], nslots).astype(np.int64)


def designed_models(V, sites):
    """Models whose value matrix at ``sites`` is V [M][nq], bits and all: model k is the nq cells at
    ``sites`` = (x, y, z), distinct and at least 1 apart, with zeta = V[k], so every node's nearest cell
    is the one at distance 0, without a tie."""
    V = np.asarray(V, dtype=np.float64)
    x, y, z = (np.ascontiguousarray(a, dtype=np.float64) for a in sites)
    assert V.ndim == 2 and len(x) == len(y) == len(z) == V.shape[1]
    P = np.stack([x, y, z], axis=1)
    d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    assert np.all(d2[~np.eye(len(x), dtype=bool)] >= 1.0), "sites must be at least 1 apart"
    return [(x, y, z, np.array(row)) for row in V]


def same_bits(a, b):
    """a and b have NaN in the same places and the same 64 bits everywhere else (the sign of a zero counts)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))
