"""The posterior comparison's definition (include/tdstar_compare.h), restated twice in numpy on two value matrices A
[MA, ncol] and B [MB, ncol] -- ``brute`` over all pairs and over every pooled value, ``by_sorting`` with np.sort and
np.searchsorted for the sizes the first cannot reach -- and the inputs the tests of both share.  The two share no step
beyond the IEEE comparisons themselves.  Needs no GPU and no library."""
import functools

import numpy as np

FIELDS = ("less", "equal", "greater", "exceed", "ks_plus", "ks_minus", "ks_at")
EXCEED = ((1.0, 0.0), (2.0, 0.0), (0.5, -1.25), (1.0, 1e300))
# (MA, MB, ncol): one model a side, non-powers of two, the wave and tile edges, the 1024 and 4096 edges
SHAPES = ((1, 1, 1), (1, 5, 3), (2, 3, 64), (63, 65, 65), (64, 64, 130), (257, 1000, 7), (1025, 130, 66), (4097, 33, 5))
KINDS = ("ties", "distinct", "hostile", "identical", "disjoint")
QNAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]


def _two(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    A = A.reshape(-1, 1) if A.ndim == 1 else A
    B = B.reshape(-1, 1) if B.ndim == 1 else B
    assert A.ndim == 2 and B.ndim == 2 and A.shape[1] == B.shape[1]
    return A, B


def _empty(ncol, ne):
    out = {f: np.zeros(ncol, dtype=np.int64) for f in FIELDS if f not in ("exceed", "ks_at")}
    out["exceed"] = np.zeros((ne, ncol), dtype=np.int64) if ne else None
    out["ks_at"] = np.full(ncol, QNAN)
    return out


def brute(A, B, exceed=EXCEED):
    """Every pair, and T at every pooled value by counting."""
    A, B = _two(A, B)
    (MA, ncol), MB = A.shape, B.shape[0]
    out = _empty(ncol, len(exceed))
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(ncol):
            a, b = A[:, q], B[:, q]
            out["less"][q] = np.count_nonzero(a[:, None] < b[None, :])
            out["equal"][q] = np.count_nonzero(a[:, None] == b[None, :])
            out["greater"][q] = np.count_nonzero(a[:, None] > b[None, :])
            for k, (s, t) in enumerate(exceed):
                f = np.float64(s) * b
                f = f + np.float64(t)
                out["exceed"][k, q] = np.count_nonzero(a[:, None] > f[None, :])
            plus = minus = best = 0
            at = QNAN
            for x in np.concatenate((a, b)):
                if x != x:
                    continue
                T = int(np.count_nonzero(a <= x)) * MB - int(np.count_nonzero(b <= x)) * MA
                plus, minus = max(plus, T), max(minus, -T)
                if abs(T) > best or (abs(T) == best and best > 0 and x < at):
                    best, at = abs(T), x
            out["ks_plus"][q], out["ks_minus"][q] = plus, minus
            out["ks_at"][q] = (at + 0.0 if at == 0 else at) if best > 0 else QNAN  # (a zero is reported as +0.0)
    return out


def by_sorting(A, B, exceed=EXCEED):
    """Sorted columns and ranks."""
    A, B = _two(A, B)
    (MA, ncol), MB = A.shape, B.shape[0]
    out = _empty(ncol, len(exceed))
    for q in range(ncol):
        a, b = (np.sort(np.where(v == 0, 0.0, v)[~np.isnan(v)]) for v in (A[:, q], B[:, q]))
        lo, hi = np.searchsorted(b, a, "left"), np.searchsorted(b, a, "right")
        out["greater"][q], out["equal"][q], out["less"][q] = lo.sum(), (hi - lo).sum(), (len(b) - hi).sum()
        with np.errstate(over="ignore"):
            for k, (s, t) in enumerate(exceed):
                f = np.float64(s) * b
                f = f + np.float64(t)
                assert np.all(f[1:] >= f[:-1])
                out["exceed"][k, q] = np.searchsorted(f, a, "left").sum()
        X = np.unique(np.concatenate((a, b)))
        if len(X) == 0:
            continue
        T = np.searchsorted(a, X, "right").astype(np.int64) * MB - np.searchsorted(b, X, "right").astype(np.int64) * MA
        out["ks_plus"][q], out["ks_minus"][q] = max(0, T.max()), max(0, (-T).max())
        best = max(out["ks_plus"][q], out["ks_minus"][q])
        if best > 0:
            out["ks_at"][q] = X[np.flatnonzero(np.abs(T) == best)[0]]
    return out


def swapped(r):
    """What compare(B, A) must give where compare(A, B) gave ``r`` (the exceed rows have no counterpart)."""
    return dict(less=r["greater"], equal=r["equal"], greater=r["less"], ks_plus=r["ks_minus"], ks_minus=r["ks_plus"],
                ks_at=r["ks_at"])


def same(a, b):
    """Exact equality: integers as integers, doubles bit for bit with every NaN equal to the quiet NaN."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def differences(got, want, fields=FIELDS):
    return [f for f in fields if not same(got[f], want[f])]


HOSTILE = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, -1.0, 1e300, -1e300,
                    0.5, 2.0, 1e-300])


@functools.lru_cache(maxsize=None)
def inputs(kind, MA, MB, ncol):
    """(A [MA, ncol], B [MB, ncol]) of one kind.  ``identical`` makes B a row permutation of A, so it has MA rows."""
    rng = np.random.default_rng([KINDS.index(kind), MA, MB, ncol])
    if kind == "ties":  # quarters, B a quarter higher: every value of B but the top one is a value of A
        A, B = rng.integers(0, 8, (MA, ncol)) / 4.0, rng.integers(0, 8, (MB, ncol)) / 4.0 + 0.25
        B[0] = A[0]  # (a tie in every column, whatever the size)
    elif kind == "distinct":
        A, B = rng.standard_normal((MA, ncol)), rng.standard_normal((MB, ncol)) + 0.3
    elif kind == "identical":
        A = np.round(rng.standard_normal((MA, ncol)), 1)
        B = A[rng.permutation(MA)]
    elif kind == "disjoint":
        A, B = rng.standard_normal((MA, ncol)), np.abs(rng.standard_normal((MB, ncol))) + 100.0
    else:  # hostile; by column: 0 a mixture, 1 NaNs in A only, 2 NaNs only, 3 NaNs in B only and all of B
        A, B = HOSTILE[rng.integers(0, len(HOSTILE), (MA, ncol))], HOSTILE[rng.integers(0, len(HOSTILE), (MB, ncol))]
        numbers = HOSTILE[1:]
        for q in range(ncol):
            if q % 4 == 1:
                B[:, q] = numbers[rng.integers(0, len(numbers), MB)]
                A[0, q] = np.nan
            elif q % 4 == 2:
                A[:, q] = B[:, q] = np.nan
            elif q % 4 == 3:
                A[:, q] = numbers[rng.integers(0, len(numbers), MA)]
                B[:, q] = np.nan
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def reference(kind, MA, MB, ncol):
    """``brute`` on ``inputs``; made once per process and not to be written to."""
    A, B = inputs(kind, MA, MB, ncol)
    r = brute(A, B)
    for v in r.values():
        v.setflags(write=False)
    return r
