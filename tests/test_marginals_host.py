"""CPU: the host side of the posterior marginals (td_rasterize_marginals): Julia's quantile position
for (M, p), restated, the argument checks made before any HIP call, the quantile kernels' launch plan
(tdt_marginals_plan) against the rule restated, and the numpy reference of the GPU tests
(marginals_ref.py) against scalar Python."""
import ctypes
import functools
import math

import numpy as np
import pytest

import marginals_ref as mref
from oracle import oracle_np

MS = (1, 2, 3, 15, 16, 100, 101, 1100)
PROBS = (0.0, 0.025, 0.05, 1 / 3, 0.5, 0.95, 1.0)


def rank(M, p):
    """Statistics.quantile's position, alpha = beta = 1: (1-based j, weight g of v[j+1])."""
    aleph = M * p + (1 - p)
    j = min(max(int(math.trunc(aleph)), 1), max(M - 1, 1))
    g = min(max(aleph - j, 0.0), 1.0)
    return j, g


def quantile_sorted(v, p):
    M = len(v)
    j, g = rank(M, p)
    a = v[j - 1]
    b = v[0] if M == 1 else v[j]
    return a + g * (b - a)


@pytest.mark.parametrize("M", MS)
def test_quantile_rank_is_the_restated_formula(tt, M):
    L = tt.lib()
    for p in PROBS:
        j, g = ctypes.c_int64(), ctypes.c_double()
        assert L.tdt_quantile_rank(M, p, ctypes.byref(j), ctypes.byref(g)) == 0
        assert (j.value, g.value) == rank(M, p), (M, p)
        assert 1 <= j.value <= max(M - 1, 1) and 0.0 <= g.value <= 1.0
    j, g = ctypes.c_int64(), ctypes.c_double()
    for bad in (-0.1, 1.5, float("nan")):
        assert L.tdt_quantile_rank(M, bad, ctypes.byref(j), ctypes.byref(g)) == 1
    assert L.tdt_quantile_rank(0, 0.5, ctypes.byref(j), ctypes.byref(g)) == 1


def test_formula_agrees_with_numpy_quantile():
    """np.quantile (linear) is the same definition in another rounding: 1e-12 relative."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for M in MS:
        v = np.sort(rng.uniform(0, 50, M))
        for p in PROBS:
            got, ref = quantile_sorted(v, p), float(np.quantile(v, p))
            worst = max(worst, abs(got - ref) / max(abs(ref), 1e-300))
    assert worst <= 1e-12, worst


def want_of(tt, nprob=0, probs=None, quant=True, nbins=0, lo=0.0, hi=0.0, hist=True, nq=4):
    _lib = __import__("importlib").import_module("mcmc_in_tonga_amd._lib")
    keep = []
    p = np.ascontiguousarray(probs if probs is not None else np.full(max(nprob, 1), 0.5), dtype=np.float64)
    q = np.zeros((max(nprob, 1), nq))
    h = np.zeros((nq, max(nbins, 0) + 3), dtype=np.int64)
    keep += [p, q, h]
    w = _lib.TdMarginals(nprob, _lib.ptr(p) if probs is not False else None, _lib.ptr(q) if quant else None, nbins,
                         lo, hi, _lib.ptr(h) if hist else None)
    return w, keep


BAD_WANTS = {
    "prob below 0": dict(nprob=2, probs=[0.5, -1e-9]),
    "prob above 1": dict(nprob=1, probs=[1.0000001]),
    "prob NaN": dict(nprob=3, probs=[0.1, float("nan"), 0.9]),
    "nprob > 64": dict(nprob=65, probs=np.linspace(0, 1, 65)),
    "nprob < 0": dict(nprob=-1),
    "nbins > 4096": dict(nbins=4097, lo=0.0, hi=1.0),
    "nbins < 0": dict(nbins=-1, lo=0.0, hi=1.0),
    "lo == hi": dict(nbins=10, lo=1.0, hi=1.0),
    "lo > hi": dict(nbins=10, lo=2.0, hi=1.0),
    "lo NaN": dict(nbins=10, lo=float("nan"), hi=1.0),
    "hi inf": dict(nbins=10, lo=0.0, hi=float("inf")),
    "lo -inf": dict(nbins=10, lo=float("-inf"), hi=0.0),
    "hi - lo overflows": dict(nbins=3, lo=-1e308, hi=1e308),
    "probs NULL": dict(nprob=2, probs=False),
    "quant_out NULL": dict(nprob=2, probs=[0.1, 0.9], quant=False),
    "hist_out NULL": dict(nbins=10, lo=0.0, hi=1.0, hist=False),
}


BINS_REFUSED = ("lo == hi", "lo > hi", "lo NaN", "hi inf", "lo -inf", "hi - lo overflows")


@pytest.mark.parametrize("case", sorted(BAD_WANTS))
def test_argument_errors_before_any_hip_call(tt, case):
    """No context is needed (none can be made without a GPU): the request is checked first, and the
    message goes to td_last_error(NULL)."""
    L = tt.lib()
    w, keep = want_of(tt, **BAD_WANTS[case])
    off = np.array([0, 1], dtype=np.int64)
    c = np.zeros(1)
    q = np.zeros(4)
    out = np.zeros(4)
    ptr = __import__("importlib").import_module("mcmc_in_tonga_amd._lib").ptr
    rc = L.td_rasterize_marginals(None, 1, ptr(off), ptr(c), ptr(c), ptr(c), ptr(c), ptr(q), ptr(q), ptr(q), 4,
                                  ptr(out), ptr(out), ctypes.byref(w))
    assert rc == 1, case
    msg = L.td_last_error(None)
    assert msg and b"td_rasterize_marginals" in msg
    if case in BINS_REFUSED:
        assert msg == b"td_rasterize_marginals: need finite lo < hi"
    rc = L.td_history_marginals(None, None, 0, ptr(q), ptr(q), ptr(q), 4, ptr(out), ptr(out), ctypes.byref(w))
    assert rc == 1, case
    msg = L.td_last_error(None)
    assert msg and b"td_history_marginals" in msg
    del keep


def test_null_want_null_context_and_hooks(tt):
    L = tt.lib()
    q = np.zeros(4)
    ptr = __import__("importlib").import_module("mcmc_in_tonga_amd._lib").ptr
    assert L.td_rasterize_marginals(None, 1, None, None, None, None, None, ptr(q), ptr(q), ptr(q), 4, ptr(q), ptr(q),
                                    None) == 1
    assert b"want is NULL" in L.td_last_error(None)
    assert L.td_history_marginals(None, None, 0, ptr(q), ptr(q), ptr(q), 4, ptr(q), ptr(q), None) == 1
    assert b"want is NULL" in L.td_last_error(None)
    # a legal request (mean and std only) gets as far as the context check
    w, keep = want_of(tt)
    assert L.td_rasterize_marginals(None, 1, None, None, None, None, None, ptr(q), ptr(q), ptr(q), 4, ptr(q), ptr(q),
                                    ctypes.byref(w)) == 1
    assert b"ctx is NULL" in L.td_last_error(None)
    assert L.td_history_marginals(None, None, 0, ptr(q), ptr(q), ptr(q), 4, ptr(q), ptr(q), ctypes.byref(w)) == 1
    assert L.td_last_error(None)
    h = np.zeros(13, dtype=np.int64)
    for nbins, lo, hi in ((0, 0.0, 1.0), (4097, 0.0, 1.0), (10, 1.0, 1.0), (10, float("nan"), 1.0), (10, 0.0, 1.0)):
        assert L.td_history_zeta_hist(None, None, 0, nbins, lo, hi, ptr(h), None) == 1  # (the last: no context)
        assert L.td_last_error(None)
    # hi - lo overflows: w = (hi - lo) / nbins would be +inf; bins as wide as the check lets through pass it
    assert L.td_history_zeta_hist(None, None, 0, 3, -1e308, 1e308, ptr(h), None) == 1
    assert L.td_last_error(None) == b"td_history_zeta_hist: need finite lo < hi"
    assert L.td_history_zeta_hist(None, None, 0, 3, -8e307, 8e307, ptr(h), None) == 1
    assert L.td_last_error(None) == b"td_history_zeta_hist: ctx is NULL"
    m = ctypes.c_int64()
    assert L.tdt_set_marginals_method(None, 1) == 1
    assert L.tdt_marginals_resident_max(None, ctypes.byref(m)) == 1


# ---- the launch plan of the quantile kernels --------------------------------------------------------------

RESIDENT_MAX = 16384  # tdt_marginals_resident_max: the keys the LDS holds
LDS_BUDGET = 160 * 1024  # a CDNA4 workgroup's LDS
STATIC_LDS = {True: 64 * 4,  # k_node_quantiles_resident: has_nan[64]
              False: 128 * 8 + 128 * 4 + 4}  # k_node_quantiles_stream: prefix[128], rem[128], nan_count


def plan_restated(M, nq, num_cus, method, nprob):
    """(resident, Mp, W, threads, dynamic LDS bytes), or None where the call refuses."""
    resident = method == 1 or (method == 0 and M <= RESIDENT_MAX)
    if not resident:
        return (False, 0, 1, 512, 2 * nprob * 1024)
    if M > RESIDENT_MAX:
        return None
    Mp = 1
    while Mp < M:
        Mp *= 2
    W = min(64, RESIDENT_MAX // Mp)
    while W > 8 and -(-nq // W) < 2 * num_cus:
        W //= 2
    threads = 64
    while threads < Mp // 2 * W and threads < 1024:
        threads *= 2
    return (True, Mp, W, threads, 8 * Mp * W)


PLAN_MS = sorted({m for e in range(15) for m in ((1 << e) - 1, 1 << e, (1 << e) + 1) if m >= 1})
PLAN_NQS = (1, 7, 8, 9, 4095, 8176, 8177, 16353, 32704, 32705, 70000)


def test_plan_ms_reach_the_limit():
    assert PLAN_MS[0] == 1 and PLAN_MS[-3:] == [16383, 16384, 16385]


@pytest.mark.parametrize("num_cus", [1, 64, 256, 304])
def test_marginals_plan_is_the_restated_rule(tt, num_cus):
    widths = set()
    for M in PLAN_MS:
        for nq in PLAN_NQS:
            for method in (0, 1, 2):
                for nprob in (1, 7, 23, 24, 64):
                    want = plan_restated(M, nq, num_cus, method, nprob)
                    if want is None:
                        with pytest.raises(tt.TdError):
                            tt.TdContext.marginals_plan(M, nq, num_cus, method, nprob)
                        continue
                    got = tt.TdContext.marginals_plan(M, nq, num_cus, method, nprob)
                    assert got == want, (M, nq, num_cus, method, nprob)
                    resident, Mp, W, threads, lds = got
                    assert Mp * W <= RESIDENT_MAX and 1 <= W <= 64 and W & (W - 1) == 0
                    assert resident == (Mp >= M and Mp > 0) and (not resident or Mp < 2 * M)
                    assert threads in (64, 128, 256, 512, 1024)
                    assert lds <= LDS_BUDGET - STATIC_LDS[resident]
                    if resident:
                        widths.add(W)
    assert widths == {1, 2, 4, 8, 16, 32, 64}  # (the sweep reaches every tile width)


def test_marginals_plan_widths_at_256_cus(tt):
    """The node counts from which a 256-CU device keeps the wider tiles (M = 200: Mp = 256, 64 fit)."""
    W = lambda nq: tt.TdContext.marginals_plan(200, nq, 256)[2]
    assert [W(nq) for nq in (8176, 8177, 16352, 16353, 32704, 32705)] == [8, 16, 16, 32, 32, 64]
    assert tt.TdContext.marginals_plan(200, 70000, 1)[2] == 64 and tt.TdContext.marginals_plan(200, 1, 1)[2] == 8


def test_marginals_plan_refuses(tt):
    L = tt.lib()
    out = np.zeros(5, dtype=np.int64)
    p = __import__("importlib").import_module("mcmc_in_tonga_amd._lib").ptr(out, ctypes.POINTER(ctypes.c_int64))
    assert L.tdt_marginals_plan(100, 10, 256, 0, 7, p) == 0
    for M, nq, cus, method, nprob in ((0, 10, 256, 0, 7), (100, 0, 256, 0, 7), (100, 10, -1, 0, 7), (100, 10, 256, 3, 7),
                                      (100, 10, 256, -1, 7), (100, 10, 256, 0, -1), (100, 10, 256, 0, 65),
                                      (RESIDENT_MAX + 1, 10, 256, 1, 7)):
        assert L.tdt_marginals_plan(M, nq, cus, method, nprob, p) == 1, (M, nq, cus, method, nprob)
    assert L.tdt_marginals_plan(100, 10, 256, 0, 7, None) == 1


# ---- marginals_ref against scalar Python ---------------------------------------------------------------


def isless(a, b):
    """Julia's isless on floats: numbers ascending, -0.0 before 0.0, NaN after everything."""
    if math.isnan(a) or math.isnan(b):
        return not math.isnan(a) and math.isnan(b)
    if a == b:
        return math.copysign(1.0, a) < math.copysign(1.0, b)
    return a < b


def by_isless(a, b):
    return -1 if isless(a, b) else (1 if isless(b, a) else 0)


def scalar_quantile(col, p):
    """One column, one probability, in Python floats: the header's lines."""
    v = sorted((float(x) for x in col), key=functools.cmp_to_key(by_isless))
    if any(math.isnan(x) for x in v):
        return math.nan
    M = len(v)
    j, g = rank(M, p)
    a = v[j - 1]
    b = v[0] if M == 1 else v[j]
    d = b - a  # (Python floats: inf - inf is NaN, an overflow is inf, neither raises)
    return a + g * d


def scalar_slot(v, nbins, lo, hi):
    """The header's four lines."""
    w = (hi - lo) / nbins
    if math.isnan(v):
        return nbins + 2
    if v < lo:
        return 0
    if v >= hi:
        return nbins + 1
    return 1 + min(int(math.floor((v - lo) / w)), nbins - 1)


def ref_columns():
    """{name: column}: what the sort and the formula can get wrong."""
    inf, nan = math.inf, math.nan
    rng = np.random.default_rng(5)
    cols = {
        "M = 1": [3.5], "M = 1, -0.0": [-0.0], "M = 1, inf": [inf], "M = 1, NaN": [nan],
        "M = 2": [2.0, -7.0], "M = 2, zeros": [0.0, -0.0], "M = 2, infinities": [inf, -inf],
        "M = 2, equal infinities": [-inf, -inf], "M = 2, NaN": [nan, 1.0],
        "M = 3": [1.0, -1.0, 0.5], "M = 3, zeros": [0.0, -0.0, 0.0], "M = 3, NaN": [1.0, nan, -0.0],
        "zeros, + first": [0.0, -0.0] * 6, "zeros, - first": [-0.0, 0.0] * 6 + [-0.0],
        "zeros among numbers": [1.0, 0.0, -1.0, -0.0, 0.0, -0.0, 5e-324, -5e-324, -0.0],
        "all -0.0": [-0.0] * 7, "all 0.0": [0.0] * 7,
        "equal infinities": [inf] * 9, "equal -infinities": [-inf] * 8,
        "infinities both ends": [inf, -inf, 1.0, inf, -inf, 2.0, 0.0, -0.0, inf, inf, -inf],
        "the largest doubles": [mref.DBL_MAX, -mref.DBL_MAX] * 5 + [0.0],
        "one NaN first": [nan] + list(rng.choice(mref.SPECIAL, 12)),
        "one NaN last": list(rng.choice(mref.SPECIAL, 12)) + [nan],
        "one NaN in the middle": list(rng.choice(mref.SPECIAL, 6)) + [nan] + list(rng.choice(mref.SPECIAL, 6)),
    }
    for M in (1, 2, 3, 16, 17, 40):
        cols["SPECIAL, M = %d" % M] = list(rng.choice(mref.SPECIAL, M))
        cols["normal, M = %d" % M] = list(rng.standard_normal(M) * 10.0 ** rng.integers(-300, 300, M))
    return cols


REF_PROBS = PROBS + (0.25, 1 - 1e-16, 1e-16, 0.75)


@pytest.mark.parametrize("name", sorted(ref_columns()))
def test_ref_quantiles_is_the_scalar_loop(name):
    col = np.array(ref_columns()[name], dtype=np.float64)
    probs = REF_PROBS + ((1 / (len(col) - 1),) if len(col) > 1 else ())
    # the column alone, and among others of its length (the reference sorts a matrix)
    rng = np.random.default_rng(len(col))
    V = np.stack([col, rng.permutation(col), rng.choice(mref.SPECIAL, len(col)), col[::-1]], axis=1)
    got = mref.ref_quantiles(V, probs)
    assert got.shape == (len(probs), 4)
    want = np.array([[scalar_quantile(V[:, c], p) for c in range(4)] for p in probs])
    assert mref.same_bits(got, want), (name, got, want)
    assert mref.same_bits(got[:, 0], got[:, 1]) and mref.same_bits(got[:, 0], got[:, 3])  # the row order is nothing
    assert mref.same_bits(mref.ref_quantiles(col.reshape(-1, 1), probs)[:, 0], want[:, 0])
    if "NaN" in name:
        assert np.all(np.isnan(got[:, 0]))


def test_ref_sort_puts_negative_zero_first():
    S = mref.sort_columns(np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -1.0, -0.0]]))
    assert np.array_equal(np.signbit(S), [[True, True, True], [True, True, True], [False, True, False],
                                          [False, False, False]])
    assert np.array_equal(S[:, 1], [-1.0, -0.0, -0.0, 0.0]) and np.array_equal(S[:, 2], [-0.0, -0.0, 0.0, 1.0])
    # what the pinned cases mean.  a + g * (b - a) with a == b is a + 0.0: of zeros only, 0.0 whatever their signs
    q = mref.ref_quantiles(np.array([[0.0, -0.0], [-0.0, -0.0]]), (0.0, 0.5, 1.0))
    assert np.all(q == 0.0) and not np.signbit(q).any()
    inf = math.inf
    assert math.isnan(mref.ref_quantiles(np.array([[inf], [inf]]), (0.5,))[0, 0])
    assert mref.ref_quantiles(np.array([[-mref.DBL_MAX], [mref.DBL_MAX]]), (0.5,))[0, 0] == inf
    assert not mref.same_bits([0.0], [-0.0]) and mref.same_bits([math.nan, -0.0], [math.nan, -0.0])
    assert not mref.same_bits([math.nan, 1.0], [1.0, math.nan])


@pytest.mark.parametrize("bins", [(8, -4.0, 4.0), (5, -1e300, 1e300), (4, -1e300, 1e300), (4096, -1.0, 1.0),
                                  (4, -10.0, 30.0), (25, 0.0, 50.0), (7, 3.0, 41.5), (1, -5e-324, 5e-324)])
def test_ref_slots_is_the_scalar_restatement(bins):
    rng = np.random.default_rng(9)
    nbins, lo, hi = bins
    w = (hi - lo) / nbins
    edges = [lo + k * w for k in range(nbins + 1)]
    v = np.array(list(mref.SPECIAL) + [math.nan, lo, hi, np.nextafter(lo, -math.inf), np.nextafter(hi, -math.inf),
                                       np.nextafter(lo, math.inf), np.nextafter(hi, math.inf)]
                 + edges[:64] + edges[-64:] + list(rng.uniform(lo, hi, 200) if hi - lo < 1e300 else
                                                   rng.standard_normal(200) * 10.0 ** rng.integers(290, 301, 200)))
    got = mref.ref_slots(v, bins)
    assert got.dtype == np.int64 and got.tolist() == [scalar_slot(float(x), *bins) for x in v]
    assert got.min() >= 0 and got.max() == nbins + 2
    H = mref.ref_hist(np.stack([v, v[::-1], np.full(len(v), lo)], axis=1), bins)
    assert H.shape == (3, nbins + 3) and H.dtype == np.int64
    assert np.array_equal(H[0], np.bincount(got, minlength=nbins + 3)) and np.array_equal(H[0], H[1])
    assert H[2, 1] == len(v) and H[2].sum() == len(v)


def test_designed_models_rasterize_to_the_design():
    """A 40 x 96 matrix drawn from SPECIAL, with NaN in two columns: oracle_np.rasterize returns it bit for bit."""
    rng = np.random.default_rng(21)
    V = rng.choice(mref.SPECIAL, (40, 96))
    V[3, 5] = V[39, 90] = math.nan
    i = np.arange(96)
    sites = (20.0 + 10.0 * (i % 12), -100.0 + 7.0 * (i // 12), 5.0 + 3.0 * (i % 5))
    models = mref.designed_models(V, sites)
    assert len(models) == 40 and all(len(m[3]) == 96 for m in models)
    with np.errstate(all="ignore"):
        got = oracle_np.rasterize(models, *sites)[2]
    assert mref.same_bits(got, V) and np.isnan(got).sum() == 2
    assert {float(x) for x in mref.SPECIAL} <= {float(x) for x in V.ravel() if not math.isnan(x)}
    assert np.signbit(got[V == 0]).any() and not np.signbit(got[V == 0]).all()
    with pytest.raises(AssertionError):
        mref.designed_models(V[:, :2], ([0.0, 0.5], [0.0, 0.0], [0.0, 0.0]))
