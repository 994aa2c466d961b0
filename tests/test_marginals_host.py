"""CPU: the host side of the posterior marginals (td_rasterize_marginals): Julia's quantile position
for (M, p), restated, and the argument checks made before any HIP call."""
import ctypes
import math

import numpy as np
import pytest

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
    "probs NULL": dict(nprob=2, probs=False),
    "quant_out NULL": dict(nprob=2, probs=[0.1, 0.9], quant=False),
    "hist_out NULL": dict(nbins=10, lo=0.0, hi=1.0, hist=False),
}


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
    m = ctypes.c_int64()
    assert L.tdt_set_marginals_method(None, 1) == 1
    assert L.tdt_marginals_resident_max(None, ctypes.byref(m)) == 1
