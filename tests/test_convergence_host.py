"""CPU: the host side of the convergence diagnostics (td_convergence_values, td_rasterize_convergence,
td_history_convergence): the plan the chain lengths decide, restated; the argument checks made before
any HIP call; and the sanity of the numpy restatement itself (tests/convergence_ref.py) on AR(1) columns,
the reference the GPU tests compare with bit for bit."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

import convergence_ref as cref

LAYOUTS = ([4], [5], [4, 5], [9, 8, 31], [400] * 4)
MAX_LAGS = (0, 1, 5, 10 ** 6)


def _lib():
    return import_module("mcmc_in_tonga_amd._lib")


@pytest.mark.parametrize("lens", LAYOUTS, ids=lambda v: "x".join(map(str, v[:3])) + ("x%d" % len(v) if len(v) > 3 else ""))
def test_plan_is_the_restated_plan(tt, lens):
    L = tt.lib()
    ptr = _lib().ptr
    cl = np.array(lens, dtype=np.int64)
    for max_lag in MAX_LAGS:
        ref = cref.plan(lens, max_lag)
        out = np.zeros(4, dtype=np.int64)
        seq = np.zeros(2 * len(lens), dtype=np.int64)
        tau = ctypes.c_double()
        assert L.tdt_convergence_plan(len(lens), ptr(cl), max_lag, ptr(out), ptr(seq), ctypes.byref(tau)) == 0
        assert list(out) == [ref["n"], ref["m"], ref["T"], ref["seq_start"][0]], (lens, max_lag)
        assert list(seq) == ref["seq_start"]
        assert tau.value == ref["tau_floor"]
        assert ref["n"] >= 2 and 1 <= ref["T"] <= ref["n"] - 1
        # the sequences are the last 2n rows of every chain, inside it, the halves adjacent
        pos = 0
        for c, Lc in enumerate(lens):
            a, b = seq[2 * c], seq[2 * c + 1]
            assert pos <= a and b == a + ref["n"] and b + ref["n"] == pos + Lc
            pos += Lc
        # nullable outputs
        assert L.tdt_convergence_plan(len(lens), ptr(cl), max_lag, ptr(out), None, None) == 0
    assert L.tdt_convergence_plan(len(lens), ptr(cl), -1, ptr(out), None, None) == 1
    assert L.tdt_convergence_plan(0, ptr(cl), 0, ptr(out), None, None) == 1
    assert L.tdt_convergence_plan(len(lens), None, 0, ptr(out), None, None) == 1
    assert L.tdt_convergence_plan(len(lens), ptr(cl), 0, None, None, None) == 1


def test_plan_values():
    """The restated plan on cases worked by hand."""
    assert cref.plan([4, 5]) == dict(n=2, m=4, T=1, seq_start=[0, 2, 5, 7], tau_floor=1.0 / np.log10(8.0))
    p = cref.plan([9, 8, 31], 2)
    assert (p["n"], p["m"], p["T"], p["seq_start"]) == (4, 6, 2, [1, 5, 9, 13, 40, 44])
    assert cref.plan([65])["seq_start"] == [1, 33] and cref.plan([65])["T"] == 31


def want_of(max_lag=0, rhat=True, ess=True, lags=True, ncol=4):
    lib = _lib()
    keep = [np.zeros(ncol), np.zeros(ncol), np.zeros(ncol, dtype=np.int32)]
    w = lib.TdConvergence(max_lag, lib.ptr(keep[0]) if rhat else None, lib.ptr(keep[1]) if ess else None,
                          lib.ptr(keep[2]) if lags else None)
    return w, keep


BIG = np.full(65536, 65536, dtype=np.int64)  # m n = 2^17 * 2^15 > INT32_MAX

# case -> (want kwargs or None for a NULL want, nchains, chain_len or None, M)
BAD = {
    "want NULL": (None, 1, [8], 8),
    "max_lag < 0": (dict(max_lag=-1), 1, [8], 8),
    "all outputs NULL": (dict(rhat=False, ess=False, lags=False), 1, [8], 8),
    "nchains < 1": (dict(), 0, [8], 8),
    "chain_len NULL": (dict(), 1, None, 8),
    "a length < 4": (dict(), 2, [5, 3], 8),
    "sum != M": (dict(), 2, [4, 5], 8),
    "m n > INT32_MAX": (dict(), len(BIG), BIG, int(BIG.sum())),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_argument_errors_before_any_hip_call(tt, case):
    """No context is needed (none can be made without a GPU): the request is checked first, and the
    message, which names the entry point, goes to td_last_error(NULL)."""
    L = tt.lib()
    ptr = _lib().ptr
    kw, nchains, lens, M = BAD[case]
    w, keep = want_of(**kw) if kw is not None else (None, None)
    wp = ctypes.byref(w) if w is not None else None
    cl = np.ascontiguousarray(lens, dtype=np.int64) if lens is not None else None
    v = np.zeros((8, 4))
    q = np.zeros(4)
    off = np.arange(M + 1, dtype=np.int64) if M < 100 else None
    rc = L.td_convergence_values(None, ptr(v), M, 4, nchains, ptr(cl), wp)
    assert rc == 1, case
    assert b"td_convergence_values" in L.td_last_error(None) and b"ctx is NULL" not in L.td_last_error(None)
    rc = L.td_rasterize_convergence(None, M, ptr(off), ptr(q), ptr(q), ptr(q), ptr(q), ptr(q), ptr(q), ptr(q), 4,
                                    nchains, ptr(cl), ptr(q), ptr(q), wp)
    assert rc == 1, case
    assert b"td_rasterize_convergence" in L.td_last_error(None) and b"ctx is NULL" not in L.td_last_error(None)
    if lens is not None and nchains == 1 and list(lens) == [8]:  # the request's own errors: no chain_len argument here
        rc = L.td_history_convergence(None, None, 0, ptr(q), ptr(q), ptr(q), 4, ptr(q), ptr(q), wp)
        assert rc == 1, case
        assert b"td_history_convergence" in L.td_last_error(None)
    del keep


def test_legal_request_reaches_the_context_check(tt):
    L = tt.lib()
    ptr = _lib().ptr
    cl = np.array([4, 5], dtype=np.int64)
    v = np.zeros((9, 4))
    q = np.zeros(4)
    off = np.arange(10, dtype=np.int64)
    for kw in (dict(), dict(ess=False, lags=False), dict(rhat=False, lags=False), dict(rhat=False, ess=False),
               dict(max_lag=10 ** 6)):
        w, keep = want_of(**kw)
        assert L.td_convergence_values(None, ptr(v), 9, 4, 2, ptr(cl), ctypes.byref(w)) == 1
        assert b"ctx is NULL" in L.td_last_error(None)
        assert L.td_rasterize_convergence(None, 9, ptr(off), ptr(q), ptr(q), ptr(q), ptr(q), ptr(q), ptr(q), ptr(q), 4,
                                          2, ptr(cl), ptr(q), ptr(q), ctypes.byref(w)) == 1
        assert b"ctx is NULL" in L.td_last_error(None)
        assert L.td_history_convergence(None, None, 0, ptr(q), ptr(q), ptr(q), 4, ptr(q), ptr(q), ctypes.byref(w)) == 1
        assert b"ctx is NULL" in L.td_last_error(None)
    assert L.tdt_set_convergence_round(None, 2) == 1
    assert L.tdt_set_convergence_lag_block(None, 8) == 1


# ------------------------------------------------- the restatement itself ----
NCH, LEN, NCOL = 4, 400, 50


@pytest.fixture(scope="module")
def ar_half():
    """phi = 0.5, 4 chains x 400 samples x 50 columns, chain after chain."""
    rng = np.random.default_rng(2024)
    return np.concatenate([cref.ar1(rng, 0.5, LEN, NCOL) for _ in range(NCH)])


def test_restatement_on_mixing_chains(ar_half):
    r = cref.convergence(ar_half, [LEN] * NCH)
    ratio = r["ess"] / (2 * NCH * (LEN // 2))
    print("rhat %.4f..%.4f  ess/(mn) %.3f..%.3f" % (r["rhat"].min(), r["rhat"].max(), ratio.min(), ratio.max()))
    assert np.all(r["rhat"] < 1.05)
    assert np.all((ratio >= 0.15) & (ratio <= 0.6))  # (1 - phi) / (1 + phi) = 1/3
    assert np.all(r["lags"] > 0)  # every column stopped on its own


def test_restatement_catches_a_shifted_chain(ar_half):
    V = ar_half.copy()
    V[LEN:2 * LEN] += 2.0
    r = cref.convergence(V, [LEN] * NCH, max_lag=1)
    print("rhat %.4f..%.4f" % (r["rhat"].min(), r["rhat"].max()))
    assert np.all(r["rhat"] > 1.1)


def test_restatement_catches_a_trend():
    """One chain, iid, with a linear trend of 3 sigma: only the split shows it."""
    rng = np.random.default_rng(7)
    V = rng.standard_normal((LEN, NCOL)) + np.linspace(0.0, 3.0, LEN)[:, None]
    r = cref.convergence(V, [LEN], max_lag=1)
    print("rhat %.4f..%.4f" % (r["rhat"].min(), r["rhat"].max()))
    assert np.all(r["rhat"] > 1.1)


def test_restatement_edge_columns():
    n2 = 40
    alt = np.where(np.arange(n2) % 2 == 0, 1.0, -1.0)
    const = np.full(n2, 3.5)
    nan = np.arange(n2, dtype=np.float64)
    nan[7] = np.nan
    r = cref.convergence(np.column_stack([alt, const, nan]), [n2])
    p = cref.plan([n2])
    assert r["ess"][0] == p["m"] * p["n"] / p["tau_floor"]  # the floor
    assert np.isnan(r["rhat"][1]) and np.isnan(r["ess"][1]) and r["lags"][1] == 1
    assert np.isnan(r["rhat"][2]) and np.isnan(r["ess"][2]) and r["lags"][2] == 1
