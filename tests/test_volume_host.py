"""CPU: the host side of the posterior volumes (td_rasterize_volume, td_history_volume): the slab plan,
restated, and the argument checks made before any HIP call."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

GIB = 1 << 30
INT32_MAX = 2 ** 31 - 1


def plan(nmodels, nq, budget, forced):
    """include/tdstar_testing.h, tdt_volume_plan, restated: (nodes per slab, slabs)."""
    b = budget if budget > 0 else GIB
    nodes = forced // 64 * 64 if forced > 0 else b // 8 // nmodels // 64 * 64
    nodes = min(max(nodes, 64), 1 << 18)
    groups = 8 * ((nmodels + 7) // 8)
    nodes = min(nodes, max(64, INT32_MAX // groups * 128))
    return nodes, (nq + nodes - 1) // nodes


CASES = [
    (10 ** 4, 516_000, GIB, 0),     # a 10 km lattice, the documented ensemble
    (10 ** 4, 67_048, 0, 0),        # the shipped lattice, the default budget
    (1, 1, GIB, 0),
    (1, 1, 1, 0),
    (3, 65, GIB, 64),               # 64 nodes forced: two slabs, the second of one node
    (3, 65, GIB, 100),              # forced sizes round down to a tile
    (3, 65, GIB, 1),
    (13, 316, GIB, 128),
    (10 ** 4, 516_000, 8 * 10 ** 4 * 63, 0),  # a budget below one tile
    (7, 10 ** 7, 1 << 40, 0),       # the cap on a slab's nodes
    (3 * 10 ** 8, 1000, GIB, 1 << 17),  # so many models that one launch's blocks bound the slab
    (5, 0, GIB, 0),
]


@pytest.mark.parametrize("case", CASES)
def test_plan_is_the_restated_formula(tt, case):
    L = tt.lib()
    nmodels, nq, budget, forced = case
    out = (ctypes.c_int64 * 2)()
    assert L.tdt_volume_plan(nmodels, nq, budget, forced, out) == 0
    nodes, nslabs = out[0], out[1]
    assert (nodes, nslabs) == plan(nmodels, nq, budget, forced)
    assert tt.TdContext.volume_plan(nmodels, nq, budget, forced) == (nodes, nslabs)
    # the slabs [k nodes, min((k + 1) nodes, nq)) cover [0, nq) exactly once; all but the last are whole tiles
    assert nodes >= 64 and nodes % 64 == 0
    edges = [min(k * nodes, nq) for k in range(nslabs + 1)]
    assert edges[0] == 0 and edges[-1] == nq and all(b > a for a, b in zip(edges, edges[1:]))
    assert all((b - a) % 64 == 0 for a, b in zip(edges[:-2], edges[1:-1]))
    if forced == 0 and nodes < 1 << 18 and 8 * nmodels * 64 <= (budget or GIB):
        assert 8 * nmodels * nodes <= (budget or GIB) < 8 * nmodels * (nodes + 64)
    # one launch of either sweep (128 or 256 nodes per block, models dealt over 8 XCDs) fits 32 bits
    assert 8 * ((nmodels + 7) // 8) * ((nodes + 127) // 128) <= INT32_MAX


def test_plan_of_the_documented_shapes(tt):
    assert tt.TdContext.volume_plan(10 ** 4, 516_000) == (13_376, 39)  # 209 tiles of 64 columns
    assert tt.TdContext.volume_plan(1, 1) == (1 << 18, 1)
    assert tt.TdContext.volume_plan(3, 65, forced=64) == (64, 2)
    assert tt.TdContext.volume_plan(10 ** 4, 516_000, budget=1000) == (64, 8063)
    L = tt.lib()
    out = (ctypes.c_int64 * 2)()
    for bad in ((0, 1, 0, 0), (1, -1, 0, 0), (1, 1, -1, 0), (1, 1, 0, -1)):
        assert L.tdt_volume_plan(*bad, out) == 1
    assert L.tdt_volume_plan(1, 1, 0, 0, None) == 1


def volume_of(_lib, nq=4, q=True, mean=True, std=True, marg=None, conv=None):
    keep = [np.zeros(max(nq, 1)) for _ in range(5)]
    v = _lib.TdVolume(*(_lib.ptr(a) if q else None for a in keep[:3]), nq, _lib.ptr(keep[3]) if mean else None,
                      _lib.ptr(keep[4]) if std else None, None, ctypes.addressof(marg) if marg is not None else None,
                      ctypes.addressof(conv) if conv is not None else None)
    return v, keep


def both(tt, vol, nchains=0, lens=None, expect=None):
    """Both entry points without a context (none can be made without a GPU): TD_ERR_ARG, the message
    through td_last_error(NULL) with the entry point named (and `expect` in td_rasterize_volume's)."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    off = np.array([0, 1], dtype=np.int64)
    c = np.zeros(1)
    pv = ctypes.byref(vol) if vol is not None else None
    rc = L.td_rasterize_volume(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, nchains, _lib.ptr(lens), pv)
    assert rc == 1
    msg = L.td_last_error(None)
    assert msg and b"td_rasterize_volume" in msg, msg
    if expect:
        assert expect in msg, msg
    rc = L.td_history_volume(None, None, 0, pv)
    assert rc == 1
    msg2 = L.td_last_error(None)
    assert msg2 and b"td_history_volume" in msg2, msg2
    return msg, msg2


def test_volume_argument_errors_before_any_hip_call(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    both(tt, None, expect=b"vol is NULL")
    v, keep = volume_of(_lib, nq=-1)
    both(tt, v, expect=b"nq must be >= 0")
    for kw in (dict(q=False), dict(mean=False), dict(std=False)):
        v, keep = volume_of(_lib, **kw)
        _, m2 = both(tt, v, expect=b"must be given for nq > 0")
        assert b"must be given for nq > 0" in m2
    # a legal request gets as far as the context check, nq == 0 included (no array is needed for it)
    v, keep = volume_of(_lib)
    m1, m2 = both(tt, v, expect=b"ctx is NULL")
    assert b"ctx is NULL" in m2
    v, keep = volume_of(_lib, nq=0, q=False, mean=False, std=False)
    both(tt, v, expect=b"ctx is NULL")
    del keep


BAD_MARG = {
    "prob above 1": dict(nprob=1, probs=[1.0000001]),
    "prob NaN": dict(nprob=3, probs=[0.1, float("nan"), 0.9]),
    "nprob > 64": dict(nprob=65, probs=np.linspace(0, 1, 65)),
    "nbins > 4096": dict(nbins=4097, lo=0.0, hi=1.0),
    "lo == hi": dict(nbins=10, lo=1.0, hi=1.0),
    "hi inf": dict(nbins=10, lo=0.0, hi=float("inf")),
    "probs NULL": dict(nprob=2, probs=False),
    "quant_out NULL": dict(nprob=2, probs=[0.1, 0.9], quant=False),
    "hist_out NULL": dict(nbins=10, lo=0.0, hi=1.0, hist=False),
}


@pytest.mark.parametrize("case", sorted(BAD_MARG))
def test_marginal_requests_are_checked_as_by_the_section_calls(tt, case):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    kw = dict(nprob=0, probs=None, quant=True, nbins=0, lo=0.0, hi=0.0, hist=True)
    kw.update(BAD_MARG[case])
    given = kw["probs"] is not None and kw["probs"] is not False
    p = np.ascontiguousarray(kw["probs"] if given else np.full(max(kw["nprob"], 1), 0.5), dtype=np.float64)
    q = np.zeros((max(kw["nprob"], 1), 4))
    h = np.zeros((4, max(kw["nbins"], 0) + 3), dtype=np.int64)
    w = _lib.TdMarginals(kw["nprob"], _lib.ptr(p) if kw["probs"] is not False else None,
                         _lib.ptr(q) if kw["quant"] else None, kw["nbins"], kw["lo"], kw["hi"],
                         _lib.ptr(h) if kw["hist"] else None)
    v, keep = volume_of(_lib, marg=w)
    m1, m2 = both(tt, v)
    assert b"ctx is NULL" not in m1 and b"ctx is NULL" not in m2
    # the same words as td_rasterize_marginals', under this entry point's name
    L = tt.lib()
    off, c, o = np.array([0, 1], dtype=np.int64), np.zeros(1), np.zeros(4)
    assert L.td_rasterize_marginals(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, *(_lib.ptr(o),) * 3, 4, _lib.ptr(o),
                                    _lib.ptr(o), ctypes.byref(w)) == 1
    assert L.td_last_error(None).replace(b"td_rasterize_marginals", b"td_rasterize_volume") == m1
    del keep


BAD_CONV = {
    "max_lag < 0": (dict(max_lag=-1), 1, [4], b"max_lag"),
    "no output": (dict(rhat=False, ess=False, lags=False), 1, [4], b"all NULL"),
    "nchains < 1": (dict(), 0, [4], b"nchains"),
    "chain_len NULL": (dict(), 1, None, b"chain_len is NULL"),
    "a length < 4": (dict(), 2, [3, 5], b"at least 4"),
    "lengths that do not sum to the models": (dict(), 1, [5], b"do not sum"),
}


@pytest.mark.parametrize("case", sorted(BAD_CONV))
def test_convergence_requests_are_checked_as_by_the_section_calls(tt, case):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    kw, nchains, lens, words = BAD_CONV[case]
    r, e, g = np.zeros(4), np.zeros(4), np.zeros(4, dtype=np.int32)
    w = _lib.TdConvergence(kw.get("max_lag", 0), _lib.ptr(r) if kw.get("rhat", True) else None,
                           _lib.ptr(e) if kw.get("ess", True) else None, _lib.ptr(g) if kw.get("lags", True) else None)
    v, keep = volume_of(_lib, conv=w)
    L = tt.lib()
    off = np.arange(5, dtype=np.int64)  # four models of one cell: the only legal chains are [4]
    c = np.zeros(4)
    la = np.ascontiguousarray(lens, dtype=np.int64) if lens is not None else None
    rc = L.td_rasterize_volume(None, 4, _lib.ptr(off), *(_lib.ptr(c),) * 4, nchains, _lib.ptr(la), ctypes.byref(v))
    assert rc == 1
    msg = L.td_last_error(None)
    assert b"td_rasterize_volume" in msg and words in msg, msg
    if case in ("max_lag < 0", "no output"):  # (a history's chains are its own: nothing else to reject without one)
        assert L.td_history_volume(None, None, 0, ctypes.byref(v)) == 1
        assert b"td_history_volume" in L.td_last_error(None) and words in L.td_last_error(None)
    del keep
    # the legal request reaches the context check
    w = _lib.TdConvergence(0, _lib.ptr(r), _lib.ptr(e), _lib.ptr(g))
    v, keep = volume_of(_lib, conv=w)
    la = np.array([4], dtype=np.int64)
    assert L.td_rasterize_volume(None, 4, _lib.ptr(off), *(_lib.ptr(c),) * 4, 1, _lib.ptr(la), ctypes.byref(v)) == 1
    assert b"ctx is NULL" in L.td_last_error(None)


def test_hooks_without_a_context(tt):
    L = tt.lib()
    out = (ctypes.c_int64 * 4)()
    assert L.tdt_set_volume_slab_nodes(None, 64) == 1
    assert L.tdt_set_volume_method(None, 1) == 1
    assert L.tdt_volume_counters(None, out) == 1
    assert L.tdt_set_volume_counting(None, 1) == 1
