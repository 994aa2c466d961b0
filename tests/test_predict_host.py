"""CPU: the host side of the posterior predictive calls (td_rasterize_predict, td_history_predict): the plan
of slabs and model chunks, restated, the argument checks made before any HIP call, and the binding."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest

GIB = 1 << 30
MAX_POINTS = 1 << 18
MAX_CHUNK = 1 << 19
MAX_RAYS = 1 << 20


def plan(nmodels, ray_points, budget, forced_points, forced_chunk):
    """include/tdstar_testing.h, tdt_predict_plan, restated: (points per slab, models per sweep, ray edges)."""
    b = budget if budget > 0 else GIB
    longest = max(ray_points, default=0)
    pts = forced_points // 64 * 64 if forced_points > 0 else b // 8 // nmodels // 64 * 64
    pts = min(max(pts, 64, (longest + 63) // 64 * 64), MAX_POINTS)
    chunk = forced_chunk if forced_chunk > 0 else max(1, b // (8 * pts))
    chunk = min(chunk, nmodels, MAX_CHUNK)
    edges, used = [0], 0
    for i, p in enumerate(ray_points):
        if i > edges[-1] and (used + p > pts or i - edges[-1] == MAX_RAYS):
            edges.append(i)
            used = 0
        used += p
    if len(ray_points):
        edges.append(len(ray_points))
    return pts, chunk, edges


def shipped_like(n=381, seed=3):
    return [int(v) for v in np.random.default_rng(seed).integers(20, 70, n)]


CASES = {
    "the documented ensemble on 381 rays": (10 ** 4, shipped_like(), GIB, 0, 0),
    "the default budget": (10 ** 4, shipped_like(), 0, 0, 0),
    "one model, one ray of one point": (1, [1], GIB, 0, 0),
    "no rays": (5, [], GIB, 0, 0),
    "rays without points only": (5, [0, 0, 0], GIB, 0, 0),
    "the longest ray above the budget's slab: the models are chunked": (10 ** 6, [10, 300, 0, 129, 64, 64, 1], GIB, 0, 0),
    "a ray of exactly the slab's points": (10 ** 6, [64, 128, 128, 1, 127, 128], GIB, 0, 0),
    "a budget below one tile of one model": (7, shipped_like(40), 100, 0, 0),
    "so many models that they are chunked": (3 * 10 ** 7, [30, 40, 50], GIB, 0, 0),
    "more models than one sweep takes": (3 * 10 ** 6, [3], GIB, 0, 0),
    "forced sizes that are no multiples of 64": (9, shipped_like(60), GIB, 100, 3),
    "a forced slab below the longest ray": (9, [2100, 3, 9, 17, 1025, 0, 1, 2], GIB, 64, 1),
    "a forced slab below one tile": (9, shipped_like(30), GIB, 1, 4),
    "a forced chunk above the models": (9, shipped_like(30), GIB, 4096, 100),
    "the longest ray the call takes": (2, [MAX_POINTS, 5, MAX_POINTS - 1, 1], GIB, 0, 0),
    "the cap on a slab's points": (1, [1000] * 600, 1 << 40, 0, 0),
    "more rays without points than one slab takes": (2, [0] * (MAX_RAYS + 5) + [7], GIB, 0, 0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_is_the_restated_formula(tt, case):
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    nmodels, rays, budget, fp, fc = CASES[case]
    rp = np.ascontiguousarray(rays, dtype=np.int64)
    out = (ctypes.c_int64 * 3)()
    edges = np.full(len(rays) + 1, -1, dtype=np.int64)
    assert L.tdt_predict_plan(nmodels, len(rays), _lib.ptr(rp), budget, fp, fc, out, _lib.ptr(edges)) == 0
    pts, chunk, nslabs = out[0], out[1], out[2]
    got = [int(e) for e in edges[:nslabs + 1]]
    assert (pts, chunk, got) == plan(nmodels, rays, budget, fp, fc)
    assert tt.TdContext.predict_plan(nmodels, rays, budget, fp, fc) == (pts, chunk, got)
    assert L.tdt_predict_plan(nmodels, len(rays), _lib.ptr(rp), budget, fp, fc, out, None) == 0  # (edges are optional)
    assert (out[0], out[1], out[2]) == (pts, chunk, nslabs)
    b = budget or GIB
    assert pts % 64 == 0 and 64 <= pts <= MAX_POINTS and 1 <= chunk <= min(nmodels, MAX_CHUNK)
    assert pts >= max(rays, default=0)
    # every slab holds whole rays, and the slabs cover all rays exactly once, in order
    assert got[0] == 0 and got[-1] == len(rays) and all(b2 > a for a, b2 in zip(got, got[1:]))
    assert nslabs == (0 if not rays else len(got) - 1)
    load = [sum(rays[a:b2]) for a, b2 in zip(got, got[1:])]
    assert all(v <= pts for v in load) and all(b2 - a <= MAX_RAYS for a, b2 in zip(got, got[1:]))
    # greedy: the next slab's first ray did not fit
    for k in range(len(load) - 1):
        assert load[k] + rays[got[k + 1]] > pts or got[k + 1] - got[k] == MAX_RAYS
    if fp == 0 and fc == 0:  # the automatic sizes against the budget
        tile = max(64, (max(rays, default=0) + 63) // 64 * 64)
        if pts > tile:
            assert 8 * nmodels * pts <= b < 8 * nmodels * (pts + 64) or pts == MAX_POINTS
        if chunk < min(nmodels, MAX_CHUNK):
            assert chunk == 1 or 8 * chunk * pts <= b < 8 * (chunk + 1) * pts
        else:
            assert 8 * chunk * pts <= b or chunk == 1 or chunk == MAX_CHUNK
    # one launch of either sweep of one chunk (128 or 256 points per block, models dealt over 8 XCDs) fits 32 bits
    assert 8 * ((chunk + 7) // 8) * ((pts + 127) // 128) <= 2 ** 31 - 1


def test_plan_of_the_documented_shapes_and_bad_arguments(tt):
    P = tt.TdContext.predict_plan
    rays = [44] * 381
    assert P(10 ** 4, rays) == (13_376, 10 ** 4, [0, 304, 381])  # 304 rays of 44 points fill 13 376
    assert P(1, [1]) == (1 << 18, 1, [0, 1])
    assert P(9, [2100, 3, 9], forced_points=64, forced_chunk=4) == (2112, 4, [0, 3])
    assert P(9, [2100, 13, 9], forced_points=64) == (2112, 9, [0, 1, 3])
    assert P(5, []) == (1 << 18, 5, [0])
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    out = (ctypes.c_int64 * 3)()
    rp = np.array([3, 4], dtype=np.int64)
    for bad in ((0, 2, 0, 0, 0), (1, -1, 0, 0, 0), (1, 2, -1, 0, 0), (1, 2, 0, -1, 0), (1, 2, 0, 0, -1)):
        assert L.tdt_predict_plan(bad[0], bad[1], _lib.ptr(rp), *bad[2:], out, None) == 1
    assert L.tdt_predict_plan(1, 2, None, 0, 0, 0, out, None) == 1
    assert L.tdt_predict_plan(1, 2, _lib.ptr(rp), 0, 0, 0, None, None) == 1
    assert L.tdt_predict_plan(1, 2, _lib.ptr(np.array([3, -1], dtype=np.int64)), 0, 0, 0, out, None) == 1
    # a ray longer than a slab can be
    assert L.tdt_predict_plan(1, 2, _lib.ptr(np.array([3, MAX_POINTS + 1], dtype=np.int64)), 0, 0, 0, out, None) == 1


def predict_of(_lib, n=4, ptS=True, phi=True, mean=True, std=True, marg=None, conv=None):
    keep = [np.zeros(n), np.zeros(1), np.zeros(n), np.zeros(n)]
    r = _lib.TdPredict(*(_lib.ptr(a) if on else None for a, on in zip(keep, (ptS, phi, mean, std))),
                       ctypes.addressof(marg) if marg is not None else None,
                       ctypes.addressof(conv) if conv is not None else None)
    return r, keep


def both(tt, req, nchains=0, lens=None, expect=None):
    """Both entry points without a context (none can be made without a GPU): TD_ERR_ARG, the message through
    td_last_error(NULL) with the entry point named (and `expect` in td_rasterize_predict's)."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    off = np.array([0, 1], dtype=np.int64)
    c = np.zeros(1)
    pr = ctypes.byref(req) if req is not None else None
    rc = L.td_rasterize_predict(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, nchains, _lib.ptr(lens), pr)
    assert rc == 1
    msg = L.td_last_error(None)
    assert msg and b"td_rasterize_predict" in msg, msg
    if expect:
        assert expect in msg, msg
    rc = L.td_history_predict(None, None, 0, pr)
    assert rc == 1
    msg2 = L.td_last_error(None)
    assert msg2 and b"td_history_predict" in msg2, msg2
    return msg, msg2


def test_predict_argument_errors_before_any_hip_call(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    _, m2 = both(tt, None, expect=b"out is NULL")
    assert b"out is NULL" in m2
    r, keep = predict_of(_lib, ptS=False, phi=False, mean=False, std=False)
    _, m2 = both(tt, r, expect=b"nothing asked for")
    assert b"nothing asked for" in m2
    for kw in (dict(mean=False), dict(std=False)):
        r, keep = predict_of(_lib, **kw)
        _, m2 = both(tt, r, expect=b"mean_out and std_out must be given together")
        assert b"must be given together" in m2
    # legal requests get as far as the context check (a history list without a sample stops one step earlier)
    for kw in (dict(), dict(ptS=False, phi=False), dict(mean=False, std=False), dict(ptS=False, mean=False, std=False)):
        r, keep = predict_of(_lib, **kw)
        _, m2 = both(tt, r, expect=b"ctx is NULL")
        assert b"the histories hold no sample" in m2
    L = tt.lib()
    r, keep = predict_of(_lib)
    c = np.zeros(4)
    # the order after the request itself: the offsets, then the models, then the context
    off = np.array([0, 3, 2, 4], dtype=np.int64)
    assert L.td_rasterize_predict(None, 3, _lib.ptr(off), *(_lib.ptr(c),) * 4, 0, None, ctypes.byref(r)) == 1
    assert L.td_last_error(None) == b"td_rasterize_predict: offsets not monotone"
    off = np.array([1, 3], dtype=np.int64)
    assert L.td_rasterize_predict(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, 0, None, ctypes.byref(r)) == 1
    assert b"td_rasterize_predict: bad cell offsets" in L.td_last_error(None)
    off = np.array([0, 3], dtype=np.int64)
    assert L.td_rasterize_predict(None, 1, _lib.ptr(off), None, *(_lib.ptr(c),) * 3, 0, None, ctypes.byref(r)) == 1
    assert b"td_rasterize_predict: bad cell offsets" in L.td_last_error(None)
    for nm, po in ((0, _lib.ptr(off)), (1, None)):
        assert L.td_rasterize_predict(None, nm, po, *(_lib.ptr(c),) * 4, 0, None, ctypes.byref(r)) == 1
        assert L.td_last_error(None) == b"td_rasterize_predict: need nmodels >= 1 and cell_off"
    hs = (ctypes.c_void_p * 1)(None)
    assert L.td_history_predict(None, hs, 1, ctypes.byref(r)) == 1
    assert L.td_last_error(None) == b"td_history_predict: a history is NULL"
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
    r, keep = predict_of(_lib, marg=w)
    m1, m2 = both(tt, r)
    assert b"ctx is NULL" not in m1 and b"hold no sample" not in m2
    assert m2 == m1.replace(b"td_rasterize_predict", b"td_history_predict")
    # the same words as td_rasterize_marginals', under this entry point's name
    L = tt.lib()
    off, c, o = np.array([0, 1], dtype=np.int64), np.zeros(1), np.zeros(4)
    assert L.td_rasterize_marginals(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, *(_lib.ptr(o),) * 3, 4, _lib.ptr(o),
                                    _lib.ptr(o), ctypes.byref(w)) == 1
    assert L.td_last_error(None).replace(b"td_rasterize_marginals", b"td_rasterize_predict") == m1
    # a request for the marginals alone is a request
    r, keep = predict_of(_lib, ptS=False, phi=False, mean=False, std=False, marg=w)
    m1b, _ = both(tt, r)
    assert m1b == m1
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
    rh, e, g = np.zeros(4), np.zeros(4), np.zeros(4, dtype=np.int32)
    w = _lib.TdConvergence(kw.get("max_lag", 0), _lib.ptr(rh) if kw.get("rhat", True) else None,
                           _lib.ptr(e) if kw.get("ess", True) else None, _lib.ptr(g) if kw.get("lags", True) else None)
    r, keep = predict_of(_lib, conv=w)
    L = tt.lib()
    off = np.arange(5, dtype=np.int64)  # four models of one cell: the only legal chains are [4]
    c = np.zeros(4)
    la = np.ascontiguousarray(lens, dtype=np.int64) if lens is not None else None
    rc = L.td_rasterize_predict(None, 4, _lib.ptr(off), *(_lib.ptr(c),) * 4, nchains, _lib.ptr(la), ctypes.byref(r))
    assert rc == 1
    msg = L.td_last_error(None)
    assert b"td_rasterize_predict" in msg and words in msg, msg
    # the same words as td_convergence_values', under this entry point's name
    v = np.zeros((4, 4))
    assert L.td_convergence_values(None, _lib.ptr(v), 4, 4, nchains, _lib.ptr(la), ctypes.byref(w)) == 1
    assert L.td_last_error(None).replace(b"td_convergence_values", b"td_rasterize_predict") == msg
    if case in ("max_lag < 0", "no output"):  # (a history's chains are its own: nothing else to reject without one)
        assert L.td_history_predict(None, None, 0, ctypes.byref(r)) == 1
        assert L.td_last_error(None) == msg.replace(b"td_rasterize_predict", b"td_history_predict")
    # the offsets are checked after the request, before the chains
    bad_off = np.array([0, 2, 1, 3, 4], dtype=np.int64)
    if case not in ("max_lag < 0", "no output"):
        assert L.td_rasterize_predict(None, 4, _lib.ptr(bad_off), *(_lib.ptr(c),) * 4, nchains, _lib.ptr(la),
                                      ctypes.byref(r)) == 1
        assert b"offsets not monotone" in L.td_last_error(None)
    del keep
    # the legal request reaches the context check
    w = _lib.TdConvergence(0, _lib.ptr(rh), _lib.ptr(e), _lib.ptr(g))
    r, keep = predict_of(_lib, ptS=False, phi=False, mean=False, std=False, conv=w)
    la = np.array([4], dtype=np.int64)
    assert L.td_rasterize_predict(None, 4, _lib.ptr(off), *(_lib.ptr(c),) * 4, 1, _lib.ptr(la), ctypes.byref(r)) == 1
    assert L.td_last_error(None) == b"td_rasterize_predict: ctx is NULL"


def test_symbols_hooks_and_layout(tt):
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    for name in ("td_rasterize_predict", "td_history_predict", "tdt_predict_plan", "tdt_set_predict_plan",
                 "tdt_set_predict_placement"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.tdt_set_predict_plan(None, 64, 1) == 1
    assert L.tdt_set_predict_placement(None, 1) == 1
    for name in ("predict", "predict_history", "set_predict_plan", "set_predict_placement", "predict_plan"):
        assert callable(getattr(tt.TdContext, name)), name
    assert callable(tt.posterior_predictive)
    # TdPredict is the header's td_predict, field by field (pointers only: 8 bytes each, no padding)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tdstar.h")).read()
    body = re.search(r"typedef struct td_predict \{(.*?)\} td_predict;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert "*" in decl, decl
        names += [v.strip().lstrip("*") for v in decl[decl.index("*"):].split(",")]
    assert names == [f for f, _ in _lib.TdPredict._fields_] == ["ptS_out", "phi_out", "mean_out", "std_out", "marg", "conv"]
    assert all(t is ctypes.c_void_p for _, t in _lib.TdPredict._fields_)
    assert ctypes.sizeof(_lib.TdPredict) == 8 * len(names)
    assert [getattr(_lib.TdPredict, f).offset for f in names] == [8 * k for k in range(len(names))]
