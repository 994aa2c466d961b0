"""CPU: the host side of the posterior covariance calls (td_rasterize_covariance, td_history_covariance): every
argument check made before any HIP call, in the header's order, the binding, and the numpy restatement the GPU
is compared against (tests/covariance_ref.py) against numpy's own covariance."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest

import covariance_ref as cref


def request(_lib, nq=4, nt=2, nseries=1, q=(True,) * 3, t=(True,) * 3, series=True, cov=True, corr=True, mean=True,
            std=True, tmean=True, tstd=True):
    """A td_covariance over small arrays; False leaves a pointer NULL.  -> (the struct, what it points into)."""
    n = max(nq, 1)
    T = max(nt + nseries, 1)
    keep = dict(q=[np.zeros(n) for _ in range(3)], t=[np.zeros(max(nt, 1)) for _ in range(3)],
                series=np.zeros((1, max(nseries, 1))), cov=np.zeros((T, n)), corr=np.zeros((T, n)), mean=np.zeros(n),
                std=np.zeros(n), tmean=np.zeros(T), tstd=np.zeros(T))
    p = _lib.ptr
    r = _lib.TdCovariance(*(p(a) if on else None for a, on in zip(keep["q"], q)), nq,
                          *(p(a) if on else None for a, on in zip(keep["t"], t)), nt,
                          p(keep["series"]) if series else None, nseries, p(keep["cov"]) if cov else None,
                          p(keep["corr"]) if corr else None, p(keep["mean"]) if mean else None,
                          p(keep["std"]) if std else None, p(keep["tmean"]) if tmean else None,
                          p(keep["tstd"]) if tstd else None)
    return r, keep


def both(tt, req, words):
    """Both entry points without a context (none can be made without a GPU), on one model of one cell and on
    no history: TD_ERR_ARG, and the message through td_last_error(NULL) names the entry point and holds
    `words` (a pair: td_rasterize_covariance's and td_history_covariance's)."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    w1, w2 = words if isinstance(words, tuple) else (words, words)
    off = np.array([0, 1], dtype=np.int64)
    c = np.zeros(1)
    pr = ctypes.byref(req) if req is not None else None
    assert L.td_rasterize_covariance(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_rasterize_covariance: ") and w1 in msg, msg
    assert L.td_history_covariance(None, None, 0, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_history_covariance: ") and w2 in msg, msg


# in the header's order; each request is wrong in this way and in every LATER way that can be combined with it,
# so the message shows which check ran first
ORDER = [
    ("struct NULL", None, b"cov is NULL"),
    ("nq < 0", dict(nq=-1, nt=0, nseries=0, cov=False, corr=False), b"must be >= 0"),
    ("nt < 0", dict(nt=-1, nseries=1, cov=False, corr=False), b"must be >= 0"),
    ("nseries < 0", dict(nt=1, nseries=-1, cov=False, corr=False), b"must be >= 0"),
    ("no target", dict(nt=0, nseries=0, cov=False, corr=False, q=(False,) * 3), b"no target"),
    ("no output", dict(cov=False, corr=False, q=(True, False, True)), b"cov_out and corr_out are both NULL"),
    ("qx NULL", dict(q=(False, True, True), series=False), b"qx, qy and qz"),
    ("qy NULL", dict(q=(True, False, True), t=(False,) * 3), b"qx, qy and qz"),
    ("qz NULL", dict(q=(True, True, False), mean=False), b"qx, qy and qz"),
    ("tx NULL", dict(t=(False, True, True), series=False), b"tx, ty and tz"),
    ("ty NULL", dict(t=(True, False, True), mean=False), b"tx, ty and tz"),
    ("tz NULL", dict(t=(True, True, False), tstd=False), b"tx, ty and tz"),
    ("series NULL", dict(series=False, mean=False, tmean=False), b"series is NULL"),
    ("mean without std", dict(std=False, tmean=False), b"mean_out and std_out must be given together"),
    ("std without mean", dict(mean=False, tstd=False), b"mean_out and std_out must be given together"),
    ("tmean without tstd", dict(tstd=False), b"tmean_out and tstd_out must be given together"),
    ("tstd without tmean", dict(tmean=False), b"tmean_out and tstd_out must be given together"),
]


@pytest.mark.parametrize("case", [c[0] for c in ORDER])
def test_request_errors_in_the_documented_order(tt, case):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    _, kw, words = next(c for c in ORDER if c[0] == case)
    req, keep = request(_lib, **kw) if kw is not None else (None, None)
    both(tt, req, words)
    del keep


LEGAL = {
    "everything": dict(),
    "cov only": dict(corr=False),
    "corr only, no statistics": dict(cov=False, mean=False, std=False, tmean=False, tstd=False),
    "points only": dict(nseries=0, series=False),
    "series only": dict(nt=0, t=(False,) * 3),
    "no nodes": dict(nq=0, q=(False,) * 3),
}


@pytest.mark.parametrize("case", sorted(LEGAL))
def test_legal_requests_reach_the_models_then_the_context(tt, case):
    """After the request: the offsets, then the models (no model / no sample at all), then the context."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    req, keep = request(_lib, **LEGAL[case])
    both(tt, req, (b"ctx is NULL", b"the histories hold no sample"))
    pr = ctypes.byref(req)
    c = np.zeros(4)
    off = np.array([0, 3, 2, 4], dtype=np.int64)
    assert L.td_rasterize_covariance(None, 3, _lib.ptr(off), *(_lib.ptr(c),) * 4, pr) == 1
    assert L.td_last_error(None) == b"td_rasterize_covariance: offsets not monotone"
    off = np.array([1, 3], dtype=np.int64)
    assert L.td_rasterize_covariance(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, pr) == 1
    assert b"td_rasterize_covariance: bad cell offsets" in L.td_last_error(None)
    off = np.array([0, 3], dtype=np.int64)
    assert L.td_rasterize_covariance(None, 1, _lib.ptr(off), None, *(_lib.ptr(c),) * 3, pr) == 1
    assert b"td_rasterize_covariance: bad cell offsets" in L.td_last_error(None)
    for nm, po in ((0, _lib.ptr(off)), (-1, _lib.ptr(off)), (1, None)):
        assert L.td_rasterize_covariance(None, nm, po, *(_lib.ptr(c),) * 4, pr) == 1
        assert L.td_last_error(None) == b"td_rasterize_covariance: need nmodels >= 1 and cell_off"
    hs = (ctypes.c_void_p * 1)(None)
    assert L.td_history_covariance(None, hs, 1, pr) == 1
    assert L.td_last_error(None) == b"td_history_covariance: a history is NULL"
    del keep


def test_the_request_is_checked_before_the_models(tt):
    """A wrong request on wrong models: the request's message."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    req, keep = request(_lib, tstd=False)
    off = np.array([0, 3, 2], dtype=np.int64)
    c = np.zeros(4)
    assert L.td_rasterize_covariance(None, 2, _lib.ptr(off), *(_lib.ptr(c),) * 4, ctypes.byref(req)) == 1
    assert b"tmean_out and tstd_out" in L.td_last_error(None)
    assert L.td_rasterize_covariance(None, 0, None, *(None,) * 4, ctypes.byref(req)) == 1
    assert b"tmean_out and tstd_out" in L.td_last_error(None)
    del keep


def test_binding_rejects_a_series_of_the_wrong_shape(tt):
    T = tt.TdContext
    ctx = object.__new__(T)  # (no device: the shapes are checked before the library is called)
    ctx.h = None
    models = [(np.zeros(1),) * 4] * 5
    q = np.zeros(3)
    for bad in (np.zeros((4, 2)), np.zeros((6, 1)), np.zeros(4), np.zeros((5, 2, 2))):
        with pytest.raises(ValueError, match="series must be"):
            ctx.covariance(models, q, q, q, targets=[[0.0, 0.0, 0.0]], series=bad)

    class H:  # what covariance_history reads of a History before the call
        h = None

        def __len__(self):
            return 5

    with pytest.raises(ValueError, match="series must be"):
        ctx.covariance_history([H()], q, q, q, series=np.zeros((4, 1)))
    with pytest.raises(ValueError, match="same length"):
        ctx.covariance(models, q, q[:2], q, targets=[[0.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match="want"):
        ctx.covariance(models, q, q, q, targets=[[0.0, 0.0, 0.0]], want=("cov", "std"))


def test_symbols_getter_and_layout(tt):
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    for name in ("td_rasterize_covariance", "td_history_covariance", "tdt_covariance_group"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    G = L.tdt_covariance_group()
    assert G >= 1 and tt.TdContext.covariance_group() == G
    for name in ("covariance", "covariance_history", "covariance_group"):
        assert callable(getattr(tt.TdContext, name)), name
    assert callable(tt.posterior_covariance)
    # TdCovariance is the header's td_covariance, field by field (8 bytes each, no padding)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tdstar.h")).read()
    body = re.search(r"typedef struct td_covariance \{(.*?)\} td_covariance;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, counts = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:
            names += [v.strip().lstrip("*") for v in decl[decl.index("*"):].split(",")]
        else:
            assert decl.startswith("int64_t "), decl
            names.append(decl.split()[1])
            counts.append(names[-1])
    assert names == [f for f, _ in _lib.TdCovariance._fields_]
    assert counts == ["nq", "nt", "nseries"]
    assert all(t is (ctypes.c_int64 if f in counts else ctypes.c_void_p) for f, t in _lib.TdCovariance._fields_)
    assert ctypes.sizeof(_lib.TdCovariance) == 8 * len(names)
    assert [getattr(_lib.TdCovariance, f).offset for f in names] == [8 * k for k in range(len(names))]


@pytest.mark.parametrize("M", [40, 3000])
def test_the_restatement_is_a_covariance(M):
    """covariance_ref.cross_moment against np.cov / np.corrcoef, 1e-12 relative: columns that do co-vary (each
    node a positive mix of the targets plus noise, so no entry is a difference of large numbers), off zero mean."""
    rng = np.random.default_rng(M)
    T, nq = 5, 23
    A = rng.normal(size=(M, T)) + rng.uniform(-3, 3, T)
    V = A @ rng.uniform(0.5, 1.5, (T, nq)) + 0.3 * rng.normal(size=(M, nq)) + rng.uniform(-3, 3, nq)
    mean, std = cref.column_stats(V)
    tmean, tstd = cref.column_stats(A)
    assert np.allclose(mean, V.mean(axis=0), rtol=1e-12, atol=0) and np.allclose(std, V.std(axis=0, ddof=1), rtol=1e-12, atol=0)
    cov, corr = cref.cross_moment(V, mean, std, A, tmean, tstd)
    full = np.cov(np.hstack([A, V]).T)
    fullr = np.corrcoef(np.hstack([A, V]).T)
    assert cov.shape == corr.shape == (T, nq)
    err_cov = np.max(np.abs(cov - full[:T, T:]) / np.abs(full[:T, T:]))
    err_corr = np.max(np.abs(corr - fullr[:T, T:]) / np.abs(fullr[:T, T:]))
    print("M = %d: relative error cov %.3g corr %.3g" % (M, err_cov, err_corr))
    assert err_cov <= 1e-12 and err_corr <= 1e-12
    assert np.all(np.abs(corr) <= 1.0 + 1e-15) and np.min(np.abs(fullr[:T, T:])) > 0.05
    # a target that is a node: the diagonal is the variance, the correlation 1
    c2, r2 = cref.cross_moment(V, mean, std, V[:, :3], mean[:3], std[:3])
    assert np.array_equal(np.sqrt(np.diag(c2[:, :3])), std[:3])
    # c / (sqrt(c) * sqrt(c)): four roundings (two roots, the product, the quotient) of at most 2^-53 each
    assert np.allclose(np.diag(r2[:, :3]), 1.0, rtol=0, atol=4.5e-16)
