"""CPU: every argument check of td_rasterize_recovery / td_history_recovery made before any HIP call, without a
context, in the order include/tdstar_recovery.h writes down (the status and the text of td_last_error(NULL)), and the
binding of the header.  Needs no GPU."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("below", "equal", "above", "dmean", "dstd", "series", "weight", "mean", "std")


def request(_lib, npts=6, reg_off=(0, 2, 6), nreg=None, px=None, py=None, pz=None, w=None, truth=None, vec=(True,) * 3,
            off_ptr=True, truth_ptr=True, npoints=None, normalize=1, marg=None, conv=None, **outputs):
    """A td_recovery over small arrays; False leaves a pointer NULL.  -> (the struct, what it points into)."""
    p = _lib.ptr
    n = max(npts, 1)
    v = [np.asarray(a if a is not None else np.arange(n, dtype=np.float64), dtype=np.float64) for a in (px, py, pz)]
    tr = np.asarray(truth if truth is not None else np.ones(n), dtype=np.float64)
    off = np.asarray(reg_off, dtype=np.int64)
    R = max(len(off) - 1, 1)
    wv = np.asarray(w, dtype=np.float64) if w is not None else None
    keep = dict(v=v, off=off, w=wv, truth=tr, below=np.zeros(n, dtype=np.int64), equal=np.zeros(n, dtype=np.int64),
                above=np.zeros(n, dtype=np.int64), dmean=np.zeros(n), dstd=np.zeros(n), series=np.zeros((1, R)),
                weight=np.zeros(R), mean=np.zeros(R), std=np.zeros(R), marg=marg, conv=conv)
    assert set(outputs) <= set(OUTPUTS)
    r = _lib.TdRecovery(*(p(a) if on else None for a, on in zip(v, vec)), p(wv), npts if npoints is None else npoints,
                        p(off) if off_ptr else None, len(off) - 1 if nreg is None else nreg, p(tr) if truth_ptr else None,
                        normalize, *(p(keep[f]) if outputs.get(f, True) else None for f in OUTPUTS),
                        ctypes.addressof(marg) if marg is not None else None,
                        ctypes.addressof(conv) if conv is not None else None)
    return r, keep


def both(tt, req, words, chains=(0, None)):
    """Both entry points without a context (none can be made without a GPU), on one model of one cell and on no
    history: TD_ERR_ARG, and the message through td_last_error(NULL) names the entry point and holds `words`
    (a pair: td_rasterize_recovery's and td_history_recovery's)."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    w1, w2 = words if isinstance(words, tuple) else (words, words)
    off = np.array([0, 1], dtype=np.int64)
    c = np.zeros(1)
    pr = ctypes.byref(req) if req is not None else None
    assert L.td_rasterize_recovery(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, chains[0], _lib.ptr(chains[1]), pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_rasterize_recovery: ") and w1 in msg, msg
    assert L.td_history_recovery(None, None, 0, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_history_recovery: ") and w2 in msg, msg


def conv_want(_lib, outputs=True):
    out = np.zeros(2)
    return _lib.TdConvergence(0, _lib.ptr(out) if outputs else None, None, None), out


NONE_OUT = {f: False for f in OUTPUTS}
# in the header's order; each request is wrong in this way and in LATER ways, so the message shows which check ran first
ORDER = [
    ("struct NULL", None, b"want is NULL"),
    ("np < 1", dict(npoints=0, vec=(False,) * 3), b"np and nreg must be >= 1"),
    ("nreg < 1", dict(nreg=0, off_ptr=False), b"np and nreg must be >= 1"),
    ("px NULL", dict(vec=(False, True, True), reg_off=(1, 2, 6)), b"px, py, pz, reg_off and truth must be given"),
    ("pz NULL", dict(vec=(True, True, False), normalize=2), b"px, py, pz, reg_off and truth must be given"),
    ("reg_off NULL", dict(off_ptr=False, px=[np.nan] * 6), b"px, py, pz, reg_off and truth must be given"),
    ("truth NULL", dict(truth_ptr=False, reg_off=(1, 2, 6), px=[np.nan] * 6), b"px, py, pz, reg_off and truth must be given"),
    ("reg_off[0] != 0", dict(reg_off=(1, 2, 6), truth=[np.nan] * 6), b"reg_off[0] must be 0"),
    ("reg_off not monotone", dict(reg_off=(0, 4, 2, 6), py=[np.inf] * 6), b"reg_off is not monotone"),
    ("an empty region", dict(reg_off=(0, 2, 2, 6), w=[np.nan] * 6), b"a region without points"),
    ("reg_off[nreg] below np", dict(reg_off=(0, 2, 5), normalize=-1), b"reg_off[nreg] must be np"),
    ("reg_off[nreg] above np", dict(reg_off=(0, 2, 7), truth=[np.inf] * 6), b"reg_off[nreg] must be np"),
    ("px NaN", dict(px=[0, 1, np.nan, 3, 4, 5], truth=[np.nan] * 6), b"px is not finite"),
    ("py infinite", dict(py=[0, 1, 2, 3, 4, -np.inf], w=[np.nan] * 6), b"py is not finite"),
    ("pz NaN", dict(pz=[np.nan] * 6, **NONE_OUT), b"pz is not finite"),
    ("w infinite before truth NaN", dict(w=[1, 1, 1, np.inf, 1, 1], truth=[np.nan] * 6), b"w is not finite"),
    ("w NaN", dict(w=[1, 1, 1, 1, 1, np.nan], **NONE_OUT), b"w is not finite"),
    ("truth NaN", dict(truth=[1, 1, np.nan, 1, 1, 1], normalize=2), b"truth is not finite"),
    ("truth infinite", dict(truth=[1, 1, 1, 1, 1, -np.inf], **NONE_OUT), b"truth is not finite"),
    ("normalize 2", dict(normalize=2, **NONE_OUT), b"normalize must be 0 or 1"),
    ("normalize -1", dict(normalize=-1, dstd=False), b"normalize must be 0 or 1"),
    ("no output", dict(**NONE_OUT), b"no output asked for"),
    ("dmean without dstd", dict(dstd=False, std=False), b"dmean_out and dstd_out must be given together"),
    ("dstd without dmean", dict(dmean=False, mean=False), b"dmean_out and dstd_out must be given together"),
    ("mean without std", dict(std=False, conv="empty"), b"mean_out and std_out must be given together"),
    ("std without mean", dict(mean=False, conv="given"), b"mean_out and std_out must be given together"),
    ("conv without outputs", dict(conv="empty"), b"rhat_out, ess_out and lags_out are all NULL"),
    ("conv without chains", dict(conv="given"), (b"nchains must be >= 1", b"the histories hold no sample")),
]


@pytest.mark.parametrize("case", [c[0] for c in ORDER])
def test_request_errors_in_the_documented_order(tt, case):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    _, kw, words = next(c for c in ORDER if c[0] == case)
    held = None
    if kw is not None and "conv" in kw:
        kw = dict(kw)
        cw, held = conv_want(_lib, outputs=kw["conv"] == "given")
        kw["conv"] = cw
    req, keep = request(_lib, **kw) if kw is not None else (None, None)
    both(tt, req, words)
    if keep is not None:  # a refused call wrote nothing
        assert all(not keep[f].any() for f in OUTPUTS)
    del keep, held


def test_the_header_states_the_order_the_cases_follow():
    """The words of the header's refusal paragraph, in the order ORDER tries them."""
    hdr = " ".join(open(os.path.join(ROOT, "include", "tdstar_recovery.h")).read().replace("*", " ").split())
    para = hdr[hdr.index("TD_ERR_ARG, before any HIP call"):]
    marks = ["want NULL", "np < 1 or nreg < 1", "px, py, pz, reg_off or truth NULL", "reg_off[0] != 0", "not monotone",
             "an empty region", "reg_off[nreg] != np", "a coordinate, a weight or a truth value that is not finite",
             "px, py, pz, w, truth in this order", "normalize not 0 or 1", "no output asked for",
             "only one of dmean_out / dstd_out", "only one of mean_out / std_out", "a marg or conv",
             "conv given without chains", "offsets not monotone", "no model or no sample", "a history on another device",
             "ctx NULL", "more than 2^18 regions", "bytes of F", "leaves bytes", "A refused call changes nothing"]
    at = [para.index(m) for m in marks]
    assert at == sorted(at)


def test_conv_with_bad_chains_is_refused_before_the_models(tt):
    """conv given: the chains are checked (td_rasterize_volume's checks) before the offsets of the models."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    cw, held = conv_want(_lib)
    req, keep = request(_lib, conv=cw)
    lens = np.array([4, 4], dtype=np.int64)
    off = np.array([0, 3, 2, 4, 5, 6, 7, 8, 9], dtype=np.int64)  # (not monotone: a later check)
    c = np.zeros(9)
    p = _lib.ptr
    assert L.td_rasterize_recovery(None, 8, p(off), *(p(c),) * 4, 2, None, ctypes.byref(req)) == 1
    assert L.td_last_error(None) == b"td_rasterize_recovery: chain_len is NULL"
    assert L.td_rasterize_recovery(None, 7, p(off), *(p(c),) * 4, 2, p(lens), ctypes.byref(req)) == 1
    assert b"td_rasterize_recovery: the chain lengths do not sum" in L.td_last_error(None)
    assert L.td_rasterize_recovery(None, 8, p(off), *(p(c),) * 4, 2, p(lens), ctypes.byref(req)) == 1
    assert L.td_last_error(None) == b"td_rasterize_recovery: offsets not monotone"
    del keep, held


LEGAL = {
    "everything": dict(),
    "weighted": dict(w=[1.0, -1.0, 0.5, 2.0, 1.0, 1.0]),
    "sums": dict(normalize=0),
    "truth of zeros of both signs": dict(truth=[0.0, -0.0, 0.0, -0.0, 1.0, -1.0]),
    "counts only": dict(dmean=False, dstd=False, series=False, weight=False, mean=False, std=False),
    "below only": dict(NONE_OUT, below=True),
    "the error's statistics only": dict(NONE_OUT, dmean=True, dstd=True),
    "series only": dict(NONE_OUT, series=True),
    "weight only": dict(NONE_OUT, weight=True),
    "one region of one point": dict(npts=1, reg_off=(0, 1)),
    "a point per region": dict(npts=3, reg_off=(0, 1, 2, 3)),
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
    p = _lib.ptr
    off = np.array([0, 3, 2, 4], dtype=np.int64)
    assert L.td_rasterize_recovery(None, 3, p(off), *(p(c),) * 4, 0, None, pr) == 1
    assert L.td_last_error(None) == b"td_rasterize_recovery: offsets not monotone"
    off = np.array([1, 3], dtype=np.int64)
    assert L.td_rasterize_recovery(None, 1, p(off), *(p(c),) * 4, 0, None, pr) == 1
    assert b"td_rasterize_recovery: bad cell offsets" in L.td_last_error(None)
    for nm, po in ((0, p(off)), (-1, p(off)), (1, None)):
        assert L.td_rasterize_recovery(None, nm, po, *(p(c),) * 4, 0, None, pr) == 1
        assert L.td_last_error(None) == b"td_rasterize_recovery: need nmodels >= 1 and cell_off"
    hs = (ctypes.c_void_p * 1)(None)
    assert L.td_history_recovery(None, hs, 1, pr) == 1
    assert L.td_last_error(None) == b"td_history_recovery: a history is NULL"
    assert all(not keep[f].any() for f in OUTPUTS)  # a refused call wrote nothing
    del keep


def test_a_marginals_request_is_checked_as_the_volume_checks_it(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    probs = np.array([0.5, 1.5])
    quant = np.zeros((2, 2))
    marg = _lib.TdMarginals(2, _lib.ptr(probs), _lib.ptr(quant), 0, 0.0, 0.0, None)
    req, keep = request(_lib, marg=marg)
    both(tt, req, b"every probability must lie in [0, 1]")
    del keep


# ---------------------------------------------------------------- the binding

def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b((?:td|tdt)_\w+)\s*\(", src, flags=re.M))


def test_the_binding_table_covers_the_header_exactly(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    L = tt.lib()
    own = header_symbols("tdstar_recovery.h")
    assert own == {"td_rasterize_recovery", "td_history_recovery"} == set(_lib.SIGNATURES_RECOVERY)
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_INTERFACES) | set(_lib.SIGNATURES_REGIONS) | set(_lib.SIGNATURES_SUPPORT)
    assert not (own & others)
    for name, (res, args) in _lib.SIGNATURES_RECOVERY.items():
        f = getattr(L, name)
        assert f.restype is res and len(f.argtypes) == len(args), name
    # tdstar.h does not include the new header, and its ABI version did not move
    hdr = open(os.path.join(ROOT, "include", "tdstar.h")).read()
    assert "tdstar_recovery.h" not in hdr and re.search(r"#define TDSTAR_ABI_VERSION 2\b", hdr)
    for name in ("recovery", "recovery_history"):
        assert callable(getattr(tt.TdContext, name)), name
    for name in ("posterior_recovery", "checkerboard_model", "synthetic_data"):
        assert callable(getattr(tt, name)), name


def test_struct_layout_is_the_headers(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "tdstar_recovery.h")).read()
    body = re.search(r"typedef struct td_recovery \{(.*?)\} td_recovery;", hdr, re.S).group(1)
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
            got = [v.strip() for v in decl[len("int64_t "):].split(",")]
            names += got
            counts += got
    assert names == [f for f, _ in _lib.TdRecovery._fields_]
    assert counts == ["np", "nreg", "normalize"]
    assert all(t is (ctypes.c_int64 if f in counts else ctypes.c_void_p) for f, t in _lib.TdRecovery._fields_)
    assert ctypes.sizeof(_lib.TdRecovery) == 8 * len(names)
    assert [getattr(_lib.TdRecovery, f).offset for f in names] == [8 * k for k in range(len(names))]
