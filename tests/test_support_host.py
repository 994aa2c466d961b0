"""CPU: the posterior data support's restatement (tests/support_ref.py) against plain loops, the quantisation of the
weights (the restatement's and the library's own, tdt_support_quantise) on hostile inputs, the refusals of both entry
points in the header's order before any HIP call, the binding, and support_weights against the forward model."""
import ctypes
import math
import os
import re
from importlib import import_module

import numpy as np
import pytest

import support_ref as sref
from oracle import oracle_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement

def small_case(seed=3, P=60, sizes=(5, 0, 1, 9), metres=False):
    rng = np.random.default_rng(seed)
    s = 1e4 if metres else 1.0  # (metres: a box of 100 km, the sentinel reaches 31.6 km)
    pts = tuple(rng.uniform(0, 10, P) * s for _ in range(3))
    models = [tuple(rng.uniform(0, 10, n) * s for _ in range(3)) for n in sizes]
    nodes = tuple(rng.uniform(0, 10, 17) * s for _ in range(3))
    return pts, models, nodes, rng.normal(0.0, 1.0, P)


def loops(models, pts, w, nodes, thr):
    """The definition with one Python loop per sum and per search: strict <, the first minimum, the 1e9 sentinel."""
    P = len(pts[0])
    if w is None:
        k, e = [1] * P, 0
    else:
        A = 0.0
        for v in w:
            A = A + abs(float(v))
        e = 0 if A == 0.0 else 61 - math.frexp(A)[1]
        k = [int(np.rint(math.ldexp(float(v), e))) for v in w]

    def nearest(x, y, z, cells):
        best, bi = 1e9, -1
        for i in range(len(cells[0])):
            dx, dy, dz = cells[0][i] - x, cells[1][i] - y, cells[2][i] - z
            d = (dx * dx + dy * dy) + dz * dz
            if d < best:
                best, bi = d, i
        return bi

    cell, count, barren, orphans, U = [], [], [], [], []
    for cells in models:
        nc = len(cells[0])
        K, C, lost = [0] * nc, [0] * nc, 0
        for p in range(P):
            i = nearest(pts[0][p], pts[1][p], pts[2][p], cells)
            if i < 0:
                lost += 1
            else:
                K[i] += k[p]  # (Python integers: exact)
                C[i] += 1
        sup = [math.ldexp(float(v), -e) for v in K]
        cell += sup
        count += C
        barren.append(sum(1 for c in C if c == 0))
        orphans.append(lost)
        row = []
        for q in range(len(nodes[0])):
            i = nearest(nodes[0][q], nodes[1][q], nodes[2][q], cells)
            row.append(sup[i] if i >= 0 else 0.0)
        U.append(row)
    exceed = [[sum(1 for m in range(len(models)) if U[m][q] > t) for q in range(len(nodes[0]))] for t in thr]
    return dict(cell=np.array(cell), count=np.array(count, dtype=np.int64), barren=np.array(barren, dtype=np.int64),
                orphans=np.array(orphans, dtype=np.int64), values=np.array(U), exceed=np.array(exceed, dtype=np.int64))


@pytest.mark.parametrize("metres", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_equals_plain_loops(metres, weighted):
    pts, models, nodes, w = small_case(metres=metres)
    w = w if weighted else None
    thr = (0.0, 1.0, -0.5)
    ref = sref.support(models, *pts, w, *nodes, thr=thr)
    want = loops(models, pts, w, nodes, thr)
    for f in want:
        assert ref[f].dtype == want[f].dtype and np.array_equal(ref[f], want[f]), f
    if metres:  # the one cell of model 2 reaches some points and not others
        assert 0 < ref["orphans"][2] < len(pts[0])
    else:
        assert not ref["orphans"][[0, 2, 3]].any()
    assert ref["orphans"][1] == len(pts[0]) and not ref["values"][1].any()  # the model without cells
    assert ref["count"][5] == len(pts[0]) - ref["orphans"][2]  # the model of one cell owns what it can reach


def test_null_weights_are_an_array_of_ones():
    """k = 1, e = 0 against k = 2^(61 - E), e = 61 - E: the same sup, bit for bit, because count < 2^E."""
    pts, models, nodes, _ = small_case(P=777)
    a = sref.support(models, *pts, None, *nodes, thr=(0.0, 3.0))
    b = sref.support(models, *pts, np.ones(777), *nodes, thr=(0.0, 3.0))
    assert a["e"] == 0 and b["e"] == 61 - 10 and np.all(b["k"] == 1 << 51)
    for f in ("cell", "count", "barren", "orphans", "values", "mean", "std", "exceed"):
        assert np.array_equal(a[f], b[f]), f
    assert np.array_equal(a["cell"], a["count"].astype(np.float64))


@pytest.mark.parametrize("metres", [False, True])
def test_conservation_per_model(metres):
    pts, models, nodes, w = small_case(seed=5, P=300, sizes=(7, 0, 1, 30, 2), metres=metres)
    r = sref.support(models, *pts, w)
    off = np.concatenate(([0], np.cumsum([len(m[0]) for m in models])))
    P = len(pts[0])
    for m, cells in enumerate(models):
        own = sref.owners(cells, *pts)
        cnt = r["count"][off[m]:off[m + 1]]
        assert cnt.sum() + r["orphans"][m] == P
        assert r["barren"][m] == np.sum(cnt == 0)
        # the integer sums themselves: every owned point's k, once
        Kref = np.zeros(len(cells[0]), dtype=np.int64)
        for p in np.flatnonzero(own >= 0):
            Kref[own[p]] += r["k"][p]
        assert Kref.sum() == r["k"][own >= 0].sum()
        assert np.array_equal(np.ldexp(Kref.astype(np.float64), -r["e"]), r["cell"][off[m]:off[m + 1]])


# ---------------------------------------------------------------- the quantisation

def c_quantise(tt, w):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    w = np.ascontiguousarray(w, dtype=np.float64)
    k = np.full(len(w), -7, dtype=np.int64)
    e = ctypes.c_int64(-7)
    rc = tt.lib().tdt_support_quantise(_lib.ptr(w), len(w), _lib.ptr(k, _lib._pi64), ctypes.byref(e))
    return rc, k, e.value


HOSTILE = {
    "tiny beside one": [1.0, 1e-300, 1.0, 5e-324],
    "mixed signs": [3.5, -2.25, 1e-3, -1e3, 0.0, 7.0],
    "all zero": [0.0, -0.0, 0.0],
    "ties go to even": [1.0, 2.0 ** -61, 3 * 2.0 ** -61, -(2.0 ** -61), -3 * 2.0 ** -61, 5 * 2.0 ** -61],
    "huge": [1e300, -3e299, 1e-300],
    "subnormal only": [5e-324, -1e-323, 2e-320],
    "one weight": [0.1],
    "thousands": list(np.random.default_rng(9).normal(0, 1, 5000)),
    "cancelling": [1.0, -1.0] * 50,
}


@pytest.mark.parametrize("case", sorted(HOSTILE))
def test_quantisation_on_hostile_weights(tt, case):
    w = np.array(HOSTILE[case], dtype=np.float64)
    k, e = sref.quantise(w, len(w))
    rc, kc, ec = c_quantise(tt, w)
    assert rc == 0 and ec == e and np.array_equal(kc, k), (e, ec)
    A = float(np.sum(np.abs(w)))
    total = sum(abs(int(v)) for v in k)
    assert total < (1 << 61) + len(w)  # the int64 sums cannot overflow (A's own rounding is far below that here)
    if A > 0:
        assert total >= (1 << 60) - len(w)  # and the 61 bits are used
        back = np.ldexp(k.astype(np.float64), -e)
        assert np.all(np.abs(back - w) <= np.ldexp(0.5, -e) + np.abs(w) * 2.0 ** -52)
        assert np.all(np.sign(back) * np.sign(w) >= 0)
    else:
        assert e == 0 and not k.any()
    if case == "tiny beside one":
        assert e == 59 and list(k) == [1 << 59, 0, 1 << 59, 0]  # a weight below 2^(-e-1) supports nothing
    if case == "ties go to even":
        assert e == 60 and list(k) == [1 << 60, 0, 2, 0, -2, 2]
    if case == "cancelling":
        assert int(k.sum()) == 0


def test_quantisation_refuses_what_is_not_finite(tt):
    for w in ([1.0, np.nan], [np.inf, 1.0], [-np.inf], [1e308, 1e308]):
        rc, k, e = c_quantise(tt, w)
        assert rc == 1 and e == -7 and np.all(k == -7), w
    rc, k, e = c_quantise(tt, np.zeros(0))
    assert rc == 0 and e == 0
    assert tt.TdContext.support_lds_cells() == tt.lib().tdt_support_lds_cells() == 5120
    assert tt.lib().tdt_set_support_scatter(None, 1) == 1  # (no context)


# ---------------------------------------------------------------- the refusals

def request(_lib, nq=4, qx=None, qy=None, qz=None, vec=(True,) * 3, thr=(0.0,), nthr=None, thr_ptr=True, w=None,
            cell=True, count=True, barren=True, orphans=True, values=True, mean=True, std=True, exceed=True, marg=None,
            conv=None):
    """A td_support over small arrays; False leaves a pointer NULL.  -> (the struct, what it points into)."""
    p = _lib.ptr
    v = [np.asarray(a if a is not None else np.arange(max(nq, 1), dtype=np.float64), dtype=np.float64) for a in (qx, qy, qz)]
    t = np.asarray(thr, dtype=np.float64)
    wv = np.asarray(w, dtype=np.float64) if w is not None else None
    n = max(nq, 1)
    keep = dict(v=v, t=t, w=wv, cell=np.zeros(1), count=np.zeros(1, dtype=np.int64), barren=np.zeros(1, dtype=np.int64),
                orphans=np.zeros(1, dtype=np.int64), values=np.zeros((1, n)), mean=np.zeros(n), std=np.zeros(n),
                exceed=np.zeros((max(len(t), 1), n), dtype=np.int64), marg=marg, conv=conv)
    on = dict(cell=cell, count=count, barren=barren, orphans=orphans, values=values, mean=mean, std=std, exceed=exceed)
    out = {f: (p(keep[f]) if on[f] else None) for f in on}
    r = _lib.TdSupport(p(wv), *(p(a) if use else None for a, use in zip(v, vec)), nq, p(t) if thr_ptr else None,
                       len(t) if nthr is None else nthr, out["cell"], out["count"], out["barren"], out["orphans"],
                       out["values"], out["mean"], out["std"], out["exceed"],
                       ctypes.addressof(marg) if marg is not None else None,
                       ctypes.addressof(conv) if conv is not None else None)
    return r, keep


def both(tt, req, words, chains=(0, None)):
    """Both entry points without a context (none can be made without a GPU), on one model of one cell and on no
    history: TD_ERR_ARG, and the message through td_last_error(NULL) names the entry point and holds `words` (a pair:
    td_rasterize_support's and td_history_support's)."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    w1, w2 = words if isinstance(words, tuple) else (words, words)
    off = np.array([0, 1], dtype=np.int64)
    c = np.zeros(1)
    pr = ctypes.byref(req) if req is not None else None
    assert L.td_rasterize_support(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 3, chains[0], _lib.ptr(chains[1]), pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_rasterize_support: ") and w1 in msg, msg
    assert L.td_history_support(None, None, 0, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_history_support: ") and w2 in msg, msg


def conv_want(_lib, outputs=True):
    out = np.zeros(4)
    return _lib.TdConvergence(0, _lib.ptr(out) if outputs else None, None, None), out


NODE_OUT = dict(values=False, mean=False, std=False, thr=(), exceed=False)
NONE_OUT = dict(cell=False, count=False, barren=False, orphans=False, **NODE_OUT)
# in the header's order; each request is wrong in this way and in LATER ways, so the message shows which check ran first
ORDER = [
    ("struct NULL", None, b"want is NULL"),
    ("nq < 0", dict(nq=-1, nthr=-1), b"nq must be >= 0"),
    ("qx NULL", dict(vec=(False, True, True), nthr=-1), b"qx, qy and qz must be given for nq > 0"),
    ("qz NULL", dict(vec=(True, True, False), thr_ptr=False), b"qx, qy and qz must be given for nq > 0"),
    ("nthr < 0", dict(nthr=-2, qx=[np.nan] * 4), b"nthr must be >= 0"),
    ("thr NULL", dict(thr_ptr=False, qx=[np.nan] * 4), b"thr and exceed_out must be given for nthr > 0"),
    ("exceed_out NULL", dict(exceed=False, qy=[np.inf] * 4), b"thr and exceed_out must be given for nthr > 0"),
    ("qx NaN", dict(qx=[0, 1, np.nan, 3], qy=[np.nan] * 4), b"qx is not finite"),
    ("qy infinite", dict(qy=[0, 1, 2, -np.inf], qz=[np.nan] * 4), b"qy is not finite"),
    ("qz NaN", dict(qz=[np.nan] * 4, thr=(np.nan,)), b"qz is not finite"),
    ("thr NaN", dict(thr=(0.0, np.nan), std=False), b"thr is not finite"),
    ("thr infinite", dict(thr=(np.inf,), **{k: False for k in ("cell", "count", "barren", "orphans", "values", "mean", "std")}),
     b"thr is not finite"),
    ("std alone", dict(std=True, **{k: v for k, v in NONE_OUT.items() if k != "std"}), b"mean_out and std_out"),
    ("nothing at all", dict(**NONE_OUT), b"no output asked for"),
    ("nothing, no nodes", dict(nq=0, **NONE_OUT), b"no output asked for"),
    ("values without nodes", dict(nq=0, thr=(), exceed=False, mean=False), b"an output that needs nodes with nq == 0"),
    ("thresholds without nodes", dict(nq=0, values=False, mean=False, std=False), b"an output that needs nodes with nq == 0"),
    ("conv without nodes", dict(nq=0, conv="empty", **NODE_OUT), b"an output that needs nodes with nq == 0"),
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
    del keep, held


LEGAL = {
    "everything": dict(),
    "no nodes": dict(nq=0, **NODE_OUT),
    "nodes nobody reads": dict(**NODE_OUT),
    "counts only": dict(cell=False, barren=False, orphans=False, **NODE_OUT),
    "thresholds only": dict(cell=False, count=False, barren=False, orphans=False, values=False, mean=False, std=False),
    # (without a context the weights are not read: they hold P numbers, and P is the context's)
    "weights without a context": dict(w=[np.nan, np.inf]),
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
    assert L.td_rasterize_support(None, 3, p(off), *(p(c),) * 3, 0, None, pr) == 1
    assert L.td_last_error(None) == b"td_rasterize_support: offsets not monotone"
    off = np.array([1, 3], dtype=np.int64)
    assert L.td_rasterize_support(None, 1, p(off), *(p(c),) * 3, 0, None, pr) == 1
    assert b"td_rasterize_support: bad cell offsets" in L.td_last_error(None)
    for nm, po in ((0, p(off)), (-1, p(off)), (1, None)):
        assert L.td_rasterize_support(None, nm, po, *(p(c),) * 3, 0, None, pr) == 1
        assert L.td_last_error(None) == b"td_rasterize_support: need nmodels >= 1 and cell_off"
    hs = (ctypes.c_void_p * 1)(None)
    assert L.td_history_support(None, hs, 1, pr) == 1
    assert L.td_last_error(None) == b"td_history_support: a history is NULL"
    # a refused call wrote nothing
    assert all(not keep[f].any() for f in ("cell", "count", "barren", "orphans", "values", "mean", "std", "exceed"))
    del keep


def test_conv_with_bad_chains_is_refused_before_the_models(tt):
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    cw, held = conv_want(_lib)
    req, keep = request(_lib, conv=cw)
    lens = np.array([4, 4], dtype=np.int64)
    off = np.array([0, 3, 2, 4, 5, 6, 7, 8, 9], dtype=np.int64)  # (not monotone: a later check)
    c = np.zeros(9)
    p = _lib.ptr
    assert L.td_rasterize_support(None, 8, p(off), *(p(c),) * 3, 2, None, ctypes.byref(req)) == 1
    assert L.td_last_error(None) == b"td_rasterize_support: chain_len is NULL"
    assert L.td_rasterize_support(None, 7, p(off), *(p(c),) * 3, 2, p(lens), ctypes.byref(req)) == 1
    assert b"td_rasterize_support: the chain lengths do not sum" in L.td_last_error(None)
    assert L.td_rasterize_support(None, 8, p(off), *(p(c),) * 3, 2, p(lens), ctypes.byref(req)) == 1
    assert L.td_last_error(None) == b"td_rasterize_support: offsets not monotone"
    del keep, held


def test_a_marginals_request_is_checked_as_the_volume_checks_it(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    probs = np.array([0.5, 1.5])
    quant = np.zeros((2, 4))
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
    own = header_symbols("tdstar_support.h")
    assert own == {"td_rasterize_support", "td_history_support", "tdt_support_lds_cells", "tdt_set_support_scatter",
                   "tdt_support_quantise"}
    assert set(_lib.SIGNATURES_SUPPORT) == own
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_INTERFACES) | set(_lib.SIGNATURES_REGIONS)
    assert not (own & others)
    for name, (res, args) in _lib.SIGNATURES_SUPPORT.items():
        f = getattr(L, name)
        assert f.restype is res and len(f.argtypes) == len(args), name
    # tdstar.h does not include the new header, and its ABI version did not move
    hdr = open(os.path.join(ROOT, "include", "tdstar.h")).read()
    assert "tdstar_support.h" not in hdr and re.search(r"#define TDSTAR_ABI_VERSION 2\b", hdr)
    for name in ("support", "support_history", "support_lds_cells", "set_support_scatter"):
        assert callable(getattr(tt.TdContext, name)), name
    for name in ("posterior_support", "support_weights", "ray_density"):
        assert callable(getattr(tt, name)), name


def test_struct_layout_is_the_headers(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "tdstar_support.h")).read()
    body = re.search(r"typedef struct td_support \{(.*?)\} td_support;", hdr, re.S).group(1)
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
    assert names == [f for f, _ in _lib.TdSupport._fields_]
    assert counts == ["nq", "nthr"]
    assert all(t is (ctypes.c_int64 if f in counts else ctypes.c_void_p) for f, t in _lib.TdSupport._fields_)
    assert ctypes.sizeof(_lib.TdSupport) == 8 * len(names)
    assert [getattr(_lib.TdSupport, f).offset for f in names] == [8 * k for k in range(len(names))]


# ---------------------------------------------------------------- the weights

def test_support_weights_count_and_kinds(tt, ds):
    assert tt.support_weights(ds, "count") is None
    with pytest.raises(ValueError):
        tt.support_weights(ds, "fisher")
    npts, px, py, pz = sref.csr_points(ds.rayX, ds.rayY, ds.rayZ)
    for kind in ("tstar", "length"):
        w = tt.support_weights(ds, kind)
        assert w.shape == (npts.sum(),) and np.all(w >= 0) and np.all(np.isfinite(w))
    # "length": every ray's weights sum to its length
    length = tt.support_weights(ds, "length")
    off = np.concatenate(([0], np.cumsum(npts)))
    for i in (0, 17, 380):
        assert np.isclose(length[off[i]:off[i + 1]].sum(), np.nansum(ds.rayL[:npts[i] - 1, i]), rtol=1e-13)


@pytest.mark.parametrize("ncells,seed", [(200, 1), (1000, 2), (1, 4)])
def test_tstar_weights_give_the_sum_of_the_predicted_data(tt, ds, ncells, seed):
    """sum over the points of g[p] * zeta(owner of p) is the sum of ptS over the rays (MCsub.jl:147-160): two
    associations of the same sum, so to 1e-12 relative and not bit for bit."""
    npts, px, py, pz = sref.csr_points(ds.rayX, ds.rayY, ds.rayZ)
    seg = np.concatenate([np.concatenate([ds.rayL[:c - 1, i] * ds.rayU[:c - 1, i], [0.0]]) if c > 0 else []
                          for i, c in enumerate(npts)])
    cells = tt.random_model(ncells, seed).cells()
    ptS, _, _, idx = oracle_np.evaluate_csr(npts, px, py, pz, seg, ds.tS, ds.allSig, cells)
    g = tt.support_weights(ds, "tstar")
    zeta = np.where(idx >= 0, np.asarray(cells[3])[np.maximum(idx, 0)], 0.0)
    total = math.fsum(g * zeta)
    assert abs(total - math.fsum(ptS)) <= 1e-12 * math.fsum(ptS) and total > 0
    # and a cell's support is the derivative of that sum with respect to its zeta: linear, so exact up to rounding
    r = sref.support([cells], px, py, pz, g)
    assert abs(math.fsum(r["cell"] * np.asarray(cells[3])) - total) <= 1e-12 * total
