"""CPU: the host side of the posterior regions calls (td_rasterize_regions, td_history_regions): the numpy
restatement the GPU is compared against (tests/regions_ref.py) against plain loops, the inputs on which the
association matters, every argument check made before any HIP call, in the header's order, the binding, the plan
(tdt_regions_plan) and the Python layer's masks and weights."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest

import regions_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement against plain definitions

def loop_tree(a):
    """The sum of the Python floats a in td_rasterize's association, as an explicit tree."""
    n = len(a)

    def ltr(lo, hi):
        s = a[lo]
        for k in range(lo + 1, hi + 1):
            s = s + a[k]
        return s

    def impl(lo, hi):
        if hi - lo < 1024:
            return ltr(lo, hi)
        mid = (lo + hi) >> 1
        return impl(lo, mid) + impl(mid + 1, hi)

    return ltr(0, n - 1) if n < 16 else impl(0, n - 1)


@pytest.fixture(scope="module")
def base():
    models, px, py, pz, w, off = rref.base_case()
    ref = {(wt, nz): rref.regions(models, px, py, pz, off, w if wt else None, nz) for wt in (True, False) for nz in (True, False)}
    return dict(models=models, px=px, py=py, pz=pz, w=w, off=off, ref=ref)


def test_restatement_equals_plain_loops_over_explicit_trees(base):
    V, w, off = base["ref"][(True, True)]["values"], base["w"], base["off"]
    for normalize in (True, False):
        F, W = base["ref"][(True, normalize)]["series"], base["ref"][(True, normalize)]["weight"]
        for r in range(len(off) - 1):
            lo, hi = int(off[r]), int(off[r + 1])
            Wr = loop_tree([float(x) for x in w[lo:hi]])
            assert Wr == W[r]
            for m in (0, 17, 64):
                S = loop_tree([float(w[p]) * float(V[m][p]) for p in range(lo, hi)])
                assert (S / Wr if normalize else S) == F[m][r], (r, m)
    # w = None is an array of ones, bit for bit
    ones = rref.series(V, off, np.ones(len(w)), True)
    assert np.array_equal(ones[0], base["ref"][(False, True)]["series"]) and np.array_equal(ones[1], np.diff(off).astype(float))


def test_restatement_is_a_weighted_average(base):
    V, w, off = base["ref"][(True, True)]["values"], base["w"], base["off"]
    F = base["ref"][(True, True)]["series"]
    for r in range(len(off) - 1):
        lo, hi = int(off[r]), int(off[r + 1])
        plain = np.average(V[:, lo:hi], axis=1, weights=w[lo:hi])
        assert np.allclose(F[:, r], plain, rtol=1e-12, atol=0)


def test_greater_counts_every_model_once(base):
    for key, ref in base["ref"].items():
        F, g = ref["series"], ref["greater"]
        M, R = F.shape
        assert np.all(np.diag(g) == 0)
        for a in range(R):
            for b in range(R):
                ties = int(np.sum(~(F[:, a] > F[:, b]) & ~(F[:, b] > F[:, a])))
                assert g[a][b] + g[b][a] + ties == M
    # NaN and ties follow IEEE: neither side is greater
    F = np.array([[1.0, 1.0, np.nan], [2.0, 1.0, 0.0], [np.nan, np.nan, 3.0]])
    assert rref.greater(F).tolist() == [[0, 1, 1], [0, 0, 1], [0, 0, 0]]


def test_the_association_matters_on_the_base_case(base):
    """Above 1024 points the tree differs from the left-to-right sum in most models (61, 63 and 61 of 65 for the
    regions of 1025, 2049 and 3000 points), at or below it in none; all 65 series values of every region are
    distinct and every region's average is contested against all 11 partners: a kernel that sums in another order,
    or a test that compares constants, cannot pass."""
    ref = base["ref"][(True, False)]
    V, w, off = ref["values"], base["w"], base["off"]
    M = len(V)
    for r, n in enumerate(rref.BASE_SIZES):
        lo, hi = int(off[r]), int(off[r + 1])
        t = w[lo:hi] * V[:, lo:hi]
        s = t[:, 0].copy()
        for k in range(1, n):
            s = s + t[:, k]
        differ = int(np.sum(s != ref["series"][:, r]))
        print("region of %d points: %d of %d models differ from left to right" % (n, differ, M))
        assert differ == 0 if n <= 1024 else differ >= (M + 1) // 2
    for key, rf in base["ref"].items():
        F, g = rf["series"], rf["greater"]
        for r in range(F.shape[1]):
            assert len(set(F[:, r].tolist())) == M, (key, r)
            if not key[1]:  # (the plain sums grow with the region's size: only the averages can be contested)
                continue
            partners = np.delete(g[r], r)
            assert len(partners) == 11 and np.all((partners > 0) & (partners < M)), (key, r)


# ---------------------------------------------------------------- the refusals

def request(_lib, npts=6, reg_off=(0, 2, 6), nreg=None, px=None, py=None, pz=None, w=None, vec=(True,) * 3, off_ptr=True,
            npoints=None, normalize=1, series=True, weight=True, mean=True, std=True, greater=True, marg=None, conv=None):
    """A td_regions over small arrays; False leaves a pointer NULL.  -> (the struct, what it points into)."""
    p = _lib.ptr
    v = [np.asarray(a if a is not None else np.arange(max(npts, 1), dtype=np.float64), dtype=np.float64) for a in (px, py, pz)]
    off = np.asarray(reg_off, dtype=np.int64)
    R = max(len(off) - 1, 1)
    wv = np.asarray(w, dtype=np.float64) if w is not None else None
    keep = dict(v=v, off=off, w=wv, series=np.zeros((1, R)), weight=np.zeros(R), mean=np.zeros(R), std=np.zeros(R),
                greater=np.zeros((R, R), dtype=np.int64), marg=marg, conv=conv)
    r = _lib.TdRegions(*(p(a) if on else None for a, on in zip(v, vec)), p(wv), npts if npoints is None else npoints,
                       p(off) if off_ptr else None, len(off) - 1 if nreg is None else nreg, normalize,
                       p(keep["series"]) if series else None, p(keep["weight"]) if weight else None,
                       p(keep["mean"]) if mean else None, p(keep["std"]) if std else None,
                       p(keep["greater"]) if greater else None,
                       ctypes.addressof(marg) if marg is not None else None,
                       ctypes.addressof(conv) if conv is not None else None)
    return r, keep


def both(tt, req, words, chains=(0, None)):
    """Both entry points without a context (none can be made without a GPU), on one model of one cell and on no
    history: TD_ERR_ARG, and the message through td_last_error(NULL) names the entry point and holds `words`
    (a pair: td_rasterize_regions' and td_history_regions')."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    w1, w2 = words if isinstance(words, tuple) else (words, words)
    off = np.array([0, 1], dtype=np.int64)
    c = np.zeros(1)
    pr = ctypes.byref(req) if req is not None else None
    assert L.td_rasterize_regions(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, chains[0], _lib.ptr(chains[1]), pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_rasterize_regions: ") and w1 in msg, msg
    assert L.td_history_regions(None, None, 0, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_history_regions: ") and w2 in msg, msg


def conv_want(_lib, outputs=True):
    out = np.zeros(2)
    return _lib.TdConvergence(0, _lib.ptr(out) if outputs else None, None, None), out


NONE_OUT = dict(series=False, weight=False, mean=False, std=False, greater=False)
# in the header's order; each request is wrong in this way and in LATER ways, so the message shows which check ran first
ORDER = [
    ("struct NULL", None, b"want is NULL"),
    ("np < 1", dict(npoints=0, vec=(False,) * 3), b"np and nreg must be >= 1"),
    ("nreg < 1", dict(nreg=0, off_ptr=False), b"np and nreg must be >= 1"),
    ("px NULL", dict(vec=(False, True, True), reg_off=(1, 2, 6)), b"px, py, pz and reg_off must be given"),
    ("pz NULL", dict(vec=(True, True, False), normalize=2), b"px, py, pz and reg_off must be given"),
    ("reg_off NULL", dict(off_ptr=False, px=[np.nan] * 6), b"px, py, pz and reg_off must be given"),
    ("reg_off[0] != 0", dict(reg_off=(1, 2, 6), px=[np.nan] * 6), b"reg_off[0] must be 0"),
    ("reg_off not monotone", dict(reg_off=(0, 4, 2, 6), py=[np.inf] * 6), b"reg_off is not monotone"),
    ("an empty region", dict(reg_off=(0, 2, 2, 6), w=[np.nan] * 6), b"a region without points"),
    ("reg_off[nreg] below np", dict(reg_off=(0, 2, 5), normalize=-1), b"reg_off[nreg] must be np"),
    ("reg_off[nreg] above np", dict(reg_off=(0, 2, 7), normalize=-1), b"reg_off[nreg] must be np"),
    ("px NaN", dict(px=[0, 1, np.nan, 3, 4, 5], normalize=2), b"px is not finite"),
    ("py infinite", dict(py=[0, 1, 2, 3, 4, -np.inf], w=[np.nan] * 6), b"py is not finite"),
    ("pz NaN", dict(pz=[np.nan] * 6, **NONE_OUT), b"pz is not finite"),
    ("w infinite", dict(w=[1, 1, 1, np.inf, 1, 1], normalize=2), b"w is not finite"),
    ("w NaN", dict(w=[1, 1, 1, 1, 1, np.nan], **NONE_OUT), b"w is not finite"),
    ("normalize 2", dict(normalize=2, **NONE_OUT), b"normalize must be 0 or 1"),
    ("normalize -1", dict(normalize=-1, std=False), b"normalize must be 0 or 1"),
    ("no output", dict(**NONE_OUT), b"no output asked for"),
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
    assert L.td_rasterize_regions(None, 8, p(off), *(p(c),) * 4, 2, None, ctypes.byref(req)) == 1
    assert L.td_last_error(None) == b"td_rasterize_regions: chain_len is NULL"
    assert L.td_rasterize_regions(None, 7, p(off), *(p(c),) * 4, 2, p(lens), ctypes.byref(req)) == 1
    assert b"td_rasterize_regions: the chain lengths do not sum" in L.td_last_error(None)
    assert L.td_rasterize_regions(None, 8, p(off), *(p(c),) * 4, 2, p(lens), ctypes.byref(req)) == 1
    assert L.td_last_error(None) == b"td_rasterize_regions: offsets not monotone"
    del keep, held


LEGAL = {
    "everything": dict(),
    "weighted": dict(w=[1.0, -1.0, 0.5, 2.0, 1.0, 1.0]),
    "sums": dict(normalize=0),
    "series only": dict(weight=False, mean=False, std=False, greater=False),
    "greater only": dict(series=False, weight=False, mean=False, std=False),
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
    assert L.td_rasterize_regions(None, 3, p(off), *(p(c),) * 4, 0, None, pr) == 1
    assert L.td_last_error(None) == b"td_rasterize_regions: offsets not monotone"
    off = np.array([1, 3], dtype=np.int64)
    assert L.td_rasterize_regions(None, 1, p(off), *(p(c),) * 4, 0, None, pr) == 1
    assert b"td_rasterize_regions: bad cell offsets" in L.td_last_error(None)
    for nm, po in ((0, p(off)), (-1, p(off)), (1, None)):
        assert L.td_rasterize_regions(None, nm, po, *(p(c),) * 4, 0, None, pr) == 1
        assert L.td_last_error(None) == b"td_rasterize_regions: need nmodels >= 1 and cell_off"
    hs = (ctypes.c_void_p * 1)(None)
    assert L.td_history_regions(None, hs, 1, pr) == 1
    assert L.td_last_error(None) == b"td_history_regions: a history is NULL"
    # a refused call wrote nothing
    assert all(not keep[f].any() for f in ("series", "weight", "mean", "std", "greater"))
    del keep


def test_a_marginals_request_is_checked_as_the_volume_checks_it(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    probs = np.array([0.5, 1.5])
    quant = np.zeros((2, 2))
    marg = _lib.TdMarginals(2, _lib.ptr(probs), _lib.ptr(quant), 0, 0.0, 0.0, None)
    req, keep = request(_lib, marg=marg)
    both(tt, req, b"every probability must lie in [0, 1]")
    del keep


# ---------------------------------------------------------------- the binding and the plan

def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b((?:td|tdt)_\w+)\s*\(", src, flags=re.M))


def test_the_three_binding_tables_cover_the_four_headers_exactly(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    L = tt.lib()
    own = header_symbols("tdstar_regions.h")
    assert own == {"td_rasterize_regions", "td_history_regions", "tdt_regions_plan"}
    assert set(_lib.SIGNATURES_REGIONS) == own
    iface = header_symbols("tdstar_interfaces.h")
    assert set(_lib.SIGNATURES_INTERFACES) == iface
    older = header_symbols("tdstar.h") | header_symbols("tdstar_testing.h")
    assert set(_lib.SIGNATURES) == older
    assert not (own & older) and not (own & iface) and not (iface & older)
    for name, (res, args) in _lib.SIGNATURES_REGIONS.items():
        f = getattr(L, name)
        assert f.restype is res and len(f.argtypes) == len(args), name
    # tdstar.h does not include the new header, and its ABI version did not move
    hdr = open(os.path.join(ROOT, "include", "tdstar.h")).read()
    assert "tdstar_regions.h" not in hdr and re.search(r"#define TDSTAR_ABI_VERSION 2\b", hdr)
    for name in ("regions", "regions_history", "regions_plan"):
        assert callable(getattr(tt.TdContext, name)), name
    for name in ("posterior_regions", "depth_layers", "box_region", "voxel_weights", "region_points"):
        assert callable(getattr(tt, name)), name


def test_struct_layout_is_the_headers(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "tdstar_regions.h")).read()
    body = re.search(r"typedef struct td_regions \{(.*?)\} td_regions;", hdr, re.S).group(1)
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
    assert names == [f for f, _ in _lib.TdRegions._fields_]
    assert counts == ["np", "nreg", "normalize"]
    assert all(t is (ctypes.c_int64 if f in counts else ctypes.c_void_p) for f, t in _lib.TdRegions._fields_)
    assert ctypes.sizeof(_lib.TdRegions) == 8 * len(names)
    assert [getattr(_lib.TdRegions, f).offset for f in names] == [8 * k for k in range(len(names))]


def volume_plan_restated(M, nq, budget, forced):
    """volume_plan (csrc/volume.hip): the largest multiple of 64 nodes with 8 M nodes <= budget, or `forced`
    rounded down to one; at least 64, at most 2^18 and what one launch's blocks allow."""
    b = budget if budget > 0 else 1 << 30
    nodes = forced // 64 * 64 if forced > 0 else b // 8 // M // 64 * 64
    nodes = min(max(nodes, 64), 1 << 18)
    groups = 8 * ((M + 7) // 8)
    nodes = min(nodes, max(64, (2**31 - 1) // groups * 128))
    return nodes, (nq + nodes - 1) // nodes


@pytest.mark.parametrize("M,npts,budget,forced", [(65, 8347, 0, 0), (65, 8347, 0, 64), (65, 8347, 0, 128), (65, 8347, 0, 100),
                                                  (10000, 58 * 34 * 34, 0, 0), (1, 10**7, 0, 0), (3, 1, 0, 0),
                                                  (130, 8347, 8 * 130 * 700, 0), (10**6, 5000, 0, 0), (7, 999, 1, 0)])
def test_plan_is_the_volumes(tt, M, npts, budget, forced):
    got = tt.TdContext.regions_plan(M, npts, budget, forced)
    assert got == volume_plan_restated(M, npts, budget, forced) == tt.TdContext.volume_plan(M, npts, budget, forced)
    assert got[0] % 64 == 0 and got[0] * got[1] >= npts > got[0] * (got[1] - 1)


def test_plan_refusals(tt):
    L = tt.lib()
    out = np.zeros(2, dtype=np.int64)
    p = import_module("mcmc_in_tonga_amd._lib").ptr
    for bad in ((0, 1, 0, 0), (1, 0, 0, 0), (1, 1, -1, 0), (1, 1, 0, -1)):
        assert L.tdt_regions_plan(*bad, p(out)) == 1, bad
    assert L.tdt_regions_plan(1, 1, 0, 0, None) == 1


# ---------------------------------------------------------------- the Python layer

AXES = [
    (np.array([0.0, 10.0, 30.0, 35.0]), np.array([-5.0, 5.0]), np.array([0.0, 50.0, 150.0])),
    (np.array([3.0]), np.array([-5.0, 5.0, 6.0]), np.array([7.0])),  # axes of one node
]


@pytest.mark.parametrize("k", range(len(AXES)))
def test_voxel_weights_against_loops(tt, k):
    xs, ys, zs = AXES[k]

    def width(v, i):
        if len(v) == 1:
            return 1.0
        lo = v[0] if i == 0 else 0.5 * (v[i - 1] + v[i])
        hi = v[-1] if i == len(v) - 1 else 0.5 * (v[i] + v[i + 1])
        return hi - lo

    vol = tt.voxel_weights(xs, ys, zs)
    assert vol.shape == (len(xs), len(ys), len(zs))
    for i in range(len(xs)):
        for j in range(len(ys)):
            for kk in range(len(zs)):
                assert vol[i, j, kk] == (width(xs, i) * width(ys, j)) * width(zs, kk)
    # the voxels tile the hull of the nodes (an axis of one node counts 1)
    hull = np.prod([v[-1] - v[0] if len(v) > 1 else 1.0 for v in (xs, ys, zs)])
    assert np.isclose(vol.sum(), hull, rtol=1e-14)


def test_depth_layers_and_box_region_against_loops(tt):
    xs, ys, zs = AXES[0]
    layers = tt.depth_layers(zs, [0.0, 50.0, 100.0, 200.0])
    assert list(layers) == ["z 0-50", "z 50-100", "z 100-200"]
    for (lo, hi), mask in zip(((0, 50), (50, 100), (100, 200)), layers.values()):
        assert mask.shape == (1, 1, len(zs)) and mask.dtype == bool
        assert mask.ravel().tolist() == [bool(lo <= z < hi) for z in zs]
    assert list(tt.depth_layers(zs, [60.0, 100.0, 151.0])) == ["z 100-151"]  # a layer without a node is left out
    lo, hi = (5.0, -5.0, 50.0), (30.0, 0.0, 150.0)
    box = tt.box_region(xs, ys, zs, lo, hi)
    assert box.shape == (4, 2, 3) and box.dtype == bool
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            for k, z in enumerate(zs):
                assert box[i, j, k] == (lo[0] <= x <= hi[0] and lo[1] <= y <= hi[1] and lo[2] <= z <= hi[2])
    assert box.sum() == 2 * 1 * 2
    one = tt.box_region(*AXES[1], (0, 0, 0), (10, 10, 10))
    assert one.shape == (1, 3, 1) and one.ravel().tolist() == [False, True, True]


def test_region_points_orders_nodes_x_fastest_with_their_weights(tt):
    xs, ys, zs = AXES[0]
    vol = tt.voxel_weights(xs, ys, zs)
    box = tt.box_region(xs, ys, zs, (5.0, -5.0, 50.0), (35.0, 5.0, 150.0))
    regs = dict(tt.depth_layers(zs, [0.0, 100.0, 200.0]), box=box, path=([1.0, 2.0], [0.0, 0.0], [3.0, 4.0], [2.0, -1.0]),
                bare=([9.0], [8.0], [7.0]))
    names, px, py, pz, w, off = tt.region_points(regs, xs, ys, zs)
    assert names == ["z 0-100", "z 100-200", "box", "path", "bare"]
    want, wts = [], []
    for mask in (regs["z 0-100"], regs["z 100-200"], box):
        m = np.broadcast_to(mask, vol.shape)
        for k in range(len(zs)):
            for j in range(len(ys)):
                for i in range(len(xs)):
                    if m[i, j, k]:
                        want.append((xs[i], ys[j], zs[k]))
                        wts.append(vol[i, j, k])
    want += [(1.0, 0.0, 3.0), (2.0, 0.0, 4.0), (9.0, 8.0, 7.0)]
    wts += [2.0, -1.0, 1.0]
    assert list(zip(px, py, pz)) == want and w.tolist() == wts
    assert off.tolist() == [0, 16, 24, 36, 38, 39] and off.dtype == np.int64
    # plain averages: no weights at all unless a region brings its own
    assert tt.region_points(dict(box=box), xs, ys, zs, weights=None)[4] is None
    assert tt.region_points(regs, xs, ys, zs, weights=None)[4].tolist() == [1.0] * 36 + [2.0, -1.0, 1.0]
    with pytest.raises(ValueError, match="holds no point"):
        tt.region_points(dict(empty=np.zeros((4, 2, 3), dtype=bool)), xs, ys, zs)
    with pytest.raises(ValueError, match="weights"):
        tt.region_points(dict(box=box), xs, ys, zs, weights="mass")
