"""CPU: the host side of the posterior interfaces calls (td_rasterize_interfaces, td_history_interfaces): the numpy
restatement the GPU is compared against (tests/interfaces_ref.py) against plain definitions, the halo plan
(tdt_interfaces_plan), every argument check made before any HIP call, in the header's order, and the binding."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest

import interfaces_ref as iref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX_LO, BOX_HI = np.array([0.0, -200.0, 0.0]), np.array([1000.0, 400.0, 660.0])


def uniform_models(M, seed, lo=3, hi=12):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(M):
        n = int(rng.integers(lo, hi + 1))
        p = BOX_LO + rng.random((n, 3)) * (BOX_HI - BOX_LO)
        out.append((p[:, 0], p[:, 1], p[:, 2], rng.uniform(0, 50, n)))
    return out


def axes(nx, ny, nz):
    return np.linspace(0.0, 1000.0, nx), np.linspace(-200.0, 400.0, ny), np.linspace(0.0, 660.0, nz)


# ---------------------------------------------------------------- the restatement against plain definitions

@pytest.mark.parametrize("M", [17, 2500])
def test_jump_is_the_mean_absolute_difference(M):
    nx, ny, nz = 5, 4, 3
    ref = iref.interfaces(uniform_models(M, 100 + M), *axes(nx, ny, nz), thresholds=(0.0, 5.0, 25.0))
    V = ref["values"].reshape(M, nz, ny, nx)
    nfaces, mid, zero = iref.contested(ref, M)
    print("M = %d: %d faces, %d with 0 < count < M, %d with count == 0" % (M, nfaces, mid, zero))
    assert nfaces == 133 and mid > nfaces // 2
    for a, axis in enumerate((3, 2, 1)):  # x is the last axis of V[M][nz][ny][nx]
        plain = np.mean(np.abs(np.diff(V, axis=axis)), axis=0)  # [nz][ny][nx] minus one along the axis
        jump = ref["jump"][a].reshape(nz, ny, nx)
        has = ~np.isnan(jump)
        assert has.sum() == plain.size and np.allclose(jump[has], plain.ravel(), rtol=1e-12, atol=0)
        count = ref["count"][a].reshape(nz, ny, nx)
        assert np.array_equal(count[has], np.sum(np.diff(V, axis=axis) != 0, axis=0).ravel())
        assert np.all(count[~has] == -1)
        # |d| > 0 is "differs"; the thresholds only lose models
        assert np.array_equal(ref["exceed"][0][a], ref["count"][a])
        assert np.all(ref["exceed"][1][a] <= ref["exceed"][0][a]) and np.all(ref["exceed"][2][a] <= ref["exceed"][1][a])
    assert np.all(ref["any"] >= ref["count"].max(axis=0)) and np.all(ref["any"] <= np.maximum(ref["count"], 0).sum(axis=0))
    assert ref["any"][-1] == -1 and np.sum(ref["any"] == -1) == 1  # the last node alone has no forward face


def test_counts_against_a_triple_loop():
    nx, ny, nz = 3, 2, 2
    M = 9
    xs, ys, zs = axes(nx, ny, nz)
    models = uniform_models(M, 7)
    thr = (0.0, 10.0)
    ref = iref.interfaces(models, xs, ys, zs, thr)
    V = ref["values"]
    count = np.full((3, nx * ny * nz), -1, dtype=np.int64)
    anyc = np.full(nx * ny * nz, -1, dtype=np.int64)
    exceed = np.full((2, 3, nx * ny * nz), -1, dtype=np.int64)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                n = i + nx * (j + ny * k)
                nb = [(i + 1 < nx, n + 1), (j + 1 < ny, n + nx), (k + 1 < nz, n + nx * ny)]
                if any(h for h, _ in nb):
                    anyc[n] = sum(1 for m in range(M) if any(h and V[m][n] != V[m][o] for h, o in nb))
                for a, (h, o) in enumerate(nb):
                    if h:
                        count[a][n] = sum(1 for m in range(M) if V[m][n] != V[m][o])
                        for t in range(2):
                            exceed[t][a][n] = sum(1 for m in range(M) if abs(V[m][o] - V[m][n]) > thr[t])
    assert np.array_equal(ref["count"], count) and np.array_equal(ref["any"], anyc) and np.array_equal(ref["exceed"], exceed)
    assert (count > 0).any()


def test_nan_and_equal_values_follow_ieee():
    """A NaN value differs from everything (itself included) and exceeds nothing; equal columns give 0 and 0.0."""
    V = np.array([[1.0, 1.0, np.nan, 4.0], [2.0, 2.0, 3.0, 3.0]])
    count, anyc, exceed, jump = iref.face_statistics(V, 4, 1, 1, (0.5,))
    assert count[0].tolist() == [0, 2, 1, -1] and anyc.tolist() == [0, 2, 1, -1]
    assert exceed[0][0].tolist() == [0, 1, 0, -1]  # |NaN| exceeds nothing; 2 -> 3 exceeds 0.5; 3 -> 3 does not
    assert jump[0][0] == 0.0 and np.isnan(jump[0][1]) and np.isnan(jump[0][2]) and np.isnan(jump[0][3])
    assert np.all(count[1:] == -1) and np.isnan(jump[1:]).all()
    exceed = iref.face_statistics(np.array([[1.0, 2.0, 3.5]]), 3, 1, 1, (0.5, 1.0))[2]
    assert exceed[:, 0, :].tolist() == [[1, 1, -1], [0, 1, -1]]


def test_density_against_the_loop_and_its_sum():
    xs, ys, zs = np.array([0.0, 10.0, 30.0]), np.array([-5.0, 5.0]), np.array([7.0])
    x = np.array([-1e9, 4.99, 5.0, 5.01, 20.0, 19.99, 31.0, np.inf, -np.inf, np.nan, 1.0, 2.0])
    y = np.array([0.0, 0.0, 0.0, -0.1, 0.0, 1e300, -1e300, 0.0, 0.0, 0.0, np.nan, 0.0])
    z = np.array([7.0, 0.0, 1e9, -1e9, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, np.nan])
    models = [(x[:5], y[:5], z[:5], np.zeros(5)), (np.zeros(0),) * 4, (x[5:], y[5:], z[5:], np.full(7, np.nan))]
    dens, skipped = iref.density(models, xs, ys, zs)
    loop = np.zeros(6, dtype=np.int64)
    skip = 0
    for cx, cy, cz in zip(x, y, z):
        if cx != cx or cy != cy or cz != cz:
            skip += 1
            continue
        i = sum(1 for m in (5.0, 20.0) if m <= cx)
        j = sum(1 for m in (0.0,) if m <= cy)
        loop[i + 3 * j] += 1  # (one node along z: 0)
    assert np.array_equal(dens, loop) and skipped == skip == 3
    assert dens.sum() + skipped == len(x)
    # by hand: a cell on a midpoint (x = 5.0, x = 20.0, y = 0.0) belongs to the upper voxel, -inf and -1e9 to the
    # first, +inf and 31 to the last
    assert dens.tolist() == [0, 1, 1, 3, 2, 2]


# ---------------------------------------------------------------- the halo plan

def plan(tt, M, nx, ny, nz, budget=0, forced=0):
    return tt.TdContext.interfaces_plan(M, nx, ny, nz, budget, forced)


def slab_columns(nx, ny, nz, q0, nodes):
    """The documented column set of the slab that owns [q0, q0 + nodes): its nodes and halo, as sorted node ids."""
    nq, sxy = nx * ny * nz, nx * ny
    ns = min(nodes, nq - q0)
    h = nx if ny > 1 else (1 if nx > 1 else 0)
    r1 = range(q0, min(q0 + ns + h, nq))
    r2 = range(min(q0 + sxy, nq), min(q0 + ns + sxy, nq)) if nz > 1 else range(0)
    return ns, sorted(set(r1) | set(r2))


LATTICES = [(7, 6, 5), (20, 9, 3), (5, 4, 3), (1, 1, 1), (6, 1, 4), (1, 5, 1), (1, 1, 300), (300, 1, 1), (3, 70, 2),
            (58, 34, 34)]


@pytest.mark.parametrize("shape", LATTICES)
@pytest.mark.parametrize("forced", [64, 128, 0])
def test_plan_tiles_the_lattice_and_holds_every_neighbour(tt, shape, forced):
    nx, ny, nz = shape
    nq = nx * ny * nz
    M = 16
    budget = 8 * M * 700 if not forced else 0  # (auto: a budget of 700 columns, so that there are several slabs)
    nodes, nslabs, maxcols = plan(tt, M, nx, ny, nz, budget, forced)
    assert nodes % 64 == 0 and nodes >= 64
    if forced:
        assert nodes == forced
    owned = []
    most = 0
    for s in range(nslabs):
        q0 = s * nodes
        ns, cols = slab_columns(nx, ny, nz, q0, nodes)
        assert ns >= 1
        owned += list(range(q0, q0 + ns))
        colset = set(cols)
        for n in range(q0, q0 + ns):
            i, j, k = n % nx, (n // nx) % ny, n // (nx * ny)
            assert n in colset
            assert i + 1 >= nx or n + 1 in colset
            assert j + 1 >= ny or n + nx in colset
            assert k + 1 >= nz or n + nx * ny in colset
        most = max(most, len(cols))
        h = nx if ny > 1 else (1 if nx > 1 else 0)
        assert len(cols) <= 2 * ns + h
    assert owned == list(range(nq))  # the owned ranges tile [0, nq) without overlap
    assert most == maxcols
    if not forced:
        h = nx if ny > 1 else (1 if nx > 1 else 0)
        if 2 * 64 + h <= 700:  # the smallest slab allows it
            assert 8 * M * maxcols <= budget
            # and the slab is the largest that does
            assert nodes == (700 - h) // 2 // 64 * 64


def test_plan_defaults_and_refusals(tt):
    L = tt.lib()
    # the shipped lattice, 10^4 samples, 1 GiB: 13 421 columns
    nodes, nslabs, maxcols = plan(tt, 10000, 58, 34, 34)
    assert nodes == (13421 - 58) // 2 // 64 * 64 == 6656 and nslabs == -(-58 * 34 * 34 // 6656)
    assert 8 * 10000 * maxcols <= 1 << 30 and maxcols == 6656 + 58 * 34  # (the plane is smaller than the slab: one range)
    # few models: the slab's ceiling on columns, 2^18
    nodes, _, maxcols = plan(tt, 1, 58, 34, 34)
    assert nodes == ((1 << 18) - 58) // 2 // 64 * 64 and maxcols == 58 * 34 * 34
    out = np.zeros(3, dtype=np.int64)
    p = import_module("mcmc_in_tonga_amd._lib").ptr
    for bad in ((0, 1, 1, 1, 0, 0), (1, 0, 1, 1, 0, 0), (1, 1, 0, 1, 0, 0), (1, 1, 1, 0, 0, 0), (1, 1, 1, 1, -1, 0),
                (1, 1, 1, 1, 0, -1), (1, 1 << 31, 1 << 31, 1 << 31, 0, 0)):
        assert L.tdt_interfaces_plan(*bad, p(out)) == 1, bad
    assert L.tdt_interfaces_plan(1, 1, 1, 1, 0, 0, None) == 1


# ---------------------------------------------------------------- the refusals

def request(_lib, nx=3, ny=2, nz=2, xs=None, ys=None, zs=None, vec=(True,) * 3, thr=(5.0,), thr_ptr=True, nthr=None,
            count=True, any_=True, exceed=None, jump=True, mean=True, std=True, density=True, skipped=True):
    """A td_interfaces over small arrays; False leaves a pointer NULL.  -> (the struct, what it points into)."""
    p = _lib.ptr
    v = [np.asarray(a if a is not None else np.arange(max(n, 1), dtype=np.float64), dtype=np.float64)
         for a, n in ((xs, nx), (ys, ny), (zs, nz))]
    nq = max(nx, 1) * max(ny, 1) * max(nz, 1)
    t = np.asarray(thr, dtype=np.float64)
    nthr = len(t) if nthr is None else nthr
    exceed = (nthr > 0) if exceed is None else exceed
    i64 = lambda *s: np.zeros(s, dtype=np.int64)  # noqa: E731
    keep = dict(v=v, t=t, count=i64(3, nq), any=i64(nq), exceed=i64(max(nthr, 1), 3, nq), jump=np.zeros((3, nq)),
                mean=np.zeros(nq), std=np.zeros(nq), density=i64(nq), skipped=i64(1))
    r = _lib.TdInterfaces(*(p(a) if on else None for a, on in zip(v, vec)), nx, ny, nz, p(t) if thr_ptr and len(t) else None,
                          nthr, p(keep["count"]) if count else None, p(keep["any"]) if any_ else None,
                          p(keep["exceed"]) if exceed else None, p(keep["jump"]) if jump else None,
                          p(keep["mean"]) if mean else None, p(keep["std"]) if std else None,
                          p(keep["density"]) if density else None, p(keep["skipped"]) if skipped else None)
    return r, keep


def both(tt, req, words):
    """Both entry points without a context (none can be made without a GPU), on one model of one cell and on no
    history: TD_ERR_ARG, and the message through td_last_error(NULL) names the entry point and holds `words`
    (a pair: td_rasterize_interfaces' and td_history_interfaces')."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    w1, w2 = words if isinstance(words, tuple) else (words, words)
    off = np.array([0, 1], dtype=np.int64)
    c = np.zeros(1)
    pr = ctypes.byref(req) if req is not None else None
    assert L.td_rasterize_interfaces(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_rasterize_interfaces: ") and w1 in msg, msg
    assert L.td_history_interfaces(None, None, 0, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_history_interfaces: ") and w2 in msg, msg


NONE_OUT = dict(count=False, any_=False, jump=False, mean=False, std=False, density=False, skipped=False)
# in the header's order; each request is wrong in this way and in LATER ways, so the message shows which check ran first
ORDER = [
    ("struct NULL", None, b"want is NULL"),
    ("nx < 1", dict(nx=0, vec=(False,) * 3), b"nx, ny and nz must be >= 1"),
    ("ny < 1", dict(ny=-3, xs=[1.0, 1.0, 2.0]), b"nx, ny and nz must be >= 1"),
    ("nz < 1", dict(nz=0, nthr=9), b"nx, ny and nz must be >= 1"),
    ("xs NULL", dict(vec=(False, True, True), ys=[0.0, np.nan]), b"xs, ys and zs must be given"),
    ("zs NULL", dict(vec=(True, True, False), nthr=-1), b"xs, ys and zs must be given"),
    ("xs not increasing", dict(xs=[0.0, 2.0, 2.0], ys=[0.0, np.inf]), b"xs is not strictly increasing"),
    ("ys decreasing", dict(ys=[1.0, 0.5], nthr=9), b"ys is not strictly increasing"),
    ("zs NaN", dict(zs=[0.0, np.nan], thr=(-1.0,)), b"zs is not finite"),
    ("xs infinite", dict(xs=[0.0, 1.0, np.inf], **NONE_OUT), b"xs is not finite"),
    ("nthr > 8", dict(thr=tuple(range(9)), exceed=False), b"nthr must be 0 .. 8"),
    ("nthr < 0", dict(nthr=-1, **NONE_OUT), b"nthr must be 0 .. 8"),
    ("thr NULL", dict(thr_ptr=False, exceed=False), b"thr is NULL"),
    ("threshold negative", dict(thr=(1.0, -0.5), exceed=False), b"every threshold must be finite and >= 0"),
    ("threshold NaN", dict(thr=(np.nan,), std=False), b"every threshold must be finite and >= 0"),
    ("threshold infinite", dict(thr=(np.inf,), std=False), b"every threshold must be finite and >= 0"),
    ("exceed_out missing", dict(exceed=False, std=False), b"exceed_out must be given exactly when nthr > 0"),
    ("exceed_out without thresholds", dict(thr=(), exceed=True, mean=False), b"exceed_out must be given exactly when"),
    ("no output", dict(thr=(), **NONE_OUT), b"no output asked for"),
    ("mean without std", dict(std=False, density=False), b"mean_out and std_out must be given together"),
    ("std without mean", dict(mean=False, density=False), b"mean_out and std_out must be given together"),
    ("skipped without density", dict(density=False), b"skipped_out needs density_out"),
]


@pytest.mark.parametrize("case", [c[0] for c in ORDER])
def test_request_errors_in_the_documented_order(tt, case):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    _, kw, words = next(c for c in ORDER if c[0] == case)
    req, keep = request(_lib, **kw) if kw is not None else (None, None)
    both(tt, req, words)
    del keep


def test_a_lattice_beyond_64_bits_is_refused(tt):
    """nx ny nz overflows: refused after the vectors were read, so they must be real -- 2^21 nodes each."""
    _lib = import_module("mcmc_in_tonga_amd._lib")
    n = 1 << 21
    v = np.arange(n, dtype=np.float64)
    out = np.zeros(1, dtype=np.int64)  # (never written: the call is refused)
    p = _lib.ptr
    req = _lib.TdInterfaces(p(v), p(v), p(v), n, n, n, None, 0, None, p(out), None, None, None, None, None, None)
    both(tt, req, b"nx ny nz does not fit 64 bits")
    assert out[0] == 0


LEGAL = {
    "everything": dict(),
    "no thresholds": dict(thr=()),
    "counts only": dict(thr=(), any_=False, jump=False, mean=False, std=False, density=False, skipped=False),
    "density only": dict(thr=(), count=False, any_=False, jump=False, mean=False, std=False),
    "density without skipped": dict(skipped=False),
    "one node": dict(nx=1, ny=1, nz=1),
    "eight thresholds": dict(thr=tuple(float(t) for t in range(8))),
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
    assert L.td_rasterize_interfaces(None, 3, _lib.ptr(off), *(_lib.ptr(c),) * 4, pr) == 1
    assert L.td_last_error(None) == b"td_rasterize_interfaces: offsets not monotone"
    off = np.array([1, 3], dtype=np.int64)
    assert L.td_rasterize_interfaces(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, pr) == 1
    assert b"td_rasterize_interfaces: bad cell offsets" in L.td_last_error(None)
    off = np.array([0, 3], dtype=np.int64)
    assert L.td_rasterize_interfaces(None, 1, _lib.ptr(off), None, *(_lib.ptr(c),) * 3, pr) == 1
    assert b"td_rasterize_interfaces: bad cell offsets" in L.td_last_error(None)
    for nm, po in ((0, _lib.ptr(off)), (-1, _lib.ptr(off)), (1, None)):
        assert L.td_rasterize_interfaces(None, nm, po, *(_lib.ptr(c),) * 4, pr) == 1
        assert L.td_last_error(None) == b"td_rasterize_interfaces: need nmodels >= 1 and cell_off"
    hs = (ctypes.c_void_p * 1)(None)
    assert L.td_history_interfaces(None, hs, 1, pr) == 1
    assert L.td_last_error(None) == b"td_history_interfaces: a history is NULL"
    # a refused call wrote nothing
    assert all(not keep[f].any() for f in ("count", "any", "exceed", "jump", "mean", "std", "density", "skipped"))
    del keep


def test_the_request_is_checked_before_the_models(tt):
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    req, keep = request(_lib, std=False)
    off = np.array([0, 3, 2], dtype=np.int64)
    c = np.zeros(4)
    assert L.td_rasterize_interfaces(None, 2, _lib.ptr(off), *(_lib.ptr(c),) * 4, ctypes.byref(req)) == 1
    assert b"mean_out and std_out" in L.td_last_error(None)
    assert L.td_rasterize_interfaces(None, 0, None, *(None,) * 4, ctypes.byref(req)) == 1
    assert b"mean_out and std_out" in L.td_last_error(None)
    del keep


# ---------------------------------------------------------------- the binding

def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b((?:td|tdt)_\w+)\s*\(", src, flags=re.M))


def test_the_two_binding_tables_cover_the_three_headers_exactly(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    L = tt.lib()
    own = header_symbols("tdstar_interfaces.h")
    assert own == {"td_rasterize_interfaces", "td_history_interfaces", "tdt_interfaces_plan"}
    assert set(_lib.SIGNATURES_INTERFACES) == own
    older = header_symbols("tdstar.h") | header_symbols("tdstar_testing.h")
    assert set(_lib.SIGNATURES) == older and not (own & older)
    for name, (res, args) in _lib.SIGNATURES_INTERFACES.items():
        f = getattr(L, name)
        assert f.restype is res and len(f.argtypes) == len(args), name
    # tdstar.h does not include the new header, and its ABI version did not move
    hdr = open(os.path.join(ROOT, "include", "tdstar.h")).read()
    assert "tdstar_interfaces.h" not in hdr and re.search(r"#define TDSTAR_ABI_VERSION 2\b", hdr)
    for name in ("interfaces", "interfaces_history", "interfaces_plan"):
        assert callable(getattr(tt.TdContext, name)), name
    assert callable(tt.posterior_interfaces)


def test_struct_layout_is_the_headers(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "tdstar_interfaces.h")).read()
    body = re.search(r"typedef struct td_interfaces \{(.*?)\} td_interfaces;", hdr, re.S).group(1)
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
    assert names == [f for f, _ in _lib.TdInterfaces._fields_]
    assert counts == ["nx", "ny", "nz", "nthr"]
    assert all(t is (ctypes.c_int64 if f in counts else ctypes.c_void_p) for f, t in _lib.TdInterfaces._fields_)
    assert ctypes.sizeof(_lib.TdInterfaces) == 8 * len(names)
    assert [getattr(_lib.TdInterfaces, f).offset for f in names] == [8 * k for k in range(len(names))]


def test_binding_rejects_an_unknown_output(tt):
    ctx = object.__new__(tt.TdContext)  # (no device: checked before the library is called)
    ctx.h = None
    with pytest.raises(ValueError, match="want"):
        ctx.interfaces([(np.zeros(1),) * 4], [0.0], [0.0], [0.0], want=("count", "values"))
