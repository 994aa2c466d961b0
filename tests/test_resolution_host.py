"""CPU: the posterior resolution's host side (include/tdstar_resolution.h) -- the window lists of
posterior.resolution_offsets, the numpy restatement of the definition (tests/resolution_ref.py) against cases worked by
hand, the plan of the ring of blocks (tdt_resolution_plan) against a restatement of csrc/resolution.h res_plan, every
argument check made before any HIP call, without a context, in the order the header writes down (the status and the
text of td_last_error(NULL)), and the binding of the header.  Needs no GPU."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest

import resolution_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the window lists

def forward(o):
    di, dj, dk = (int(v) for v in o)
    return dk > 0 or (dk == 0 and dj > 0) or (dk == 0 and dj == 0 and di > 0)


@pytest.mark.parametrize("lags", [(2, 1, 2), (2, 1, 1), (5, 3, 5), (0, 0, 1), (3, 0, 0), (0, 2, 0), (1, 1, 1)])
def test_resolution_offsets_counts_order_and_forwardness(tt, lags):
    Lx, Ly, Lz = lags
    ax = tt.resolution_offsets(lags, "axes")
    box = tt.resolution_offsets(lags, "box")
    assert ax.dtype == np.int32 and box.dtype == np.int32 and ax.shape == (Lx + Ly + Lz, 3)
    want_axes = [(l, 0, 0) for l in range(1, Lx + 1)] + [(0, l, 0) for l in range(1, Ly + 1)] + [(0, 0, l) for l in range(1, Lz + 1)]
    assert [tuple(o) for o in ax] == want_axes
    # the box: half of the window without its centre, the axes first, then dk slowest and di fastest
    assert len(box) == ((2 * Lx + 1) * (2 * Ly + 1) * (2 * Lz + 1) - 1) // 2
    assert [tuple(o) for o in box[:len(ax)]] == want_axes
    rest = [tuple(int(v) for v in o) for o in box[len(ax):]]
    assert rest == sorted(rest, key=lambda o: (o[2], o[1], o[0])) and not set(rest) & set(want_axes)
    assert all(forward(o) for o in box) and len({tuple(o) for o in box}) == len(box)
    assert all(abs(o[0]) <= Lx and abs(o[1]) <= Ly and 0 <= o[2] <= Lz for o in box)
    # with its mirror image and the centre the box is the whole window
    assert {tuple(o) for o in box} | {tuple(-o) for o in box} | {(0, 0, 0)} == {
        (i, j, k) for i in range(-Lx, Lx + 1) for j in range(-Ly, Ly + 1) for k in range(-Lz, Lz + 1)}


def test_resolution_offsets_known_counts_and_refusals(tt):
    assert len(tt.resolution_offsets((2, 1, 1))) == 22 and len(tt.resolution_offsets((5, 3, 5))) == 423
    assert len(tt.resolution_offsets((2, 1, 2))) == 37 and len(tt.resolution_offsets((5, 3, 5), "axes")) == 13
    assert tt.resolution_offsets((0, 0, 0)).shape == (0, 3)
    with pytest.raises(ValueError):
        tt.resolution_offsets((1, -1, 1))
    with pytest.raises(ValueError):
        tt.resolution_offsets((1, 1, 1), "ball")


# ---------------------------------------------------------------- the restatement, by hand

LINE_V = np.array([[1.0, 2.0, 1.0], [2.0, 4.0, -1.0], [3.0, 6.0, -1.0], [4.0, 8.0, 1.0]])  # [M = 4][3 nodes]
LINE_X = np.array([0.0, 10.0, 30.0])


def test_three_nodes_on_a_line_by_hand():
    """Nodes 0 and 1 move together (corr 1), node 2 is uncorrelated with both (the centred products cancel exactly).
    With the offsets e_x, 2 e_x and threshold 0.5: the plus run of node 0 takes one step and ends on the failing
    correlation with node 2 (no bit); the plus run of node 2 and the minus run of node 0 end on the lattice's edge (bit
    0, bit 1); the minus run of node 1 takes its step to node 0 and ends on the edge; y and z have no offset in the
    list, so both their bits are set everywhere."""
    off = [(1, 0, 0), (2, 0, 0)]
    r = rref.resolution_of_values(LINE_V, LINE_X, [0.0], [0.0], off, 0.5, [1.0, 2.0, 4.0])
    assert np.array_equal(r["mean"], [2.5, 5.0, 0.0])
    assert np.array_equal(r["std"], np.sqrt(np.array([5.0, 20.0, 4.0]) / 3.0))
    nan = np.nan
    assert np.array_equal(r["cov"], [[np.float64(10.0) / 3.0, 0.0, nan], [0.0, nan, nan]], equal_nan=True)
    assert abs(r["corr"][0, 0] - 1.0) < 4e-16 and r["corr"][0, 1] == 0.0 and r["corr"][1, 0] == 0.0
    assert np.array_equal(np.isnan(r["corr"]), [[False, False, True], [False, True, True]])
    assert np.array_equal(r["footprint"], [1.0 + 2.0, 2.0 + 1.0, 4.0])
    assert r["run"].dtype == np.int32 and r["censored"].dtype == np.int32
    assert np.array_equal(r["run"][0], [[1, 0, 0], [0, 1, 0]]) and not r["run"][1:].any()
    assert np.array_equal(r["censored"], [60 | 2, 60 | 2, 60 | 1])
    assert np.array_equal(r["extent"], [[10.0, 10.0, 0.0], [0.0] * 3, [0.0] * 3])


def test_the_line_with_other_thresholds_windows_and_weights():
    off = [(1, 0, 0), (2, 0, 0)]
    low = rref.resolution_of_values(LINE_V, LINE_X, [0.0], [0.0], off, -np.inf)  # every pair on the lattice passes
    assert np.array_equal(low["run"][0], [[2, 1, 0], [0, 1, 2]]) and np.array_equal(low["censored"] & 3, [3, 3, 3])
    assert np.array_equal(low["footprint"], [3.0, 3.0, 3.0]) and np.array_equal(low["extent"][0], [30.0, 30.0, 30.0])
    high = rref.resolution_of_values(LINE_V, LINE_X, [0.0], [0.0], off, np.inf)  # nothing passes
    assert not high["run"].any() and np.array_equal(high["footprint"], [1.0, 1.0, 1.0])
    assert np.array_equal(high["censored"] & 3, [2, 0, 1])  # only the edges
    # a list with a gap: 2 e_x without e_x gives no run at all, both x bits everywhere; the footprint still counts it
    gap = rref.resolution_of_values(LINE_V, LINE_X, [0.0], [0.0], [(2, 0, 0)], -1.0)
    assert not gap["run"].any() and np.array_equal(gap["censored"], [63, 63, 63])
    assert np.array_equal(gap["footprint"], [2.0, 1.0, 2.0])
    # an offset longer than the lattice: NaN rows, nothing else changes
    far = rref.resolution_of_values(LINE_V, LINE_X, [0.0], [0.0], off + [(3, 0, 0), (0, 0, 1)], 0.5, [1.0, 2.0, 4.0])
    assert np.isnan(far["corr"][2:]).all() and np.isnan(far["cov"][2:]).all()
    assert np.array_equal(far["footprint"], [3.0, 3.0, 4.0]) and np.array_equal(far["censored"], [60 | 2, 60 | 2, 60 | 1])
    # one model: NaN everywhere, runs of 0, the lattice-edge bits alone (and the axes without offsets)
    one = rref.resolution_of_values(LINE_V[:1], LINE_X, [0.0], [0.0], off, 0.5)
    assert np.isnan(one["corr"]).all() and not one["run"].any() and np.array_equal(one["censored"], [60 | 2, 60, 60 | 1])


def test_the_restatement_is_the_covariance_restatement_at_a_point_target():
    """corr[o][n] is the covariance restatement's number for the series of column n against column n + f, and the
    other way round."""
    import covariance_ref as cref

    rng = np.random.default_rng(5)
    V = rng.normal(size=(33, 24)) + rng.normal(size=(33, 1))
    xs, ys, zs = np.arange(4.0), np.arange(3.0), np.arange(2.0)
    off = [(1, 0, 0), (-1, 1, 0), (2, -1, 1), (0, 0, 1)]
    r = rref.resolution_of_values(V, xs, ys, zs, off)
    mean, std = cref.column_stats(V)
    for t, o in enumerate(off):
        on, f = rref.on_lattice(4, 3, 2, o)
        assert f > 0 and on.any() and not on.all()
        for n in np.flatnonzero(on):
            cov, corr = cref.cross_moment(V, mean, std, V[:, [n]], mean[[n]], std[[n]])
            assert cov[0, n + f] == r["cov"][t, n] and corr[0, n + f] == r["corr"][t, n]
            cov, corr = cref.cross_moment(V, mean, std, V[:, [n + f]], mean[[n + f]], std[[n + f]])
            assert cov[0, n] == r["cov"][t, n] and corr[0, n] == r["corr"][t, n]
        assert np.isnan(r["corr"][t, ~on]).all()


# ---------------------------------------------------------------- the plan

def ceiling(M):
    """volume_plan's ceiling of a slab (csrc/volume.hip): 2^18 nodes, and one launch's blocks for the sweep with the
    fewest nodes per block."""
    groups = 8 * ((M + 7) // 8)
    return min(1 << 18, max(64, (2 ** 31 - 1) // groups * 128))


def res_plan(M, nq, reach, budget=0, forced=0):
    """csrc/resolution.h res_plan, restated: (ns, R, nblocks) or None."""
    b = budget if budget > 0 else 2 << 30
    ring = lambda ns: -(-reach // ns) + 1
    if forced > 0:
        ns = min(max(forced // 64 * 64, 64), ceiling(M))
    else:
        top = min(ceiling(M), -(-nq // 64) * 64)
        ns = next((n for n in range(top, 63, -64) if 8 * M * n * ring(n) <= b), None)
        if ns is None:
            return None
    return ns, ring(ns), -(-nq // ns)


PLAN_GRID = [(M, nq, reach, budget, forced)
             for M in (1, 40, 10000, 1 << 25)
             for nq, reaches in ((1, (0,)), (60, (0, 1, 59)), (540, (0, 63, 64, 65, 223, 372, 539)),
                                 (97 * 61 * 45, (0, 5, 97 * 61 * 5 + 300)), (1 << 27, (1 << 20,)))
             for reach in reaches
             for budget in (0, 1 << 20, 1 << 30, 4 << 30)
             for forced in (0, 1, 64, 100, 128, 1 << 20)]


def test_the_plan_is_the_restatement(tt):
    plan = tt.TdContext.resolution_plan
    seen_refusal = seen_small = seen_many = 0
    for M, nq, reach, budget, forced in PLAN_GRID:
        want = res_plan(M, nq, reach, budget, forced)
        if want is None:
            with pytest.raises(tt.TdError):
                plan(M, nq, reach, budget, forced)
            seen_refusal += 1
            continue
        got = plan(M, nq, reach, budget, forced)
        assert got == want, (M, nq, reach, budget, forced, got, want)
        ns, R, nblocks = got
        assert ns % 64 == 0 and ns >= 64 and (R - 1) * ns >= reach > (R - 2) * ns and (nblocks - 1) * ns < nq <= nblocks * ns
        if not forced:
            assert 8 * M * ns * R <= (budget or 2 << 30)
        seen_small += reach < ns
        seen_many += reach > 3 * ns
    assert seen_refusal > 10 and seen_small > 100 and seen_many > 30


def test_the_plan_at_known_shapes(tt):
    plan = tt.TdContext.resolution_plan
    assert plan(40, 540, 223, 0, 64) == (64, 5, 9) and plan(40, 540, 223, 0, 128) == (128, 3, 5)
    assert plan(40, 540, 223) == (576, 2, 1) and plan(16, 210, 100) == (256, 2, 1) and plan(1, 1, 0) == (64, 1, 1)
    # 10^4 models: 2 GiB are 26 843 columns; a reach of 30 000 nodes cannot fit them with its own block on top
    assert plan(10000, 266265, 5000) == res_plan(10000, 266265, 5000) and plan(10000, 266265, 5000)[1] == 2
    for bad in ((0, 10, 1), (1, 0, 0), (1, 10, 10), (1, 10, -1), (1, 10, 1, -1), (1, 10, 1, 0, -1), (1, (1 << 56) + 1, 0)):
        with pytest.raises(tt.TdError):
            plan(*bad)
    with pytest.raises(tt.TdError):
        plan(10000, 266265, 30000)


# ---------------------------------------------------------------- the refusals

OUTPUTS = ("cov", "corr", "footprint", "run", "extent", "censored", "mean", "std")


def request(_lib, shape=(3, 2, 2), off=((1, 0, 0), (0, 1, 0), (-1, 1, 1)), noff=None, off_ptr=True, threshold=0.5, weights=None,
            xs=None, ys=None, zs=None, vec=(True,) * 3, dims=None, **outputs):
    """A td_resolution over small arrays; False leaves a pointer NULL.  -> (the struct, what it points into)."""
    p = _lib.ptr
    nx, ny, nz = shape
    nq = nx * ny * nz
    v = [np.asarray(a if a is not None else np.arange(n, dtype=np.float64), dtype=np.float64)
         for a, n in zip((xs, ys, zs), shape)]
    o = np.ascontiguousarray(np.reshape(off, (-1, 3)), dtype=np.int32)
    no = len(o)
    wv = np.asarray(weights, dtype=np.float64) if weights is not None else None
    keep = dict(v=v, off=o, w=wv, cov=np.zeros((no, nq)), corr=np.zeros((no, nq)), footprint=np.zeros(nq),
                run=np.zeros((3, 2, nq), dtype=np.int32), extent=np.zeros((3, nq)), censored=np.zeros(nq, dtype=np.int32),
                mean=np.zeros(nq), std=np.zeros(nq))
    assert set(outputs) <= set(OUTPUTS)
    r = _lib.TdResolution(*(p(a) if on else None for a, on in zip(v, vec)), *(dims if dims is not None else shape),
                          p(o) if off_ptr else None, no if noff is None else noff, threshold, p(wv),
                          *(p(keep[f]) if outputs.get(f, True) else None for f in OUTPUTS))
    return r, keep


def both(tt, req, words):
    """Both entry points without a context (none can be made without a GPU), on one model of one cell and on no
    history: TD_ERR_ARG, and the message through td_last_error(NULL) names the entry point and holds `words` (a pair:
    td_rasterize_resolution's and td_history_resolution's)."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    w1, w2 = words if isinstance(words, tuple) else (words, words)
    off = np.array([0, 1], dtype=np.int64)
    c = np.zeros(1)
    pr = ctypes.byref(req) if req is not None else None
    assert L.td_rasterize_resolution(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_rasterize_resolution: ") and w1 in msg, msg
    assert L.td_history_resolution(None, None, 0, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_history_resolution: ") and w2 in msg, msg


NONE_OUT = {f: False for f in OUTPUTS}
NAN12 = [np.nan] * 12
# in the header's order; each request is wrong in this way and in LATER ways, so the message shows which check ran first
ORDER = [
    ("struct NULL", None, b"want is NULL"),
    ("noff 0", dict(noff=0, off_ptr=False), b"noff must be 1 .. 4096"),
    ("noff 4097", dict(noff=4097, off=((0, 0, 0),)), b"noff must be 1 .. 4096"),
    ("off NULL", dict(off_ptr=False, threshold=np.nan), b"off is NULL"),
    ("the null offset", dict(off=((1, 0, 0), (0, 0, 0)), threshold=np.nan), b"an offset is not forward"),
    ("a backward offset", dict(off=((1, 0, 0), (1, -1, 0)), **NONE_OUT), b"an offset is not forward"),
    ("dk below 0", dict(off=((5, 5, -1),), weights=NAN12), b"an offset is not forward"),
    ("not forward before twice", dict(off=((1, 0, 0), (1, 0, 0), (-1, 0, 0))), b"an offset is not forward"),
    ("an offset twice", dict(off=((1, 0, 0), (0, 1, 0), (1, 0, 0)), threshold=np.nan), b"an offset appears twice"),
    ("threshold NaN", dict(threshold=np.nan, **NONE_OUT), b"threshold is NaN"),
    ("no output", dict(weights=NAN12, **NONE_OUT), b"no output asked for"),
    ("a weight NaN", dict(weights=[1.0] * 11 + [np.nan], xs=[0.0, np.nan, 1.0]), b"weights is not finite"),
    ("a weight infinite", dict(weights=[np.inf] + [1.0] * 11, vec=(False, True, True)), b"weights is not finite"),
    ("nx 0", dict(dims=(0, 2, 2), weights=NAN12, vec=(False,) * 3), b"nx, ny and nz must be >= 1"),
    ("nz -1", dict(dims=(3, 2, -1), vec=(False,) * 3), b"nx, ny and nz must be >= 1"),
    ("xs NULL", dict(vec=(False, True, True), ys=[0.0, np.nan]), b"xs, ys and zs must be given"),
    ("zs NULL", dict(vec=(True, True, False), mean=False), b"xs, ys and zs must be given"),
    ("xs NaN", dict(xs=[0.0, np.nan, 1.0], ys=[1.0, 0.0]), b"xs is not finite"),
    ("ys infinite", dict(ys=[0.0, np.inf], zs=[1.0, 1.0]), b"ys is not finite"),
    ("xs descending", dict(xs=[0.0, 2.0, 1.0], std=False), b"xs is not strictly increasing"),
    ("zs repeated", dict(zs=[1.0, 1.0], mean=False), b"zs is not strictly increasing"),
    ("mean without std", dict(std=False), b"mean_out and std_out must be given together"),
    ("std without mean", dict(mean=False), b"mean_out and std_out must be given together"),
]


@pytest.mark.parametrize("case", [c[0] for c in ORDER])
def test_request_errors_in_the_documented_order(tt, case):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    _, kw, words = next(c for c in ORDER if c[0] == case)
    req, keep = request(_lib, **kw) if kw is not None else (None, None)
    both(tt, req, words)
    if keep is not None:  # a refused call wrote nothing
        assert all(not keep[f].any() for f in OUTPUTS)
    del keep


def test_a_lattice_beyond_64_bits_is_refused_after_its_vectors(tt):
    """2^21 nodes along each axis: the weights are not looked at (there is no nq), the vectors are read over their own
    lengths (one vector of 16 MiB serves as all three), then the product is refused."""
    _lib = import_module("mcmc_in_tonga_amd._lib")
    v = np.arange(float(1 << 21))
    req, keep = request(_lib, shape=(1, 1, 1), dims=(1 << 21,) * 3, weights=[np.nan])
    req.xs = req.ys = req.zs = _lib.ptr(v)
    both(tt, req, b"nx ny nz does not fit 64 bits")
    del keep


def test_the_header_states_the_order_the_cases_follow():
    hdr = " ".join(open(os.path.join(ROOT, "include", "tdstar_resolution.h")).read().replace("*", " ").split())
    para = hdr[hdr.index("TD_ERR_ARG, before any HIP call"):]
    marks = ["want NULL", "noff < 1 or > 4096", "off NULL", "not forward", "appears twice", "a NaN threshold",
             "no output asked for", "a weight that is not finite", "nx, ny or nz < 1", "xs, ys or zs NULL",
             "not finite or not strictly increasing", "nx ny nz beyond 64 bits", "only one of mean_out / std_out",
             "offsets not monotone", "no model or no sample", "a history on another device", "ctx NULL",
             "more than 2^25 models", "more than 2^30 nodes", "more than 1 GiB", "names M and reach",
             "A refused call changes nothing"]
    at = [para.index(m) for m in marks]
    assert at == sorted(at)


LEGAL = {
    "everything": dict(),
    "weighted": dict(weights=[1.0, -1.0, 0.5, 2.0] * 3),
    "threshold -inf": dict(threshold=-np.inf),
    "threshold +inf": dict(threshold=np.inf),
    "an offset beyond the lattice": dict(off=((7, 0, 0), (0, 0, 100), (-2000000000, 2000000000, 2000000000))),
    "4096 offsets": dict(off=[(i, 1, 0) for i in range(4096)]),
    "corr only": dict(NONE_OUT, corr=True),
    "censored only": dict(NONE_OUT, censored=True),
    "statistics only": dict(NONE_OUT, mean=True, std=True),
    "a single node": dict(shape=(1, 1, 1), off=((1, 0, 0),)),
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
    assert L.td_rasterize_resolution(None, 3, p(off), *(p(c),) * 4, pr) == 1
    assert L.td_last_error(None) == b"td_rasterize_resolution: offsets not monotone"
    off = np.array([1, 3], dtype=np.int64)
    assert L.td_rasterize_resolution(None, 1, p(off), *(p(c),) * 4, pr) == 1
    assert b"td_rasterize_resolution: bad cell offsets" in L.td_last_error(None)
    for nm, po in ((0, p(off)), (-1, p(off)), (1, None)):
        assert L.td_rasterize_resolution(None, nm, po, *(p(c),) * 4, pr) == 1
        assert L.td_last_error(None) == b"td_rasterize_resolution: need nmodels >= 1 and cell_off"
    hs = (ctypes.c_void_p * 1)(None)
    assert L.td_history_resolution(None, hs, 1, pr) == 1
    assert L.td_last_error(None) == b"td_history_resolution: a history is NULL"
    assert all(not keep[f].any() for f in OUTPUTS)  # a refused call wrote nothing
    del keep


# ---------------------------------------------------------------- the binding

def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b((?:td|tdt)_\w+)\s*\(", src, flags=re.M))


def test_the_binding_table_covers_the_header_exactly(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    L = tt.lib()
    own = header_symbols("tdstar_resolution.h")
    assert own == {"td_rasterize_resolution", "td_history_resolution", "tdt_resolution_plan", "tdt_set_resolution"}
    assert own == set(_lib.SIGNATURES_RESOLUTION)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_INTERFACES) | set(_lib.SIGNATURES_REGIONS) | set(_lib.SIGNATURES_SUPPORT) |
              set(_lib.SIGNATURES_RECOVERY))
    assert not (own & others)
    for name, (res, args) in _lib.SIGNATURES_RESOLUTION.items():
        f = getattr(L, name)
        assert f.restype is res and len(f.argtypes) == len(args), name
    # tdstar.h does not include the new header, and its ABI version did not move
    hdr = open(os.path.join(ROOT, "include", "tdstar.h")).read()
    assert "tdstar_resolution.h" not in hdr and re.search(r"#define TDSTAR_ABI_VERSION 2\b", hdr)
    assert L.tdt_set_resolution(None, 0, 0) == 1  # (no context: refused)
    for name in ("resolution", "resolution_history", "resolution_plan", "set_resolution"):
        assert callable(getattr(tt.TdContext, name)), name
    for name in ("posterior_resolution", "resolution_offsets"):
        assert callable(getattr(tt, name)), name


def test_struct_layout_is_the_headers(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "tdstar_resolution.h")).read()
    body = re.search(r"typedef struct td_resolution \{(.*?)\} td_resolution;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, kinds = [], {}
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:
            got = [v.strip().lstrip("*") for v in decl[decl.index("*"):].split(",")]
            kind = ctypes.c_void_p
        else:
            base = "int64_t " if decl.startswith("int64_t ") else "double "
            assert decl.startswith(base), decl
            got = [v.strip() for v in decl[len(base):].split(",")]
            kind = ctypes.c_int64 if base == "int64_t " else ctypes.c_double
        names += got
        kinds.update({g: kind for g in got})
    assert names == [f for f, _ in _lib.TdResolution._fields_]
    assert [f for f in names if kinds[f] is ctypes.c_int64] == ["nx", "ny", "nz", "noff"]
    assert [f for f in names if kinds[f] is ctypes.c_double] == ["threshold"]
    assert all(t is kinds[f] for f, t in _lib.TdResolution._fields_)
    assert ctypes.sizeof(_lib.TdResolution) == 8 * len(names)
    assert [getattr(_lib.TdResolution, f).offset for f in names] == [8 * k for k in range(len(names))]
    assert int(re.search(r"#define TD_RESOLUTION_MAX_OFFSETS (\d+)", hdr).group(1)) == 4096
