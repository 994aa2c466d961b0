"""CPU: the host side of the ensemble Gram and distance calls (td_rasterize_gram, td_history_gram): the numpy
restatement the GPU is compared against (tests/gram_ref.py) against plain loops and against X @ X.T within the
bound any order of summation obeys, the inputs on which the contract's association shows in the bits, every argument
check made before any HIP call, in the header's order, the binding, the plan and the tile bookkeeping
(tdt_gram_plan, tdt_gram_tile, tdt_gram_tiles) and the Python layer's summaries (distance_summary,
pattern_summary)."""
import ctypes
import math
import os
import re
from importlib import import_module

import numpy as np
import pytest

import gram_ref as gref
import regions_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def base():
    models, px, py, pz, w = gref.base_case()
    return dict(models=models, px=px, py=py, pz=pz, w=w, ref=gref.gram(models, px, py, pz, w),
                plain=gref.gram(models, px, py, pz, None))


# ---------------------------------------------------------------- the restatement against plain definitions

def test_restatement_equals_plain_loops_on_python_floats(base):
    ref, w = base["ref"], base["w"]
    V, mean = ref["values"], ref["mean"]
    n = V.shape[1]
    assert n == gref.BASE_POINTS and n % 64 not in (0, 1)

    def x(m, p):
        return math.sqrt(float(w[p])) * (float(V[m][p]) - float(mean[p]))

    for a, b in ((0, 0), (3, 1), (1, 3), (69, 64), (17, 69)):
        G = D = 0.0
        for p0 in range(0, n, 64):
            bg = bd = None
            for p in range(p0, min(p0 + 64, n)):
                xa, xb = x(a, p), x(b, p)
                t = xa * xb
                e = xa - xb
                q = e * e
                bg = t if bg is None else bg + t
                bd = q if bd is None else bd + q
            G, D = G + bg, D + bd
        assert G == ref["gram"][a][b] and D == ref["dist2"][a][b], (a, b)
    assert ref["wsum"] == rref.tree_sum(w) and base["plain"]["wsum"] == float(n)
    # w = None is an array of ones, bit for bit
    ones = gref.gram(base["models"], base["px"], base["py"], base["pz"], np.ones(n))
    assert all(gref.same_bits(ones[f], base["plain"][f]) for f in ("gram", "dist2", "mean", "std")) and ones["wsum"] == float(n)


def test_symmetry_and_the_zero_diagonal_are_the_arithmetics_own(base):
    for ref in (base["ref"], base["plain"]):
        G, D = ref["gram"], ref["dist2"]
        assert np.array_equal(G.view(np.int64), G.T.copy().view(np.int64))
        assert np.array_equal(D.view(np.int64), D.T.copy().view(np.int64))
        assert np.all(np.diag(D).view(np.int64) == 0)  # +0.0
        assert np.all(np.diag(G) > 0) and np.all(D[~np.eye(len(D), dtype=bool)] > 0)
    # a NaN value spreads along its model's row and column, and nowhere else
    V = base["ref"]["values"][:5, :130].copy()
    V[2, 77] = np.nan
    X, mean, _ = gref.centred(V, base["w"][:130])
    assert np.isnan(mean[77]) and np.isnan(X[:, 77]).all()  # (the mean of the column is NaN: every model's term there)
    G, D = gref.blocked(X)
    assert np.isnan(G).all() and np.isnan(D).all()


def test_against_the_matrix_product_within_the_bound_of_any_order(base):
    """|fl(sum) - sum| <= gamma_n sum |terms| with n = np + 1 (one rounding per product, at most np additions) for any
    order of summation (Higham, Accuracy and Stability, 3.1): not a tuned tolerance.  dist2 against the identity
    |a - b|^2 = G_aa + G_bb - 2 G_ab, whose terms have the same bound, with a few more roundings."""
    u = 2.0 ** -53
    for ref in (base["ref"], base["plain"]):
        X = ref["X"]
        n = X.shape[1] + 1
        gamma = n * u / (1 - n * u)
        exact = np.array([[math.fsum((X[a] * X[b]).tolist()) for b in range(len(X))] for a in range(0, len(X), 9)])
        absum = np.abs(X[::9]) @ np.abs(X).T
        assert np.all(np.abs(ref["gram"][::9] - exact) <= gamma * absum)
        assert np.all(np.abs(X[::9] @ X.T - exact) <= gamma * absum)
        # (the blocked order and numpy's agree to that bound with each other, twice over)
        assert np.all(np.abs(ref["gram"][::9] - X[::9] @ X.T) <= 2 * gamma * absum)
        g = np.diag(ref["gram"])
        ident = g[:, None] + g[None, :] - 2 * ref["gram"]
        scale = g[:, None] + g[None, :] + 2 * np.abs(X) @ np.abs(X).T
        assert np.all(np.abs(ref["dist2"] - ident) <= 4 * (n + 4) * u * scale)


def test_the_association_shows_in_the_bits_on_the_base_case(base):
    """On the base case the contract's order (blocks of 64) differs in most entries from the two orders a kernel
    would most likely take instead: the plain left-to-right sum over all points, and td_rasterize's pairwise tree
    (1301 points: halves of 651 and 650, each left to right).  A kernel in another order cannot pass the GPU test."""
    for ref in (base["ref"], base["plain"]):
        X = ref["X"]
        M, n = X.shape
        T = X[:, None, :] * X[None, :, :]
        E = X[:, None, :] - X[None, :, :]
        Q = E * E
        for name, terms in (("gram", T), ("dist2", Q)):
            ltr = terms[..., 0].copy()
            for p in range(1, n):
                ltr = ltr + terms[..., p]
            tree = rref.tree_sum(terms)
            off = ~np.eye(M, dtype=bool) if name == "dist2" else np.ones((M, M), dtype=bool)
            d_ltr, d_tree = int(np.sum((ltr != ref[name]) & off)), int(np.sum((tree != ref[name]) & off))
            both = int(np.sum((ltr != ref[name]) & (tree != ref[name]) & off))
            print("%s: %d of %d entries differ from left to right, %d from the tree, %d from both" % (name, d_ltr, off.sum(), d_tree, both))
            assert both >= off.sum() // 2
            # and all three orders are sums of the same terms
            assert np.allclose(ltr, ref[name], rtol=1e-9, atol=1e-6) and np.allclose(tree, ref[name], rtol=1e-9, atol=1e-6)


# ---------------------------------------------------------------- the refusals

def request(_lib, npts=6, px=None, py=None, pz=None, w=None, vec=(True,) * 3, npoints=None, gram=True, dist2=True, mean=True,
            std=True, wsum=True):
    """A td_gram over small arrays; False leaves a pointer NULL.  -> (the struct, what it points into)."""
    p = _lib.ptr
    v = [np.asarray(a if a is not None else np.arange(max(npts, 1), dtype=np.float64), dtype=np.float64) for a in (px, py, pz)]
    wv = np.asarray(w, dtype=np.float64) if w is not None else None
    keep = dict(v=v, w=wv, gram=np.zeros((1, 1)), dist2=np.zeros((1, 1)), mean=np.zeros(max(npts, 1)), std=np.zeros(max(npts, 1)),
                wsum=np.zeros(1))
    r = _lib.TdGram(*(p(a) if on else None for a, on in zip(v, vec)), p(wv), npts if npoints is None else npoints,
                    p(keep["gram"]) if gram else None, p(keep["dist2"]) if dist2 else None, p(keep["mean"]) if mean else None,
                    p(keep["std"]) if std else None, p(keep["wsum"]) if wsum else None)
    return r, keep


def both(tt, req, words):
    """Both entry points without a context (none can be made without a GPU), on one model of one cell and on no
    history: TD_ERR_ARG, and the message through td_last_error(NULL) names the entry point and holds `words` (a
    pair: td_rasterize_gram's and td_history_gram's)."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    w1, w2 = words if isinstance(words, tuple) else (words, words)
    off = np.array([0, 1], dtype=np.int64)
    c = np.zeros(1)
    pr = ctypes.byref(req) if req is not None else None
    assert L.td_rasterize_gram(None, 1, _lib.ptr(off), *(_lib.ptr(c),) * 4, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_rasterize_gram: ") and w1 in msg, msg
    assert L.td_history_gram(None, None, 0, pr) == 1
    msg = L.td_last_error(None)
    assert msg.startswith(b"td_history_gram: ") and w2 in msg, msg


NONE_OUT = dict(gram=False, dist2=False, mean=False, std=False, wsum=False)
# in the header's order; each request is wrong in this way and in LATER ways, so the message shows which check ran first
ORDER = [
    ("struct NULL", None, b"want is NULL"),
    ("np < 1", dict(npoints=0, vec=(False,) * 3), b"np must be >= 1"),
    ("np negative", dict(npoints=-3, w=[np.nan] * 6), b"np must be >= 1"),
    ("px NULL", dict(vec=(False, True, True), py=[np.nan] * 6), b"px, py and pz must be given"),
    ("pz NULL", dict(vec=(True, True, False), w=[-1.0] * 6), b"px, py and pz must be given"),
    ("px NaN", dict(px=[0, 1, np.nan, 3, 4, 5], w=[-1.0] * 6), b"a coordinate is not finite"),
    ("py infinite", dict(py=[0, 1, 2, 3, 4, -np.inf], **NONE_OUT), b"a coordinate is not finite"),
    ("pz NaN", dict(pz=[np.nan] * 6, std=False), b"a coordinate is not finite"),
    ("w infinite", dict(w=[1, 1, 1, np.inf, 1, 1], **NONE_OUT), b"every weight must be finite and >= 0"),
    ("w NaN", dict(w=[1, 1, 1, 1, 1, np.nan], std=False), b"every weight must be finite and >= 0"),
    ("w negative", dict(w=[1, 1, -1e-300, 1, 1, 1], **NONE_OUT), b"every weight must be finite and >= 0"),
    ("no output", dict(**NONE_OUT), b"no output asked for"),
    ("mean without std", dict(std=False), b"mean_out and std_out must be given together"),
    ("std without mean", dict(mean=False, gram=False, dist2=False), b"mean_out and std_out must be given together"),
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
    "weighted, a zero weight and a negative zero": dict(w=[1.0, 0.0, 0.5, 2.0, -0.0, 1.0]),
    "gram only": dict(dist2=False, mean=False, std=False, wsum=False),
    "dist2 only": dict(gram=False, mean=False, std=False, wsum=False),
    "the weights' sum only": dict(gram=False, dist2=False, mean=False, std=False),
    "mean and std only": dict(gram=False, dist2=False, wsum=False),
    "one point": dict(npts=1),
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
    assert L.td_rasterize_gram(None, 3, p(off), *(p(c),) * 4, pr) == 1
    assert L.td_last_error(None) == b"td_rasterize_gram: offsets not monotone"
    off = np.array([1, 3], dtype=np.int64)
    assert L.td_rasterize_gram(None, 1, p(off), *(p(c),) * 4, pr) == 1
    assert b"td_rasterize_gram: bad cell offsets" in L.td_last_error(None)
    for nm, po in ((0, p(off)), (-1, p(off)), (1, None)):
        assert L.td_rasterize_gram(None, nm, po, *(p(c),) * 4, pr) == 1
        assert L.td_last_error(None) == b"td_rasterize_gram: need nmodels >= 1 and cell_off"
    hs = (ctypes.c_void_p * 1)(None)
    assert L.td_history_gram(None, hs, 1, pr) == 1
    assert L.td_last_error(None) == b"td_history_gram: a history is NULL"
    # a refused call wrote nothing
    assert all(not keep[f].any() for f in ("gram", "dist2", "mean", "std", "wsum"))
    del keep


# ---------------------------------------------------------------- the binding, the plan and the tiles

def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b((?:td|tdt)_\w+)\s*\(", src, flags=re.M))


def test_the_binding_table_covers_the_header_exactly(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    L = tt.lib()
    own = header_symbols("tdstar_gram.h")
    assert own == {"td_rasterize_gram", "td_history_gram", "tdt_gram_plan", "tdt_set_gram_form", "tdt_gram_tile", "tdt_gram_tiles"}
    assert set(_lib.SIGNATURES_GRAM) == own
    older = header_symbols("tdstar.h") | header_symbols("tdstar_testing.h")
    assert set(_lib.SIGNATURES) == older and not (own & older)
    for name, (res, args) in _lib.SIGNATURES_GRAM.items():
        f = getattr(L, name)
        assert f.restype is res and len(f.argtypes) == len(args), name
    # tdstar.h does not include the new header, and its ABI version did not move
    hdr = open(os.path.join(ROOT, "include", "tdstar.h")).read()
    assert "tdstar_gram.h" not in hdr and re.search(r"#define TDSTAR_ABI_VERSION 2\b", hdr)
    for name in ("gram", "gram_history", "gram_plan", "set_gram_form", "gram_tile"):
        assert callable(getattr(tt.TdContext, name)), name
    for name in ("ensemble_distances", "posterior_patterns", "distance_summary", "pattern_summary"):
        assert callable(getattr(tt, name)), name


def test_struct_layout_is_the_headers(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "tdstar_gram.h")).read()
    body = re.search(r"typedef struct td_gram \{(.*?)\} td_gram;", hdr, re.S).group(1)
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
    assert names == [f for f, _ in _lib.TdGram._fields_]
    assert counts == ["np"]
    assert all(t is (ctypes.c_int64 if f in counts else ctypes.c_void_p) for f, t in _lib.TdGram._fields_)
    assert ctypes.sizeof(_lib.TdGram) == 8 * len(names)
    limit = int(re.search(r"#define TD_GRAM_MAX_MODELS (\d+)", hdr).group(1))
    assert limit == tt.TdContext.GRAM_MAX_MODELS == 11585 and 8 * limit**2 <= 1 << 30 < 8 * (limit + 1) ** 2


@pytest.mark.parametrize("M,npts,budget,forced", [(70, 1301, 0, 0), (70, 1301, 0, 64), (70, 1301, 0, 128), (70, 1301, 0, 100),
                                                  (10000, 58 * 34 * 34, 0, 0), (11585, 58 * 34 * 34, 0, 0), (1, 10**7, 0, 0),
                                                  (3, 1, 0, 0), (130, 8347, 8 * 130 * 700, 0), (7, 999, 1, 0)])
def test_plan_is_the_volumes(tt, M, npts, budget, forced):
    got = tt.TdContext.gram_plan(M, npts, budget, forced)
    assert got == tt.TdContext.volume_plan(M, npts, budget, forced) == tt.TdContext.regions_plan(M, npts, budget, forced)
    assert got[0] % 64 == 0 and got[0] * got[1] >= npts > got[0] * (got[1] - 1)  # no block of 64 straddles two slabs


def test_plan_and_form_refusals(tt):
    L = tt.lib()
    out = np.zeros(2, dtype=np.int64)
    p = import_module("mcmc_in_tonga_amd._lib").ptr
    for bad in ((0, 1, 0, 0), (1, 0, 0, 0), (1, 1, -1, 0), (1, 1, 0, -1)):
        assert L.tdt_gram_plan(*bad, p(out)) == 1, bad
    assert L.tdt_gram_plan(1, 1, 0, 0, None) == 1
    assert L.tdt_set_gram_form(-1) == 1 and L.tdt_set_gram_form(3) == 1 and L.tdt_gram_tile(3) == -1 and L.tdt_gram_tile(-1) == -1
    try:
        for form in (1, 2, 0):
            assert L.tdt_set_gram_form(form) == 0
    finally:
        L.tdt_set_gram_form(0)
    assert (tt.TdContext.gram_tile(1), tt.TdContext.gram_tile(2)) == (64, 128)
    assert tt.TdContext.gram_tile(0) in (64, 128)
    assert L.tdt_gram_tiles(0, 0, 0, None) == -1 and L.tdt_gram_tiles(11586, 0, 0, None) == -1 and L.tdt_gram_tiles(5, 3, 0, None) == -1


@pytest.mark.parametrize("form", (1, 2))
@pytest.mark.parametrize("M", (1, 63, 64, 65, 128, 129, 300, 11585))
def test_the_tiles_cover_the_lower_triangle_once(tt, form, M):
    L = tt.lib()
    p = import_module("mcmc_in_tonga_amd._lib").ptr
    T = tt.TdContext.gram_tile(form)
    nt = (M + T - 1) // T
    n = L.tdt_gram_tiles(M, form, 0, None)
    assert n == nt * (nt + 1) // 2
    out = np.zeros(2, dtype=np.int64)
    seen = []
    for i in range(n) if n <= 4000 else list(range(2000)) + list(range(n - 2000, n)):
        assert L.tdt_gram_tiles(M, form, i, p(out)) == n
        seen.append((int(out[0]), int(out[1])))
        assert 0 <= out[1] <= out[0] < nt and out[0] * (out[0] + 1) // 2 + out[1] == i
    assert len(set(seen)) == len(seen)
    assert L.tdt_gram_tiles(M, form, n, p(out)) == -1 and L.tdt_gram_tiles(M, form, -1, p(out)) == -1


# ---------------------------------------------------------------- the Python layer

def test_distance_summary_on_hand_made_matrices(tt):
    pts = np.array([0.0, 1.0, 2.0, 10.0, 11.0])  # samples on a line: dist2 = 4 (difference)^2 with wsum = 4
    d2 = 4.0 * (pts[:, None] - pts[None, :]) ** 2
    s = tt.distance_summary(d2, 4.0, [3, 2])
    assert np.array_equal(s["dist"], np.abs(pts[:, None] - pts[None, :]))
    assert s["medoid"] == 2 and s["chain_of"].tolist() == [0, 0, 0, 1, 1]  # row sums 24, 21, 20, 28, 31
    assert np.array_equal(s["row_mean"], np.array([24.0, 21.0, 20.0, 28.0, 31.0]) / 4)
    # a != b: the diagonal's zeros are not averaged in
    assert s["chain_distance"].tolist() == [[(1 + 2 + 1) * 2 / 6, (10 + 11 + 9 + 10 + 8 + 9) / 6],
                                            [(10 + 11 + 9 + 10 + 8 + 9) / 6, 1.0]]
    # ties: the first index; a chain of one sample has no pair within itself; a NaN row never wins
    tie = tt.distance_summary(np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]]), 1.0, [1, 2])
    assert tie["medoid"] == 0 and np.isnan(tie["chain_distance"][0, 0]) and tie["chain_distance"][1, 1] == 1.0
    assert tie["chain_distance"][0, 1] == tie["chain_distance"][1, 0] == 1.0
    d2n = d2.copy()
    d2n[2, :] = d2n[:, 2] = np.nan
    assert tt.distance_summary(d2n, 4.0, [5])["medoid"] in (0, 1, 3, 4)
    one = tt.distance_summary(np.zeros((1, 1)), 2.0, [1])
    assert one["medoid"] == 0 and one["row_mean"].tolist() == [0.0]
    with pytest.raises(ValueError, match="sum to the samples"):
        tt.distance_summary(d2, 4.0, [3, 3])


def test_pattern_summary_on_hand_made_matrices(tt):
    # rank one: scores along s, the component of largest magnitude (-3) made positive
    s = np.array([1.0, -3.0, 2.0, 0.0])
    p = tt.pattern_summary(np.outer(s, s), k=2)
    assert np.allclose(p["eigenvalues"], [14.0, 0.0], atol=1e-12) and np.isclose(p["explained"][0], 1.0, rtol=1e-14)
    assert np.allclose(p["scores"][:, 0], -s, rtol=1e-12, atol=1e-12) and p["scores"][1, 0] > 0
    assert np.isclose(p["participation"], 1.0, rtol=1e-12)
    assert np.allclose(p["scores"][:, 1], 0.0, atol=1e-6)
    # two orthogonal patterns of strengths 9 and 4; a tie in magnitude takes the first index
    a, b = np.array([1.0, -1.0, 0.0, 0.0]) / np.sqrt(2), np.array([0.0, 0.0, -1.0, 1.0]) / np.sqrt(2)
    G = 9.0 * np.outer(a, a) + 4.0 * np.outer(b, b)
    p = tt.pattern_summary(G, k=8)  # k is capped at M
    assert p["scores"].shape == (4, 4) and np.allclose(p["eigenvalues"], [9.0, 4.0, 0.0, 0.0], atol=1e-12)
    assert np.allclose(p["explained"][:2], [9 / 13, 4 / 13], rtol=1e-12)
    assert np.isclose(p["participation"], 13.0**2 / (81 + 16), rtol=1e-12)
    for j, (v, lam) in enumerate(((a, 9.0), (b, 4.0))):
        u = p["vectors"][:, j]
        first = int(np.argmax(np.abs(u)))
        assert u[first] > 0 and np.allclose(np.abs(u), np.abs(v), atol=1e-12)
        assert np.allclose(p["scores"][:, j], u * np.sqrt(lam), rtol=1e-12, atol=1e-12)
    # the scores reproduce the matrix: G = S S^T
    assert np.allclose(p["scores"] @ p["scores"].T, G, atol=1e-12)
    assert tt.pattern_summary(G, k=0)["scores"].shape == (4, 0)
