"""CPU: the posterior comparison's host side (include/tdstar_compare.h) -- the two numpy restatements of the contract
(tests/compare_ref.py) against each other and against scipy, every argument check of td_rasterize_compare /
td_history_compare / td_compare_values made before any HIP call, without a context, in the order the header writes
down, the binding of the header, and what posterior.py derives from the integer outputs.  Needs no GPU."""
import ctypes
import math
import os
import re
from importlib import import_module

import numpy as np
import pytest

import compare_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatements

@pytest.mark.parametrize("shape", cr.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("kind", cr.KINDS)
def test_the_two_restatements_agree(kind, shape):
    A, B = cr.inputs(kind, *shape)
    r, s = cr.reference(kind, *shape), cr.by_sorting(A, B)
    assert cr.differences(r, s) == []
    assert np.array_equal(r["exceed"][0], r["greater"])  # the pair (1, 0)
    assert np.array_equal(r["less"] + r["equal"] + r["greater"],
                          np.sum(~np.isnan(A), axis=0) * np.sum(~np.isnan(B), axis=0))
    sw = cr.brute(B, A, ())
    assert cr.differences(sw, cr.swapped(r), tuple(cr.swapped(r))) == []
    if kind == "ties":
        assert r["equal"].sum() > 0
    if kind == "identical":
        assert not r["ks_plus"].any() and not r["ks_minus"].any() and np.isnan(r["ks_at"]).all()
    if kind == "disjoint":
        assert np.all(r["less"] == A.shape[0] * B.shape[0]) and np.all(r["ks_plus"] == A.shape[0] * B.shape[0])
        assert np.array_equal(r["ks_at"], A.max(axis=0))


def test_the_hostile_inputs_hold_what_they_claim():
    for shape in cr.SHAPES:
        A, B = cr.inputs("hostile", *shape)
        na, nb = np.isnan(A), np.isnan(B)
        if shape[2] >= 4:
            assert np.any(na.all(axis=0) & nb.all(axis=0))  # NaN-only columns
            assert np.any(na.any(axis=0) & ~nb.any(axis=0)) and np.any(~na.any(axis=0) & nb.all(axis=0))  # one side only
        if A.size + B.size >= 200:
            for v in (A, B):
                zeros = v[v == 0]
                assert np.any(np.signbit(zeros)) and np.any(~np.signbit(zeros))
            assert np.any(np.isinf(A)) and np.any(np.abs(A[np.isfinite(A)]) < 2.3e-308)


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (37, 150), (64, 65)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ties", [False, True])
def test_against_scipy(shape, ties):
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(shape[0] + 7 * ties)
    a, b = rng.standard_normal(shape[0]), rng.standard_normal(shape[1]) + 0.4
    if ties:
        a, b = np.round(a, 1), np.round(b, 1)
    r = cr.brute(a, b, ())
    pairs = shape[0] * shape[1]
    ks = max(r["ks_plus"][0], r["ks_minus"][0]) / pairs
    assert ks == pytest.approx(stats.ks_2samp(a, b).statistic, abs=1e-14)
    assert stats.mannwhitneyu(a, b).statistic == r["greater"][0] + r["equal"][0] / 2


# ---------------------------------------------------------------- the refusals

COUNTS = ("less", "equal", "greater")
OUTPUTS = COUNTS + ("exceed", "ks_plus", "ks_minus", "ks_at", "mean_a", "std_a", "mean_b", "std_b")


def request(_lib, nq=4, coords=(True,) * 3, nexceed=1, scale=(1.0,), shift=(0.0,), scale_ptr=True, shift_ptr=True,
            marg_a=None, marg_b=None, **outputs):
    """A td_compare over small arrays; False leaves a pointer NULL.  -> (the struct, what it points into)."""
    p = _lib.ptr
    n = max(nq, 1)
    v = [np.arange(n, dtype=np.float64) for _ in range(3)]
    sc, sh = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    keep = dict(v=v, sc=sc, sh=sh, marg_a=marg_a, marg_b=marg_b, exceed=np.zeros((max(nexceed, 1), n), dtype=np.int64),
                ks_at=np.zeros(n), **{f: np.zeros(n, dtype=np.int64) for f in COUNTS + ("ks_plus", "ks_minus")},
                **{f: np.zeros(n) for f in OUTPUTS[7:]})
    assert set(outputs) <= set(OUTPUTS)
    r = _lib.TdCompare(*(p(a) if on else None for a, on in zip(v, coords)), nq, nexceed, p(sc) if scale_ptr else None,
                       p(sh) if shift_ptr else None, *(p(keep[f]) if outputs.get(f, True) else None for f in OUTPUTS),
                       ctypes.addressof(marg_a) if marg_a is not None else None,
                       ctypes.addressof(marg_b) if marg_b is not None else None)
    return r, keep


def refused(tt, req, words, entries="rhv"):
    """The entry points without a context (none can be made without a GPU), each on sides that are in order but for
    the histories, of which there are none: TD_ERR_ARG, and the message through td_last_error(NULL) names the entry
    point and holds `words` (one, or one per entry point)."""
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    p = _lib.ptr
    words = words if isinstance(words, tuple) else (words,) * len(entries)
    off, c = np.array([0, 1], dtype=np.int64), np.zeros(1)
    pr = ctypes.byref(req) if req is not None else None
    calls = dict(r=("td_rasterize_compare", lambda: L.td_rasterize_compare(None, 1, p(off), *(p(c),) * 4, 1, p(off), *(p(c),) * 4, pr)),
                 h=("td_history_compare", lambda: L.td_history_compare(None, None, 0, None, 0, pr)),
                 v=("td_compare_values", lambda: L.td_compare_values(None, p(c), 1, p(c), 1, 1, pr)))
    for e, w in zip(entries, words):
        name, fn = calls[e]
        assert fn() == 1, name
        msg = L.td_last_error(None)
        assert msg.startswith(name.encode() + b": ") and w in msg, msg


NONE_OUT = {f: False for f in OUTPUTS}
NO_SAMPLE = b"side A hold no sample"
# in the header's order; each request is wrong in this way and in LATER ways, so the message shows which check ran first
ORDER = [
    ("struct NULL", None, b"want is NULL", "rhv"),
    ("nq < 0", dict(nq=-1, coords=(False,) * 3), b"counts must be >= 0", "rh"),
    ("nexceed 17", dict(nexceed=17, scale_ptr=False), b"nexceed at most 16", "rhv"),
    ("nexceed -1", dict(nexceed=-1, coords=(False,) * 3), b"nexceed at most 16", "rhv"),
    ("qx NULL", dict(coords=(False, True, True), scale_ptr=False), b"the columns' inputs must be given", "rh"),
    ("qz NULL", dict(coords=(True, True, False), scale=(-1.0,)), b"the columns' inputs must be given", "rh"),
    ("scale NULL", dict(scale_ptr=False, shift=(np.nan,)), b"scale, shift and exceed_out must be given", "rhv"),
    ("shift NULL", dict(shift_ptr=False, scale=(np.nan,)), b"scale, shift and exceed_out must be given", "rhv"),
    ("exceed_out NULL", dict(NONE_OUT, scale=(0.0,)), b"scale, shift and exceed_out must be given", "rhv"),
    ("scale 0", dict(NONE_OUT, exceed=True, scale=(0.0,), ks_at=True), b"every scale must be finite and > 0", "rhv"),
    ("scale negative", dict(scale=(1.0, -2.0), shift=(0.0, 0.0), nexceed=2, ks_plus=False), b"every scale must be finite", "rhv"),
    ("scale infinite", dict(scale=(np.inf,), std_a=False), b"every scale must be finite", "rhv"),
    ("scale NaN", dict(scale=(np.nan,), std_b=False), b"every scale must be finite", "rhv"),
    ("shift NaN", dict(shift=(np.nan,), ks_minus=False), b"every shift finite", "rhv"),
    ("shift infinite", dict(shift=(-np.inf,), mean_a=False), b"every shift finite", "rhv"),
    ("no output", dict(NONE_OUT, nexceed=0), b"no output asked for", "rhv"),
    ("ks_plus without ks_minus", dict(ks_minus=False, mean_a=False), b"ks_plus_out and ks_minus_out must be given together", "rhv"),
    ("ks_minus without ks_plus", dict(ks_plus=False, std_b=False), b"ks_plus_out and ks_minus_out must be given together", "rhv"),
    ("ks_at alone", dict(ks_plus=False, ks_minus=False, std_a=False), b"ks_at_out needs ks_plus_out and ks_minus_out", "rhv"),
    ("mean_a without std_a", dict(std_a=False, mean_b=False), b"mean_a_out and std_a_out must be given together", "rhv"),
    ("std_a without mean_a", dict(mean_a=False, std_b=False), b"mean_a_out and std_a_out must be given together", "rhv"),
    ("mean_b without std_b", dict(std_b=False, marg_a="probs"), b"mean_b_out and std_b_out must be given together", "rhv"),
    ("std_b without mean_b", dict(mean_b=False, marg_b="bins"), b"mean_b_out and std_b_out must be given together", "rhv"),
    ("marg_a refused", dict(marg_a="probs", marg_b="bins"), b"every probability must lie in [0, 1]", "rhv"),
    ("marg_b refused", dict(marg_a="good", marg_b="bins"), b"nbins must be 0..4096", "rhv"),
    ("in order", dict(marg_a="good", marg_b="good"), (b"ctx is NULL", NO_SAMPLE, b"ctx is NULL"), "rhv"),
]


def marginals(_lib, how):
    probs = np.array([0.5, 1.5 if how == "probs" else 0.9])
    quant = np.zeros((2, 4))
    return _lib.TdMarginals(2, _lib.ptr(probs), _lib.ptr(quant), 5000 if how == "bins" else 0, 0.0, 1.0, None), (probs, quant)


@pytest.mark.parametrize("case", [c[0] for c in ORDER])
def test_request_errors_in_the_documented_order(tt, case):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    _, kw, words, entries = next(c for c in ORDER if c[0] == case)
    held = []
    if kw is not None:
        kw = dict(kw)
        for side in ("marg_a", "marg_b"):
            if side in kw:
                kw[side], h = marginals(_lib, kw[side])
                held.append(h)
    req, keep = request(_lib, **kw) if kw is not None else (None, None)
    refused(tt, req, words, entries)
    if keep is not None:  # a refused call wrote nothing
        assert all(not keep[f].any() for f in OUTPUTS)
    del keep, held


def test_the_sides_are_checked_after_the_request_and_before_the_context(tt):
    L = tt.lib()
    _lib = import_module("mcmc_in_tonga_amd._lib")
    p = _lib.ptr
    req, keep = request(_lib)
    pr = ctypes.byref(req)
    good, c = np.array([0, 1], dtype=np.int64), np.zeros(4)
    side = lambda off, n=None: (len(off) - 1 if n is None else n, p(off), *(p(c),) * 4)  # noqa: E731
    big = np.zeros(16386, dtype=np.int64)

    def ras(a, b, words):
        assert L.td_rasterize_compare(None, *a, *b, pr) == 1
        msg = L.td_last_error(None)
        assert msg.startswith(b"td_rasterize_compare") and all(w in msg for w in words), msg

    not_monotone = np.array([0, 3, 2, 4], dtype=np.int64)
    ras(side(good, 0), side(not_monotone), (b"(side A)", b"need nmodels >= 1 and cell_off"))
    ras((1, None, *(p(c),) * 4), side(good), (b"(side A)", b"need nmodels >= 1 and cell_off"))
    ras(side(np.array([1, 3], dtype=np.int64)), side(good, -1), (b"(side A)", b"bad cell offsets"))
    ras(side(not_monotone), side(good, 0), (b"(side A)", b"offsets not monotone"))
    ras(side(good), side(good, 0), (b"(side B)", b"need nmodels >= 1 and cell_off"))
    ras(side(big), side(not_monotone), (b"(side B)", b"offsets not monotone"))
    ras(side(big), side(big), (b"side A holds 16385 models",))
    ras(side(good), side(big), (b"side B holds 16385 models",))
    ras(side(big[:-1]), side(big[:-1]), (b"ctx is NULL",))  # 16384 a side is in order
    hs = (ctypes.c_void_p * 1)(None)
    for a, b in (((hs, 1), (None, 0)), ((None, 0), (hs, 1))):
        assert L.td_history_compare(None, *a, *b, pr) == 1
        assert L.td_last_error(None) == b"td_history_compare: a history is NULL"
    A = np.zeros((16385, 1))
    for ma, mb, ncol, words in ((-1, 1, 1, b"counts must be >= 0"), (1, -1, 1, b"counts must be >= 0"), (1, 1, -1, b"counts must be >= 0"),
                                (0, 0, 1, b"side A holds no row"), (1, 0, 1, b"side B holds no row"),
                                (16385, 0, 1, b"side B holds no row"), (16385, 16385, 1, b"side A holds 16385 models"),
                                (16384, 16385, 1, b"side B holds 16385 models"), (16384, 16384, 1, b"ctx is NULL"),
                                (16384, 1, 0, b"ctx is NULL")):
        assert L.td_compare_values(None, p(A), ma, p(A), mb, ncol, pr) == 1
        msg = L.td_last_error(None)
        assert msg.startswith(b"td_compare_values: ") and words in msg, (ma, mb, ncol, msg)
    for a, b in ((None, p(A)), (p(A), None)):
        assert L.td_compare_values(None, a, 2, b, 2, 1, pr) == 1
        assert b"td_compare_values: the columns' inputs must be given" in L.td_last_error(None)
    assert all(not keep[f].any() for f in OUTPUTS)  # a refused call wrote nothing
    del keep


def test_the_header_states_the_order_the_cases_follow():
    """The words of the header's refusal paragraph, in the order ORDER tries them."""
    hdr = " ".join(open(os.path.join(ROOT, "include", "tdstar_compare.h")).read().replace("*", " ").split())
    para = hdr[hdr.index("TD_ERR_ARG, before any HIP call"):]
    marks = ["want NULL", "nq < 0", "nexceed < 0 or > 16", "without qx, qy, qz", "without scale, shift or exceed_out",
             "a scale that is not finite and > 0", "a shift that is not finite", "no output asked for",
             "only one of ks_plus_out / ks_minus_out", "ks_at_out without them", "only one of mean_a_out / std_a_out",
             "mean_b_out / std_b_out", "a marg_a, then a marg_b", "a NULL history", "no model", "not monotone offsets",
             "beyond 16384 models", "a history on another device", "ctx NULL", "nq == 0", "A refused call changes nothing"]
    at = [para.index(m) for m in marks]
    assert at == sorted(at)


# ---------------------------------------------------------------- the binding

def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b((?:td|tdt)_\w+)\s*\(", src, flags=re.M))


def test_the_binding_table_covers_the_header_exactly(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    L = tt.lib()
    own = header_symbols("tdstar_compare.h")
    assert own == {"td_rasterize_compare", "td_history_compare", "td_compare_values", "tdt_set_compare_form"}
    assert own == set(_lib.SIGNATURES_COMPARE)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_INTERFACES) | set(_lib.SIGNATURES_REGIONS) | set(_lib.SIGNATURES_SUPPORT) |
              set(_lib.SIGNATURES_RECOVERY) | set(_lib.SIGNATURES_RESOLUTION))
    assert not (own & others)
    for name, (res, args) in _lib.SIGNATURES_COMPARE.items():
        f = getattr(L, name)
        assert f.restype is res and len(f.argtypes) == len(args), name
    # tdstar.h does not include the new header, and its ABI version did not move
    hdr = open(os.path.join(ROOT, "include", "tdstar.h")).read()
    assert "tdstar_compare.h" not in hdr and re.search(r"#define TDSTAR_ABI_VERSION 2\b", hdr)
    for name in ("compare", "compare_history", "compare_values"):
        assert callable(getattr(tt.TdContext, name)), name
    for name in ("posterior_compare", "compare_summary", "info_gain_bits"):
        assert callable(getattr(tt, name)), name


def test_the_form_hook_takes_what_the_header_says(tt):
    L = tt.lib()
    for bad in ((2, 0, 0), (-1, 0, 0), (0, 32, 0), (0, 100, 0), (0, 2048, 0), (0, 0, 96), (0, 0, -64)):
        assert L.tdt_set_compare_form(*bad) == 1, bad
    for good in ((1, 64, 1024), (0, 1024, 64), (0, 0, 0)):
        assert L.tdt_set_compare_form(*good) == 0, good


def test_struct_layout_is_the_headers(tt):
    _lib = import_module("mcmc_in_tonga_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "tdstar_compare.h")).read()
    body = re.search(r"typedef struct td_compare \{(.*?)\} td_compare;", hdr, re.S).group(1)
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
    assert names == [f for f, _ in _lib.TdCompare._fields_]
    assert counts == ["nq", "nexceed"]
    assert all(t is (ctypes.c_int64 if f in counts else ctypes.c_void_p) for f, t in _lib.TdCompare._fields_)
    assert ctypes.sizeof(_lib.TdCompare) == 8 * len(names)
    assert [getattr(_lib.TdCompare, f).offset for f in names] == [8 * k for k in range(len(names))]


# ---------------------------------------------------------------- what posterior.py derives

def test_the_derived_quantities_against_plain_loops(tt):
    rng = np.random.default_rng(5)
    MA, MB, n, nbins = 37, 150, 40, 6
    r = dict(less=rng.integers(0, 2000, n), equal=rng.integers(0, 1500, n), greater=rng.integers(0, 2000, n),
             exceed=rng.integers(0, MA * MB, (2, n)), ks_plus=rng.integers(0, 3, n) * 700, ks_minus=rng.integers(0, 3, n) * 700,
             mean_a=rng.standard_normal(n), mean_b=rng.standard_normal(n),
             hist_a=rng.multinomial(MA, np.full(nbins + 3, 1.0 / (nbins + 3)), n),
             hist_b=rng.multinomial(MB, [0.5, 0.5] + [0.0] * (nbins + 1), n))
    assert np.any(r["hist_b"] == 0) and {-1, 0, 1} == set(np.sign(r["ks_plus"] - r["ks_minus"]).tolist())
    d = tt.compare_summary(r, MA, MB)
    for q in range(n):
        assert d["prob_greater"][q] == (int(r["greater"][q]) + 0.5 * int(r["equal"][q])) / (MA * MB)
        assert d["ks"][q] == max(int(r["ks_plus"][q]), int(r["ks_minus"][q])) / (MA * MB)
        p, m = int(r["ks_plus"][q]), int(r["ks_minus"][q])
        assert d["ks_sign"][q] == (1 if p > m else (-1 if m > p else 0))
        assert d["mean_diff"][q] == r["mean_a"][q] - r["mean_b"][q]
        assert all(d["prob_exceed"][k, q] == int(r["exceed"][k, q]) / (MA * MB) for k in range(2))
        bits = 0.0
        for s in range(nbins + 3):
            pa = (int(r["hist_a"][q, s]) + 0.5) / (MA + 0.5 * (nbins + 3))
            pb = (int(r["hist_b"][q, s]) + 0.5) / (MB + 0.5 * (nbins + 3))
            bits += pa * math.log2(pa / pb)
        assert d["info_gain_bits"][q] == pytest.approx(bits, rel=1e-12, abs=1e-15) and bits > 0
    same = tt.info_gain_bits(r["hist_a"], r["hist_a"], MA, MA)
    assert np.all(same == 0.0)
    assert tt.compare_summary(dict(greater=None, exceed=None, ks_plus=None, mean_a=None, hist_a=None), 1, 1) == {}
