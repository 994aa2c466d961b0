"""A catalogue of calls on one context, for tests/test_gpu_context_state.py (GPU) and
tests/test_context_ops_host.py (CPU): every public entry point that issues GPU work, at the sizes where it
switches path or makes a grow-only workspace of the context (csrc/ctx.h) grow, as a named operation
`fn(session) -> tuple of arrays and scalars` with seeded, fixed inputs on the 381 shipped rays.

The reference of an operation is what it returns on a fresh context that did nothing else (created, called
once, closed; `References`), and, where the project has a CPU oracle, the oracle's numbers (`Op.oracle`), so
the comparison is not circular.  Every comparison is exact: `same` compares uint64 views, NaN equal to NaN.

A `Session` is one context plus what the operations keep on it from call to call: the last evaluated model
(what `evaluate_edit_*` edits), the sigma scale (`set_sigma_*` change it; a reference is made at the same
sigma), recorded histories (made once per session and sigma) and a tempering ladder left resident.  A plain
module that the tests import, as they import chain_cases and frames; importing it touches neither the
library nor the GPU."""
import ctypes
import functools
import hashlib
import re
import zlib

import numpy as np

import tonga

# ---- shapes (tests/test_context_ops_host.py checks that they cross what they claim to cross) ----
GRID_MIN_CELLS = 256  # csrc/internal.h kGridMinCells: uses_grid's threshold
EVAL_CELLS = (63, 300, 2500)  # brute force / bucket grid / more buckets: the count buffer grows
INTERP = ((1, 40), (700, 40), (1, 1200), (700, 1200))  # (points, cells)
BATCH_CELLS = (5, 300, 1200)
MISFIT_N = (381, 100)
RASTER_BATCHED = ((5, 40, 0, 300, 1200, 90), 200)  # (model sizes; one empty, one given NaN cells), nodes
RASTER_PER_MODEL = ((4500, 5000), 60000)
RASTER_BUDGET = 1 << 28  # csrc/raster.hip raster_batched: nodes x mean cells
MARG_MODELS, MARG_NODES = 12, 200
CONV_CHAINS = ((40, 40), (9, 9, 9, 9))
CONV_LAGS = (0, 5)
ENSEMBLES = {8: 500, 16: 2000}  # models -> nodes (volume, covariance); predict sweeps the context's rays
FORCED_SLAB_NODES = 128
FORCED_PREDICT = (2048, 3)  # (slab points, model chunk)
HISTORY = dict(cells=300, max_cells=400, iterations=120, first=10, every=10, samples=12)
CHAIN = dict(cells=300, max_cells=500, iterations=50)
BATCHES = (1, 5, 2)
LADDER = dict(chains=4, cells=200, max_cells=400, K=20)
TRI_GRIDS = ((2, 2, 2), (40, 33, 60), (4100, 2, 2))
TRI_POINTS = (5000, 50)
TRI_KNOTS_LDS = 4096  # csrc/ingest.hip kKnotsLds: more knots in all are read from global memory
SIGMA_SCALE = 1.5
MARG_MAX_BINS = 4096

# the operations that take longest, paired with one representative per family instead of with every entry
HEAVY = ("rasterize_per_model", "volume_16_auto", "volume_16_forced", "predict_16_auto", "predict_16_forced",
         "covariance_16_auto", "covariance_16_forced", "ladder_step")


def tt():
    return tonga.load()


@functools.lru_cache(maxsize=None)
def rays():
    return tt().load_data_Tonga()


@functools.lru_cache(maxsize=None)
def cells(n, seed):
    return tuple(np.array(a) for a in tt().random_model(n, seed).cells())


def same(a, b):
    """Exact equality of two results (tuples of arrays / scalars / None): shapes, then uint64 views of the
    doubles with NaN equal to NaN, integers as they are."""
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        return (isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b)
                and all(same(x, y) for x, y in zip(a, b)))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or (a.dtype.kind == "f") != (b.dtype.kind == "f"):
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def first_difference(a, b):
    """Where two results differ, for a failure message."""
    if len(a) != len(b):
        return "%d outputs against %d" % (len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        if not same(x, y):
            x, y = np.asarray(x), np.asarray(y)
            if x.shape != y.shape:
                return "output %d: shape %s against %s" % (i, x.shape, y.shape)
            bad = np.flatnonzero([not same(p, q) for p, q in zip(x.ravel(), y.ravel())])
            k = int(bad[0]) if len(bad) else 0
            return "output %d: %d of %d differ, first at %d: %r against %r" % (i, len(bad), x.size, k, x.ravel()[k],
                                                                              y.ravel()[k])
    return "equal"


class Session:
    """One context and the state the catalogue's operations keep on it."""

    def __init__(self, sigma_scale=1.0):
        ds = rays()
        self.sigma_scale = sigma_scale
        self.ctx = tt().TdContext(ds.rayX, ds.rayY, ds.rayZ, ds.rayL, ds.rayU, ds.tS, self.sigma())
        self.last_cells = None  # the model of the last evaluate (what evaluate_edit_* edit)
        self.edit_prop = None  # the model the last evaluate_edit_* evaluated
        self.histories = {}  # sigma scale -> two recorded histories
        self.ladder = None  # (TemperingLadder, chains) left resident by ladder_step

    def sigma(self):
        return np.asarray(rays().allSig, dtype=np.float64) * self.sigma_scale

    def drop_ladder(self):
        if self.ladder is not None:
            lad, chains = self.ladder
            if lad.rounds is not None:
                lad.rounds.close()
            for c in chains:
                c.close()
            self.ladder = None

    def close(self):
        self.drop_ladder()
        for hs in self.histories.values():
            for h in hs:
                h.close()
        self.histories = {}
        self.ctx.close()

    def resident_count(self):
        n = ctypes.c_int64(-1)
        assert tt().lib().tdt_resident_count(ctypes.byref(n)) == 0
        return n.value


class Op:
    """name, family, fn(session) -> tuple; `reaches`: the C entry points of include/tdstar.h the call goes
    through; `gpu`: it issues GPU work (so it must leave no resident launch of this thread behind, unless
    `keeps`: documented to keep td_evaluate's server); `oracle() -> {output index: expected}` on the CPU;
    `stateful`: the answer depends on the session's last model (its reference is made from that model)."""

    def __init__(self, name, family, fn, reaches, gpu=True, keeps=False, oracle=None, stateful=False, sigma=False):
        self.name, self.family, self.fn, self.reaches = name, family, fn, tuple(reaches)
        self.gpu, self.keeps, self.oracle, self.stateful = gpu, keeps, oracle, stateful
        self.sigma = sigma  # the oracle takes the session's sigma

    def __repr__(self):
        return self.name


OPS = []


def op(name, family, reaches, **kw):
    def deco(fn):
        OPS.append(Op(name, family, fn, reaches, **kw))
        return fn
    return deco


def flat(d, keys):
    return tuple(d[k] for k in keys if d.get(k) is not None)


def queries(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-100, 1100, n), rng.uniform(-200, 500, n), rng.uniform(-10, 700, n)


# ---------------------------------------------------------------- evaluate
def _oracle_evaluate(c, sig, nearest):
    import oracle

    ds = rays()
    r = oracle.evaluate(ds.rayX, ds.rayY, ds.rayZ, ds.rayL, ds.rayU, ds.tS, sig, c)
    out = {0: r["ptS"], 1: r["phi"], 2: r["likelihood"]}
    if nearest:
        out[3] = r["nearest"]
    return out


def _add_evaluate(n, nearest):
    name = "evaluate_%d%s" % (n, "_nearest" if nearest else "")

    def fn(s):
        c = cells(n, 40 + n)
        ptS, phi, lk, near = s.ctx.evaluate(c, want_nearest=nearest)
        s.last_cells = c
        return (ptS, phi, lk) + ((near,) if nearest else ())

    OPS.append(Op(name, "evaluate", fn, ["td_evaluate"], keeps=not nearest, sigma=True,
                  oracle=lambda sig: _oracle_evaluate(cells(n, 40 + n), sig, nearest)))


for _n in EVAL_CELLS:
    for _near in (False, True):
        _add_evaluate(_n, _near)

EDIT_BASE = (300, 7)  # evaluate_edit_* without an evaluate before them edit this model


def edited(base, kind):
    """One reference-shaped edit of `base` (test_gpu_incremental.edit's moves, births and deaths), seeded by
    the model itself."""
    x, y, z, ze = (np.array(a, dtype=np.float64) for a in base)
    rng = np.random.default_rng([zlib.crc32(x.tobytes()), zlib.crc32(ze.tobytes()), len(x), len(kind)])
    box = tt().box()
    if kind == "birth" or len(x) <= 2:
        p = [rng.uniform(box[0], box[1]), rng.uniform(box[2], box[3]), rng.uniform(box[4], box[5])]
        return np.append(x, p[0]), np.append(y, p[1]), np.append(z, p[2]), np.append(ze, rng.uniform(0, 50))
    k = int(rng.integers(len(x)))
    if kind == "death":
        return tuple(np.delete(v, k) for v in (x, y, z, ze))
    x[k] += rng.normal(0, 100)
    y[k] += rng.normal(0, 60)
    z[k] += rng.normal(0, 60)
    return x, y, z, ze


def _add_edit(kind):
    def fn(s):
        prop = edited(s.last_cells if s.last_cells is not None else cells(*EDIT_BASE), kind)
        s.edit_prop = prop
        ptS, phi, lk, _ = s.ctx.evaluate(prop)
        s.last_cells = prop
        return ptS, phi, lk

    OPS.append(Op("evaluate_edit_" + kind, "evaluate_edit", fn, ["td_evaluate"], keeps=True, stateful=True))


for _k in ("move", "birth", "death"):
    _add_edit(_k)


# ---------------------------------------------------------------- interpolate, batch, misfit, sigma
def _add_interpolate(npts, ncells):
    def args():
        return cells(ncells, 60 + ncells), queries(npts, 1000 + npts)

    def fn(s):
        c, (X, Y, Z) = args()
        return s.ctx.interpolate(c, X, Y, Z, want_nearest=npts > 1)[:2 if npts > 1 else 1]

    def orc():
        import oracle

        c, (X, Y, Z) = args()
        v, ids = oracle.interpolation(c, X, Y, Z)
        return {0: v, 1: ids.astype(np.int32)} if npts > 1 else {0: v}

    OPS.append(Op("interpolate_%dpt_%dcells" % (npts, ncells), "interpolate", fn, ["td_interpolate"], oracle=orc))


for _p, _c in INTERP:
    _add_interpolate(_p, _c)


def _batch_models():
    return [cells(n, 80 + k) for k, n in enumerate(BATCH_CELLS)]


def _oracle_batch(sig):
    rows = [_oracle_evaluate(c, sig, False) for c in _batch_models()]
    return {0: np.array([r[0] for r in rows]), 1: np.array([r[1] for r in rows]), 2: np.array([r[2] for r in rows])}


@op("evaluate_batch", "evaluate_batch", ["td_evaluate_batch"], sigma=True, oracle=_oracle_batch)
def _evaluate_batch(s):
    return s.ctx.evaluate_batch(_batch_models())


def misfit_inputs(n, pair):
    """(ptS, tS, sigma): pair B is pair A with another sigma, pair C pair A with another tS -- td_misfit
    re-uploads the two only when a memcmp says that one of them changed, so each must change alone."""
    rng = np.random.default_rng(500 + n)
    ptS = rng.uniform(0.0, 0.4, n)
    tS = np.random.default_rng(600 + (pair == "C")).uniform(0.0, 0.4, n)
    sig = np.random.default_rng(700 + (pair == "B")).uniform(0.01, 0.1, n)
    return ptS, tS, sig


def _add_misfit(n, pair):
    def fn(s):
        return s.ctx.misfit(*misfit_inputs(n, pair))

    def orc():
        import oracle

        ptS, tS, sig = misfit_inputs(n, pair)
        return {0: oracle.chi2(ptS, tS, sig), 1: oracle.likelihood(sig)}

    OPS.append(Op("misfit_%d_%s" % (n, pair), "misfit", fn, ["td_misfit"], oracle=orc))


for _pair in "ABC":
    _add_misfit(MISFIT_N[0], _pair)
_add_misfit(MISFIT_N[1], "A")


def _add_sigma(name, scale):
    def fn(s):
        s.sigma_scale = scale
        s.ctx.set_sigma(s.sigma())
        return (s.ctx.likelihood_const,)

    def orc():
        import oracle

        return {0: oracle.likelihood(np.asarray(rays().allSig, dtype=np.float64) * scale)}

    OPS.append(Op(name, "set_sigma", fn, ["td_set_sigma", "td_get_info"], oracle=orc))


_add_sigma("set_sigma_1p5", SIGMA_SCALE)
_add_sigma("set_sigma_back", 1.0)


# ---------------------------------------------------------------- rasterize and what is built on it
def raster_batched_models():
    out = []
    for k, n in enumerate(RASTER_BATCHED[0]):
        c = tuple(a.copy() for a in cells(n, 120 + k)) if n else tuple(np.zeros(0) for _ in range(4))
        if n == 300:
            c[0][::17] = np.nan  # NaN cells never win
        out.append(c)
    return out


def _raster_inputs(which):
    if which == "batched":
        return raster_batched_models(), queries(RASTER_BATCHED[1], 21)
    if which == "per_model":
        return [cells(n, 400 + k) for k, n in enumerate(RASTER_PER_MODEL[0])], queries(RASTER_PER_MODEL[1], 22)
    return [cells(300, 300)], queries(RASTER_BATCHED[1], 23)


def _add_rasterize(which):
    def fn(s):
        m, q = _raster_inputs(which)
        return s.ctx.rasterize(m, *q, want_values=True)

    def orc():
        from oracle import oracle_np

        m, q = _raster_inputs(which)
        mean, std, vals = oracle_np.rasterize(m, *q)
        return {0: mean, 1: std, 2: vals}

    OPS.append(Op("rasterize_" + which, "rasterize", fn, ["td_rasterize"], oracle=orc))


for _w in ("batched", "per_model", "one_model"):
    _add_rasterize(_w)


def marg_models():
    sizes = np.random.default_rng(31).integers(5, 400, MARG_MODELS)
    return [cells(int(n), 140 + k) for k, n in enumerate(sizes)]


MARG_PROBS = (0.05, 0.5, 0.95)


def _add_marginals(name, probs, bins, method):
    def fn(s):
        s.ctx.set_marginals_method(method)
        try:
            r = s.ctx.marginals(marg_models(), *queries(MARG_NODES, 32), probs=probs, bins=bins)
        finally:
            s.ctx.set_marginals_method(0)
        return flat(r, ("mean", "std", "quantiles", "hist"))

    def orc():
        from oracle import oracle_np

        mean, std, vals = oracle_np.rasterize(marg_models(), *queries(MARG_NODES, 32))
        out = {0: mean, 1: std}
        if len(probs):  # Julia's default quantile (include/tdstar.h), the weights from the host hook
            v = np.sort(vals, axis=0)
            M = len(v)
            rows = []
            for p in probs:
                j, g = ctypes.c_int64(), ctypes.c_double()
                assert tt().lib().tdt_quantile_rank(M, float(p), ctypes.byref(j), ctypes.byref(g)) == 0
                a, b = v[j.value - 1], v[j.value] if M > 1 else v[0]
                rows.append(a + g.value * (b - a))
            out[2] = np.array(rows)
        if bins is not None:
            nb, lo, hi = bins
            w = (hi - lo) / nb
            slot = np.where(vals < lo, 0, np.where(vals >= hi, nb + 1,
                                                  1 + np.minimum(np.floor((vals - lo) / w), nb - 1))).astype(np.int64)
            hist = np.zeros((vals.shape[1], nb + 3), dtype=np.int64)
            for q in range(vals.shape[1]):
                hist[q] = np.bincount(slot[:, q], minlength=nb + 3)
            out[3 if len(probs) else 2] = hist
        return out

    OPS.append(Op(name, "marginals", fn, ["td_rasterize_marginals"], oracle=orc))


_add_marginals("marginals_hist50", (), (50, 0.0, 50.0), 0)
for _m, _mn in ((1, "resident"), (2, "streaming")):
    _add_marginals("marginals_3probs_8bins_" + _mn, MARG_PROBS, (8, 0.0, 50.0), _m)
    _add_marginals("marginals_3probs_nobins_" + _mn, MARG_PROBS, None, _m)


def conv_values(lens):
    from convergence_ref import ar1

    return ar1(np.random.default_rng(50 + len(lens)), 0.6, int(sum(lens)), 7)


def conv_models(lens):
    sizes = np.random.default_rng(60 + len(lens)).integers(5, 60, int(sum(lens)))
    return [cells(int(n), 1000 + k) for k, n in enumerate(sizes)]


CONV_NODES = 50


def _add_convergence(lens, lag):
    tag = "%dx%d_lag%d" % (len(lens), lens[0], lag)

    def fn_values(s):
        return flat(s.ctx.convergence(conv_values(lens), lens, max_lag=lag), ("rhat", "ess", "lags"))

    def orc_values():
        import convergence_ref

        r = convergence_ref.convergence(conv_values(lens), lens, lag)
        return {0: r["rhat"], 1: r["ess"], 2: r["lags"]}

    def fn_models(s):
        r = s.ctx.convergence_models(conv_models(lens), lens, *queries(CONV_NODES, 61), max_lag=lag)
        return flat(r, ("mean", "std", "rhat", "ess", "lags"))

    def orc_models():
        import convergence_ref
        from oracle import oracle_np

        mean, std, vals = oracle_np.rasterize(conv_models(lens), *queries(CONV_NODES, 61))
        r = convergence_ref.convergence(vals, lens, lag)
        return {0: mean, 1: std, 2: r["rhat"], 3: r["ess"], 4: r["lags"]}

    OPS.append(Op("convergence_" + tag, "convergence", fn_values, ["td_convergence_values"], oracle=orc_values))
    OPS.append(Op("convergence_models_" + tag, "convergence_models", fn_models, ["td_rasterize_convergence"],
                  oracle=orc_models))


for _l in CONV_CHAINS:
    for _g in CONV_LAGS:
        _add_convergence(_l, _g)


def ensemble(nm):
    sizes = np.random.default_rng(70 + nm).integers(100, 700, nm)
    return [cells(int(n), 2000 + 10 * nm + k) for k, n in enumerate(sizes)]


COV_TARGETS = np.array([[200.0, 100.0, 150.0], [800.0, -50.0, 400.0], [500.0, 300.0, 50.0]])


def cov_series(nm):
    return np.random.default_rng(90 + nm).normal(0.0, 1.0, (nm, 2))


def _add_ensemble_ops(nm, forced):
    tag = "%d_%s" % (nm, "forced" if forced else "auto")
    q = lambda: queries(ENSEMBLES[nm], 80 + nm)  # noqa: E731

    def fn_volume(s):
        s.ctx.set_volume_slab_nodes(FORCED_SLAB_NODES if forced else 0)
        try:
            r = s.ctx.volume(ensemble(nm), *q(), probs=MARG_PROBS, bins=(8, 0.0, 50.0), chain_len=[nm // 2, nm // 2],
                             want_values=True)
        finally:
            s.ctx.set_volume_slab_nodes(0)
        return flat(r, ("mean", "std", "values", "quantiles", "hist", "rhat", "ess", "lags"))

    def orc_volume():
        from oracle import oracle_np

        mean, std, vals = oracle_np.rasterize(ensemble(nm), *q())
        return {0: mean, 1: std, 2: vals}

    def fn_predict(s):
        s.ctx.set_predict_plan(*(FORCED_PREDICT if forced else (0, 0)))
        try:
            r = s.ctx.predict(ensemble(nm), probs=MARG_PROBS, bins=(8, 0.0, 0.5), chain_len=[nm // 2, nm // 2],
                              want_values=True)
        finally:
            s.ctx.set_predict_plan(0, 0)
        return flat(r, ("phi", "mean", "std", "ptS", "quantiles", "hist", "rhat", "ess", "lags"))

    def orc_predict(sig):
        rows = [_oracle_evaluate(c, sig, False) for c in ensemble(nm)]
        return {0: np.array([r[1] for r in rows]), 3: np.array([r[0] for r in rows])}

    def fn_cov(s):
        s.ctx.set_volume_slab_nodes(FORCED_SLAB_NODES if forced else 0)
        try:
            r = s.ctx.covariance(ensemble(nm), *q(), targets=COV_TARGETS, series=cov_series(nm))
        finally:
            s.ctx.set_volume_slab_nodes(0)
        return flat(r, ("cov", "corr", "mean", "std", "target_mean", "target_std"))

    def orc_cov():
        import covariance_ref

        r = covariance_ref.covariance(ensemble(nm), *q(), *COV_TARGETS.T, series=cov_series(nm))
        return {k: r[n] for k, n in enumerate(("cov", "corr", "mean", "std", "target_mean", "target_std"))}

    OPS.append(Op("volume_" + tag, "volume", fn_volume, ["td_rasterize_volume"], oracle=orc_volume))
    OPS.append(Op("predict_" + tag, "predict", fn_predict, ["td_rasterize_predict"], oracle=orc_predict, sigma=True))
    OPS.append(Op("covariance_" + tag, "covariance", fn_cov, ["td_rasterize_covariance"], oracle=orc_cov))


for _nm in ENSEMBLES:
    for _f in (False, True):
        _add_ensemble_ops(_nm, _f)


# ---------------------------------------------------------------- histories
def chain_of(s, ncells, max_cells, seed, engine=None, start_seed=None):
    t = tt()
    prm = t.define_TDstructrure().replace(max_cells=max_cells)
    p = t.chain_params(prm, None, seed=seed, chain=1, engine=t.TD_ENGINE_DEVICE if engine is None else engine)
    return t.Chain(s.ctx, p, t.random_model(ncells, seed if start_seed is None else start_seed))


def record(s, seed):
    """A DEVICE chain of 300 cells recording 12 samples into a new History."""
    H = HISTORY
    ch = chain_of(s, H["cells"], H["max_cells"], seed)
    hist = tt().History(s.ctx, H["samples"], H["samples"] * H["max_cells"])
    try:
        ch.run_recorded(H["iterations"], H["first"], H["every"], hist)
    finally:
        ch.close()
    return hist


def session_histories(s, k):
    if s.sigma_scale not in s.histories:
        s.histories[s.sigma_scale] = [record(s, 71), record(s, 72)]
    return s.histories[s.sigma_scale][:k]


def read_tuple(h):
    a = h.read_arrays()
    return flat(a, ("off", "x", "y", "z", "zeta", "phi", "iter", "action", "accept", "ptS"))


@op("history_record", "history", ["td_history_create", "td_chain_create", "td_chain_run_recorded", "td_history_count",
                                  "td_history_read", "td_history_destroy", "td_chain_destroy"])
def _history_record(s):
    h = record(s, 73)
    try:
        return read_tuple(h)
    finally:
        h.close()


H_NODES = 150


def _add_history_ops(k):
    hq = lambda: queries(H_NODES, 75)  # noqa: E731
    hs = lambda s: session_histories(s, k)  # noqa: E731
    tag = "_%dh" % k

    def add(name, reaches, fn):
        OPS.append(Op("history_" + name + tag, "history", fn, reaches))

    add("read", ["td_history_read", "td_history_count"], lambda s: sum((read_tuple(h) for h in hs(s)), ()))
    add("rasterize", ["td_history_rasterize"], lambda s: s.ctx.rasterize_history(hs(s), *hq(), want_values=True))
    add("marginals", ["td_history_marginals"],
        lambda s: flat(s.ctx.marginals_history(hs(s), *hq(), probs=MARG_PROBS, bins=(8, 0.0, 50.0)),
                       ("mean", "std", "quantiles", "hist")))
    add("zeta_hist", ["td_history_zeta_hist"],
        lambda s: flat(s.ctx.zeta_hist(hs(s), (20, 0.0, 50.0)), ("zeta_hist", "ncells")))
    add("convergence", ["td_history_convergence"],
        lambda s: flat(s.ctx.convergence_history(hs(s), *hq(), max_lag=3), ("mean", "std", "rhat", "ess", "lags")))
    add("volume", ["td_history_volume"],
        lambda s: flat(s.ctx.volume_history(hs(s), *hq(), probs=MARG_PROBS, bins=(8, 0.0, 50.0), convergence=True,
                                            want_values=True),
                       ("mean", "std", "values", "quantiles", "hist", "rhat", "ess", "lags")))
    add("predict", ["td_history_predict"],
        lambda s: flat(s.ctx.predict_history(hs(s), probs=MARG_PROBS, convergence=True, want_values=True),
                       ("phi", "mean", "std", "ptS", "quantiles", "rhat", "ess", "lags")))
    add("covariance", ["td_history_covariance"],
        lambda s: flat(s.ctx.covariance_history(hs(s), *hq(), targets=COV_TARGETS),
                       ("cov", "corr", "mean", "std", "target_mean", "target_std")))


for _k in (1, 2):
    _add_history_ops(_k)


# ---------------------------------------------------------------- chains
STAT_KEYS = ("iterations", "accepted", "proposed", "phi", "ncells", "last_action", "last_accept")


def chain_tuple(ch):
    st, m = ch.stats(), ch.model()
    return tuple(np.asarray(st[k]) for k in STAT_KEYS) + (m.xCell, m.yCell, m.zCell, m.zeta, m.phi, m.ptS)


CHAIN_CALLS = ["td_chain_create", "td_chain_run", "td_chain_stats_get", "td_chain_get_model", "td_chain_destroy"]


def _add_chain(name, engine, lds_mode=None, keeps=False):
    def fn(s):
        ch = chain_of(s, CHAIN["cells"], CHAIN["max_cells"], 91, engine=engine)
        try:
            if lds_mode is not None:
                assert tt().lib().tdt_chain_set_lds_mode(ch.h, lds_mode) == 0
            ch.run(CHAIN["iterations"])
            return chain_tuple(ch)
        finally:
            ch.close()

    OPS.append(Op(name, "chain", fn, CHAIN_CALLS, keeps=keeps))


for _mode in range(4):
    _add_chain("chain_device_lds%d" % _mode, 0, _mode)
_add_chain("chain_host", 1)
_add_chain("chain_dropin", 2, keeps=True)


def _add_batch(n):
    def fn(s):
        chains = [chain_of(s, CHAIN["cells"], CHAIN["max_cells"], 93 + k) for k in range(n)]
        try:
            tt().run_batch(chains, CHAIN["iterations"])
            return sum((chain_tuple(c) for c in chains), ())
        finally:
            for c in chains:
                c.close()

    OPS.append(Op("chain_batch_%d" % n, "chain", fn, CHAIN_CALLS[:1] + ["td_chain_run_batch"] + CHAIN_CALLS[2:]))


for _n in BATCHES:
    _add_batch(_n)


@op("ladder_step", "chain", ["td_chain_create", "td_chain_set_temperature", "td_rounds_create", "td_rounds_run",
                             "td_chain_stats_get", "td_chain_get_model", "td_rounds_destroy", "td_chain_destroy"])
def _ladder_step(s):
    """Three rounds of a resident 4-chain ladder; the last one leaves its launch resident on the session."""
    s.drop_ladder()
    L = LADDER
    chains = [chain_of(s, L["cells"], L["max_cells"], 101 + k) for k in range(L["chains"])]
    lad = tt().TemperingLadder(chains, seed=5)
    s.ladder = (lad, chains)
    out = (lad.step(L["K"]), lad.step(L["K"]))
    out += sum((chain_tuple(c) for c in chains), ())  # (reading the chains ends the launch; the next step restarts it)
    return out + (lad.step(L["K"]), np.array(lad.levels))


def _add_ladder_run(name, recorded, reaches):
    def fn(s):
        """Four rounds and their swap steps inside the library, the cold replica recorded or not."""
        L = LADDER
        chains = [chain_of(s, L["cells"], L["max_cells"], 111 + k) for k in range(L["chains"])]
        lad = tt().TemperingLadder(chains, seed=6)
        hist = tt().History(s.ctx, 4, 4 * L["max_cells"]) if recorded else None
        try:
            out = (lad.run(4, L["K"], history=hist, first=1, every=2), np.array(lad.levels))
            out += sum((chain_tuple(c) for c in chains), ())
            return out + (read_tuple(hist) if recorded else ())
        finally:
            if lad.rounds is not None:
                lad.rounds.close()
            if hist is not None:
                hist.close()
            for c in chains:
                c.close()

    OPS.append(Op(name, "chain", fn, ["td_rounds_create", "td_rounds_destroy", "td_chain_set_temperature"] + reaches))


_add_ladder_run("ladder_run", False, ["td_rounds_temper"])
_add_ladder_run("ladder_run_recorded", True, ["td_rounds_temper_recorded"])


@op("chain_batch_recorded", "chain", ["td_chain_run_batch_recorded"])
def _chain_batch_recorded(s):
    H = HISTORY
    chains = [chain_of(s, H["cells"], H["max_cells"], 121 + k) for k in range(3)]
    hists = [tt().History(s.ctx, H["samples"], H["samples"] * H["max_cells"]) for _ in chains]
    try:
        tt().run_batch_recorded(chains, H["iterations"], H["first"], H["every"], hists)
        return sum((read_tuple(h) for h in hists), ())
    finally:
        for h in hists:
            h.close()
        for c in chains:
            c.close()


# ---------------------------------------------------------------- trilinear (context-free, thread-local cache)
def tri_inputs(shape, npts):
    rng = np.random.default_rng(sum(shape) + npts)
    axes = [np.cumsum(rng.uniform(0.5, 2.0, n)) for n in shape]
    values = rng.uniform(0.05, 0.2, shape)
    pts = [rng.uniform(a[0] - 0.2, a[-1] + 0.2, npts) for a in axes]  # a few outside: NaN
    for p, a in zip(pts, axes):
        p[:3] = a[[0, -1, len(a) // 2]]  # on the first, the last and an inner knot
    return axes, values, pts


def _add_trilinear(shape, npts):
    def fn(s):
        axes, values, pts = tri_inputs(shape, npts)
        v = np.ascontiguousarray(values.ravel(order="F"))
        out = np.empty(npts)
        nout = ctypes.c_int64()
        lib, P = tt().lib(), tt()._lib.ptr
        rc = lib.td_trilinear(s.ctx.device, P(axes[0]), shape[0], P(axes[1]), shape[1], P(axes[2]), shape[2], P(v),
                              P(pts[0]), P(pts[1]), P(pts[2]), npts, P(out), ctypes.byref(nout))
        assert rc == 0, rc
        return out, nout.value

    def orc():
        from oracle import oracle_np

        axes, values, pts = tri_inputs(shape, npts)
        out = oracle_np.trilinear(*axes, values, *pts)
        return {0: out, 1: int(np.isnan(out).sum())}

    OPS.append(Op("trilinear_%dx%dx%d_%dpts" % (shape + (npts,)), "trilinear", fn, ["td_trilinear"], oracle=orc))


for _s in TRI_GRIDS:
    for _p in TRI_POINTS:
        _add_trilinear(_s, _p)


# ---------------------------------------------------------------- modifiers: documented to leave answers unchanged
def _add_modifier(name, call, reaches=()):
    def fn(s):
        call(s)
        return ()

    OPS.append(Op(name, "modifier", fn, reaches, gpu=False))


_add_modifier("timing_on", lambda s: s.ctx.timing(True), ["td_timing_enable"])
_add_modifier("timing_off", lambda s: (s.ctx.timing(kernel="chi2"), s.ctx.timing(False, reset=True)),
              ["td_timing_get", "td_timing_enable", "td_timing_reset"])
for _v in (1, 2, 3, 0):  # (each list ends on the default)
    _add_modifier("set_nn_method_%d" % _v, lambda s, v=_v: s.ctx.set_nn_method(v))
for _v in (0, 1, 2):
    _add_modifier("set_incremental_%d" % _v, lambda s, v=_v: s.ctx.set_incremental(v), ["td_set_incremental"])
for _v in (1, 2, 0):
    _add_modifier("set_volume_method_%d" % _v, lambda s, v=_v: s.ctx.set_volume_method(v))
for _v in (1, 0):
    _add_modifier("set_predict_placement_%d" % _v, lambda s, v=_v: s.ctx.set_predict_placement(v))

BY_NAME = {o.name: o for o in OPS}
assert len(BY_NAME) == len(OPS)
LIGHT = [o for o in OPS if o.name not in HEAVY]
FAMILIES = sorted({o.family for o in OPS})


def pair_list():
    """The ordered pairs (A, B) of the pair test: every pair of light entries, and each heavy entry as A and as
    B against one light entry of every family (the family's k-th, k = the heavy entry's rank, so they spread)."""
    pairs = [(a.name, b.name) for a in LIGHT for b in LIGHT]
    for k, h in enumerate(HEAVY):
        for fam in FAMILIES:
            members = [o for o in LIGHT if o.family == fam]
            m = members[k % len(members)].name
            pairs += [(h, m), (m, h)]
    return pairs


# ---------------------------------------------------------------- references
class References:
    """An operation's answer on a fresh context that did nothing else: created (at the session's sigma),
    called once, closed.  Computed once per (operation, sigma, model edited) and never modified."""

    def __init__(self):
        self.cache = {}

    def key(self, o, s_before_sigma, prop):
        extra = hashlib.sha1(b"".join(np.ascontiguousarray(a).tobytes() for a in prop)).hexdigest() if o.stateful else None
        return (o.name, s_before_sigma, extra)

    def get(self, o, sigma_scale, prop=None):
        k = self.key(o, sigma_scale, prop)
        if k not in self.cache:
            f = Session(sigma_scale)
            try:
                if o.stateful:  # a full evaluate of the edited model: the incremental path off
                    f.ctx.set_incremental(0)
                    ptS, phi, lk, _ = f.ctx.evaluate(prop)
                    out = (ptS, phi, lk)
                else:
                    out = o.fn(f)
            finally:
                f.close()
            self.cache[k] = out
        return self.cache[k]


def run_checked(o, s, refs, counted=False):
    """Run `o` on the session and hold its answer to the reference; -> the answer, or with `counted` the
    resident launches registered to this thread on the call's return (read before the reference is looked
    up: making one runs a fresh context on this thread, which stops them)."""
    sigma = s.sigma_scale
    out = o.fn(s)
    n = s.resident_count() if counted else None
    ref = refs.get(o, sigma, s.edit_prop if o.stateful else None)
    assert same(out, ref), "%s differs from its fresh-context reference: %s" % (o.name, first_difference(out, ref))
    return n if counted else out


# ---------------------------------------------------------------- the header's entry points (coverage guard)
def header_entry_points(path):
    """Every td_* function declared in include/tdstar.h."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(td_[a-z0-9_]+)\s*\(", text)))


# entry points no catalogue operation has to reach, each with one of the three allowed reasons
NO_GPU, CTOR, MULTI_RANK = "does no GPU work", "constructor or destructor", "needs more than one rank"
EXCLUDED = {
    "td_create": CTOR, "td_destroy": CTOR, "td_last_error": NO_GPU, "td_swap_decide": NO_GPU,
    "td_history_clear": NO_GPU,
    "td_comm_unique_id": MULTI_RANK, "td_comm_create": MULTI_RANK, "td_comm_allgather": MULTI_RANK,
    "td_comm_destroy": MULTI_RANK, "td_rounds_exchange": MULTI_RANK, "td_rounds_exchange_recorded": MULTI_RANK,
}
