"""GPU: the convergence diagnostics (td_convergence_values, td_rasterize_convergence,
td_history_convergence) against the numpy restatement of tests/convergence_ref.py, bit for bit: R-hat and
ESS with np.array_equal(equal_nan=True), lags exactly."""
import numpy as np
import pytest

import convergence_ref as cref

pytestmark = pytest.mark.gpu

LAYOUTS = ([4], [5], [4, 5], [9, 8, 31], [64, 64], [65], [129, 130, 131], [40] * 8, [6] * 33)
NCOLS = (1, 64, 130)  # 130: three tiles, the last one partial
MAX_LAGS = (0, 1, 2, 5, 1000)
NKINDS = 8


@pytest.fixture(scope="module")
def ctx(tt, ds):
    return tt.TdContext.from_datastruct(ds)


def mixed_columns(lens, ncol, seed):
    """V[M, ncol], column k of kind k % 8, so every 64-column tile holds every kind: iid normal; AR(1)
    with phi = 0.9; alternating +-1 (the floor); constant (NaN); constant within each sequence but
    different across them (W = 0: rhat = +inf, every rho = 1 until the cap); one NaN entry; +-1e300
    (the squares overflow); three distinct values (the ties a Voronoi node shows)."""
    rng = np.random.default_rng(seed)
    M = int(np.sum(lens))
    p = cref.plan(lens)
    V = np.empty((M, ncol))
    V[:, 0::NKINDS] = rng.standard_normal((M, len(range(0, ncol, NKINDS))))
    for k in range(ncol):
        kind = k % NKINDS
        if kind == 1:
            V[:, k] = cref.ar1(rng, 0.9, M, 1)[:, 0]
        elif kind == 2:
            V[:, k] = np.where(np.arange(M) % 2 == 0, 1.0, -1.0)
        elif kind == 3:
            V[:, k] = 17.25
        elif kind == 4:
            V[:, k] = -1.0
            for s, a in enumerate(p["seq_start"]):
                V[a:a + p["n"], k] = 3.0 + 0.25 * s
        elif kind == 5:
            V[:, k] = rng.uniform(0, 50, M)
            V[p["seq_start"][-1] + 1, k] = np.nan
        elif kind == 6:
            V[:, k] = rng.choice([-1e300, 1e300], M)
        elif kind == 7:
            V[:, k] = rng.choice([12.5, 20.0, 31.25], M, p=[0.6, 0.3, 0.1])
    return V


def assert_same(got, ref, ncol=None, fields=("rhat", "ess", "lags")):
    for f in fields:
        r = ref[f] if ncol is None else ref[f][:ncol]
        assert got[f].shape == r.shape and got[f].dtype == r.dtype, f
        assert np.array_equal(got[f], r, equal_nan=f != "lags"), (f, got[f], r)


@pytest.mark.parametrize("lens", LAYOUTS, ids=lambda v: "x".join(map(str, v[:3])) + ("_%d" % len(v) if len(v) > 3 else ""))
def test_values_against_the_restatement(ctx, lens):
    """The restatement is column by column, so one reference over 130 columns serves the narrower calls."""
    V = mixed_columns(lens, max(NCOLS), seed=len(lens) * 1000 + lens[0])
    for max_lag in MAX_LAGS:
        ref = cref.convergence(V, lens, max_lag)
        for ncol in NCOLS:
            got = ctx.convergence(V[:, :ncol], lens, max_lag)
            assert_same(got, ref, ncol)
    # the kinds do what they are there for (the last reference: max_lag above n)
    p = cref.plan(lens)
    assert np.all(np.isnan(ref["rhat"][3::NKINDS])) and np.all(np.isnan(ref["ess"][3::NKINDS]))
    assert np.all(np.isposinf(ref["rhat"][4::NKINDS])) and np.all(ref["lags"][4::NKINDS] < 0)
    assert np.all(np.isnan(ref["rhat"][5::NKINDS])) and np.all(np.isnan(ref["ess"][5::NKINDS]))
    if p["n"] % 2 == 0:  # every half holds as many +1 as -1
        assert np.all(ref["ess"][2::NKINDS] == p["m"] * p["n"] / p["tau_floor"])


def test_one_column_vector_and_scalar_shapes(ctx):
    rng = np.random.default_rng(3)
    v = rng.standard_normal(37)
    got = ctx.convergence(v, [17, 20], 4)
    assert_same(got, cref.convergence(v, [17, 20], 4))
    assert got["rhat"].shape == (1,) and got["lags"].dtype == np.int32


def test_rounds_and_lag_blocks_give_the_same(ctx):
    lens = [129, 130, 131]
    V = mixed_columns(lens, 130, seed=99)
    ref = cref.convergence(V, lens, 0)
    # columns of one tile stop in different rounds of two lags
    assert len(set((np.abs(ref["lags"][:64]) // 2).tolist())) >= 3
    try:
        for LB in (8, 16, 0):
            ctx.set_convergence_lag_block(LB)
            for R in (2, 6, 64, 0):
                ctx.set_convergence_round(R)
                assert_same(ctx.convergence(V, lens, 0), ref)
        ctx.set_convergence_round(2)
        ctx.timing(enable=True, reset=True)
        ctx.convergence(V, lens, 0)
        rounds = ctx.timing(kernel="conv_geyer")[0]
        assert ctx.timing(kernel="conv_moments")[0] == 1 and ctx.timing(kernel="conv_autocov")[0] == rounds
        assert rounds == 32  # n = 64: lags 1 | 2, 3 | ... | 62, 63; the W = 0 columns go on to the end
        ctx.timing(reset=True)
        early = [0, 2, 3, 7]  # iid, the floor, a constant, three values: all stop on their own, early
        assert np.all(ref["lags"][early] > 0)
        ctx.convergence(V[:, early], lens, 0)
        # the pair after lag `last` fails in round (last + 1) / 2, counted from 0; then the count is zero
        assert ctx.timing(kernel="conv_geyer")[0] == ref["lags"][early].max() // 2 + 2 < 32
        ctx.timing(reset=True)
        ctx.convergence(V, lens, 0, want=("rhat",))
        assert ctx.timing(kernel="conv_autocov")[0] == 0 and ctx.timing(kernel="conv_moments")[0] == 1
        with pytest.raises(Exception):
            ctx.set_convergence_round(3)
        with pytest.raises(Exception):
            ctx.set_convergence_lag_block(4)
    finally:
        ctx.timing(enable=False)
        ctx.set_convergence_round(0)
        ctx.set_convergence_lag_block(0)


def test_request_subsets(ctx):
    lens = [9, 8, 31]
    V = mixed_columns(lens, 130, seed=5)
    full = ctx.convergence(V, lens, 0)
    assert_same(full, cref.convergence(V, lens, 0))
    for f in ("rhat", "ess", "lags"):
        one = ctx.convergence(V, lens, 0, want=(f,))
        assert set(one) == {f}
        assert np.array_equal(one[f], full[f], equal_nan=f != "lags"), f


def test_argument_errors_with_a_context(tt, ctx):
    V = np.zeros((9, 3))
    for lens in ([4, 4], [3, 6], []):
        with pytest.raises(tt.TdError, match="td_convergence_values"):
            ctx.convergence(V, lens)
    with pytest.raises(tt.TdError, match="td_convergence_values"):
        ctx.convergence(V, [9], max_lag=-1)
    with pytest.raises(tt.TdError, match="td_convergence_values"):
        ctx.convergence(V, [9], want=())


@pytest.fixture(scope="module")
def ensemble(tt, ctx):
    """Three chains on the shipped geometry, every 10th of 300 proposals recorded in one launch; the first
    chain goes on for 50 more, so the lengths are 35, 30, 30 and its first rows are skipped."""
    prm = tt.define_TDstructrure().replace(max_cells=300)
    chains = [tt.Chain(ctx, tt.chain_params(prm, None, seed=40 + k, chain=k + 1), tt.random_model(150, 40 + k))
              for k in range(3)]
    hists = [tt.History(ctx, 40, 40 * 300, with_ptS=False) for _ in chains]
    tt.run_batch_recorded(chains, 300, 10, 10, hists)
    chains[0].run_recorded(50, 10, 10, hists[0])
    assert [len(h) for h in hists] == [35, 30, 30]
    rng = np.random.default_rng(21)
    qx = np.concatenate([rng.uniform(-100, 1100, 130), [9e4]])  # the last: far outside the cells' box
    qy = np.concatenate([rng.uniform(-200, 500, 130), [9e4]])
    qz = np.concatenate([rng.uniform(-10, 700, 130), [9e4]])
    return chains, hists, (qx, qy, qz)


def test_three_routes_on_an_ensemble(ctx, ensemble):
    _, hists, q = ensemble
    lens = [len(h) for h in hists]
    mean, std, V = ctx.rasterize_history(hists, *q, want_values=True)
    for max_lag in (0, 3):
        a = ctx.convergence_history(hists, *q, max_lag=max_lag)
        b = ctx.convergence(V, lens, max_lag)
        c = ctx.convergence_models([m.cells() for h in hists for m in h.read()], lens, *q, max_lag=max_lag)
        assert_same(a, b)
        assert_same(c, b)
        assert_same(b, cref.convergence(V, lens, max_lag))
        for r in (a, c):
            assert np.array_equal(r["mean"], mean) and np.array_equal(r["std"], std, equal_nan=True)
    # a history without samples is skipped
    empty = type(hists[0])(ctx, 4, 4 * 300, with_ptS=False)
    d = ctx.convergence_history([hists[0], empty, hists[1], hists[2]], *q)
    assert_same(d, ctx.convergence(V, lens))


def test_trace_diagnostics(tt, ctx, ensemble):
    _, hists, _ = ensemble
    arrs = [h.read_arrays() for h in hists]
    T = np.concatenate([np.column_stack([a["phi"], np.diff(a["off"]).astype(np.float64)]) for a in arrs])
    lens = [len(h) for h in hists]
    ref = ctx.convergence(T, lens)
    assert_same(ref, cref.convergence(T, lens))
    got = tt.trace_diagnostics(hists)
    for k, name in enumerate(("phi", "ncells")):
        for f in ("rhat", "ess", "lags"):
            assert np.array_equal(got[name][f], ref[f][k], equal_nan=True), (name, f)
    one = tt.trace_diagnostics(hists[0], max_lag=2)
    ref1 = ctx.convergence(T[:35], [35], 2)
    assert np.array_equal(one["phi"]["ess"], ref1["ess"][0], equal_nan=True) and one["ncells"]["lags"] == ref1["lags"][1]


def test_convergence_maps(tt, ds):
    prm = tt.define_TDstructrure().replace(xzMap=True, ySlice=[0, 150], xyMap=True, zSlice=[100])
    hist = [[tt.random_model(80 + 10 * j, 10 * c + j) for j in range(6 + c)] for c in range(2)]  # chains of 6 and 7
    cred = tt.credible_maps(hist, ds, prm, probs=(0.5,))
    maps = tt.convergence_maps(hist, ds, prm, max_lag=0)
    assert set(maps) == set(cred) == {("xz", 0), ("xz", 150), ("xy", 100)}
    ctx = tt.context_for(ds)
    flat = [m.cells() for chain in hist for m in chain]
    xv, yv, zv = (np.asarray(v, dtype=np.float64) for v in (ds.xVec, ds.yVec, ds.zVec))
    i, j = 7, 11
    for key, m in maps.items():
        n2 = len(zv) if key[0] == "xz" else len(yv)
        for f in ("rhat", "ess", "lags", "mean", "std"):
            assert m[f].shape == cred[key]["mean"].shape == (len(xv), n2), f
        assert m["lags"].dtype == np.int32
        assert np.array_equal(m["mean"], cred[key]["mean"]) and np.array_equal(m["std"], cred[key]["std"], equal_nan=True)
        node = ([xv[i]], [key[1]], [zv[j]]) if key[0] == "xz" else ([xv[i]], [yv[j]], [key[1]])
        one = ctx.convergence_models(flat, [6, 7], *node)
        for f in ("rhat", "ess", "lags"):
            assert np.array_equal(m[f][i, j], one[f][0], equal_nan=True), (key, f)
        V = ctx.rasterize(flat, *node, want_values=True)[2]
        assert_same(one, cref.convergence(V, [6, 7]), fields=("rhat", "ess", "lags"))
        s = m["summary"]
        assert (s["n"], s["m"]) == (3, 4)
        rh, es, lg = m["rhat"], m["ess"], m["lags"]
        assert s["rhat_max"] == np.nanmax(rh) and s["ess_min"] == np.nanmin(es)
        assert s["frac_rhat_above_1_01"] == np.mean(rh > 1.01) and s["frac_capped"] == np.mean(lg < 0)
        assert s["nan_columns"] == int(np.sum(np.isnan(rh) | np.isnan(es)))
    # a flat list is one chain; a list of histories is one chain per history
    one_chain = tt.convergence_maps(hist[1], ds, prm.replace(xyMap=False, ySlice=[0]))[("xz", 0)]
    assert (one_chain["summary"]["n"], one_chain["summary"]["m"]) == (3, 2)


def test_does_not_disturb_marginals_and_rasterize(tt, ds, ctx, ensemble):
    """The cached device buffers are shared: what follows a diagnostics call is what it is alone."""
    _, hists, q = ensemble
    rng = np.random.default_rng(8)
    models = [tt.random_model(20 + k, 300 + k).cells() for k in range(12)]
    probs, bins = (0.05, 0.5, 0.95), (10, 0.0, 50.0)
    alone = tt.TdContext.from_datastruct(ds)
    m0 = alone.marginals(models, *q, probs, bins)
    r0 = alone.rasterize(models, *q, want_values=True)
    V = rng.standard_normal((500, 200))  # larger than the value matrix of the calls around it
    ctx.convergence_models(models, [12], *q)
    ctx.convergence(V, [250, 250])
    m1 = ctx.marginals(models, *q, probs, bins)
    ctx.convergence_history(hists, *q)
    r1 = ctx.rasterize(models, *q, want_values=True)
    for f in ("mean", "std", "quantiles", "hist"):
        assert np.array_equal(m0[f], m1[f], equal_nan=True), f
    for a, b in zip(r0, r1):
        assert np.array_equal(a, b, equal_nan=True)
    c1 = ctx.convergence_models(models, [12], *q)
    assert_same(c1, alone.convergence(r0[2], [12]))
