"""The chain's nearest-cell query with a killed and a moved cell, on live chains (tdt_chain_nearest), and the
bucket grid against the cell arrays (tdt_chain_grid_check).

Every death query, every orphan re-search of a death or a move and every drop-in query with a pending edit
passes a killed slot (`skip`) or a moved slot with its proposed site to wave_grid_search and, unproven, to
wave_full_scan (csrc/chain_search.h).  Here each query is asked with its exact nearest cell killed, moved
away, a far cell moved onto it, a cell moved onto the winner's exact site (a tie) and with no edit, through
the product's grid search (mode 0), the descriptor form (6) and wave_nearest (7), against
nearest_ref.model_nearest on the chain's model in Julia order.  A failure names the variant and the query."""
import numpy as np
import pytest

import nearest_ref as nr

pytestmark = pytest.mark.gpu

VARIANTS = ["a: nearest cell killed", "b: nearest cell moved to a far corner", "c: a far cell moved onto the query",
            "d: a lower cell moved onto the nearest cell's site", "d: a higher cell moved onto the nearest cell's site",
            "e: no edit"]


def P(a):
    return a.ctypes.data


@pytest.fixture(scope="module")
def ctx(tt, ds):
    return tt.TdContext.from_datastruct(ds)


@pytest.fixture
def make(tt, ctx):
    """make(prm, model, seed): a device chain on the module's context, closed when the test ends -- also when
    it fails (a chain must not outlive its context)."""
    made = []

    def factory(prm, model, seed, chain=1):
        p = tt.chain_params(prm, None, seed=seed, chain=chain, temperature=1.0, engine=tt.TD_ENGINE_DEVICE)
        made.append(tt.Chain(ctx, p, model))
        return made[-1]

    yield factory
    for ch in made:
        ch.close()


def grid_check(tt, ch):
    out = np.full(8, -1, dtype=np.int64)
    assert tt.lib().tdt_chain_grid_check(ch.h, P(out)) == 0
    return dict(none=int(out[0]), many=int(out[1]), differ=int(out[2]), misplaced=int(out[3]), badslot=int(out[4]),
                overflow=int(out[5]), maxcount=int(out[6]), nslots=int(out[7]))


def assert_grid_sound(g, what):
    """All counts 0 while the overflow flag is clear; with it set, cells may only be missing from the grid."""
    bad = {k: g[k] for k in ("many", "differ", "misplaced", "badslot") if g[k]}
    assert not bad, (what, g)
    if not g["overflow"]:
        assert g["none"] == 0, (what, g)
        assert g["maxcount"] <= 32, (what, g)


def chain_model(tt, clustered):
    """The two chains of test_grid_query_forms_agree (test_gpu_chain.py)."""
    rng = np.random.default_rng(9 if clustered else 8)
    if clustered:
        xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
        k = 300
        x = np.concatenate([rng.uniform(400, 402, k), rng.uniform(xmin, xmax, 200)])
        y = np.concatenate([rng.uniform(100, 102, k), rng.uniform(ymin, ymax, 200)])
        z = np.concatenate([rng.uniform(300, 302, k), rng.uniform(zmin, zmax, 200)])
        x[7], y[7], z[7] = x[6], y[6], z[6]
        x[k + 5], y[k + 5], z[k + 5] = x[k + 4], y[k + 4], z[k + 4]
        return tt.Model(float(len(x)), x, y, z, rng.uniform(1, 49, len(x))), rng
    model = tt.random_model(5000, 3)
    for a, b in ((10, 11), (200, 4000)):  # exact duplicates: a query at the site ties at distance 0
        model.xCell[b], model.yCell[b], model.zCell[b] = model.xCell[a], model.yCell[a], model.zCell[a]
    return model, rng


def ask(tt, ch, mode, pts, kill, moved, msite):
    nq = len(pts)
    d, z = np.full(nq, -7.0), np.full(nq, -7.0)
    proven, pos = np.full(nq, -7, dtype=np.int32), np.full(nq, -7, dtype=np.int32)
    info = np.zeros(4, dtype=np.int64)
    rc = tt.lib().tdt_chain_nearest(ch.h, P(pts), P(kill), P(moved), P(msite), nq, mode, P(d), P(z), P(proven), P(pos),
                                    P(info))
    assert rc == 0, (mode, rc)
    return d, z, proven != 0, pos, dict(nslots=int(info[0]), cap=int(info[1]), ncells=int(info[2]),
                                         overflow=int(info[3]))


@pytest.mark.parametrize("clustered", [False, True])
def test_killed_and_moved_cells_through_the_grid(tt, ds, make, clustered):
    model, rng = chain_model(tt, clustered)
    prm = tt.define_TDstructrure().replace(max_cells=10000)
    ch = make(prm, model, 23)
    assert_grid_sound(grid_check(tt, ch), "after creation")
    ch.run(300)
    m = ch.model()
    cells = np.stack([m.xCell, m.yCell, m.zCell], 1).astype(np.float64)
    zeta = np.asarray(m.zeta, dtype=np.float64)
    n = len(cells)
    # ---- the queries: ray points, points over the rays' box, far points, cells' own sites ----
    X, Y, Z = (np.asarray(a, dtype=np.float64).ravel() for a in (ds.rayX, ds.rayY, ds.rayZ))
    ok = ~np.isnan(X)
    X, Y, Z = X[ok], Y[ok], Z[ok]
    sel = rng.integers(0, len(X), 600)
    lo, hi = np.array([X.min(), Y.min(), Z.min()]), np.array([X.max(), Y.max(), Z.max()])
    over = lo - 50.0 + (hi - lo + 100.0) * rng.random((600, 3))
    far = lo - 1000.0 + (hi - lo + 2000.0) * rng.random((150, 3))
    sites = cells[rng.integers(0, n, 150)]
    q = np.ascontiguousarray(np.concatenate([np.stack([X[sel], Y[sel], Z[sel]], 1), over, far, sites]))
    nq = len(q)
    assert nq == 1500
    # ---- the edits, from the exact nearest cell c1 and the runner-up c2 ----
    c1, c2 = nr.model_two_nearest(cells, q)
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    blo, bhi = np.array([xmin, ymin, zmin]), np.array([xmax, ymax, zmax])
    corner = np.where(np.abs(q - blo) > np.abs(q - bhi), blo, bhi)  # the prior box's corner farthest from the query
    other = (c1 + 1 + rng.integers(0, n - 1, nq)) % n  # a cell other than c1 ...
    dist_other = nr.dist2(cells[other, 0], cells[other, 1], cells[other, 2], q[:, 0], q[:, 1], q[:, 2])
    d1 = nr.dist2(cells[c1, 0], cells[c1, 1], cells[c1, 2], q[:, 0], q[:, 1], q[:, 2])
    assert (dist_other >= d1).all()
    lower = np.where(c1 > 0, (rng.random(nq) * c1).astype(np.int64), -1)  # a position below c1 (none below 0)
    higher = np.where(c1 < n - 1, c1 + 1 + (rng.random(nq) * (n - 1 - c1)).astype(np.int64), -1)
    assert ((lower < c1) & (lower >= -1)).all() and ((higher == -1) | ((higher > c1) & (higher < n))).all()
    none = np.full(nq, -1, dtype=np.int64)
    zero = np.zeros((nq, 3))
    edits = [(c1, none, zero), (none, c1, corner), (none, other, q), (none, lower, cells[c1]), (none, higher, cells[c1]),
             (none, none, zero)]
    used = [np.ones(nq, bool)] * 3 + [lower >= 0, higher >= 0, np.ones(nq, bool)]
    assert all(u.sum() > nq // 2 for u in used)
    pts = np.ascontiguousarray(np.concatenate([q] * len(edits)))
    kill = np.ascontiguousarray(np.concatenate([e[0] for e in edits]), dtype=np.int32)
    moved = np.ascontiguousarray(np.concatenate([e[1] for e in edits]), dtype=np.int32)
    msite = np.ascontiguousarray(np.concatenate([e[2] for e in edits]), dtype=np.float64)
    used = np.concatenate(used)
    variant = np.repeat(np.arange(len(edits)), nq)
    rd, rp, rz = nr.model_nearest(cells, zeta, pts, kill, moved, msite)
    # (the reference against the construction: a and b give the runner-up, c the moved cell at d = 0 unless a
    # cell's own site ties it, d the lower of the two positions)
    assert np.array_equal(rp[:nq], c2) and np.array_equal(rp[nq:2 * nq], c2)
    assert (rd[2 * nq:3 * nq] == 0.0).all() and (rp[2 * nq:3 * nq] <= other).all()
    assert np.array_equal(rp[3 * nq:4 * nq][lower >= 0], lower[lower >= 0])
    assert np.array_equal(rp[4 * nq:5 * nq], c1) and np.array_equal(rp[5 * nq:], c1)

    def first_bad(mask):
        i = int(np.flatnonzero(mask)[0])
        return "%s, query %d at %s (kill %d, moved %d at %s)" % (VARIANTS[variant[i]], i % nq, pts[i], kill[i], moved[i],
                                                                  msite[i])

    got = {mode: ask(tt, ch, mode, pts, kill, moved, msite) for mode in (0, 6, 7)}
    info = got[7][4]
    assert info["ncells"] == n and info["nslots"] <= info["cap"]
    if clustered:
        assert info["overflow"] == 1  # (the packed buckets overflow: every mode-7 answer is the full scan's)
    else:
        assert info["overflow"] == 0
        assert info["nslots"] > info["ncells"], info  # (interior free slots: deaths left holes below the mark)
    # mode 7 equals the reference on every query of every variant
    d, z, _, pos, _ = got[7]
    bad = used & ((d != rd) | (pos != rp) | (z != rz))
    assert not bad.any(), ("mode 7: %d differ; first: %s: got (d, pos, z) = (%r, %d, %r), expected (%r, %d, %r)"
                           % (bad.sum(), first_bad(bad), d[bad][0], pos[bad][0], z[bad][0], rd[bad][0], rp[bad][0],
                              rz[bad][0]))
    # modes 0 and 6: every proven answer equals the reference; the two agree on (d, z, proven) everywhere
    for mode in (0, 6):
        d, z, pv, pos, _ = got[mode]
        bad = used & pv & ((d != rd) | (pos != rp) | (z != rz))
        assert not bad.any(), ("mode %d: %d proven answers differ; first: %s: got (d, pos, z) = (%r, %d, %r), "
                               "expected (%r, %d, %r)" % (mode, bad.sum(), first_bad(bad), d[bad][0], pos[bad][0],
                                                          z[bad][0], rd[bad][0], rp[bad][0], rz[bad][0]))
        tie = used & pv & ((variant == 3) | (variant == 4))
        assert not tie.any(), "mode %d proves a tie: %s" % (mode, first_bad(tie))
    bad = used & ((got[0][0] != got[6][0]) | (got[0][1] != got[6][1]) | (got[0][2] != got[6][2]))
    assert not bad.any(), "modes 0 and 6 differ: %s" % first_bad(bad)
    if not clustered:
        for v in range(3):  # (without this the proven-only check could pass empty)
            share = got[0][2][variant == v].mean()
            print("variant %s: %.3f of the queries proven in mode 0" % (VARIANTS[v], share))
            assert share > 0.5, (VARIANTS[v], share)
    else:
        assert not got[0][2].any() and not got[6][2].any()
    assert_grid_sound(grid_check(tt, ch), "after 300 iterations")


def test_chain_nearest_refuses_bad_positions(tt, make):
    ch = make(tt.define_TDstructrure().replace(max_cells=60), tt.random_model(50, 4), 5)
    pts, ms = np.zeros((1, 3)), np.zeros((1, 3))
    for kill, moved in ((50, -1), (-1, 50), (-2, -1), (-1, -2)):
        k, mv = np.array([kill], dtype=np.int32), np.array([moved], dtype=np.int32)
        with pytest.raises(AssertionError):
            ask(tt, ch, 7, pts, k, mv, ms)
    with pytest.raises(AssertionError):
        ask(tt, ch, 3, pts, np.array([-1], dtype=np.int32), np.array([-1], dtype=np.int32), ms)
    d, z, pv, pos, info = ask(tt, ch, 7, pts, np.array([49], dtype=np.int32), np.array([0], dtype=np.int32), ms)
    assert info["ncells"] == 50 and 0 <= pos[0] < 49


# ------------------------------------------------ the grid against the cells ----
@pytest.mark.parametrize("lds_mode", [0, 1])
def test_grid_matches_cells_after_a_run(tt, make, lds_mode):
    """300 cells, 600 iterations on the Tonga rays: births insert, deaths and moves remove by swapping in the
    bucket's last entry, a move inside one bucket, changes write the value into the entry."""
    prm = tt.define_TDstructrure().replace(max_cells=400)
    ch = make(prm, tt.random_model(300, 17), 17)
    assert tt.lib().tdt_chain_set_lds_mode(ch.h, lds_mode) == 0
    g = grid_check(tt, ch)
    assert_grid_sound(g, "after creation")
    assert g["overflow"] == 0 and g["nslots"] == 300
    for _ in range(3):
        ch.run(200)
        g = grid_check(tt, ch)
        assert_grid_sound(g, "after a run")
        assert g["overflow"] == 0, g
    acc = ch.stats()["accepted"]
    print("lds_mode %d: accepted (birth, death, change, move):" % lds_mode, acc)
    assert sum(acc) > 20, acc  # (the model really moved)
    assert tt.lib().tdt_chain_own_check(ch.h) == 0


def test_grid_matches_cells_under_the_prior(tt, make):
    """debug_prior = 1: every valid proposal is accepted, so every kind of grid update runs many times."""
    prm = tt.define_TDstructrure().replace(debug_prior=1)
    ch = make(prm, None, 21)
    assert_grid_sound(grid_check(tt, ch), "after creation")
    for _ in range(6):  # (400 iterations accept 25 births and 24 deaths; 600 for a margin over 20)
        ch.run(100)
        g = grid_check(tt, ch)
        assert_grid_sound(g, "after a run")
        assert g["overflow"] == 0, g
    acc = ch.stats()["accepted"]
    print("accepted (birth, death, change, move):", acc)
    assert all(a >= 20 for a in acc), acc
