"""CPU: the catalogue of tests/context_ops.py holds what tests/test_gpu_context_state.py relies on -- every
public entry point is reached or excluded for a stated reason, the sizes cross the path switches they claim
to cross (by the library's own host functions and constants), the oracle halves of the references run, and
no heavy entry can drop out of the pair list.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import context_ops as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc-in-tonga_amd", "csrc")


def constant(path, name):
    """`constexpr ... name = <integer expression>;` of a source file, evaluated."""
    m = re.search(r"constexpr\s+[\w:]+\s+%s\s*=\s*([^;]+);" % name, open(os.path.join(CSRC, path)).read())
    assert m, (path, name)
    return int(eval(m.group(1), {"__builtins__": {}}))  # "256", "1 << 16"


# ---- coverage guard
def test_every_entry_point_is_reached_or_excluded_with_a_reason():
    declared = set(co.header_entry_points(os.path.join(ROOT, "include", "tdstar.h")))
    assert len(declared) > 50 and {"td_evaluate", "td_rounds_exchange_recorded", "td_trilinear"} <= declared
    reached = {f for o in co.OPS for f in o.reaches}
    assert reached <= declared, sorted(reached - declared)  # no misspelt name in the catalogue
    assert set(co.EXCLUDED) <= declared, sorted(set(co.EXCLUDED) - declared)
    assert set(co.EXCLUDED.values()) <= {co.NO_GPU, co.CTOR, co.MULTI_RANK}
    assert not (reached & set(co.EXCLUDED)), sorted(reached & set(co.EXCLUDED))
    missing = declared - reached - set(co.EXCLUDED)
    assert not missing, "entry points neither exercised by the catalogue nor excluded: %s" % sorted(missing)


def test_the_guard_sees_a_new_entry_point(tmp_path):
    p = tmp_path / "h.h"
    p.write_text("/* td_in_a_comment(x) */\nint td_brand_new(td_ctx *ctx);\nint td_evaluate (td_ctx *c);\n"
                 "typedef struct td_info { int a; } td_info;\n")
    assert co.header_entry_points(str(p)) == ["td_brand_new", "td_evaluate"]


def test_every_operation_has_a_unique_name_and_family():
    assert len({o.name for o in co.OPS}) == len(co.OPS)
    assert set(co.HEAVY) <= set(co.BY_NAME)
    for o in co.OPS:
        assert o.gpu == (o.family != "modifier"), o.name
        assert o.reaches or not o.gpu, o.name


# ---- the sizes cross what they claim to cross
def test_evaluate_sizes_straddle_the_grid_threshold_and_grow_the_buckets(tt):
    kmin = constant("internal.h", "kGridMinCells")
    assert kmin == co.GRID_MIN_CELLS == 256
    small, grid, more = co.EVAL_CELLS
    assert small < kmin <= grid < more
    assert all(c < kmin for _, c in co.INTERP[:2]) and all(c >= kmin for _, c in co.INTERP[2:])
    assert min(co.BATCH_CELLS) < kmin <= max(co.BATCH_CELLS)
    # api.cpp nearest_uploaded: make_cell_grid(box of the cells, ncells / 2, 4096, kGridMaxBuckets)
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    buckets = []
    for n in (grid, more):
        c = co.cells(n, 40 + n)
        lo = np.array([a.min() for a in c[:3]])
        hi = np.array([a.max() for a in c[:3]])
        dims = np.zeros(3, dtype=np.int32)
        p = np.zeros(1)
        ijk, lb = np.zeros(3, dtype=np.int32), np.zeros(1)
        rc = tt.lib().tdt_grid_lb(lo.ctypes.data_as(pd), hi.ctypes.data_as(pd), n / 2.0, 4096,
                                  constant("internal.h", "kGridMaxBuckets"), p.ctypes.data_as(pd), p.ctypes.data_as(pd),
                                  p.ctypes.data_as(pd), 1, 1, ijk.ctypes.data_as(pi), lb.ctypes.data_as(pd),
                                  dims.ctypes.data_as(pi), None, None)
        assert rc == 0
        buckets.append(int(np.prod(dims.astype(np.int64))))
    assert buckets[1] > 2 * buckets[0] > 0, buckets


def raster_batched(sizes, nq):
    """csrc/raster.hip raster_batched, restated on its own constants."""
    nm, total = len(sizes), sum(sizes)
    xcds, nodes = constant("raster.hip", "kXcds"), 64 * constant("raster.hip", "kRasterPPL")
    src = open(os.path.join(CSRC, "raster.hip")).read()
    assert "nq * (total / std::max<int64_t>(nmodels, 1)) <= (int64_t)1 << 28" in src  # the budget below
    return (nq * (total // max(nm, 1)) <= co.RASTER_BUDGET
            and xcds * ((nm + xcds - 1) // xcds) * ((nq + nodes - 1) // nodes) <= 2 ** 31 - 1)


def test_raster_shapes_take_the_two_launches():
    assert raster_batched(*co.RASTER_BATCHED)
    assert not raster_batched(*co.RASTER_PER_MODEL)
    assert min(co.RASTER_PER_MODEL[0]) >= co.GRID_MIN_CELLS  # the per-model path's bucket-grid search
    assert raster_batched([300], co.RASTER_BATCHED[1])
    assert 0 in co.RASTER_BATCHED[0]  # an empty model
    assert any(np.isnan(m[0]).any() for m in co.raster_batched_models())  # NaN cells
    # the histories' consumers stay on the batched launch (the per-model path fetches the cells instead)
    assert raster_batched([co.HISTORY["max_cells"]] * 2 * co.HISTORY["samples"], co.H_NODES)


def test_forced_plans_give_several_slabs_and_chunks(tt, ds):
    for nm, nq in co.ENSEMBLES.items():
        nodes, slabs = tt.TdContext.volume_plan(nm, nq, forced=co.FORCED_SLAB_NODES)
        assert nodes == co.FORCED_SLAB_NODES and slabs == -(-nq // nodes) > 1
        assert tt.TdContext.volume_plan(nm, nq)[1] == 1  # auto: one slab
        rp = (~np.isnan(ds.rayX)).sum(axis=0)
        points, chunk, edges = tt.TdContext.predict_plan(nm, rp, forced_points=co.FORCED_PREDICT[0],
                                                         forced_chunk=co.FORCED_PREDICT[1])
        assert len(edges) - 1 > 1 and chunk == co.FORCED_PREDICT[1] < nm
        points, chunk, edges = tt.TdContext.predict_plan(nm, rp)
        assert len(edges) - 1 == 1 and chunk == nm
        sizes = [len(c[0]) for c in co.ensemble(nm)]
        assert sum(sizes) // nm >= constant("volume.hip", "kVolGridMinMeanCells")  # auto: the bucket grids


def test_trilinear_grids_straddle_the_knots_that_fit_the_lds():
    lds = constant("ingest.hip", "kKnotsLds")
    assert lds == co.TRI_KNOTS_LDS
    sums = [sum(g) for g in co.TRI_GRIDS]
    assert sums[0] < sums[1] <= lds < sums[2]
    assert co.TRI_POINTS[0] > co.TRI_POINTS[1]  # the thread-local buffer grows, then holds a stale tail


def test_marginals_and_convergence_shapes(tt):
    assert co.MARG_MODELS <= 16384 and all(min(lens) >= 4 for lens in co.CONV_CHAINS)
    assert all(sum(lens) == len(co.conv_models(lens)) for lens in co.CONV_CHAINS)
    import convergence_ref

    # max_lag 5 binds for the long chains only: n - 1 = 19 and 3
    assert [convergence_ref.plan(lens, 5)["T"] for lens in co.CONV_CHAINS] == [5, 3]
    h = co.HISTORY
    assert len(range(h["first"], h["iterations"] + 1, h["every"])) == h["samples"]


# ---- the oracle halves of the references
def trilinear_pointwise(axes, v, pts):
    """oracle_np.trilinear restated per point in plain Python floats (include/tdstar.h td_trilinear)."""
    out = []
    for x, y, z in zip(*pts):
        idx, t = [], []
        for k, p in zip(axes, (x, y, z)):
            if not (k[0] <= p <= k[-1]):
                break
            i = 0
            while i + 2 < len(k) and k[i + 1] <= p:
                i += 1
            idx.append(i)
            t.append((float(p) - float(k[i])) / (float(k[i + 1]) - float(k[i])))
        if len(idx) < 3:
            out.append(float("nan"))
            continue
        (i, j, k), (tx, ty, tz) = idx, t
        c2 = []
        for dz in (0, 1):
            c1 = [(1.0 - tx) * float(v[i, j + dy, k + dz]) + tx * float(v[i + 1, j + dy, k + dz]) for dy in (0, 1)]
            c2.append((1.0 - ty) * c1[0] + ty * c1[1])
        out.append((1.0 - tz) * c2[0] + tz * c2[1])
    return np.array(out)


@pytest.mark.parametrize("shape", co.TRI_GRIDS, ids=str)
def test_trilinear_oracle_equals_a_pointwise_restatement(shape):
    npts = co.TRI_POINTS[1] if shape != co.TRI_GRIDS[2] else 400
    axes, values, pts = co.tri_inputs(shape, npts)
    from oracle import oracle_np

    a = oracle_np.trilinear(*axes, values, *pts)
    assert co.same(a, trilinear_pointwise(axes, values, pts))
    assert 0 < np.isnan(a).sum() < npts  # some points outside, most inside
    o = co.BY_NAME["trilinear_%dx%dx%d_%dpts" % (shape + (co.TRI_POINTS[1],))].oracle()
    assert o[1] == int(np.isnan(o[0]).sum())


@pytest.mark.parametrize("name", [o.name for o in co.OPS if o.oracle and o.name not in co.HEAVY])
def test_oracle_half_runs(name, orc):
    o = co.BY_NAME[name]
    sig = np.asarray(co.rays().allSig, dtype=np.float64)
    exp = o.oracle(sig) if o.sigma else o.oracle()
    assert exp and all(isinstance(k, int) for k in exp)
    for v in exp.values():
        assert np.asarray(v).size > 0


def test_sigma_reaches_the_oracles(orc):
    o = co.BY_NAME["evaluate_63"]
    sig = np.asarray(co.rays().allSig, dtype=np.float64)
    a, b = o.oracle(sig), o.oracle(sig * co.SIGMA_SCALE)
    assert co.same(a[0], b[0]) and a[1] != b[1] and a[2] != b[2]  # ptS stays, phi and the likelihood move
    assert b[1] == orc.chi2(a[0], co.rays().tS, sig * co.SIGMA_SCALE)


def test_misfit_pairs_change_one_input_at_a_time():
    n = co.MISFIT_N[0]
    (pa, ta, sa), (pb, tb, sb), (pc, tc, sc) = (co.misfit_inputs(n, p) for p in "ABC")
    assert co.same((pa, pa), (pb, pc))
    assert co.same(ta, tb) and not co.same(sa, sb)  # B: another sigma alone
    assert co.same(sa, sc) and not co.same(ta, tc)  # C: another tS alone
    assert co.MISFIT_N[1] < n == co.rays().rayX.shape[1]


def test_edits_are_reference_shaped_and_seeded():
    base = co.cells(*co.EDIT_BASE)
    for kind, dn in (("move", 0), ("birth", 1), ("death", -1)):
        a, b = co.edited(base, kind), co.edited(base, kind)
        assert co.same(a, b) and len(a[0]) == len(base[0]) + dn
        assert not co.same(a, base)
    m = co.edited(base, "move")
    assert sum(int((m[k] != base[k]).sum()) for k in range(3)) == 3 and co.same(m[3], base[3])  # one site moved


def test_same_is_exact():
    a = np.array([1.0, np.nan, -0.0])
    assert co.same((a, 3), (a.copy(), 3))
    assert not co.same((a,), (np.array([1.0, np.nan, 0.0]),))  # -0.0 is not 0.0
    assert not co.same((a,), (np.array([1.0 + 2 ** -52, np.nan, -0.0]),))
    assert not co.same((a,), (a[:2],)) and not co.same((a,), (a, a))
    assert not co.same((np.array([1, 2]),), (np.array([1.0, 2.0]),))
    assert "first at 2" in co.first_difference((a,), (np.array([1.0, np.nan, 0.0]),))


# ---- a heavy entry cannot be dropped silently
def test_pair_list_holds_every_light_pair_and_every_heavy_entry_both_ways():
    pairs = co.pair_list()
    ps = set(pairs)
    light = [o.name for o in co.LIGHT]
    assert all((a, b) in ps for a in light for b in light)
    assert len(co.HEAVY) == 8 and len(light) + len(co.HEAVY) == len(co.OPS)
    for h in co.HEAVY:
        assert co.BY_NAME[h].gpu
        for fam in co.FAMILIES:
            assert any(a == h and co.BY_NAME[b].family == fam for a, b in pairs), (h, "as A against", fam)
            assert any(b == h and co.BY_NAME[a].family == fam for a, b in pairs), (h, "as B against", fam)
    for name in ("rasterize_per_model", "volume_16_auto", "predict_16_forced", "covariance_16_auto", "ladder_step"):
        assert name in co.HEAVY
