"""GPU: the device-resident sample history (td_history, td_chain_run_recorded).

The twin is always an identically seeded chain driven the old way -- td_chain_run up to each sample
iteration, then td_chain_get_model -- and every recorded sample must equal the twin's model bit for
bit: iteration, ncells, the four cell arrays (Julia order), phi, ptS, action and accept; after the runs
the stats and the final model too.  Shapes are test_gpu_chain's."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(tt, ds):
    return tt.TdContext.from_datastruct(ds)


def make(tt, ctx, prm, model, seed, engine=None, chain=1, lds_mode=None):
    engine = tt.TD_ENGINE_DEVICE if engine is None else engine
    c = tt.Chain(ctx, tt.chain_params(prm, None, seed=seed, chain=chain, engine=engine), model)
    if lds_mode is not None:
        assert tt.lib().tdt_chain_set_lds_mode(c.h, lds_mode) == 0
    return c


def sample_iters(iterations, first, every):
    return list(range(first, iterations + 1, every))


def twin_samples(ch, iterations, first, every, done=0):
    """The old way: run to each sample iteration and read the model; -> [(iteration, Model)]."""
    out, at = [], 0
    for s in sample_iters(iterations, first, every):
        ch.run(s - at)
        at = s
        out.append((done + s, ch.model()))
    ch.run(iterations - at)
    return out


def assert_samples(hist, want, first=0):
    a = hist.read_arrays(first, len(want))
    ms = hist.read(first, len(want))
    assert len(ms) == len(want)
    for k, (it, m) in enumerate(want):
        lo, hi = int(a["off"][k]), int(a["off"][k + 1])
        assert a["iter"][k] == it, (k, a["iter"][k], it)
        assert hi - lo == len(m.xCell) == ms[k].nCells, k
        for name, ref in (("x", m.xCell), ("y", m.yCell), ("z", m.zCell), ("zeta", m.zeta)):
            assert np.array_equal(a[name][lo:hi], ref), (k, name)
        assert a["phi"][k] == m.phi, (k, a["phi"][k], m.phi)
        assert np.array_equal(a["ptS"][k], m.ptS), k
        assert (a["action"][k], a["accept"][k]) == (m.action, m.accept), k
        r = ms[k]  # the Model copies carry the same
        assert np.array_equal(r.xCell, m.xCell) and np.array_equal(r.zeta, m.zeta) and r.phi == m.phi
        assert np.array_equal(r.ptS, m.ptS) and (r.action, r.accept) == (m.action, m.accept)


def assert_same_end(a, b):
    sa, sb = a.stats(), b.stats()
    assert sa == sb, (sa, sb)
    ma, mb = a.model(), b.model()
    for f in ("xCell", "yCell", "zCell", "zeta", "ptS"):
        assert np.array_equal(getattr(ma, f), getattr(mb, f)), f
    assert ma.phi == mb.phi


SHAPES = [(8, 12, 600, 1, 1, 4), (200, 300, 400, 37, 20, 1), (1000, 1100, 250, 50, 50, 2), (5000, 5100, 120, 10, 30, 3)]


@pytest.mark.parametrize("ncells,max_cells,iters,first,every,seed", SHAPES)
def test_recorded_run_equals_stretch_per_sample(tt, ctx, ncells, max_cells, iters, first, every, seed):
    prm = tt.define_TDstructrure().replace(max_cells=max_cells)
    model = tt.random_model(ncells, seed)
    rec, twin = make(tt, ctx, prm, model, seed), make(tt, ctx, prm, model, seed)
    ns = len(sample_iters(iters, first, every))
    hist = tt.History(ctx, ns, ns * max_cells)
    rec.run_recorded(iters, first, every, hist)
    want = twin_samples(twin, iters, first, every)
    assert hist.count()[0] == ns == len(want)
    assert hist.count()[1] == sum(len(m.xCell) for _, m in want)
    assert_samples(hist, want)
    assert_same_end(rec, twin)
    # the one oracle that is not the chain kernel: a full evaluate of EVERY sample's cells gives its phi and ptS
    for k, m in enumerate(hist.read()):
        ptS, phi, _, _ = ctx.evaluate(m.cells())
        assert phi == m.phi and np.array_equal(ptS, m.ptS), k
    if ncells == 200:
        # the HOST engine records from its host loop into the same buffers: the parity twin
        host = make(tt, ctx, prm, model, seed, tt.TD_ENGINE_HOST)
        hh = tt.History(ctx, ns, ns * max_cells)
        host.run_recorded(iters, first, every, hh)
        assert_samples(hh, want)
        assert host.stats()["phi"] == rec.stats()["phi"] and host.stats()["accepted"] == rec.stats()["accepted"]
        hh.close()
    hist.close()


def test_split_calls_accumulate_into_one_history(tt, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=300)
    model = tt.random_model(200, 1)
    one, two, twin = (make(tt, ctx, prm, model, 1) for _ in range(3))
    first, every = 37, 20
    ns = len(sample_iters(400, first, every))
    h1, h2 = tt.History(ctx, ns, ns * 300), tt.History(ctx, ns, ns * 300)
    one.run_recorded(400, first, every, h1)
    two.run_recorded(150, first, every, h2)
    taken = len(sample_iters(150, first, every))
    assert len(h2) == taken
    two.run_recorded(250, first + taken * every - 150, every, h2)  # `first` carried over the cut
    want = twin_samples(twin, 400, first, every)
    assert_samples(h1, want)
    assert_samples(h2, want)
    assert_same_end(one, two)
    assert_same_end(one, twin)
    # clear: the history starts again, its capacity kept
    h2.clear()
    assert h2.count() == (0, 0)
    two.run_recorded(40, 40, 1, h2)
    twin.run(40)
    assert_samples(h2, [(440, twin.model())])


@pytest.mark.parametrize("ncells", [300, 2000])
def test_hbm_layout_records(tt, ctx, ncells):
    prm = tt.define_TDstructrure().replace(max_cells=ncells + 200)
    model = tt.random_model(ncells, 40)
    rec, twin = make(tt, ctx, prm, model, 40, lds_mode=1), make(tt, ctx, prm, model, 40, lds_mode=1)
    hist = tt.History(ctx, 12, 12 * (ncells + 200))
    rec.run_recorded(120, 10, 10, hist)
    assert_samples(hist, twin_samples(twin, 120, 10, 10))
    assert_same_end(rec, twin)


@pytest.mark.parametrize("mode", [2, 3])
def test_two_chains_per_cu_variants_record(tt, ctx, mode):
    """lds_mode 2 / 3 (the 256-thread kernels) through a batch of three chains, two launches."""
    prm = tt.define_TDstructrure().replace(max_cells=1300)
    sizes = (1000, 400, 1200)
    recs = [make(tt, ctx, prm, tt.random_model(n, 70 + k), 70 + k, chain=k + 1, lds_mode=mode)
            for k, n in enumerate(sizes)]
    twins = [make(tt, ctx, prm, tt.random_model(n, 70 + k), 70 + k, chain=k + 1, lds_mode=mode)
             for k, n in enumerate(sizes)]
    hists = [tt.History(ctx, 22, 22 * 1300) for _ in sizes]
    tt.run_batch_recorded(recs, 70, 9, 9, hists)       # samples at 9, 18, ..., 63
    tt.run_batch_recorded(recs, 130, 2, 9, hists)      # 72 = 70 + 2, ...
    for r, t, h in zip(recs, twins, hists):
        want = twin_samples(t, 70, 9, 9) + twin_samples(t, 130, 2, 9, done=70)
        assert len(h) == len(want) == 7 + 15
        assert_samples(h, want)
        assert_same_end(r, t)


def test_many_rays_chain_records(tt):
    """3000 synthetic rays x 700 cells: tiles, rays and the order in HBM."""
    ds = tt.synthetic_rays(3000, seed=8)
    ctx = tt.TdContext.from_datastruct(ds)
    prm = tt.define_TDstructrure().replace(max_cells=900)
    model = tt.random_model(700, 21)
    rec, twin = make(tt, ctx, prm, model, 21), make(tt, ctx, prm, model, 21)
    hist = tt.History(ctx, 5, 5 * 900)
    rec.run_recorded(40, 7, 7, hist)
    assert_samples(hist, twin_samples(twin, 40, 7, 7))
    assert_same_end(rec, twin)


def test_batch_recorded_equals_solo_recorded(tt, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=700)
    sizes = (60, 300, 600, 150, 8)
    batch = [make(tt, ctx, prm, tt.random_model(n, 30 + k), 30 + k, chain=k + 1) for k, n in enumerate(sizes)]
    solo = [make(tt, ctx, prm, tt.random_model(n, 30 + k), 30 + k, chain=k + 1) for k, n in enumerate(sizes)]
    hb = [tt.History(ctx, 30, 30 * 700) for _ in sizes]
    hs = [tt.History(ctx, 30, 30 * 700) for _ in sizes]
    tt.run_batch_recorded(batch, 150, 6, 6, hb)
    for c, h in zip(solo, hs):
        c.run_recorded(150, 6, 6, h)
    for b, s, x, y in zip(batch, solo, hb, hs):
        assert len(x) == len(y) == 25
        ax, ay = x.read_arrays(), y.read_arrays()
        for key in ax:
            assert np.array_equal(ax[key], ay[key]), key
        assert_same_end(b, s)
    # against the old way too, for one of them
    twin = make(tt, ctx, prm, tt.random_model(600, 32), 32, chain=3)
    assert_samples(hb[2], twin_samples(twin, 150, 6, 6))


def test_capacity_is_checked_before_anything_runs(tt, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=300)
    model = tt.random_model(200, 1)
    L = tt.lib()
    probe = make(tt, ctx, prm, model, 1)
    probe.run(17)
    c1 = probe.stats()["ncells"]  # the cells of the sample the histories below already hold
    # room for one sample too few / one cell too few / one max_cells too few for the 5 samples asked
    for max_samples, max_cells_total in ((5, c1 + 5 * 300), (6, c1 + 5 * 300 - 1), (6, c1 + 4 * 300)):
        ch = make(tt, ctx, prm, model, 1)
        ch.run(10)
        hist = tt.History(ctx, max_samples, max_cells_total)
        ch.run_recorded(7, 7, 1, hist)
        before, kept = ch.stats(), hist.read_arrays()
        assert hist.count() == (1, c1)
        rc = L.td_chain_run_recorded(ch.h, 100, 20, 20, hist.h)  # samples at 20, 40, ..., 100
        assert rc == 1 and b"room" in L.td_last_error(ctx.h)  # TD_ERR_ARG
        assert ch.stats() == before  # iterations, phi, counters: nothing ran
        assert hist.count() == (1, c1)
        now = hist.read_arrays()
        assert all(np.array_equal(kept[k], now[k]) for k in kept)
        rc = L.td_chain_run_recorded(ch.h, 100, 20, 25, hist.h)  # 4 samples fit each of them
        assert rc == 0 and len(hist) == 5 and ch.stats()["iterations"] == before["iterations"] + 100
    # the same history twice in a batch
    ch, other = make(tt, ctx, prm, model, 1), make(tt, ctx, prm, model, 2, chain=2)
    before = ch.stats()
    h = tt.History(ctx, 20, 20 * 300)
    arr = (ctypes.c_void_p * 2)(ch.h, other.h)
    hs = (ctypes.c_void_p * 2)(h.h, h.h)
    rc = L.td_chain_run_batch_recorded(arr, 2, 50, 10, 10, hs)
    assert rc == 1 and b"history appears twice" in L.td_last_error(ctx.h)
    assert ch.stats() == before and len(h) == 0


def same_model(a, b):
    return (np.array_equal(a.xCell, b.xCell) and np.array_equal(a.yCell, b.yCell) and np.array_equal(a.zCell, b.zCell)
            and np.array_equal(a.zeta, b.zeta) and a.phi == b.phi and np.array_equal(a.ptS, b.ptS)
            and np.array_equal(a.tS, b.tS) and a.likelihood == b.likelihood and a.action == b.action
            and a.accept == b.accept and a.nCells == b.nCells)


@pytest.mark.parametrize("keep", [20.0, 1.0])
def test_driver_history_equals_stretch_per_sample(tt, ds, keep):
    prm = tt.define_TDstructrure().replace(n_iter=300.0, burn_in=100.0, keep_each=keep, print_each=100.0,
                                           max_cells=200)
    ctx = tt.context_for(ds)
    counts = {}
    out = {}
    for history in (True, False):
        ctx.timing(enable=True, reset=True)
        out[history] = tt.TD_inversion_function(prm, ds, 1, seed=5, history=history)
        counts[history] = ctx.timing(kernel="chain_run")[0]
        ctx.timing(enable=False)
    assert len(out[True]) == len(out[False]) == (201 if keep == 1.0 else 10)  # iterations 100..300 count
    assert all(same_model(a, b) for a, b in zip(out[True], out[False]))
    assert counts[True] == 1 and counts[False] >= 10, counts


def test_run_chains_recorded_equals_each_chain_alone(tt, ds):
    prm = tt.define_TDstructrure().replace(n_iter=200.0, burn_in=60.0, keep_each=10.0, print_each=50.0, max_cells=150)
    together = tt.run_chains(prm, ds, [1, 2, 3])
    for c, hist in zip([1, 2, 3], together):
        alone = tt.TD_inversion_function(prm, ds, c, history=False)
        assert len(hist) == len(alone) == 14
        assert all(same_model(a, b) for a, b in zip(hist, alone))


def test_driver_checkpoint_resume_through_history(tt, ds, tmp_path):
    if not tt.jld.available():
        pytest.skip("no interpreter with h5py")
    prm = tt.define_TDstructrure().replace(n_iter=500.0, burn_in=200.0, keep_each=20.0, print_each=50.0,
                                           max_cells=400)
    straight = tt.TD_inversion_function(prm, ds, 1, seed=5, model=tt.random_model(250, 5), history=False)
    d = str(tmp_path)
    part = tt.TD_inversion_function(prm, ds, 1, seed=5, model=tt.random_model(250, 5), checkpoint_dir=d,
                                    stop_after=350)
    assert len(part) == 7
    resumed = tt.TD_inversion_function(prm, ds, 1, seed=5, model=None, checkpoint_dir=d)
    assert len(resumed) == len(straight) == 15
    assert all(same_model(a, b) for a, b in zip(resumed, straight))


def test_history_rasterize_equals_rasterize_of_models(tt, ds, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=300, xzMap=True, ySlice=[0, 150], xyMap=True, zSlice=[100])
    hists, chains = [], []
    for k in range(2):
        c = make(tt, ctx, prm, tt.random_model(200, 50 + k), 50 + k, chain=k + 1)
        h = tt.History(ctx, 10, 10 * 300, with_ptS=False)
        c.run_recorded(100, 10, 10, h)
        assert len(h) == 10
        hists.append(h)
        chains.append(c)
    models = [h.read() for h in hists]
    flat = [m.cells() for ms in models for m in ms]
    gx, gz = np.meshgrid(np.linspace(-50, 1050, 37), np.linspace(0, 660, 11))
    qx, qz = gx.ravel(), gz.ravel()
    qy = np.full(qx.shape, 150.0)
    m1, s1, v1 = ctx.rasterize_history(hists, qx, qy, qz, want_values=True)
    m2, s2, v2 = ctx.rasterize(flat, qx, qy, qz, want_values=True)
    assert np.array_equal(v1, v2) and np.array_equal(m1, m2) and np.array_equal(s1, s2, equal_nan=True)
    # plot_model_hist on the histories (the context of `ds`: another one than the histories' is refused)
    ctx2 = tt.context_for(ds)
    hs2 = []
    for k in range(2):
        c = make(tt, ctx2, prm, tt.random_model(200, 50 + k), 50 + k, chain=k + 1)
        h = tt.History(ctx2, 10, 10 * 300)
        c.run_recorded(100, 10, 10, h)
        hs2.append(h)
    a = tt.plot_model_hist(hs2, ds, prm)
    b = tt.plot_model_hist(models, ds, prm)
    assert set(a) == set(b) == {("xz", 0), ("xz", 150), ("xy", 100)}
    for key in a:
        for f in ("mean", "std", "masked"):
            assert np.array_equal(a[key][f], b[key][f], equal_nan=True), (key, f)
