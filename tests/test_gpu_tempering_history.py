"""GPU: the cold replica of a tempering ladder recorded in a device history
(td_rounds_temper_recorded, td_rounds_exchange_recorded, TemperingLadder.run(history=...)).

The oracle is always a twin ladder on the code paths that existed before: the same seeds,
``TemperingLadder(chains, resident=False)`` stepped round by round, with ``j = lad.cold_local()`` taken
BEFORE ``lad.step(K)`` and ``chains[j].model()`` / ``chains[j].stats()`` after it -- the state of the
replica that ran the round at ladder level 0, before nothing but the round's swap of temperatures.
Every recorded sample must equal the twin's bit for bit (cells in order, phi, ncells, iter, action,
accept, ptS), and recording must change nothing else: trace digest, end models and stats are those of an
unrecorded resident ladder.  The pack kernel is also driven alone, on made-up slots, against numpy."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the LDS-layout ladder: the 381 shipped rays, 4 replicas of 12 cells, max_cells 16
NREP, NCELLS, MAXC, K, ROUNDS, FIRST, EVERY = 4, 12, 16, 5, 24, 3, 2
# Found on the twin (tools/tempering_history_rate.py --scan lists what each candidate gives; small models
# swap readily only on a narrow ladder): with these chain seeds, this ladder and this ladder seed the
# sampled rounds are run at level 0 by replicas 0, 2, 3, 3, 2, 3, 3, 1, 1, 1, 2 and their samples hold 14,
# 16, 10, 10, 15, 9, 10, 7, 9, 8, 16 cells -- every replica records, two samples fill their slot (16, which
# the pack leaves unmoved where nothing before it left a gap) and the others do not.  The test asserts
# these conditions on the twin.
BASE, TMAX, SEED = 470, 1.05, 4
PROTOCOLS = ("host", "device")


def sampled(rounds, first, every):
    return list(range(first, rounds + 1, every))


def lds_chains(tt, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=MAXC)
    return [tt.Chain(ctx, tt.chain_params(prm, None, seed=BASE + j, chain=1 + j, engine=tt.TD_ENGINE_DEVICE),
                     tt.random_model(NCELLS, BASE + j)) for j in range(NREP)]


def hbm_chains(tt, ctx):
    prm = tt.define_TDstructrure().replace(max_cells=900)
    return [tt.Chain(ctx, tt.chain_params(prm, None, seed=21 + j, chain=1 + j, engine=tt.TD_ENGINE_DEVICE),
                     tt.random_model(700, 21 + j)) for j in range(2)]


def twin_run(tt, chains, rounds, k, tmax, seed):
    """The old way, every round: -> [(round 1-based, cold chain, its iterations, its Model)], the ladder."""
    lad = tt.TemperingLadder(chains, tmax=tmax, seed=seed, resident=False)
    out = []
    for r in range(1, rounds + 1):
        j = lad.cold_local()
        lad.step(k)
        out.append((r, j, chains[j].stats()["iterations"], chains[j].model()))
    return out, lad


def end_state(lad, chains):
    lad.close()
    return dict(digest=lad.trace_digest(), levels=[int(x) for x in lad.levels], models=[c.model() for c in chains],
                stats=[c.stats() for c in chains], tried=list(lad.tried), accepted=list(lad.accepted))


def assert_same_end(a, b):
    assert a["digest"] == b["digest"] and a["levels"] == b["levels"]
    assert a["tried"] == b["tried"] and a["accepted"] == b["accepted"]
    for ma, mb, sa, sb in zip(a["models"], b["models"], a["stats"], b["stats"]):
        assert sa == sb, (sa, sb)
        for f in ("xCell", "yCell", "zCell", "zeta", "ptS"):
            assert np.array_equal(getattr(ma, f), getattr(mb, f)), f
        assert ma.phi == mb.phi


def assert_samples(hist, want, first=0):
    """want: [(iteration, Model)] -- the header fields as tests/test_gpu_history.py compares them."""
    a = hist.read_arrays(first, len(want))
    ms = hist.read(first, len(want))
    assert len(ms) == len(want)
    for k, (it, m) in enumerate(want):
        lo, hi = int(a["off"][k]), int(a["off"][k + 1])
        assert a["iter"][k] == it, (k, a["iter"][k], it)
        assert hi - lo == len(m.xCell) == ms[k].nCells, (k, hi - lo, len(m.xCell))
        for name, ref in (("x", m.xCell), ("y", m.yCell), ("z", m.zCell), ("zeta", m.zeta)):
            assert np.array_equal(a[name][lo:hi], ref), (k, name)
        assert a["phi"][k] == m.phi, (k, a["phi"][k], m.phi)
        if a["ptS"] is not None:
            assert np.array_equal(a["ptS"][k], m.ptS), k
        assert (a["action"][k], a["accept"][k]) == (m.action, m.accept), k
        r = ms[k]
        assert np.array_equal(r.xCell, m.xCell) and np.array_equal(r.zeta, m.zeta) and r.phi == m.phi


def ladder(tt, chains, protocol, tmax, seed):
    lad = tt.TemperingLadder(chains, tmax=tmax, seed=seed, device_swaps=protocol == "device")
    assert lad.resident and lad.device_swaps == (protocol == "device")
    return lad


def close_all(chains):
    for c in chains:
        c.close()


@pytest.fixture(scope="module")
def ctx(tt, ds):
    return tt.context_for(ds)  # (plot_model_hist takes histories of the data's own context)


@pytest.fixture(scope="module")
def twin(tt, ctx):
    """The LDS ladder's twin, once for the module: every round's cold model, and what the sampled ones show."""
    chains = lds_chains(tt, ctx)
    rounds, lad = twin_run(tt, chains, ROUNDS, K, TMAX, SEED)
    close_all(chains)
    want = [(it, m) for r, j, it, m in rounds if r in sampled(ROUNDS, FIRST, EVERY)]
    cold = [j for r, j, it, m in rounds if r in sampled(ROUNDS, FIRST, EVERY)]
    return dict(rounds=rounds, want=want, cold=cold, digest=lad.trace_digest())


@pytest.fixture(scope="module")
def unrecorded(tt, ctx):
    """An unrecorded resident ladder per protocol: what recording must not change."""
    out = {}
    for protocol in PROTOCOLS:
        chains = lds_chains(tt, ctx)
        lad = ladder(tt, chains, protocol, TMAX, SEED)
        lad.run(ROUNDS, K)
        out[protocol] = end_state(lad, chains)
        close_all(chains)
    return out


def test_the_twin_exercises_what_the_test_is_about(twin):
    """Asserted on the twin's own levels and models: several recorders, a full slot, partly filled slots."""
    sizes = [len(m.xCell) for _, m in twin["want"]]
    assert len(twin["want"]) == len(sampled(ROUNDS, FIRST, EVERY)) == 11
    assert len(set(twin["cold"])) >= 2, twin["cold"]
    assert MAXC in sizes and min(sizes) < MAXC, sizes
    assert [it for it, _ in twin["want"]] == [K * r for r in sampled(ROUNDS, FIRST, EVERY)]


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_lds_ladder_records_the_cold_replica(tt, ctx, twin, unrecorded, protocol):
    ns = len(twin["want"])
    chains = lds_chains(tt, ctx)
    lad = ladder(tt, chains, protocol, TMAX, SEED)
    hist = tt.History(ctx, ns, ns * MAXC, with_ptS=True)
    lad.run(ROUNDS, K, history=hist, first=FIRST, every=EVERY)
    assert hist.count() == (ns, sum(len(m.xCell) for _, m in twin["want"]))
    assert_samples(hist, twin["want"])
    got = end_state(lad, chains)
    assert got["digest"] == twin["digest"]
    assert_same_end(got, unrecorded[protocol])
    hist.close()
    close_all(chains)


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_hbm_ladder_records_the_cold_replica(tt, protocol):
    """3000 synthetic rays x 700 cells: tiles, rays and the order in HBM; every round sampled."""
    ds = tt.synthetic_rays(3000, seed=8)
    ctx = tt.TdContext.from_datastruct(ds)
    rounds, k, tmax, seed = 6, 4, 8.0, 3
    tw = hbm_chains(tt, ctx)
    per_round, tlad = twin_run(tt, tw, rounds, k, tmax, seed)
    close_all(tw)
    want = [(it, m) for r, j, it, m in per_round]
    plain = hbm_chains(tt, ctx)
    plad = ladder(tt, plain, protocol, tmax, seed)
    plad.run(rounds, k)
    ref = end_state(plad, plain)
    close_all(plain)
    chains = hbm_chains(tt, ctx)
    lad = ladder(tt, chains, protocol, tmax, seed)
    hist = tt.History(ctx, rounds, rounds * 900)
    lad.run(rounds, k, history=hist)
    assert len(hist) == rounds
    assert_samples(hist, want)
    got = end_state(lad, chains)
    assert got["digest"] == tlad.trace_digest()
    assert_same_end(got, ref)
    hist.close()
    close_all(chains)
    ctx.close()


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_split_calls_leave_the_history_of_one_call(tt, ctx, twin, unrecorded, protocol):
    ns = len(twin["want"])
    chains = lds_chains(tt, ctx)
    lad = ladder(tt, chains, protocol, TMAX, SEED)
    hist = tt.History(ctx, 2 * ns + 1, (2 * ns + 1) * MAXC)
    lad.run(7, K, history=hist, first=FIRST, every=EVERY)
    taken = len(sampled(7, FIRST, EVERY))
    assert len(hist) == taken == 3
    lad.run(ROUNDS - 7, K, history=hist, first=FIRST + taken * EVERY - 7, every=EVERY)  # `first` carried over
    assert_samples(hist, twin["want"])
    assert_same_end(end_state(lad, chains), unrecorded[protocol])
    close_all(chains)
    # a second ladder appends to the non-empty history: from its cells_used on
    used = hist.count()[1]
    assert used == sum(len(m.xCell) for _, m in twin["want"])
    again = lds_chains(tt, ctx)
    lad2 = ladder(tt, again, protocol, TMAX, SEED)
    lad2.run(ROUNDS, K, history=hist, first=FIRST, every=EVERY)
    assert hist.count() == (2 * ns, 2 * used)
    assert_samples(hist, twin["want"])
    assert_samples(hist, twin["want"], first=ns)
    lad2.close()
    hist.close()
    close_all(again)


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_capacity_is_checked_before_anything_runs(tt, ctx, twin, unrecorded, protocol):
    ns = len(twin["want"])
    for max_samples, max_cells_total in ((ns - 1, ns * MAXC), (ns, ns * MAXC - 1)):
        chains = lds_chains(tt, ctx)
        lad = ladder(tt, chains, protocol, TMAX, SEED)
        hist = tt.History(ctx, max_samples, max_cells_total)
        with pytest.raises(tt.TdError) as e:
            lad.run(ROUNDS, K, history=hist, first=FIRST, every=EVERY)
        assert e.value.code == 1 and "room" in str(e.value)  # TD_ERR_ARG
        assert len(hist) == 0 and lad.rnd == 0 and all(c.stats()["iterations"] == 0 for c in chains)
        lad.run(ROUNDS, K)  # ... and the ladder is the one that was never asked
        assert_same_end(end_state(lad, chains), unrecorded[protocol])
        hist.close()
        close_all(chains)


def test_arguments_are_rejected_before_any_launch(tt, ctx):
    L = tt.lib()
    chains = lds_chains(tt, ctx)
    rounds = tt.Rounds(chains)
    other = tt.TdContext.from_datastruct(tt.synthetic_rays(50, seed=1))
    foreign, own = tt.History(other, 4, 64), tt.History(ctx, 4, 64)
    temps = np.ascontiguousarray(tt.geometric_ladder(NREP, TMAX))
    levels = np.arange(NREP, dtype=np.int64)
    seed = ctypes.c_uint64(SEED)
    p = lambda a: a.ctypes.data  # noqa: E731

    def temper(first, every, h):
        return L.td_rounds_temper_recorded(rounds.h, 4, K, p(temps), p(levels), 0, seed, None, None, None, None,
                                           first, every, h)

    def exchange(first, every, h):
        return L.td_rounds_exchange_recorded(rounds.h, None, 4, K, p(temps), p(levels), 0, seed, None, None, None,
                                             None, None, first, every, h)

    for call in (temper, exchange):
        assert call(1, 1, foreign.h) == 1 and b"another context" in L.td_last_error(ctx.h)
        assert call(1, 0, own.h) == 1 and b"every >= 1" in L.td_last_error(ctx.h)
        assert call(0, 1, own.h) == 1 and b"first >= 1" in L.td_last_error(ctx.h)
        assert call(1, 1, None) == 1 and b"NULL" in L.td_last_error(ctx.h)
    assert len(own) == 0 and len(foreign) == 0 and list(levels) == list(range(NREP))
    assert all(c.stats()["iterations"] == 0 for c in chains)
    rounds.close()
    # a ladder over two ranks (described by its exchange: no second process is started) and one that is
    # not resident would fall back to step(): refused, nothing runs
    two = tt.Exchange()
    two.world = 2
    for lad in (tt.TemperingLadder(chains, two, tmax=TMAX, seed=SEED, device_swaps=True),
                tt.TemperingLadder(chains, tmax=TMAX, seed=SEED, resident=False)):
        with pytest.raises(ValueError):
            lad.run(4, K, history=own)
    assert len(own) == 0 and all(c.stats()["iterations"] == 0 for c in chains)
    for h in (foreign, own):
        h.close()
    close_all(chains)
    other.close()


def test_a_lost_launch_leaves_one_copy_of_its_sample(tt, ctx, twin, unrecorded):
    """tdt_rounds_force_exit: at the next launch the listed workgroups return at their first wait while the
    others run the posted round; the round is posted again with those marked `skip`.  Whether the round's
    recorder ran it in the lost launch or in the second one, its sample is there once, in its own slot."""
    ns = len(twin["want"])
    chains = lds_chains(tt, ctx)
    lad = ladder(tt, chains, "host", TMAX, SEED)
    hist = tt.History(ctx, ns, ns * MAXC)
    done, first = 0, FIRST
    for rounds, forced in ((2, None), (6, "cold"), (8, "others"), (ROUNDS - 16, "cold")):
        if forced is not None:  # (the call's first round -- 3, 9, 17 -- is a sampled one: first == 1)
            assert first == 1
            cold = lad.cold_local()
            slots = [cold] if forced == "cold" else [j for j in range(NREP) if j != cold][:2]
            arr = (ctypes.c_int32 * len(slots))(*slots)
            assert tt.lib().tdt_rounds_force_exit(lad.rounds.h, arr, len(slots)) == 0
        lad.run(rounds, K, history=hist, first=first, every=EVERY)
        done += rounds
        first = next(r for r in sampled(ROUNDS + EVERY, FIRST, EVERY) if r > done) - done
    assert done == ROUNDS
    assert_samples(hist, twin["want"])
    assert_same_end(end_state(lad, chains), unrecorded["host"])
    hist.close()
    close_all(chains)


def test_consumers_read_the_recorded_history(tt, ds, ctx, twin):
    prm = tt.define_TDstructrure().replace(max_cells=MAXC, xzMap=True, ySlice=[150], xyMap=False)
    ns = len(twin["want"])
    chains = lds_chains(tt, ctx)
    lad = ladder(tt, chains, "device", TMAX, SEED)
    hist = tt.History(ctx, ns, ns * MAXC)
    lad.run(ROUNDS, K, history=hist, first=FIRST, every=EVERY)
    lad.close()
    models = [m for _, m in twin["want"]]
    a, b = tt.plot_model_hist(hist, ds, prm), tt.plot_model_hist(models, ds, prm)
    assert set(a) == set(b) == {("xz", 150)}
    for f in ("mean", "std", "masked"):
        assert np.array_equal(a[("xz", 150)][f], b[("xz", 150)][f], equal_nan=True), f
    bins = (10, 0.0, 50.0)
    qa, qb = tt.credible_maps(hist, ds, prm, bins=bins), tt.credible_maps(models, ds, prm, bins=bins)
    for f in ("quantiles", "width", "mean", "std", "hist"):
        assert np.array_equal(qa[("xz", 150)][f], qb[("xz", 150)][f], equal_nan=True), f
    d = hist.distributions(bins)
    assert np.array_equal(d["ncells"], [len(m.xCell) for m in models])
    hist.close()
    close_all(chains)


def numpy_pack(cells, slot0, S, counts):
    out = cells.copy()
    at = slot0
    off = [slot0]
    for i, n in enumerate(counts):
        out[:, at:at + n] = cells[:, slot0 + i * S:slot0 + i * S + n]
        at += n
        off.append(at)
    return out, np.array(off, dtype=np.int64)


def pack_cases(chunk):
    big = 2 * chunk + 452
    return [
        ("stride 16", 16, 5, [16, 1, 0, 16, 7, 16, 16, 3, 0, 0, 9, 16]),
        ("tiny ones, then a full one", 16, 0, [1, 0, 2, 1, 1, 0, 1, 16, 16, 5]),
        ("one sample", 16, 3, [7]),
        ("one full sample", 16, 0, [16]),
        ("all full", 16, 2, [16, 16, 16]),
        ("across the chunk", big, 7, [chunk - 1, chunk, chunk + 1, big, 0, 1, 2 * chunk, big, 3]),
        ("a gap smaller than a chunk, samples larger", big, 0, [big - 5, big, big - 1, big]),
    ]


def test_pack_kernel_on_made_up_slots(tt):
    L = tt.lib()
    chunk = L.tdt_history_pack_chunk()
    assert chunk >= 64
    rng = np.random.default_rng(5)
    for name, S, slot0, counts in pack_cases(chunk):
        stride = slot0 + S * len(counts) + 11
        cells = rng.standard_normal((4, stride))
        want, want_off = numpy_pack(cells, slot0, S, counts)
        got = np.ascontiguousarray(cells.copy())
        nc = np.array(counts, dtype=np.int32)
        off = np.zeros(len(counts) + 1, dtype=np.int64)
        rc = L.tdt_history_pack(0, got.ctypes.data, stride, slot0, S, nc.ctypes.data, len(counts), off.ctypes.data)
        assert rc == 0, (name, L.td_last_error(None))
        assert np.array_equal(off, want_off), name
        end = int(want_off[-1])
        assert np.array_equal(got[:, :end], want[:, :end]), name  # the packed samples, and what lay before them
        assert np.array_equal(got[:, stride - 11:], cells[:, stride - 11:]), name  # nothing past the slots
    # slots that do not fit the stride, a sample larger than its slot: refused before any HIP call
    cells = np.zeros((4, 40))
    off = np.zeros(4, dtype=np.int64)
    nc = np.array([16, 16, 16], dtype=np.int32)
    assert L.tdt_history_pack(0, cells.ctypes.data, 40, 0, 16, nc.ctypes.data, 3, off.ctypes.data) == 1
    nc[1] = 17
    assert L.tdt_history_pack(0, cells.ctypes.data, 48, 0, 16, nc.ctypes.data, 3, off.ctypes.data) == 1
