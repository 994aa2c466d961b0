"""wave_full_scan (csrc/chain_search.h), the out-of-line fallback of every nearest-cell query the bucket
grid cannot prove, on slot layouts built for it (tdt_nearest_scan; no chain): the lexicographic minimum of
(squared distance, stamp) over the live slots below nslots, with a killed slot left out and a moved slot
taken at its proposed site -- v_nearest's first-index rule (MCsub.jl:247-263) through stamps.  Small-integer
coordinates, so that distances tie exactly; every query's (d, slot, z) bit for bit against
nearest_ref.scan_one.  A failure names the layout and the query."""
import itertools

import numpy as np
import pytest

import nearest_ref as nr

pytestmark = pytest.mark.gpu

TD_ERR_ARG = 1


def P(a):
    return a.ctypes.data


class Layout:
    def __init__(self, cap, nslots, name):
        self.cap, self.nslots, self.name = cap, nslots, name
        self.stamp = np.full(cap, -1, dtype=np.int64)
        self.xyz = np.zeros((cap, 3))
        self.zeta = 1000.0 + np.arange(cap, dtype=np.float64)  # (the value names the slot)
        self.queries = []  # (label, q, skip, moved, msite)

    def ask(self, label, q, skip=-1, moved=-1, msite=(0.0, 0.0, 0.0)):
        self.queries.append((label, tuple(map(float, q)), int(skip), int(moved), tuple(map(float, msite))))

    def ref(self, i):
        _, q, skip, moved, msite = self.queries[i]
        return nr.scan_one(self.stamp, self.xyz[:, 0], self.xyz[:, 1], self.xyz[:, 2], self.zeta, self.nslots, q, skip,
                           moved, msite)


def run(tt, lay):
    nq = len(lay.queries)
    q = np.ascontiguousarray([t[1] for t in lay.queries], dtype=np.float64)
    skip = np.array([t[2] for t in lay.queries], dtype=np.int32)
    moved = np.array([t[3] for t in lay.queries], dtype=np.int32)
    msite = np.ascontiguousarray([t[4] for t in lay.queries], dtype=np.float64)
    x, y, z = (np.ascontiguousarray(lay.xyz[:, a]) for a in range(3))
    d, s, v = np.full(nq, -7.0), np.full(nq, -7, dtype=np.int32), np.full(nq, -7.0)
    rc = tt.lib().tdt_nearest_scan(0, P(lay.stamp), P(x), P(y), P(z), P(lay.zeta), lay.cap, lay.nslots, P(q), P(skip),
                                   P(moved), P(msite), nq, P(d), P(s), P(v))
    assert rc == 0, (lay.name, rc)
    return d, s, v


def check(tt, lay):
    """Every query against the reference; returns the reference answers."""
    d, s, v = run(tt, lay)
    refs = [lay.ref(i) for i in range(len(lay.queries))]
    for i, (rd, rs, rz) in enumerate(refs):
        got = (float(d[i]), int(s[i]), float(v[i]))
        same = np.float64(got[0]).tobytes() == np.float64(rd).tobytes() and got[1] == rs and \
            np.float64(got[2]).tobytes() == np.float64(rz).tobytes()
        assert same, ("layout %s, query %d (%s): q=%s skip=%d moved=%d msite=%s: got (d, slot, z) = %r, expected %r "
                      "(stamps: got %s, expected %s)"
                      % ((lay.name, i) + lay.queries[i] + (got, (rd, rs, rz),
                         lay.stamp[got[1]] if 0 <= got[1] < lay.cap else None, lay.stamp[rs] if rs >= 0 else None)))
    return refs


# ---------------------------------------------------------------- sizes ----
SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 1025]


@pytest.mark.parametrize("free", ["none", "ends", "scattered"])
@pytest.mark.parametrize("extra", [0, 70])
@pytest.mark.parametrize("nslots", SIZES)
def test_sizes_free_slots_and_slots_past_the_mark(tt, nslots, extra, free):
    """nslots around the 64-lane row, the 512-slot round and a partial last round, with cap == nslots (the
    loads of the last round clamp to cap - 1) and cap > nslots (slots past the high-water mark hold live-looking
    cells AT the query points, with the smallest stamps: they win if read).  Free slots (stamp -1) also sit at
    the query points: at slots 0 and nslots - 1, or scattered.  Stamps are a permutation out of slot order."""
    rng = np.random.default_rng(1000 * nslots + extra + len(free))
    cap = nslots + extra
    lay = Layout(cap, nslots, "nslots=%d cap=%d free=%s" % (nslots, cap, free))
    queries = rng.integers(-12, 13, (10, 3)).astype(np.float64)
    lay.xyz[:] = rng.integers(-12, 13, (cap, 3))  # (a small cube: exact ties among the live cells too)
    lay.stamp[:nslots] = 100 + rng.permutation(nslots)
    lay.stamp[nslots:] = np.arange(extra)  # past the mark: stamps below every live one
    lay.xyz[nslots:] = queries[np.arange(extra) % len(queries)]
    if free == "ends":
        gone = sorted({0, nslots - 1})
    elif free == "scattered":
        gone = np.flatnonzero(rng.random(nslots) < 0.2).tolist()
    else:
        gone = []
    for k, s in enumerate(gone):
        lay.stamp[s] = -1
        lay.xyz[s] = queries[k % len(queries)]
    for k, q in enumerate(queries):
        lay.ask("point %d" % k, q)
    live = np.flatnonzero(lay.stamp[:nslots] >= 0)
    for k in range(min(4, len(live))):  # a live cell's own site: d = 0, duplicates tie
        lay.ask("site of slot %d" % live[-1 - k], lay.xyz[live[-1 - k]])
    refs = check(tt, lay)
    if len(live) == 0:
        assert all(r == (nr.SENTINEL, -1, 0.0) for r in refs)
    else:
        assert all(0 <= r[1] < nslots and lay.stamp[r[1]] >= 100 for r in refs)


# ----------------------------------------------------------------- ties ----
def shell(n2, count, rng):
    """`count` distinct integer offsets of squared length n2, shuffled"""
    r = int(n2 ** 0.5) + 1
    pts = [p for p in itertools.product(range(-r, r + 1), repeat=3) if p[0] * p[0] + p[1] * p[1] + p[2] * p[2] == n2]
    assert len(pts) >= count, (n2, len(pts))
    return np.array(pts, dtype=np.float64)[rng.permutation(len(pts))[:count]]


# Groups of cells at bit-equal distance from their query (all on one integer shell of squared radius 41 around
# the group's centre), by where the scan meets them.  Lane = slot % 64, round = slot // 512, DPP row = lane // 16.
TIE_GROUPS = {
    "2 in one lane, rounds 0 and 1": [5, 5 + 512],
    "2 in one lane, one round": [40, 40 + 64],
    "3 in one lane: s, s+64, s+512": [9, 9 + 64, 9 + 512],
    "64 in one lane, 8 rounds": [21 + 64 * k for k in range(64)],
    "2 in lanes of one row": [128 + 1, 128 + 14],
    "3 in lanes of one row": [192 + 16, 192 + 20, 192 + 31],
    "64 in the 16 lanes of row 2, rounds 0 and 1": [64 * k + l for k in (4, 5, 12, 13) for l in range(32, 48)],
    "2 in rows 0 and 3": [320 + 2, 320 + 50],
    "3 in rows 0, 1 and 3": [384 + 15, 384 + 16, 384 + 63],
    "64 in the 64 lanes of one round": list(range(4096, 4160)),
}
TIE_CAP, TIE_NSLOTS = 4200, 4170
assert len(set(sum(TIE_GROUPS.values(), []))) == sum(len(g) for g in TIE_GROUPS.values())  # (no slot in two groups)


def tie_layout(order, seed):
    """Every group of TIE_GROUPS in one layout, each around its own centre, the other cells far from all.
    Stamps inside a group: `asc` grow with the slot, `desc` fall with it (the smallest stamp in the highest
    slot), `random`, `big` (above 2^32, the low words in the opposite order of the high ones)."""
    rng = np.random.default_rng(seed)
    lay = Layout(TIE_CAP, TIE_NSLOTS, "ties, stamps %s" % order)
    lay.xyz[:] = np.array([0.0, 5000.0, 0.0]) + rng.integers(-40, 41, (TIE_CAP, 3))
    rank = rng.permutation(TIE_CAP)  # stamps: a permutation out of slot order
    lay.stamp[:] = rank
    lay.stamp[rng.permutation(TIE_NSLOTS)[:300]] = -1  # free slots, scattered (below, the groups' slots are live)
    pool = np.sort(rng.permutation(TIE_CAP)[:sum(len(g) for g in TIE_GROUPS.values())])
    lay.groups = {}
    at = 0
    for j, (name, slots) in enumerate(TIE_GROUPS.items()):
        centre = np.array([300.0 * (j + 1), 0.0, 0.0])
        lay.xyz[slots] = centre + shell(41, len(slots), rng)
        st = pool[at:at + len(slots)]  # distinct stamps of this group, ascending
        at += len(slots)
        if order == "desc":
            st = st[::-1]
        elif order in ("random", "big"):
            st = rng.permutation(st)
        lay.stamp[slots] = st  # (slots are listed in ascending order)
        lay.groups[name] = (centre, list(slots))
    # the rest keep stamps that collide with none of the groups'
    others = np.setdiff1d(np.arange(TIE_CAP), sum(TIE_GROUPS.values(), []))
    live = others[lay.stamp[others] >= 0]
    lay.stamp[live] = TIE_CAP + rng.permutation(len(live))
    if order == "big":  # 64-bit stamps: order by the high word; the low words run the other way
        s = lay.stamp
        lay.stamp = np.where(s >= 0, (s << 33) | ((2 * TIE_CAP - s) & 0xFFFFFFFF), -1).astype(np.int64)
    assert len(np.unique(lay.stamp[lay.stamp >= 0])) == (lay.stamp >= 0).sum()
    return lay


@pytest.mark.parametrize("order", ["asc", "desc", "random", "big"])
def test_ties_go_to_the_smallest_stamp(tt, order):
    lay = tie_layout(order, 77)
    if order == "big":
        assert lay.stamp.max() > 1 << 40
    want = {}
    for name, (centre, slots) in lay.groups.items():
        lay.ask(name, centre)
        best = min(slots, key=lambda s: lay.stamp[s])
        if order == "desc":
            assert best == max(slots)  # the smallest stamp sits in the highest slot
        want[name] = [best]
        # the winner killed: the answer moves to the next stamp of the group; killed again: to the third
        by_stamp = sorted(slots, key=lambda s: lay.stamp[s])
        lay.ask(name + ", the winner killed", centre, skip=by_stamp[0])
        want[name].append(by_stamp[1])
        # the winner moved away: the same; moved back onto the centre: it wins alone at d = 0
        lay.ask(name + ", the winner moved away", centre, moved=by_stamp[0], msite=(0.0, -9000.0, 0.0))
        want[name].append(by_stamp[1])
        lay.ask(name + ", the last of the group moved onto the query", centre, moved=by_stamp[-1], msite=centre)
        want[name].append(by_stamp[-1])
    refs = check(tt, lay)
    # (the reference itself against the group's construction)
    flat = [s for name in lay.groups for s in want[name]]
    assert [r[1] for r in refs] == flat
    assert all(r[0] == (0.0 if i % 4 == 3 else 41.0) for i, r in enumerate(refs))


# ------------------------------------------------------- killed and moved ----
def plain_layout(seed, cap=700, nslots=650):
    rng = np.random.default_rng(seed)
    lay = Layout(cap, nslots, "plain %d" % seed)
    lay.xyz[:] = rng.integers(-30, 31, (cap, 3))
    lay.stamp[:] = rng.permutation(cap)
    lay.stamp[rng.permutation(nslots)[:60]] = -1
    return lay, rng


def test_killed_cell(tt):
    """skip = the true winner (the answer is the runner-up), a free slot, a far cell (no effect either)."""
    lay, rng = plain_layout(31)
    base = []
    for k in range(40):
        q = rng.integers(-30, 31, 3).astype(np.float64)
        d0, s0, _ = nr.scan_one(lay.stamp, lay.xyz[:, 0], lay.xyz[:, 1], lay.xyz[:, 2], lay.zeta, lay.nslots, q)
        far = int(np.argmax(np.where(lay.stamp[:lay.nslots] >= 0, nr.dist2(*lay.xyz[:lay.nslots].T, *q), -1.0)))
        free = int(rng.choice(np.flatnonzero(lay.stamp[:lay.nslots] < 0)))
        lay.ask("point %d, no edit" % k, q)
        lay.ask("point %d, winner %d killed" % (k, s0), q, skip=s0)
        lay.ask("point %d, free slot %d killed" % (k, free), q, skip=free)
        lay.ask("point %d, far cell %d killed" % (k, far), q, skip=far)
        lay.ask("point %d, a slot past nslots killed" % k, q, skip=lay.nslots + k)
        base.append((d0, s0))
    refs = check(tt, lay)
    for k, (d0, s0) in enumerate(base):
        r = refs[5 * k:5 * k + 5]
        assert r[0][:2] == (d0, s0) and r[1][1] != s0 and r[1][0] >= d0
        assert r[2] == r[0] and r[3] == r[0] and r[4] == r[0]


def test_moved_cell(tt):
    """The winner moved away; a far cell moved onto the query (d = 0); a cell moved onto the exact site of
    the current winner, once with a smaller and once with a larger stamp than the winner's."""
    lay, rng = plain_layout(32)
    live = np.flatnonzero(lay.stamp[:lay.nslots] >= 0)
    n_smaller = n_larger = 0
    expect = {}
    for k in range(40):
        q = rng.integers(-30, 31, 3).astype(np.float64) + 0.5  # (off the lattice: no cell at d = 0)
        d0, s0, _ = nr.scan_one(lay.stamp, lay.xyz[:, 0], lay.xyz[:, 1], lay.xyz[:, 2], lay.zeta, lay.nslots, q)
        dist = nr.dist2(*lay.xyz[live].T, *q)
        far = int(live[np.argmax(dist)])
        lay.ask("point %d, no edit" % k, q)
        lay.ask("point %d, winner %d moved away" % (k, s0), q, moved=s0, msite=(500.0, 500.0, 500.0))
        lay.ask("point %d, far cell %d moved onto the query" % (k, far), q, moved=far, msite=q)
        others = live[(live != s0) & (dist > d0)]
        lo = others[lay.stamp[others] < lay.stamp[s0]]
        hi = others[lay.stamp[others] > lay.stamp[s0]]
        if len(lo):
            expect[len(lay.queries)] = (d0, int(lo[-1]))  # the moved cell takes the tie
            lay.ask("point %d, cell %d (smaller stamp) moved onto winner %d" % (k, lo[-1], s0), q, moved=lo[-1],
                    msite=lay.xyz[s0])
            n_smaller += 1
        if len(hi):
            expect[len(lay.queries)] = (d0, s0)  # the winner keeps it
            lay.ask("point %d, cell %d (larger stamp) moved onto winner %d" % (k, hi[0], s0), q, moved=hi[0],
                    msite=lay.xyz[s0])
            n_larger += 1
        lay.ask("point %d, a free slot moved onto the query" % k, q,
                moved=int(np.flatnonzero(lay.stamp[:lay.nslots] < 0)[k]), msite=q)
    assert n_smaller >= 10 and n_larger >= 10
    refs = check(tt, lay)
    for (label, *_), r in zip(lay.queries, refs):
        if "far cell" in label:
            assert r[0] == 0.0
    for i, want in expect.items():  # (the reference itself against the construction)
        assert refs[i][:2] == want, (lay.queries[i][0], refs[i], want)


# ------------------------------------------------------------- sentinel ----
def below_1e9():
    """A site (30000, y, 0) whose squared distance from the origin is the largest double below 1e9"""
    target = np.nextafter(1e9, 0.0)
    y = 10000.0
    for _ in range(64):
        y = np.nextafter(y, 0.0)
        if nr.dist2(30000.0, y, 0.0, 0.0, 0.0, 0.0) == target:
            return (30000.0, float(y), 0.0)
    raise AssertionError("no such site")


def test_sentinel(tt):
    """A cell wins only strictly below 1e9 (MCsub.jl:250, 255)."""
    origin = (0.0, 0.0, 0.0)
    assert nr.dist2(30000.0, 10000.0, 0.0, *origin) == 1e9
    near = below_1e9()
    for name, sites, winner in (("every cell at d >= 1e9", [(40000.0, 0.0, 0.0), (30000.0, 10000.0, 0.0),
                                                            (0.0, 0.0, 1e100), (31623.0, 0.0, 0.0)], -1),
                                ("one cell at exactly 1e9", [(30000.0, 10000.0, 0.0)], -1),
                                ("one cell at the largest double below 1e9", [near], 0),
                                ("1e9 (smaller stamp) beside the largest double below it",
                                 [(30000.0, 10000.0, 0.0), near, (10000.0, 30000.0, 0.0)], 1)):
        for cap in (len(sites), 70):
            lay = Layout(cap, cap, "%s, cap %d" % (name, cap))
            lay.xyz[:] = (1e6, 1e6, 1e6)
            lay.stamp[:] = 10 + np.arange(cap)
            at = [0, cap - 1, cap // 2, 1][:len(sites)] if cap > len(sites) else list(range(len(sites)))
            for k, (s, site) in enumerate(zip(at, sites)):
                lay.xyz[s] = site
                lay.stamp[s] = k
            lay.ask("the origin", origin)
            lay.ask("the origin, slot %d killed" % at[0], origin, skip=at[0])
            lay.ask("the origin, slot %d moved to 1e9 exactly" % at[0], origin, moved=at[0],
                    msite=(10000.0, 30000.0, 0.0))
            refs = check(tt, lay)
            assert refs[0][1] == (at[winner] if winner >= 0 else -1), (lay.name, refs[0])
            if winner < 0:
                assert refs[0] == (1e9, -1, 0.0)
            else:
                assert refs[0][0] == np.nextafter(1e9, 0.0)


def test_nearest_scan_refuses_bad_arguments(tt):
    """Checked before any HIP call: nslots > cap, a killed or moved slot outside [-1, cap)."""
    lay = Layout(8, 8, "refusals")
    lay.stamp[:] = np.arange(8)
    L = tt.lib()
    x, y, z = (np.ascontiguousarray(lay.xyz[:, a]) for a in range(3))
    q, m = np.zeros((1, 3)), np.zeros((1, 3))
    d, s, v = np.zeros(1), np.zeros(1, dtype=np.int32), np.zeros(1)

    def call(cap, nslots, skip, moved):
        sk, mv = np.array([skip], dtype=np.int32), np.array([moved], dtype=np.int32)
        return L.tdt_nearest_scan(0, P(lay.stamp), P(x), P(y), P(z), P(lay.zeta), cap, nslots, P(q), P(sk), P(mv), P(m),
                                  1, P(d), P(s), P(v))

    assert call(8, 9, -1, -1) == TD_ERR_ARG
    assert call(0, 0, -1, -1) == TD_ERR_ARG
    for bad in (8, -2, 1 << 30):
        assert call(8, 8, bad, -1) == TD_ERR_ARG
        assert call(8, 8, -1, bad) == TD_ERR_ARG
    assert call(8, 8, 7, 7) == 0
