"""tests/nearest_ref.py, the reference of the nearest-cell and wave-primitive GPU tests, against brute-force
Python loops on tiny layouts: the reference itself is under test.  No GPU, no library."""
import math
import struct

import numpy as np

import nearest_ref as nr


def d2_plain(c, q):
    dx, dy, dz = c[0] - q[0], c[1] - q[1], c[2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def scan_plain(stamp, xyz, zeta, nslots, q, skip, moved, msite):
    """A loop over the slots in slot order, keeping the best (d, stamp) pair"""
    best = None
    for s in range(nslots):
        if stamp[s] < 0 or s == skip:
            continue
        d = d2_plain(msite if s == moved else xyz[s], q)
        if not d < 1e9:
            continue
        if best is None or d < best[0] or (d == best[0] and stamp[s] < best[1]):
            best = (d, stamp[s], s)
    return (1e9, -1, 0.0) if best is None else (best[0], best[2], zeta[best[2]])


def test_dist2_operation_order():
    # ((dx^2 + dy^2) + dz^2): with these offsets the other association rounds differently
    c, q = (1e8 + 1.0, 3.0, 1.0), (0.0, 0.0, 0.0)
    a = float(nr.dist2(c[0], c[1], c[2], *q))
    assert a == d2_plain(c, q)
    found = False
    rng = np.random.default_rng(0)
    for _ in range(200):
        c = rng.random(3) * 100.0
        dx, dy, dz = c
        found = found or (dx * dx + dy * dy) + dz * dz != dx * dx + (dy * dy + dz * dz)
        assert float(nr.dist2(c[0], c[1], c[2], 0.0, 0.0, 0.0)) == (dx * dx + dy * dy) + dz * dz
    assert found
    assert float(nr.dist2(30000.0, 10000.0, 0.0, 0.0, 0.0, 0.0)) == 1e9


def test_scan_one_against_a_plain_loop():
    rng = np.random.default_rng(1)
    for case in range(300):
        cap = int(rng.integers(1, 14))
        nslots = int(rng.integers(0, cap + 1))
        xyz = rng.integers(-2, 3, (cap, 3)).astype(np.float64)  # (a tiny cube: ties everywhere)
        stamp = rng.permutation(cap).astype(np.int64) * (1 if case % 3 else (1 << 33))
        stamp[rng.random(cap) < 0.25] = -1
        zeta = rng.random(cap)
        if case % 7 == 0:
            xyz[:, 0] += 40000.0  # everything beyond the sentinel
        for _ in range(6):
            q = rng.integers(-2, 3, 3).astype(np.float64)
            skip = int(rng.integers(-1, cap))
            moved = int(rng.integers(-1, cap))
            msite = rng.integers(-2, 3, 3).astype(np.float64)
            got = nr.scan_one(stamp, xyz[:, 0], xyz[:, 1], xyz[:, 2], zeta, nslots, q, skip, moved, msite)
            want = scan_plain(stamp.tolist(), xyz.tolist(), zeta.tolist(), nslots, q.tolist(), skip, moved,
                              msite.tolist())
            assert got == want, (case, got, want)
    d, s, z = nr.scan_many(stamp, xyz[:, 0], xyz[:, 1], xyz[:, 2], zeta, nslots, np.array([q, q]),
                           np.array([skip, -1]), np.array([moved, -1]), np.array([msite, msite]))
    assert (d[0], s[0], z[0]) == got and len(d) == 2


def test_scan_one_sentinel_edges():
    stamp, zeta = np.array([0, 1], dtype=np.int64), np.array([5.0, 6.0])
    below = np.nextafter(1e9, 0.0)
    x = np.array([30000.0, math.sqrt(below)])
    y = np.array([10000.0, 0.0])
    z = np.zeros(2)
    assert nr.scan_one(stamp, x, y, z, zeta, 1, (0.0, 0.0, 0.0)) == (1e9, -1, 0.0)  # exactly 1e9: not taken
    d, s, v = nr.scan_one(stamp, x, y, z, zeta, 2, (0.0, 0.0, 0.0))
    assert (s, v) == ((1, 6.0) if d < 1e9 else (-1, 0.0))
    assert nr.scan_one(stamp, x, y, z, zeta, 0, (0.0, 0.0, 0.0)) == (1e9, -1, 0.0)


def test_model_nearest_against_a_plain_loop():
    rng = np.random.default_rng(2)
    for case in range(60):
        n = int(rng.integers(2, 12))
        cells = rng.integers(-2, 3, (n, 3)).astype(np.float64)
        zeta = rng.random(n)
        nq = 9
        q = rng.integers(-2, 3, (nq, 3)).astype(np.float64)
        kill = rng.integers(-1, n, nq)
        moved = rng.integers(-1, n, nq)
        moved[moved == kill] = -1
        msite = rng.integers(-2, 3, (nq, 3)).astype(np.float64)
        d, p, z = nr.model_nearest(cells, zeta, q, kill, moved, msite, chunk=4)
        for i in range(nq):  # Julia order IS the stamp order: positions as stamps
            want = scan_plain(list(range(n)), cells.tolist(), zeta.tolist(), n, q[i].tolist(), int(kill[i]),
                              int(moved[i]), msite[i].tolist())
            assert (d[i], p[i], z[i]) == want, (case, i)
        c1, c2 = nr.model_two_nearest(cells, q)
        for i in range(nq):
            order = sorted(range(n), key=lambda c: (d2_plain(cells[c], q[i]), c))
            assert (c1[i], c2[i]) == (order[0], order[1])


def scan_plain_tree(v):
    """wave_scan_f64's association, recursively: a row's prefix sums by doubling, then row 0's total into row
    1 and row 2's into row 3, then row 1's total into rows 2 and 3"""
    rows = []
    for r in range(4):
        w = list(v[16 * r:16 * r + 16])
        for s in (1, 2, 4, 8):
            w = [w[i] + (w[i - s] if i >= s else 0.0) for i in range(16)]
        rows.append(w)
    rows[1] = [x + rows[0][15] for x in rows[1]]
    rows[3] = [x + rows[2][15] for x in rows[3]]
    t = rows[1][15]
    rows[2] = [x + t for x in rows[2]]
    rows[3] = [x + t for x in rows[3]]
    return [x + 0.0 for x in rows[0]] + rows[1] + rows[2] + rows[3]


def test_scan_tree():
    rng = np.random.default_rng(3)
    ints = rng.integers(-1000, 1000, 64).astype(np.float64)
    assert np.array_equal(nr.scan_tree(ints), np.cumsum(ints))
    differs = False
    for _ in range(20):
        v = rng.random(64) + 0.25
        v[int(rng.integers(0, 64))] = 1e16
        got = nr.scan_tree(v)
        want = scan_plain_tree(v.tolist())
        assert [struct.pack("d", x) for x in got] == [struct.pack("d", x) for x in want]
        differs = differs or not np.array_equal(got, np.cumsum(v))
        assert np.allclose(got, np.cumsum(v), rtol=1e-13)
    assert differs  # (the association is visible in these rows)


def test_sum_bound_and_integer_helpers():
    v = np.array([1e16] + [0.3] * 63)
    assert nr.sum_error_ok(math.fsum(v), v) and nr.sum_error_ok(float(np.sum(v[::-1])), v)
    assert not nr.sum_error_ok(math.fsum(v) * (1.0 + 1e-13), v) and not nr.sum_error_ok(float("nan"), v)
    assert float(nr.GAMMA63) == 63 * 2.0 ** -53 / (1 - 63 * 2.0 ** -53)
    rows = np.array([[1 << 63] + [5] * 63, list(range(64))], dtype=np.uint64)
    assert nr.u64_min(rows).tolist() == [5, 0]
    assert nr.u64_xor(rows).tolist() == [(1 << 63) ^ 5, 0]
    assert nr.u64_row_max(rows).tolist() == [[1 << 63, 5, 5, 5], [15, 31, 47, 63]]
