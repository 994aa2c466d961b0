"""The cross-lane primitives of csrc/wave_ops.h, each on its own (tdt_wave_ops: one wave per row of 64
words, every lane's result returned), against numpy on the same row.  A wrong row mask on a row_bcast, a
wrong identity or a signed compare gives a wrong result in certain lanes or for certain keys only: the rows
below put the deciding value in every lane in turn and use keys with bits 63 and 31 set.  Bit for bit unless
stated; a failure names the row (its label and index) and the lanes."""
import numpy as np
import pytest

import nearest_ref as nr

pytestmark = pytest.mark.gpu

U = np.uint64
ALL1 = U(0xFFFFFFFFFFFFFFFF)
TD_ERR_ARG = 1
OPS = {"min_u64": 0, "min_u64_2p": 1, "min_u32": 2, "xor_u64": 3, "row_max_u64": 4, "scan_f64": 5, "sum_f64": 6,
       "readlane_f64": 7}


def P(a):
    return None if a is None else a.ctypes.data


def run(tt, op, rows, arg=None):
    rows = np.ascontiguousarray(rows, dtype=U)
    assert rows.ndim == 2 and rows.shape[1] == 64
    out = np.full_like(rows, 0xDEADBEEF)
    a = None if arg is None else np.ascontiguousarray(arg, dtype=np.int32)
    rc = tt.lib().tdt_wave_ops(0, OPS[op], P(rows), P(a), len(rows), P(out))
    assert rc == 0, (op, rc)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(U)


def hi_lo(hi, lo):
    return (np.asarray(hi, dtype=U) << U(32)) | np.asarray(lo, dtype=U)


def key_rows():
    """(label, row) for the three minima: 64-bit keys."""
    rng = np.random.default_rng(20240611)
    rows = []
    for lane in range(64):  # the unique minimum in every lane in turn, everything else larger
        r = rng.integers(1 << 20, 1 << 62, 64, dtype=np.uint64)
        r[lane] = 7 + lane
        rows.append(("unique minimum in lane %d" % lane, r))
    for lane in range(64):  # the same through the low words alone: one high word in all lanes
        r = hi_lo(np.full(64, 0x12345), rng.integers(1 << 10, 1 << 32, 64, dtype=np.uint64))
        r[lane] = hi_lo(0x12345, lane)
        rows.append(("equal high words, unique low minimum in lane %d" % lane, r))
    rows.append(("all lanes equal", np.full(64, 0x0123456789ABCDEF, dtype=U)))
    rows.append(("all lanes ~0 (the identity)", np.full(64, ALL1, dtype=U)))
    rows.append(("all lanes 0", np.zeros(64, dtype=U)))
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):  # signed compares: bit 63, bit 31
        r = np.full(64, 0x8000000000000000, dtype=U)
        r[lane] = 0x7FFFFFFFFFFFFFFF
        rows.append(("bit 63: 0x7fff... in lane %d among 0x8000..." % lane, r))
        r = np.full(64, 0x7FFFFFFFFFFFFFFF, dtype=U)
        r[lane] = 0x8000000000000000
        rows.append(("bit 63: 0x8000... in lane %d among 0x7fff..." % lane, r))
        r = hi_lo(np.full(64, 9), np.full(64, 0x80000000))
        r[lane] = hi_lo(9, 0x7FFFFFFF)
        rows.append(("bit 31: low 0x7fffffff in lane %d among 0x80000000" % lane, r))
        r = hi_lo(np.full(64, 9), np.full(64, 0x7FFFFFFF))
        r[lane] = hi_lo(9, 0x80000000)
        rows.append(("bit 31: low 0x80000000 in lane %d among 0x7fffffff" % lane, r))
        r = hi_lo(np.full(64, 0x80000000), rng.integers(0, 1 << 32, 64, dtype=np.uint64))
        r[lane] = hi_lo(0x7FFFFFFF, 0xFFFFFFFF)
        rows.append(("bit 63 through the high word, lane %d" % lane, r))
    # the two-pass minimum: one lane holds the minimal high word (its readlane arm); the others' low
    # words are all smaller than the winner's
    for lane in (0, 1, 15, 16, 31, 32, 33, 47, 48, 62, 63):
        r = hi_lo(rng.integers(101, 1 << 31, 64, dtype=np.uint64), rng.integers(0, 1000, 64, dtype=np.uint64))
        r[lane] = hi_lo(100, 0xFFFF0000)
        rows.append(("one lane (%d) holds the minimal high word" % lane, r))
    # 2, 17 and 64 lanes tie on the high word with distinct low words, the smallest in DPP row 0 / row 3;
    # every other lane has a larger high word and a SMALLER low word, which the result must ignore
    for k in (2, 17, 64):
        for row_of_min in (0, 3):
            for rep in range(3):
                lanes = rng.permutation(64)[:k]
                minlane = int(rng.integers(16 * row_of_min, 16 * row_of_min + 16))
                if minlane not in lanes:
                    lanes[0] = minlane
                lo = rng.permutation(np.arange(5000, 5000 + 64, dtype=np.uint64))
                r = hi_lo(rng.integers(78, 1 << 32, 64, dtype=np.uint64), rng.integers(0, 5000, 64, dtype=np.uint64))
                r[lanes] = hi_lo(np.full(k, 77), lo[:k])
                r[minlane] = hi_lo(77, 4999)
                rows.append(("%d lanes tie on the high word, smallest low word in lane %d" % (k, minlane), r))
    # non-negative doubles order like their bits
    special = np.array([0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 1.0, np.nextafter(1e9, 0.0), 1e9,
                        np.nextafter(1e9, 2e9), 1.7976931348623157e308, np.inf])
    for rep in range(24):
        v = special[rng.integers(0, len(special), 64)]
        if rep % 2:
            v = np.where(rng.random(64) < 0.5, v, rng.random(64) * 10.0 ** rng.integers(-300, 300, 64))
        if rep >= 12:  # without +0.0 and the denormals at the bottom: another minimum
            v = np.maximum(v, special[3 + rep % 4])
        rows.append(("doubles' bit patterns %d" % rep, bits(v)))
    rows.append(("doubles: 1e9 among +inf", bits(np.where(np.arange(64) == 40, 1e9, np.inf))))
    rows.append(("doubles: the largest below 1e9 in lane 17 among 1e9",
                 bits(np.where(np.arange(64) == 17, np.nextafter(1e9, 0.0), 1e9))))
    for rep in range(40):
        rows.append(("random 64-bit %d" % rep, rng.integers(0, 1 << 64, 64, dtype=np.uint64)))
    for rep in range(40):  # few distinct high words: the second pass decides
        rows.append(("random, high words of 3 values %d" % rep,
                     hi_lo(rng.integers(0, 3, 64) + 0x7FFFFFFE, rng.integers(0, 1 << 32, 64, dtype=np.uint64))))
    return rows


def expect_all_lanes(op, rows, got, want):
    """got[r][l] == want[r] in every lane"""
    bad = np.argwhere(got != np.asarray(want, dtype=U)[:, None])
    if bad.size:
        r = int(bad[0][0])
        lanes = bad[bad[:, 0] == r][:, 1]
        raise AssertionError("%s: row %d (%s): lanes %s return %s, expected %#x; %d rows differ"
                             % (op, r, rows[r][0], lanes[:16].tolist(), [hex(int(x)) for x in got[r, lanes[:4]]],
                                int(want[r]), len(set(bad[:, 0].tolist()))))


@pytest.mark.parametrize("op", ["min_u64", "min_u64_2p", "min_u32"])
def test_wave_minimum(tt, op):
    rows = key_rows()
    assert 300 <= len(rows) <= 600
    mat = np.stack([r for _, r in rows])
    got = run(tt, op, mat)
    want = nr.u64_min(mat & U(0xFFFFFFFF)) if op == "min_u32" else nr.u64_min(mat)
    expect_all_lanes(op, rows, got, want)
    if op != "min_u32":  # the doubles' rows: the result is the numeric minimum
        for i, (label, r) in enumerate(rows):
            if label.startswith("doubles"):
                assert got[i, 0:1].view(np.float64)[0] == r.view(np.float64).min(), (op, i, label)


def test_wave_xor(tt):
    rng = np.random.default_rng(5)
    rows = [(label, r) for label, r in key_rows() if not label.startswith("equal high")]
    for lane in range(64):  # one lane's word alone: it must reach every lane from every lane
        r = np.zeros(64, dtype=U)
        r[lane] = rng.integers(1, 1 << 64, dtype=np.uint64)
        rows.append(("one non-zero word in lane %d" % lane, r))
    mat = np.stack([r for _, r in rows])
    expect_all_lanes("xor_u64", rows, run(tt, "xor_u64", mat), nr.u64_xor(mat))


def test_row_maximum(tt):
    """row_max_u64 is specified in the last lane of each row of 16 only: lanes 15, 31, 47, 63 are read."""
    rng = np.random.default_rng(6)
    rows = []
    for lane in range(64):  # the unique maximum in every lane in turn, everything else smaller
        r = rng.integers(0, 1 << 40, 64, dtype=np.uint64)
        r[lane] = (1 << 63) + lane
        rows.append(("unique maximum in lane %d" % lane, r))
    for lane in range(64):  # decided by the low words
        r = hi_lo(np.full(64, 0xABCDE), rng.integers(0, 1 << 31, 64, dtype=np.uint64))
        r[lane] = hi_lo(0xABCDE, 0xFFFFFF00 + lane)
        rows.append(("equal high words, unique low maximum in lane %d" % lane, r))
    rows.append(("all lanes equal", np.full(64, 0x0123456789ABCDEF, dtype=U)))
    rows.append(("all lanes 0 (the identity)", np.zeros(64, dtype=U)))
    rows.append(("all lanes ~0", np.full(64, ALL1, dtype=U)))
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):
        r = np.full(64, 0x7FFFFFFFFFFFFFFF, dtype=U)
        r[lane] = 0x8000000000000000
        rows.append(("bit 63: 0x8000... in lane %d among 0x7fff..." % lane, r))
        r = hi_lo(np.full(64, 9), np.full(64, 0x7FFFFFFF))
        r[lane] = hi_lo(9, 0x80000000)
        rows.append(("bit 31: low 0x80000000 in lane %d among 0x7fffffff" % lane, r))
        r = hi_lo(np.full(64, 0x7FFFFFFF), np.full(64, 0xFFFFFFFF))
        r[lane] = hi_lo(0x80000000, 0)
        rows.append(("bit 63 through the high word, lane %d" % lane, r))
    for rep in range(60):
        rows.append(("random 64-bit %d" % rep, rng.integers(0, 1 << 64, 64, dtype=np.uint64)))
    mat = np.stack([r for _, r in rows])
    got = run(tt, "row_max_u64", mat)[:, 15::16]
    want = nr.u64_row_max(mat)
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("row_max_u64: row %d (%s): lane %d returns %#x, expected %#x; %d (row, lane) pairs differ"
                           % (bad[0][0], rows[bad[0][0]][0], 16 * bad[0][1] + 15, int(got[tuple(bad[0])]),
                              int(want[tuple(bad[0])]), len(bad)))


def test_wave_scan(tt):
    rng = np.random.default_rng(7)
    # integer-valued doubles, every partial sum below 2^53: any association is exact -- np.cumsum in every lane
    rows = [("integers %d" % i, rng.integers(-(1 << 40), 1 << 40, 64).astype(np.float64)) for i in range(40)]
    rows += [("ones", np.ones(64)), ("zeros", np.zeros(64)), ("lane numbers", np.arange(64.0)),
             ("2^46 in every lane", np.full(64, 2.0 ** 46))]
    for lane in range(64):
        rows.append(("one non-zero value in lane %d" % lane, np.where(np.arange(64) == lane, 3.0 + lane, 0.0)))
    mat = np.stack([r for _, r in rows])
    assert np.abs(np.cumsum(np.abs(mat), axis=1)).max() < 2.0 ** 53
    got = run(tt, "scan_f64", bits(mat)).view(np.float64)
    want = np.cumsum(mat, axis=1)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, ("scan_f64: row %d (%s): lane %d returns %r, expected %r; %d (row, lane) pairs differ"
                           % (bad[0][0], rows[bad[0][0]][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], len(bad)))
    # one huge and 63 tiny values: the rounding depends on the association, which the header documents
    rows = []
    for lane in (0, 1, 7, 15, 16, 30, 31, 32, 37, 47, 48, 63):
        v = rng.random(64) + 0.25
        v[lane] = 1e16 * (1.0 + rng.random())
        rows.append(("huge value in lane %d" % lane, v))
    rows += [("random doubles %d" % i, rng.standard_normal(64) * 10.0 ** rng.integers(-8, 8, 64)) for i in range(20)]
    mat = np.stack([r for _, r in rows])
    got = run(tt, "scan_f64", bits(mat)).view(np.float64)
    want = np.stack([nr.scan_tree(r) for r in mat])
    assert any(not np.array_equal(bits(np.cumsum(r)), bits(w)) for r, w in zip(mat, want))  # (the order matters here)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, ("scan_f64 (tree association): row %d (%s): lane %d returns %r, expected %r; %d pairs differ"
                           % (bad[0][0], rows[bad[0][0]][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], len(bad)))


def test_wave_sum(tt):
    rng = np.random.default_rng(8)
    ints = [("integers %d" % i, rng.integers(-(1 << 40), 1 << 40, 64).astype(np.float64)) for i in range(40)]
    for lane in range(64):
        ints.append(("one non-zero value in lane %d" % lane, np.where(np.arange(64) == lane, 3.0 + lane, 0.0)))
    ints += [("ones", np.ones(64)), ("zeros", np.zeros(64))]
    anyr = [("random doubles %d" % i, rng.standard_normal(64) * 10.0 ** rng.integers(-8, 8, 64)) for i in range(40)]
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):
        v = rng.random(64) + 0.25
        v[lane] = -1e16 * (1.0 + rng.random())
        anyr.append(("huge value in lane %d" % lane, v))
    rows = ints + anyr
    mat = np.stack([r for _, r in rows])
    got = run(tt, "sum_f64", bits(mat)).view(np.float64)
    for i, (label, r) in enumerate(rows):
        lanes = np.flatnonzero(bits(got[i]) != bits(got[i, :1]))
        assert lanes.size == 0, ("sum_f64: row %d (%s): lanes %s differ from lane 0" % (i, label, lanes[:16].tolist()))
        if i < len(ints):  # exact in any order
            assert got[i, 0] == float(np.sum(r.astype(np.int64))), ("sum_f64: row %d (%s)" % (i, label), got[i, 0])
        else:  # any order: |got - sum| <= gamma_63 sum|v|
            assert nr.sum_error_ok(got[i, 0], r), ("sum_f64: row %d (%s)" % (i, label), got[i, 0], float(np.sum(r)))


def test_readlane(tt):
    rng = np.random.default_rng(9)
    lanes = np.concatenate([np.arange(64), rng.integers(0, 64, 64)]).astype(np.int32)
    mat = rng.integers(0, 1 << 64, (len(lanes), 64), dtype=np.uint64)  # (any bits: the value is only moved)
    mat[5] = bits(np.arange(64.0))
    got = run(tt, "readlane_f64", mat, lanes)
    want = mat[np.arange(len(lanes)), lanes]
    bad = np.argwhere(got != want[:, None])
    assert bad.size == 0, ("readlane_f64: row %d (lane %d asked): lane %d returns %#x, expected %#x"
                           % (bad[0][0], lanes[bad[0][0]], bad[0][1], int(got[tuple(bad[0])]), int(want[bad[0][0]])))


def test_wave_ops_refuses_bad_arguments(tt):
    """Checked before any HIP call: a lane outside 0 .. 63 for readlane, an unknown primitive, no rows."""
    L = tt.lib()
    rows = np.zeros((2, 64), dtype=U)
    out = np.zeros_like(rows)
    for arg in ([0, 64], [-1, 3]):
        a = np.array(arg, dtype=np.int32)
        assert L.tdt_wave_ops(0, 7, P(rows), P(a), 2, P(out)) == TD_ERR_ARG
    assert L.tdt_wave_ops(0, 7, P(rows), None, 2, P(out)) == TD_ERR_ARG
    assert L.tdt_wave_ops(0, 8, P(rows), None, 2, P(out)) == TD_ERR_ARG
    assert L.tdt_wave_ops(0, 0, P(rows), None, 0, P(out)) == TD_ERR_ARG
