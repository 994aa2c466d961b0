"""Plain numpy / Python references for the chain's nearest-cell search and the wave primitives under it
(csrc/chain_search.h, csrc/wave_ops.h).  Float64 throughout, distances in the reference's own operation
order ((cx - x)^2 + (cy - y)^2) + (cz - z)^2 (MCsub.jl:254; chain_shared.h dist2).  No GPU, no library:
tests/test_nearest_ref_host.py holds this module to brute-force Python loops."""
import math
from fractions import Fraction

import numpy as np

SENTINEL = 1e9  # MCsub.jl:250: a cell wins only strictly below it


def dist2(cx, cy, cz, x, y, z):
    cx, cy, cz = (np.asarray(a, dtype=np.float64) for a in (cx, cy, cz))
    dx, dy, dz = cx - np.float64(x), cy - np.float64(y), cz - np.float64(z)
    return (dx * dx + dy * dy) + dz * dz


def scan_one(stamp, cx, cy, cz, czeta, nslots, q, skip=-1, moved=-1, msite=(0.0, 0.0, 0.0)):
    """One query of wave_full_scan's contract: the lexicographic minimum of (dist2, stamp) over the slots
    s < nslots with stamp[s] >= 0 and s != skip, slot `moved` taken at msite; (d, slot, z), or
    (1e9, -1, 0.0) when no cell lies strictly below the sentinel."""
    stamp = np.asarray(stamp, dtype=np.int64)[:nslots]
    x, y, z = (np.array(a[:nslots], dtype=np.float64) for a in (cx, cy, cz))
    if 0 <= moved < nslots:
        x[moved], y[moved], z[moved] = msite
    d = dist2(x, y, z, q[0], q[1], q[2])
    ok = stamp >= 0
    if 0 <= skip < nslots:
        ok[skip] = False
    ok &= d < SENTINEL
    if not ok.any():
        return SENTINEL, -1, 0.0
    idx = np.flatnonzero(ok)
    dmin = d[idx].min()
    tied = idx[d[idx] == dmin]
    s = int(tied[np.argmin(stamp[tied])])
    return float(dmin), s, float(czeta[s])


def scan_many(stamp, cx, cy, cz, czeta, nslots, q, skip, moved, msite):
    out = [scan_one(stamp, cx, cy, cz, czeta, nslots, q[i], int(skip[i]), int(moved[i]), msite[i])
           for i in range(len(q))]
    return (np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.int32),
            np.array([o[2] for o in out], dtype=np.float64))


def model_nearest(cells, zeta, q, kill=None, moved=None, msite=None, chunk=256):
    """v_nearest on a model in Julia order (cells [n][3], zeta [n]): per query the first minimum of dist2
    over the positions, position kill[i] left out and position moved[i] taken at msite[i] (-1 / None: no
    edit); (d, pos, z) arrays, (1e9, -1, 0.0) where no cell lies strictly below the sentinel."""
    cells = np.asarray(cells, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    nq = len(q)
    kill = np.full(nq, -1) if kill is None else np.asarray(kill)
    moved = np.full(nq, -1) if moved is None else np.asarray(moved)
    msite = np.zeros((nq, 3)) if msite is None else np.asarray(msite, dtype=np.float64)
    d_out, p_out, z_out = np.full(nq, SENTINEL), np.full(nq, -1, dtype=np.int32), np.zeros(nq)
    for a in range(0, nq, chunk):
        b = min(nq, a + chunk)
        qq = q[a:b]
        dx = cells[None, :, 0] - qq[:, None, 0]
        dy = cells[None, :, 1] - qq[:, None, 1]
        dz = cells[None, :, 2] - qq[:, None, 2]
        D = (dx * dx + dy * dy) + dz * dz
        for i in range(a, b):
            if moved[i] >= 0:
                D[i - a, moved[i]] = dist2(msite[i, 0], msite[i, 1], msite[i, 2], q[i, 0], q[i, 1], q[i, 2])
            if kill[i] >= 0:
                D[i - a, kill[i]] = np.inf
        pos = np.argmin(D, axis=1)  # (the first index of the minimum: Julia order decides ties)
        d = D[np.arange(b - a), pos]
        hit = d < SENTINEL
        d_out[a:b][hit] = d[hit]
        p_out[a:b][hit] = pos[hit]
        z_out[a:b][hit] = np.asarray(zeta, dtype=np.float64)[pos[hit]]
    return d_out, p_out, z_out


def model_two_nearest(cells, q):
    """Each query's nearest position c1 and runner-up c2 ((dist2, position) order)."""
    _, c1, _ = model_nearest(cells, np.zeros(len(cells)), q)
    _, c2, _ = model_nearest(cells, np.zeros(len(cells)), q, kill=c1)
    return c1, c2


# ---- the wave primitives, one row of 64 lanes at a time ----
def _row_step(v, shift):
    """v[l] + (v[l - shift] if l - shift is in l's row of 16, else 0.0): a DPP row_shr with zero fill"""
    src = np.zeros_like(v)
    for l in range(64):
        if l % 16 >= shift:
            src[l] = v[l - shift]
    return v + src


def _bcast_step(v, lane, rows):
    """v[l] + (v[the lane `lane` of the row before l's] if l's row is in rows, else 0.0): row_bcast:15 / :31"""
    src = np.zeros_like(v)
    for l in range(64):
        if l // 16 in rows:
            src[l] = v[lane if lane == 31 else 16 * (l // 16) - 1]
    return v + src


def scan_tree(v):
    """wave_scan_f64's six steps on one row: the inclusive prefix sums in the association the header
    documents (row_shr 1, 2, 4, 8 inside rows of 16; row_bcast:15 into rows 1 and 3; row_bcast:31 into
    rows 2 and 3)."""
    v = np.array(v, dtype=np.float64)
    for s in (1, 2, 4, 8):
        v = _row_step(v, s)
    v = _bcast_step(v, 15, (1, 3))
    v = _bcast_step(v, 31, (2, 3))
    return v


GAMMA63 = Fraction(63, 2 ** 53) / (1 - Fraction(63, 2 ** 53))  # any-order summation of 64 terms, u = 2^-53


def sum_error_ok(got, v):
    """|got - sum(v)| <= gamma_63 sum|v|, the sum and the bound exact (rationals)"""
    exact = sum(Fraction(float(t)) for t in v)
    return math.isfinite(got) and abs(Fraction(float(got)) - exact) <= GAMMA63 * sum(abs(Fraction(float(t))) for t in v)


def u64_min(rows):
    return np.min(np.asarray(rows, dtype=np.uint64), axis=1)


def u64_xor(rows):
    return np.bitwise_xor.reduce(np.asarray(rows, dtype=np.uint64), axis=1)


def u64_row_max(rows):
    """[nrows][4]: the maximum of each row of 16 lanes"""
    return np.asarray(rows, dtype=np.uint64).reshape(len(rows), 4, 16).max(axis=2)
