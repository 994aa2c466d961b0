"""GPU: the quantile and histogram kernels (csrc/marginals.hip) on value matrices designed to reach what
zeta in [0, 50] never does: the whole double range (infinities, zeros of both signs, denormals, the largest
doubles, NaN in designated columns), every tile width of the resident kernel (tdt_marginals_plan says which
shape runs which), 64 unsorted probabilities with duplicates, column lengths around the radix select's
512-thread stride, and bins whose edges are the values themselves.  Every comparison is bit for bit against
marginals_ref.py on the V that ctx.rasterize returned: NaN as a mask, everything else as 64-bit patterns."""
import numpy as np
import pytest

import marginals_ref as mref
from marginals_ref import DBL_MAX, SPECIAL

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.025, 0.05, 1 / 3, 0.5, 0.95, 1.0)
NQ = 70  # eight full tiles of 8 nodes and one of 6


@pytest.fixture(scope="module")
def ctx(tt, ds):
    return tt.TdContext.from_datastruct(ds)


def sites(nq):
    """nq lattice positions inside the data volume, at least 3 apart."""
    i = np.arange(nq)
    return 20.0 + 10.0 * (i % 12), -100.0 + 7.0 * (i // 12), 5.0 + 3.0 * (i % 5)


def special(rng, M):
    return rng.choice(SPECIAL, M)


def with_nan(where):
    def col(rng, M):
        v = special(rng, M)
        v[{"first": 0, "last": M - 1, "middle": M // 2}[where]] = np.nan
        return v

    return col


def denormals(rng, M):
    v = rng.integers(1, 1 << 52, M).astype(np.uint64).view(np.float64)
    return np.where(rng.integers(0, 2, M) == 1, -v, v)


# the columns of a designed matrix, repeated cyclically over the nodes: (rng, M) -> [M]
COLUMNS = (
    lambda rng, M: np.full(M, -np.inf),
    lambda rng, M: np.full(M, -0.0),
    lambda rng, M: np.full(M, 0.0),
    lambda rng, M: np.full(M, np.inf),
    lambda rng, M: np.full(M, -DBL_MAX),
    lambda rng, M: np.where(np.arange(M) % 2 == 0, -0.0, 0.0),  # half -0.0, half 0.0, alternating rows
    lambda rng, M: rng.choice([-3.5, 2.25], M),  # two values of opposite sign
    lambda rng, M: rng.choice([-np.inf, 17.0, np.inf], M),  # -inf / finite / +inf in thirds
    lambda rng, M: -np.abs(rng.choice(SPECIAL[1:], M)),  # only negatives (and -0.0)
    denormals,  # only denormals, of both signs
    special,  # a uniform draw from SPECIAL
    lambda rng, M: rng.standard_normal(M) * 10.0 ** rng.integers(-300, 300, M),  # every key byte varies
    lambda rng, M: (M / 2.0 - np.arange(M)) * 1.5,  # strictly descending in row order
    lambda rng, M: (np.arange(M) - M / 2.0) * 1.5,  # strictly ascending
    with_nan("first"), with_nan("last"), with_nan("middle"),
)
NAN_COLUMNS = 3


def designed(M, nq=NQ, seed=0):
    rng = np.random.default_rng([seed, M])
    V = np.stack([COLUMNS[c % len(COLUMNS)](rng, M) for c in range(nq)], axis=1)
    assert V.shape == (M, nq)
    nan_cols = np.isnan(V).any(axis=0)
    assert nan_cols.sum() == sum(c % len(COLUMNS) >= len(COLUMNS) - NAN_COLUMNS for c in range(nq))
    assert 4 * nan_cols.sum() <= nq  # at least three quarters of the columns compare numbers, not NaN == NaN
    return V


def rasterized(ctx, V):
    """The designed matrix through the device: (models, nodes, the V td_rasterize returns == the design)."""
    q = sites(V.shape[1])
    models = mref.designed_models(V, q)
    got = ctx.rasterize(models, *q, want_values=True)[2]
    assert mref.same_bits(got, V)
    return models, q, got


def check_quantiles(r, V, probs):
    want = mref.ref_quantiles(V, probs)
    assert r["quantiles"].shape == want.shape
    bad = ~((np.isnan(want) & np.isnan(r["quantiles"])) | (want.view(np.uint64) == r["quantiles"].view(np.uint64)))
    assert not bad.any(), ("(probability, node):", np.argwhere(bad)[:8].tolist(), r["quantiles"][bad][:8], want[bad][:8])
    assert mref.same_bits(r["quantiles"], want)


def check_hist(r, V, bins):
    want = mref.ref_hist(V, bins)
    assert r["hist"].shape == want.shape and r["hist"].dtype == np.int64
    assert np.array_equal(r["hist"], want), np.argwhere(r["hist"] != want)[:8].tolist()
    assert np.all(r["hist"].sum(axis=1) == len(V))


def both_regimes(tt, ctx, run):
    """run() under the resident and under the streaming regime -> its two results; the method is restored."""
    got = []
    try:
        for method in (tt.TdContext.MARG_RESIDENT, tt.TdContext.MARG_STREAMING):
            ctx.set_marginals_method(method)
            got.append(run())
    finally:
        ctx.set_marginals_method(tt.TdContext.MARG_AUTO)
    return got


BINS_A = ((8, -4.0, 4.0), (5, -1e300, 1e300))


@pytest.mark.parametrize("M", [1, 2, 3, 64, 65, 511, 512, 513, 1025])
def test_whole_double_range_in_both_regimes(tt, ctx, M):
    """Column lengths around the bitonic network's powers of two and the radix select's 512-thread stride."""
    models, q, V = rasterized(ctx, designed(M))
    probs = PROBS + ((1 / (M - 1),) if M > 1 else ()) + (1 - 1e-16,)

    def run():
        r = ctx.marginals(models, *q, probs, BINS_A[0])
        check_quantiles(r, V, probs)
        check_hist(r, V, BINS_A[0])
        r2 = ctx.marginals(models, *q, bins=BINS_A[1])
        assert r2["quantiles"] is None
        check_hist(r2, V, BINS_A[1])
        return r["quantiles"], r["hist"], r2["hist"]

    a, b = both_regimes(tt, ctx, run)
    assert mref.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # the design reaches what it is for: infinities of both signs, zeros and NaN among the quantiles
    want = mref.ref_quantiles(V, probs)
    assert (want == 0).any() and np.isnan(want[:, ~np.isnan(V).any(axis=0)]).any()  # (inf - inf: equal infinities)
    if M >= 64:
        # (an infinite a or b mostly gives NaN: -inf + g * inf, inf - inf, 0 * inf)
        assert (want < -1e300).any() and ((want != 0) & (np.abs(want) < 1e-300)).any()


def tile_shapes(num_cus):
    """(models, nodes, the tile width the plan must give them under MARG_AUTO); 51 nodes, not 50, at W = 2: the
    last tile is to be partial."""
    return ((9000, 20, 1), (5000, 51, 2), (3000, 50, 4), (1000, 130, 8), (1000, 16 * 2 * num_cus + 3, 16),
            (400, 32 * 2 * num_cus + 5, 32), (200, 64 * 2 * num_cus + 37, 64))


def test_tile_shapes_cover_every_width(tt, ctx):
    assert ctx.num_cus >= 9  # (ceil(130 / 16) = 9 tiles must be fewer than two per CU for W = 8)
    widths = set()
    for M, nq, W in tile_shapes(ctx.num_cus):
        resident, Mp, w, threads, lds = tt.TdContext.marginals_plan(M, nq, ctx.num_cus, tt.TdContext.MARG_AUTO, len(PROBS))
        print("marginals_plan: M = %d, nq = %d, %d CUs -> Mp = %d, W = %d, %d threads, %d bytes of LDS"
              % (M, nq, ctx.num_cus, Mp, w, threads, lds))
        assert resident and w == W and Mp * w <= ctx.marginals_resident_max()
        assert W == 1 or nq % W != 0  # a partial last tile (a tile of one node cannot be partial)
        assert nq > W  # more than one workgroup
        widths.add(w)
    assert widths == {1, 2, 4, 8, 16, 32, 64}


@pytest.mark.parametrize("W", [1, 2, 4, 8, 16, 32, 64])
def test_every_tile_width(tt, ctx, W):
    """6-cell models with zeta from SPECIAL at the shape whose plan is a tile of W nodes; a NaN cell in two models
    (has_nan[c] at every W).  The shapes of W = 16 and W = 64 also go through the volume route, one slab."""
    M, nq, _ = next(s for s in tile_shapes(ctx.num_cus) if s[2] == W)
    assert tt.TdContext.marginals_plan(M, nq, ctx.num_cus, tt.TdContext.MARG_AUTO, len(PROBS))[:3:2] == (True, W)
    rng = np.random.default_rng(W)
    pos = rng.uniform([0, -200, 0], [1000, 400, 600], (M, 6, 3))
    zeta = rng.choice(SPECIAL, (M, 6))
    qx, qy, qz = rng.uniform(0, 1000, nq), rng.uniform(-200, 400, nq), rng.uniform(0, 600, nq)
    # the NaN cells lie beyond opposite corners of the box, each under a node of its own: they own those
    # nodes and few others
    for k, c, node, corner in ((M // 3, 2, 0, (-300.0, -500.0, -300.0)), (M - 1, 5, nq - 1, (1300.0, 700.0, 900.0))):
        pos[k, c] = corner
        zeta[k, c] = np.nan
        qx[node], qy[node], qz[node] = corner
    models = [(pos[k, :, 0], pos[k, :, 1], pos[k, :, 2], zeta[k]) for k in range(M)]
    V = ctx.rasterize(models, qx, qy, qz, want_values=True)[2]
    nan_cols = np.isnan(V).any(axis=0)
    assert V.shape == (M, nq) and nan_cols[0] and nan_cols[-1] and 4 * nan_cols.sum() <= nq
    want_q, want_h = mref.ref_quantiles(V, PROBS), mref.ref_hist(V, BINS_A[0])
    routes = [ctx.marginals] + ([ctx.volume] if W in (16, 64) else [])
    if len(routes) == 2:
        assert tt.TdContext.volume_plan(M, nq)[1] == 1  # one slab: the same M x nq matrix
    for route in routes:
        r = route(models, qx, qy, qz, PROBS, BINS_A[0])
        assert mref.same_bits(r["quantiles"], want_q), route.__name__
        assert np.isnan(r["quantiles"][:, nan_cols]).all() and not np.isnan(r["quantiles"][:, ~nan_cols]).all()
        assert np.array_equal(r["hist"], want_h) and r["hist"].dtype == np.int64, route.__name__


def probabilities(nprob, rng):
    """Unsorted, with 0, 1 and 0.5 three times as far as nprob goes, the rest random."""
    p = np.array(([0.5, 0.0, 1.0, 0.5, 0.5] + list(rng.uniform(0, 1, 64)))[:nprob])
    p = p[rng.permutation(nprob)]
    if nprob >= 5:
        p[[0, 1, nprob - 1]] = np.sort(p[[0, 1, nprob - 1]])[::-1]  # (descending somewhere, whatever the shuffle)
        assert (p == 0.5).sum() == 3 and (p == 0.0).sum() == 1 and (p == 1.0).sum() == 1
        assert np.any(np.diff(p) < 0) and np.any(np.diff(p) > 0)
    return p


@pytest.mark.parametrize("nprob", [1, 23, 24, 64])
@pytest.mark.parametrize("M", [2, 300])
def test_up_to_64_probabilities(tt, ctx, M, nprob):
    """From 24 probabilities on the radix select's digit histograms pass 48 KiB (the LDS opt-in), at 64 they are
    128 KiB and 128 selections run at once; rem[tid] for tid >= nprob are the b order statistics."""
    assert tt.TdContext.marginals_plan(M, NQ, ctx.num_cus, tt.TdContext.MARG_STREAMING, nprob)[4] == nprob * 2048
    models, q, V = rasterized(ctx, designed(M, seed=1))
    p = probabilities(nprob, np.random.default_rng([nprob, M]))
    want = mref.ref_quantiles(V, p)
    one = {float(x): mref.ref_quantiles(V, (float(x),))[0] for x in set(p.tolist())}

    def run():
        r = ctx.marginals(models, *q, p)
        check_quantiles(r, V, p)
        for i, x in enumerate(p.tolist()):  # every row is its probability's, wherever it stands in the list
            assert mref.same_bits(r["quantiles"][i], one[x]), (i, x)
        return r["quantiles"]

    a, b = both_regimes(tt, ctx, run)
    assert mref.same_bits(a, b) and mref.same_bits(a, want)
    if nprob >= 5:
        i = np.flatnonzero(p == 0.5)
        assert len(i) == 3 and mref.same_bits(a[i[0]], a[i[1]]) and mref.same_bits(a[i[0]], a[i[2]])


def test_bins_at_the_edge_of_the_range(tt, ctx):
    """16 models; node q < 16 holds SPECIAL[q] in every model (its row of the histogram is one slot), the other
    nodes hold all of SPECIAL in rotation."""
    n = len(SPECIAL)
    assert n == 16 and SPECIAL[0] == -np.inf and SPECIAL[1] == -DBL_MAX and SPECIAL[-2] == DBL_MAX and SPECIAL[-1] == np.inf
    S = np.array(SPECIAL)
    V = np.empty((n, NQ))
    for c in range(NQ):
        V[:, c] = S[c] if c < n else np.roll(S, c)
    models, q, V = rasterized(ctx, V)
    for bins in ((4, -1e300, 1e300), (4096, -1.0, 1.0)):
        nbins = bins[0]
        slots = mref.ref_slots(S, bins)
        # beyond the range on either side: the infinities and +-DBL_MAX (|v| > 1e300 >= 1)
        assert slots[0] == slots[1] == 0 and slots[-2] == slots[-1] == nbins + 1

        def run():
            r = ctx.marginals(models, *q, (0.5,), bins)
            check_hist(r, V, bins)
            check_quantiles(r, V, (0.5,))
            h = r["hist"]
            for c in range(n):  # the slots themselves
                assert h[c, slots[c]] == n and h[c].sum() == n, (bins, SPECIAL[c])
            for c in (0, 1):
                assert h[c, 0] == n
            for c in (n - 2, n - 1):
                assert h[c, nbins + 1] == n
            assert np.all(h[n:] == np.bincount(slots, minlength=nbins + 3)) and np.all(h[:, nbins + 2] == 0)
            return h

        a, b = both_regimes(tt, ctx, run)
        assert np.array_equal(a, b)
    # (4, -1e300, 1e300): w = 5e299; lo itself opens bin 0, zero opens bin 2, hi itself is beyond
    slots = mref.ref_slots(S, (4, -1e300, 1e300)).tolist()
    assert slots == [0, 0, 1, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 5, 5, 5]
    # (4096, -1, 1): w = 2^-11; -1.0 opens bin 0, every value below 2^-53 in size is at 1.0 / w = 2048
    slots = mref.ref_slots(S, (4096, -1.0, 1.0)).tolist()
    assert slots == [0, 0, 0, 1] + [2049] * 7 + [4097] * 5
    # hi - lo overflows: w would be +inf and (v - lo) / w NaN for the largest v
    for bins in ((3, -1e308, 1e308), (1, -DBL_MAX, DBL_MAX)):
        with pytest.raises(tt.TdError, match="need finite lo < hi"):
            ctx.marginals(models, *q, (0.5,), bins)
        with pytest.raises(tt.TdError, match="need finite lo < hi"):
            ctx.marginals(models, *q, bins=bins)
    check_hist(ctx.marginals(models, *q, bins=(3, -8e307, 8e307)), V, (3, -8e307, 8e307))  # the widest that passes
