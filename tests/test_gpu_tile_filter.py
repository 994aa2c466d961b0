"""The chain's phase-B tile filter (chain_tiles.h tile_may_hit / tile_may_hit2, FP32) must never drop
a tile that holds a point within the tile's cached maximum distance: in FP64, dist2(q, p) <= maxd for some
point p of the tile => the tile passes.  Otherwise a proposal could miss a point whose nearest cell it
changes (MCsub.jl:247-263 through the chain's incremental search).  Checked on tiles of 16 real ray points
each (boxes rounded outward to FP32), queries on, near and far from them, and maxima set EXACTLY to a
query's FP64 minimum distance -- the boundary case -- for both filter forms."""
import numpy as np
import pytest

from tile_filter_ref import boundary_case, dist2, filter_hits, outward_box, tile_boxes  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", [0, 1])
def test_tile_filter_never_drops_a_tile_in_reach(tt, ds, mode):
    rng = np.random.default_rng(17 + mode)
    X, Y, Z = (np.asarray(a, dtype=np.float64).T.ravel() for a in (ds.rayX, ds.rayY, ds.rayZ))
    ok = ~np.isnan(X)
    nt, nq = 400, 300
    pts, qs, md, owner, maxd = boundary_case(rng, np.stack([X[ok], Y[ok], Z[ok]], 1), nt=nt, nq=nq)
    lo, hi = tile_boxes(pts)
    hit = filter_hits(tt, lo, hi, maxd, qs, mode)
    must = md <= maxd[None, :]
    missed = np.argwhere(must & ~hit)
    assert missed.size == 0, (missed[:5], [(md[q, t], maxd[t]) for q, t in missed[:5]])
    exact = np.setdiff1d(np.arange(nt), np.arange(0, nt, 7))
    assert must[owner[exact], exact].all()  # (the boundary pairs, maximum == the distance, are in the set)
    assert hit.mean() < 0.6  # (and it does prune)
