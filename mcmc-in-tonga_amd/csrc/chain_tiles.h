// chain_tiles.h -- the chain's tile pass (phase B): marking a changed point, and the FP32 filters that
// decide which 16-point tiles a proposal can reach (tile_may_hit, tile_may_hit2; the tests hold them to
// "never drops a tile in reach", tests/test_gpu_tile_filter.py).
#pragma once
#include <hip/hip_runtime.h>

#include "chain_shared.h"

namespace tdstar {

namespace {

__device__ __forceinline__ void mark(const DevChain &d, const Views &v, Shared &sh, int p, int r, int s, double dd,
                                     double z, int o) {
    d.cand_s[p] = s;
    d.cand_d[p] = dd;
    d.cand_z[p] = z;
    d.cand_flag[p] = 1;
    const int c = atomicAdd(&sh.n_changed, 1);
    d.changed[c] = p;
    if (c < kChgLds) sh.chg[c] = ChgRec{p, s, dd, z, o};
    if (atomicExch(&v.rflag[r], 1) == 0) {
        v.ray_put(atomicAdd(&sh.n_rays, 1), r);
        atomicMin(&sh.k0, r);
    }
}

// Tile test in FP32: can some point p of tile t have dist2(q, p) <= thr?
// Every rounding is taken against the answer (the query rounded to FP32 moves
// by <= |q| 2^-24, each FP32 operation errs by <= 2^-24 relative), so the test
// never says "no" for a tile that holds such a point; it may say "yes" for a
// tile that does not (its points are then checked exactly in FP64).
struct TileQuery {
    float x, y, z, ex, ey, ez;  // coordinates and their rounding allowance
};
__device__ __forceinline__ TileQuery tile_query(double x, double y, double z) {
    TileQuery q;
    q.x = (float)x;
    q.y = (float)y;
    q.z = (float)z;
    q.ex = fabsf(q.x) * 0x1p-23f;
    q.ey = fabsf(q.y) * 0x1p-23f;
    q.ez = fabsf(q.z) * 0x1p-23f;
    return q;
}
__device__ __forceinline__ float gap_lb(float q, float e, float l, float h) {
    const float g = fmaxf(fmaxf(l - q, q - h), 0.0f);
    return fmaxf(g * (1.0f - 0x1p-20f) - e, 0.0f);
}
// thr: an FP32 bound >= the FP64 threshold (tile_thr)
__device__ __forceinline__ bool tile_may_hit(const float *lo, const float *hi, int nt, int t, const TileQuery &q,
                                             float thr) {
    const float gx = gap_lb(q.x, q.ex, lo[t], hi[t]);
    const float gy = gap_lb(q.y, q.ey, lo[nt + t], hi[nt + t]);
    const float gz = gap_lb(q.z, q.ez, lo[2 * nt + t], hi[2 * nt + t]);
    float s = gx * gx;
    s = s + gy * gy;
    s = s + gz * gz;
    return s * (1.0f - 0x1p-20f) <= thr;
}
__device__ __forceinline__ float tile_thr(double mx) { return (float)mx * (1.0f + 0x1p-20f); }

// The same filter in about half the VALU operations (phase B's tile pass, LDS layout; TD_TILE2): the
// query's rounding folded into two per-query bounds per axis, one max3 per axis, the squares summed with
// FMAs.  Never says "no" for a tile holding a point p with dist2(q, p) <= mx (FP64), thr = tile_thr(mx):
// with E = max_a |(float)q_a| 2^-23 >= |q_a - (float)q_a| on every axis, up = fl((float)q + 2E) >= q and
// dn = fl((float)q - 2E) <= q (the rounding of the add is at most E/2); for p in the outward-rounded box,
// |p_a - q_a| >= max(lo - up, dn - hi, 0) >= g_a (1 - 2^-24) with g_a the rounded max3; the FMA sum s
// errs by at most 3 ulps, so the real sum of the squared gaps -- a lower bound of the exact squared
// distance, itself within 2^-50 of the FP64 one -- is >= s (1 - 2^-21); and thr >= mx (1 - 2^-24)^2
// (1 + 2^-20), so s > thr implies dist2(q, p) > mx for every point of the tile.
#ifndef TD_TILE2
#define TD_TILE2 1
#endif
struct TileQuery2 {
    float ux, uy, uz, dx, dy, dz;  // the query's upper and lower bounds per axis
};
__device__ __forceinline__ TileQuery2 tile_query2(double x, double y, double z) {
    const float fx = (float)x, fy = (float)y, fz = (float)z;
    const float e2 = fmaxf(fmaxf(fabsf(fx), fabsf(fy)), fabsf(fz)) * 0x1p-22f;  // 2E
    return TileQuery2{fx + e2, fy + e2, fz + e2, fx - e2, fy - e2, fz - e2};
}
struct TileBox {
    float lx, ly, lz, hx, hy, hz, thr;
};
__device__ __forceinline__ TileBox tile_box(const float *lo, const float *hi, const double *maxd, int nt, int t) {
    return TileBox{lo[t], lo[nt + t], lo[2 * nt + t], hi[t], hi[nt + t], hi[2 * nt + t], tile_thr(maxd[t])};
}
__device__ __forceinline__ bool tile_may_hit2(const TileBox &b, const TileQuery2 &q) {
    const float gx = fmaxf(fmaxf(b.lx - q.ux, q.dx - b.hx), 0.0f);
    const float gy = fmaxf(fmaxf(b.ly - q.uy, q.dy - b.hy), 0.0f);
    const float gz = fmaxf(fmaxf(b.lz - q.uz, q.dz - b.hz), 0.0f);
    float s = gx * gx;
    s = __builtin_fmaf(gy, gy, s);
    s = __builtin_fmaf(gz, gz, s);
    return s <= b.thr;
}
// x rounded up to FP32 (x >= 0; the super-tile maxima)
__device__ __forceinline__ float f32_up(double x) {
    const float f = (float)x;
    return (double)f < x ? __int_as_float(__float_as_int(f) + 1) : f;  // f >= 0 finite: the next float up
}

}  // namespace

}  // namespace tdstar
