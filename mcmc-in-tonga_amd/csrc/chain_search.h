// chain_search.h -- a chain's nearest-cell search (one wave per query): the exact scan of every slot,
// the search through the bucket grid's LDS copy, the two together (wave_nearest), and the grid's
// update for an accepted proposal (grid_prefetch / grid_apply).  The search that reads the grid's
// descriptor (DevChain) instead is the comparison form in chain_test_kernels.hip, kept for the tests:
// test_grid_query_forms_agree (no edit) and test_gpu_nearest_edits.py (a killed and a moved cell; the grid
// against the cell arrays after every kind of update) hold the two searches together and to an exact scan;
// test_gpu_nearest_scan.py holds wave_full_scan to built slot layouts, test_gpu_wave_ops.py the reductions
// under all of them.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "chain_shared.h"
#include "wave_ops.h"

namespace tdstar {

namespace {

// Exact nearest live cell by scanning every slot, ONE wave: lexicographic
// (distance, Julia position), which is what v_nearest's first-index rule
// gives (MCsub.jl:250-258) -- positions compared through the slots' stamps,
// which are in Julia order (chain_dev.h).  Fallback of the grid search (rare:
// out of line).
__device__ __attribute__((noinline)) Nearest wave_full_scan(const long long *__restrict__ stamp,
                                                           const double *__restrict__ cx,
                                                           const double *__restrict__ cy,
                                                           const double *__restrict__ cz,
                                                           const double *__restrict__ czeta, int cap, int nslots,
                                                           int lane, double x, double y, double z, int skip,
                                                           int moved, double mx, double my, double mz) {
    double bd = kSentinel;
    long long br = LLONG_MAX;
    int bs = -1;
    constexpr int kScanUnroll = 8;  // all loads of a round issued before any use
    for (int s0 = lane; s0 < nslots; s0 += kScanUnroll * 64) {
        long long r[kScanUnroll];
        double px[kScanUnroll], py[kScanUnroll], pz[kScanUnroll];
#pragma unroll
        for (int u = 0; u < kScanUnroll; ++u) {
            // unconditional loads from a clamped slot, masked afterwards
            const int s = min(s0 + u * 64, cap - 1);
            r[u] = stamp[s];
            px[u] = cx[s];
            py[u] = cy[s];
            pz[u] = cz[s];
        }
#pragma unroll
        for (int u = 0; u < kScanUnroll; ++u) {
            const int s = s0 + u * 64;
            if (s >= nslots || r[u] < 0 || s == skip) continue;  // free slot / killed cell
            if (s == moved) {
                px[u] = mx;
                py[u] = my;
                pz[u] = mz;
            }
            const double dd = dist2(px[u], py[u], pz[u], x, y, z);
            if (better(dd, r[u], bd, br)) {
                bd = dd;
                br = r[u];
                bs = s;
            }
        }
    }
    // lexicographic min: the distance first, then the position among equals
    const unsigned long long kd = wave_min_u64((unsigned long long)__double_as_longlong(bd));
    const bool at_min = (unsigned long long)__double_as_longlong(bd) == kd;
    const unsigned long long kr = wave_min_u64(at_min ? (unsigned long long)br : ~0ull);
    Nearest res;
    res.d = __longlong_as_double((long long)kd);
    res.proven = true;
    if (res.d < kSentinel && kr != ~0ull) {  // (stamps are unique: one lane holds the winner)
        const unsigned long long who = __ballot(at_min && (unsigned long long)br == kr);
        res.s = __builtin_amdgcn_readlane(bs, __builtin_ctzll(who));
        res.z = czeta[res.s];
    } else {
        res.s = -1;
        res.z = 0.0;
    }
    return res;
}

// Nearest live cell through the bucket grid, ONE wave, no block barrier.
// Lanes 0..53 cover the 3x3x3 buckets around the query, 8 entries per bucket
// (entries hold the cell coordinates inline: ONE round of loads).  The answer
// is proven when its distance is strictly below the squared distance to the
// outer faces of the block (every cell outside lies beyond a face), no other
// entry ties it and no bucket holds more than 8 entries.  `skip` = the killed
// slot; slot `moved` is taken at (mx,my,mz) instead of its stored site.
// On the LDS copy of the grid: the same loads, the same answer and the same proof as the
// descriptor-reading comparison form (chain_test_kernels.hip; test_grid_query_forms_agree holds the two
// together) -- grid_block_lb's bound, R = 1, each face taken by a select instead of a branch
__device__ __forceinline__ Nearest wave_grid_search(const GridGeo &gl, bool ovf, int lane, double x, double y,
                                                    double z, int skip, int moved, double mx, double my, double mz,
                                                    double mzeta) {
    const GridGeo G = gl;  // (one round of LDS loads, every lane the same words)
    const int bi = grid_axis(x, G.x0, G.ix, G.gx), bj = grid_axis(y, G.y0, G.iy, G.gy),
              bk = grid_axis(z, G.z0, G.iz, G.gz);
    const int nb = lane % 27, grp = lane / 27;
    const int ii = bi + nb % 3 - 1, jj = bj + (nb / 3) % 3 - 1, kk = bk + nb / 9 - 1;
    const bool inb = lane < 54 && ii >= 0 && ii < G.gx && jj >= 0 && jj < G.gy && kk >= 0 && kk < G.gz;
    const int b = inb ? (kk * G.gy + jj) * G.gx + ii : 0;
    const int cnt = gload(G.count + b);
    CellEntry e[4];
    int sl[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const CellEntry *ep = G.buckets + b * kBucketCap + grp * 4 + u;
        e[u].x = gload(&ep->x);
        e[u].y = gload(&ep->y);
        e[u].z = gload(&ep->z);
        e[u].zeta = gload(&ep->zeta);
        sl[u] = gload(G.bslot + b * kBucketCap + grp * 4 + u);
    }
    double bd = kSentinel, bz = 0.0;
    int bs = -1;
    bool tie = false;
    const bool overfull = inb && cnt > 8;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const bool ok = inb && grp * 4 + u < cnt && sl[u] != skip && sl[u] != moved;
        const double dd = dist2(e[u].x, e[u].y, e[u].z, x, y, z);
        if (ok) {
            if (dd < bd) {
                bd = dd;
                bs = sl[u];
                bz = e[u].zeta;
                tie = false;
            } else if (dd == bd && dd < kSentinel) {
                tie = true;
            }
        }
    }
    if (lane == 63 && moved >= 0) {  // the moved cell, at its proposed site
        const double dd = dist2(mx, my, mz, x, y, z);
        if (dd < bd) {
            bd = dd;
            bs = moved;
            bz = mzeta;
            tie = false;
        } else if (dd == bd && dd < kSentinel) {
            tie = true;
        }
    }
    const unsigned long long key = (unsigned long long)__double_as_longlong(bd);
    const unsigned long long kmin = wave_min_u64_2p(key);
    const unsigned long long who = __ballot(key == kmin);
    const int win = __builtin_ctzll(who);
    Nearest res;
    res.d = __longlong_as_double((long long)kmin);
    const bool found = res.d < kSentinel;
    const bool tied = found && (__popcll(who) > 1 || __builtin_amdgcn_readlane((int)tie, win) != 0);
    const bool any_over = __ballot(overfull) != 0ull;
    res.s = found ? __builtin_amdgcn_readlane(bs, win) : -1;
    res.z = found ? readlane_f64(bz, win) : 0.0;
    res.proven = !ovf && !tied && !any_over && res.d < G.lb0;
    if (!res.proven && !ovf && !tied && !any_over) {  // (wave-uniform; rare) the query's own block bound
        double lb;
        {
            const double v[3] = {x, y, z}, e3[3] = {G.ex, G.ey, G.ez};
            double o2[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {  // grid_out2
                const double below = G.lo[a] - v[a], above = v[a] - G.hi[a];
                const double o = (below > above ? below : above) - e3[a];
                o2[a] = (G.sealed && o > 0.0) ? o * o : 0.0;
            }
            lb = __builtin_huge_val();
            auto face = [&lb](double w, double w0, double h, double e1, int g, int i, double other) {
                const double gl0 = (w - (w0 + (double)(i - 1) * h)) - e1;
                const double gh0 = ((w0 + (double)(i + 2) * h) - w) - e1;
                const double fl = (gl0 > 0.0 ? gl0 * gl0 : 0.0) + other;
                const double fh = (gh0 > 0.0 ? gh0 * gh0 : 0.0) + other;
                lb = (i - 1 > 0 && fl < lb) ? fl : lb;
                lb = (i + 1 < g - 1 && fh < lb) ? fh : lb;
            };
            face(x, G.x0, G.hx, G.ex, G.gx, bi, o2[1] + o2[2]);
            face(y, G.y0, G.hy, G.ey, G.gy, bj, o2[0] + o2[2]);
            face(z, G.z0, G.hz, G.ez, G.gz, bk, o2[0] + o2[1]);
            lb = grid_lb_close(lb);
        }
        res.proven = res.d < lb;
    }
    return res;
}

// Nearest live cell for one query, one wave: grid first, full scan if unproven.
__device__ __forceinline__ Nearest wave_nearest(const DevChain &d, const Views &v, Shared &sh, int lane, double x,
                                                double y, double z, int skip, int moved, double mx, double my,
                                                double mz, double mzeta) {
    Nearest r = wave_grid_search(sh.geo, sh.grid_ovf != 0, lane, x, y, z, skip, moved, mx, my, mz, mzeta);
    if (!r.proven) {
        if (lane == 0) atomicAdd(&sh.grid_fallbacks32, 1);
        r = wave_full_scan(d.stamp, d.cx, d.cy, d.cz, d.czeta, d.cap, sh.nslots, lane, x, y, z, skip, moved,
                           mx, my, mz);
    }
    return r;
}

// Read what the bucket-grid update of an accepted proposal will need (one
// wave, during phase F, before the decision): the old site's bucket, count,
// the slot's position in it and its last entry; the new site's bucket and count.
__device__ void grid_prefetch(const DevChain &d, Shared &sh, int lane, int action, int slot, double ox, double oy,
                              double oz, double nx, double ny, double nz) {
    const bool rm = action == tdchain::kDeath || action == tdchain::kMove;
    const bool ins = action == tdchain::kBirth || action == tdchain::kMove;
    const bool upd = action == tdchain::kChange;  // the entry's value, in place
    int bo = 0, co = 0, pos = -1, bn = 0, cn = 0;
    if (rm || upd) {
        bo = grid_bucket(d.grid, ox, oy, oz);
        co = d.bucket_count[bo];
        const int s = lane < kBucketCap ? d.bslot[bo * kBucketCap + lane] : -1;
        const unsigned long long m = __ballot(lane < co && s == slot);
        pos = m ? __builtin_ctzll(m) : -1;
        if (rm && lane == 0 && co > 0) {
            sh.gp_last = d.buckets[bo * kBucketCap + co - 1];
            sh.gp_last_slot = d.bslot[bo * kBucketCap + co - 1];
        }
    }
    if (ins) {
        bn = grid_bucket(d.grid, nx, ny, nz);
        cn = d.bucket_count[bn];
    }
    if (lane == 0) {
        sh.gp_bo = bo;
        sh.gp_co = co;
        sh.gp_pos = pos;
        sh.gp_bn = bn;
        sh.gp_cn = cn;
    }
}

// Apply the accepted proposal's bucket-grid update from the prefetched data
// (lane 0 of one wave; stores only).
__device__ void grid_apply(const DevChain &d, Shared &sh) {
    const int op = sh.g_op;
    int co = sh.gp_co;
    if (op & 1) {  // remove g_slot: the bucket's last entry takes its place
        const int b = sh.gp_bo, pos = sh.gp_pos;
        if (pos < 0) {
            *d.grid_overflow = 1;  // bookkeeping lost track: stop trusting the grid
            sh.grid_ovf = 1;
        } else {
            d.buckets[b * kBucketCap + pos] = sh.gp_last;
            d.bslot[b * kBucketCap + pos] = sh.gp_last_slot;
            d.bucket_count[b] = co - 1;
            co -= 1;
        }
    }
    if (op & 4) {  // a change: the entry's value
        const int pos = sh.gp_pos;
        if (pos < 0) {
            *d.grid_overflow = 1;
            sh.grid_ovf = 1;
        } else {
            d.buckets[sh.gp_bo * kBucketCap + pos].zeta = sh.g_nzeta;
        }
    }
    if (op & 2) {  // insert at the new site
        const int b = sh.gp_bn;
        const int cnt = ((op & 1) && b == sh.gp_bo) ? co : sh.gp_cn;  // a move inside one bucket
        if (cnt < kBucketCap) {
            d.buckets[b * kBucketCap + cnt] = CellEntry{sh.g_nx, sh.g_ny, sh.g_nz, sh.g_nzeta};
            d.bslot[b * kBucketCap + cnt] = sh.g_slot;
            d.bucket_count[b] = cnt + 1;
        } else {
            *d.grid_overflow = 1;
            sh.grid_ovf = 1;
        }
    }
}

}  // namespace

}  // namespace tdstar
