// resolution.hip -- posterior resolution: for every node of a lattice, the covariance and the correlation of zeta
// there with zeta at each neighbour inside a window of lattice offsets, and what they reduce to -- the volume tied
// to the node, the contiguous reach along each axis, and where the lattice or the window cut it off
// (include/tdstar_resolution.h holds the contract, resolution.h the host arithmetic).
//
// The search structure is the volume's (volume_build).  Every partner n + f(o) lies ahead of its owner n in flat
// order, within `reach`, so the nodes are swept ONCE, in blocks of ns consecutive flat nodes, of which R =
// ceil(reach / ns) + 1 are resident (res_plan): block b is a dense V[M][ns] of its own in slot b mod R (the last
// block is filled up with its last node), k_raster_stats gives its columns' mean and sigma into arrays over all
// nodes, and k_res_center subtracts the mean in place -- the one subtraction of each factor, made once per value
// and not once per pair.  When the blocks up to b + R - 1 stand, block b's pairs are formed:
//   k_res_pairs     the plain form.  Work item = (64 owned columns, leaf of the sum's pairwise tree, group of G
//                   offsets), one wave, one lane per node.  A row of the owned tile is one coalesced 512-byte load, a
//                   partner's row one more at a fixed column distance (found as block c' / ns, slot block mod R,
//                   column c' mod ns: a tile's partners may lie in two slots); kResAhead rows are in flight per lane,
//                   G running sums per lane in registers, left to right over the leaf's models.  A pair off the
//                   lattice reads the owned column again and its sum is not used.
//   k_res_xruns     the x-run form.  Offsets that share (dj, dk) and differ by one in di have their partners in one
//                   contiguous segment of 64 + cnt - 1 columns (res_xruns: runs of at most 12).  Work item = (64
//                   owned columns, leaf, run): the segment of a row is loaded once, staged in LDS (kResAhead rows
//                   at a time, the next rows' loads in flight meanwhile) and every offset of the run reads its
//                   partner at lane + g -- one conflict-free 8-byte LDS read per product in the place of a global
//                   load.  Same products, same order, same bits.  Runs of up to kResShortRun offsets take the plain
//                   form (tdt_set_resolution forces one form for all; DESIGN 4.6m holds the measurements).
//   k_res_combine   one lane per (node, offset): the leaves' sums are added in the tree's order (k_iface_combine's
//                   walk, the waiting left halves in LDS), cov = S / (M - 1), corr = cov / (s_n s_{n + f}), NaN off
//                   the lattice, into the rows C[noff][nq] that stay on the device for the whole call.
//   k_res_summary   one lane per node, after the last block: footprint, run and censored from C in the order of
//                   the definition (a neighbour's row is read at n - f: both directions come from forward pairs).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tdstar_resolution.h"
#include "covariance.h"
#include "ctx.h"
#include "ensemble.h"
#include "history.h"
#include "resolution.h"
#include "volume.h"

namespace tdstar {

namespace {

constexpr int kResThreads = 64;  // one wave: a tile of the block
constexpr int kResGroup = 8;     // G: offsets whose sums a lane keeps in registers
constexpr int kResAhead = 4;     // rows a lane keeps in flight (1 + G loads each)
constexpr int64_t kResMaxModels = (int64_t)1 << 25;  // covariance's: cov_levels(M) <= 15, 2^15 leaves are one grid.y
constexpr int64_t kResMaxRowBytes = (int64_t)1 << 30;  // cov or corr [noff][nq]
constexpr int64_t kResLeafBytes = (int64_t)256 << 20;  // the leaf sums of one chunk of offsets

// What tdt_set_resolution asked for, kept beside the context in this unit: a field of td_ctx would change the layout
// every other unit is compiled against.
struct ResSetting {
    int64_t budget = 0;  // 0: kResDefaultBudget
    int form = 0;        // 0: the kept one (runs of up to kResShortRun offsets plain, longer ones as x-runs), 1: plain, 2: x-runs
};
constexpr int kResShortRun = 1;  // a lone offset gains nothing from a staged segment; eight of them share a load of the owned rows
std::mutex g_setting_lock;
std::unordered_map<const td_ctx *, ResSetting> g_setting;  // contexts whose setting is not the default

ResSetting res_setting(const td_ctx *ctx) {
    std::lock_guard<std::mutex> hold(g_setting_lock);
    const auto it = g_setting.find(ctx);
    return it == g_setting.end() ? ResSetting{} : it->second;
}

struct ResLattice {
    int nx, ny, nz;
    long nq;
};

// q = [3][ns]: the coordinates of the flat nodes q0 .. q0 + ns, the last node again past the lattice's end
__global__ __launch_bounds__(256) void k_res_nodes(const double *__restrict__ xyz, ResLattice L, long q0, int ns,
                                                   double *__restrict__ q) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ns) return;
    const long n = min(q0 + c, L.nq - 1);
    q[c] = xyz[n % L.nx];
    q[ns + c] = xyz[L.nx + (n / L.nx) % L.ny];
    q[2L * ns + c] = xyz[L.nx + L.ny + n / ((long)L.nx * L.ny)];
}

// V[m][c] - mean[c] in place: the factor of every pair the column takes part in
__global__ __launch_bounds__(256) void k_res_center(double *__restrict__ V, long total, int ns, const double *__restrict__ mean) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) V[i] = V[i] - mean[i % ns];
}

__device__ __forceinline__ bool res_on_lattice(const ResLattice &L, int i, int j, int k, int di, int dj, int dk) {
    return i + di >= 0 && i + di < L.nx && j + dj >= 0 && j + dj < L.ny && k + dk >= 0 && k + dk < L.nz;
}

// ring = the slots [R][M][ns], centred; block b's tiles; act[na] = the offsets of this chunk that have pairs on the
// lattice (indices into tab); sel[nsel] = the positions in act this launch takes; psum [leaf][na][ns].  Work item
// (blockIdx.x: group of G selected offsets, blockIdx.y: leaf -- the models leaves[blockIdx.y].x .. .y, blockIdx.z:
// tile): the groups of a tile follow each other, so that its rows are in the L2 for all of them.
template <int G>
__global__ __launch_bounds__(kResThreads) void k_res_pairs(const double *__restrict__ ring, int M, int ns, long R, long b,
                                                           ResLattice L, const int2 *__restrict__ leaves,
                                                           const ResOffset *__restrict__ tab, const int *__restrict__ act,
                                                           int na, const int *__restrict__ sel, int nsel,
                                                           double *__restrict__ psum) {
    const int lane = threadIdx.x;
    const int col = blockIdx.z * kResThreads + lane;
    const long slot = (long)M * ns;
    const long n = min(b * ns + col, L.nq - 1);  // (past the lattice's end: the last node again, not stored)
    const int i = (int)(n % L.nx), j = (int)((n / L.nx) % L.ny), k = (int)(n / ((long)L.nx * L.ny));
    const int2 lf = leaves[blockIdx.y];
    const double *__restrict__ p0 = ring + (b % R) * slot + (n - b * ns) + (long)lf.x * ns;
    const double *__restrict__ p[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const ResOffset o = tab[act[sel[min((int)blockIdx.x * G + g, nsel - 1)]]];
        const long c = res_on_lattice(L, i, j, k, o.di, o.dj, o.dk) ? n + o.f : n;
        const long bc = c / ns;
        p[g] = ring + (bc % R) * slot + (c - bc * ns) + (long)lf.x * ns;
    }
    double s[G];
    {
        const double d0 = p0[0];
#pragma unroll
        for (int g = 0; g < G; ++g) s[g] = d0 * p[g][0];
    }
    int m = lf.x + 1;
    long at = ns;  // the row's distance from the leaf's first
    for (; m + kResAhead <= lf.y + 1; m += kResAhead) {
        double r0[kResAhead], r[kResAhead][G];
#pragma unroll
        for (int a = 0; a < kResAhead; ++a) {
            r0[a] = p0[at + (long)a * ns];
#pragma unroll
            for (int g = 0; g < G; ++g) r[a][g] = p[g][at + (long)a * ns];
        }
#pragma unroll
        for (int a = 0; a < kResAhead; ++a) {
#pragma unroll
            for (int g = 0; g < G; ++g) s[g] = s[g] + r0[a] * r[a][g];
        }
        at += (long)kResAhead * ns;
    }
    for (; m <= lf.y; ++m) {
        const double d0 = p0[at];
#pragma unroll
        for (int g = 0; g < G; ++g) s[g] = s[g] + d0 * p[g][at];
        at += ns;
    }
    if (col >= ns) return;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int a = (int)blockIdx.x * G + g;
        if (a < nsel) psum[((long)blockIdx.y * na + sel[a]) * ns + col] = s[g];
    }
}

// The x-run form: runs[blockIdx.x] = (first position in the ordered list, cnt <= G offsets, f0), blockIdx.y the leaf,
// blockIdx.z the tile (the runs of a tile follow each other, as k_res_pairs' groups do); a0 = the chunk's first
// position, psum [leaf][na][ns] as k_res_pairs writes it.  Offset g of the run has the partner n + f0 + g: the
// staged row holds the columns n0 + f0 .. n0 + f0 + 64 + cnt - 1 (n0: the tile's first node), clipped to the lattice's
// last node (a clipped column is the partner of no pair on the lattice).
typedef __attribute__((address_space(3))) volatile double ResLdsRead;  // an LDS read that is not merged with its neighbour
template <int G>
__global__ __launch_bounds__(kResThreads) void k_res_xruns(const double *__restrict__ ring, int M, int ns, long R, long b,
                                                           ResLattice L, const int2 *__restrict__ leaves,
                                                           const ResRun *__restrict__ runs, int a0, int na,
                                                           double *__restrict__ psum) {
    constexpr int W = kResThreads + 16;  // a staged row: 64 + G - 1 <= 75 columns
    static_assert(G - 1 <= 16, "the staged row");
    __shared__ double seg[kResAhead][W];
    const int lane = threadIdx.x;
    const int col = blockIdx.z * kResThreads + lane;
    const long slot = (long)M * ns;
    const long n0 = b * ns + (long)blockIdx.z * kResThreads;
    const long n = min(n0 + lane, L.nq - 1);
    const int2 lf = leaves[blockIdx.y];
    const ResRun run = runs[blockIdx.x];
    const bool second = lane < run.cnt - 1;  // the lanes that stage the columns past the 64th
    const double *__restrict__ p0 = ring + (b % R) * slot + (n - b * ns) + (long)lf.x * ns;
    const double *__restrict__ pa, *__restrict__ pb;
    {
        const long ca = min(n0 + run.f0 + lane, L.nq - 1), cb = min(n0 + run.f0 + kResThreads + lane, L.nq - 1);
        const long ba = ca / ns, bb = cb / ns;
        pa = ring + (ba % R) * slot + (ca - ba * ns) + (long)lf.x * ns;
        pb = second ? ring + (bb % R) * slot + (cb - bb * ns) + (long)lf.x * ns : pa;
    }
    double s[G];
    const int rows = lf.y - lf.x + 1;
    double r0[kResAhead], va[kResAhead], vb[kResAhead];
    auto load = [&](int m) {  // the rows m .. m + kResAhead of the leaf (past its end: the last row again, not used)
#pragma unroll
        for (int a = 0; a < kResAhead; ++a) {
            const long at = (long)min(m + a, rows - 1) * ns;
            r0[a] = p0[at];
            va[a] = pa[at];
            vb[a] = pb[at];
        }
    };
    load(0);
    for (int m = 0; m < rows; m += kResAhead) {
        __syncthreads();  // (one wave: the staged rows' readers are done)
        double d0[kResAhead];
#pragma unroll
        for (int a = 0; a < kResAhead; ++a) {
            d0[a] = r0[a];
            seg[a][lane] = va[a];
            if (second) seg[a][kResThreads + lane] = vb[a];
        }
        __syncthreads();
        if (m + kResAhead < rows) load(m + kResAhead);
        const int cnt = min(kResAhead, rows - m);
#pragma unroll
        for (int a = 0; a < kResAhead; ++a)
            if (a < cnt) {
                // (volatile: one ds_read_b64 per partner, 256 B/clk; merged into ds_read2_b64 they read at half that)
                const ResLdsRead *row = (const ResLdsRead *)&seg[a][lane];
                if (m + a == 0) {
#pragma unroll
                    for (int g = 0; g < G; ++g) s[g] = d0[a] * row[g];
                } else {
#pragma unroll
                    for (int g = 0; g < G; ++g) s[g] = s[g] + d0[a] * row[g];
                }
            }
    }
    if (col >= ns) return;
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (g < run.cnt) psum[((long)blockIdx.y * na + (run.first - a0 + g)) * ns + col] = s[g];
}

// psum [leaf][na][ns] of block b -> cov, corr [noff][nq] (cov nullable); sd [the blocks' columns]
__global__ __launch_bounds__(256) void k_res_combine(const double *__restrict__ psum, int nleaves, int M, int ns, long b,
                                                     ResLattice L, const ResOffset *__restrict__ tab,
                                                     const int *__restrict__ act, int na, const double *__restrict__ sd,
                                                     double *__restrict__ cov, double *__restrict__ corr) {
    extern __shared__ double pend[];  // the waiting left halves [cov_levels(M)][256]
    const int col = blockIdx.x * 256 + threadIdx.x;
    const long n = b * ns + col;
    if (col >= ns || n >= L.nq) return;
    const int oi = act[blockIdx.y];
    const ResOffset o = tab[oi];
    const int i = (int)(n % L.nx), j = (int)((n / L.nx) % L.ny), k = (int)(n / ((long)L.nx * L.ny));
    double c = __builtin_nan(""), r = __builtin_nan("");
    if (res_on_lattice(L, i, j, k, o.di, o.dj, o.dk)) {
        const double *__restrict__ ps = psum + (long)blockIdx.y * ns + col;
        const long st = (long)na * ns;  // from a leaf to the next
        double total;
        if (nleaves == 1) {
            total = ps[0];
        } else {  // k_iface_combine's walk of the pairwise tree, a block of at most 1024 models being the next leaf
            unsigned path = 0;  // bit d: the right child at depth d
            int depth = 0, nv = 0, leaf = 0;
            for (;;) {
                int lo = 0, hi = M - 1;
                for (int d = 0; d < depth; ++d) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if ((path >> d) & 1u)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                while (hi - lo >= 1024) {  // down the left children to a block
                    hi = lo + ((hi - lo) >> 1);
                    path &= ~(1u << depth);
                    ++depth;
                }
                total = ps[(long)leaf * st];
                ++leaf;
                while (depth > 0 && ((path >> (depth - 1)) & 1u)) {  // a right child: its parent is left + right
                    --nv;
                    total = pend[nv * 256 + threadIdx.x] + total;
                    --depth;
                }
                if (depth == 0) break;
                pend[nv * 256 + threadIdx.x] = total;  // a left child waits (read again by this lane alone)
                ++nv;
                path |= 1u << (depth - 1);
            }
        }
        c = total / (double)(M - 1);  // M == 1: 0 / 0 = NaN, as sigma
        const double ss = sd[n] * sd[n + o.f];
        r = c / ss;
    }
    if (cov) cov[(long)oi * L.nq + n] = c;
    corr[(long)oi * L.nq + n] = r;
}

// corr [noff][nq] (the rows of offsets with f == 0 are not read); ax = the axis lists behind one another, nax[a]
// entries each; w nullable; foot [nq]; run [3][2][nq]; cens [nq] (each nullable)
struct ResAxes {
    int n[3];
};
__global__ __launch_bounds__(256) void k_res_summary(const double *__restrict__ corr, ResLattice L,
                                                     const ResOffset *__restrict__ tab, int noff,
                                                     const int *__restrict__ ax, ResAxes nax, double thr,
                                                     const double *__restrict__ w, double *__restrict__ foot,
                                                     int *__restrict__ run, int *__restrict__ cens) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= L.nq) return;
    const int idx[3] = {(int)(n % L.nx), (int)((n / L.nx) % L.ny), (int)(n / ((long)L.nx * L.ny))};
    if (foot) {
        double acc = w ? w[n] : 1.0;
        for (int oi = 0; oi < noff; ++oi) {
            const ResOffset o = tab[oi];
            if (o.f == 0) continue;  // no pair of it on the lattice
            const double *__restrict__ row = corr + (long)oi * L.nq;
            if (res_on_lattice(L, idx[0], idx[1], idx[2], o.di, o.dj, o.dk) && row[n] >= thr) acc = acc + (w ? w[n + o.f] : 1.0);
            if (res_on_lattice(L, idx[0], idx[1], idx[2], -o.di, -o.dj, -o.dk) && row[n - o.f] >= thr)
                acc = acc + (w ? w[n - o.f] : 1.0);
        }
        foot[n] = acc;
    }
    if (!run && !cens) return;
    const int len[3] = {L.nx, L.ny, L.nz};
    const long stride[3] = {1, L.nx, (long)L.nx * L.ny};
    int bits = 0;
    const int *__restrict__ list = ax;
    for (int a = 0; a < 3; ++a) {
        for (int dir = 0; dir < 2; ++dir) {
            int r = 0;
            for (;;) {
                const int l = r + 1;
                // (r + 1) e_a is not in the list, or its pair is off the lattice: the run is cut off, not ended
                if (r >= nax.n[a] || (dir == 0 ? idx[a] + l >= len[a] : idx[a] - l < 0)) {
                    bits |= 1 << (2 * a + dir);
                    break;
                }
                const long at = dir == 0 ? n : n - l * stride[a];
                if (!(corr[(long)list[r] * L.nq + at] >= thr)) break;
                r = l;
            }
            if (run) run[(long)(2 * a + dir) * L.nq + n] = r;
        }
        list += nax.n[a];
    }
    if (cens) cens[n] = bits;
}

// the pairwise tree's leaves, in order: blocks of at most 1024 models (one leaf below 1025 models)
void res_leaves(int lo, int hi, std::vector<int2> *out) {
    if (hi - lo < 1024) {
        out->push_back(make_int2(lo, hi));
        return;
    }
    const int mid = (lo + hi) >> 1;
    res_leaves(lo, mid, out);
    res_leaves(mid + 1, hi, out);
}

// nx ny nz where nx, ny, nz >= 1 and it fits 64 bits (with room for a block's 64), else 0
int64_t res_nodes(const td_resolution *w) {
    int64_t nxy = 0, nq = 0;
    if (w->nx < 1 || w->ny < 1 || w->nz < 1 || __builtin_mul_overflow(w->nx, w->ny, &nxy) || __builtin_mul_overflow(nxy, w->nz, &nq) ||
        nq > INT64_MAX / 64)
        return 0;
    return nq;
}

// the checks of both entry points that need no context and no HIP call, in the header's order
int res_check(td_ctx *ctx, const td_resolution *w, const char *who) {
    const std::string n(who);
    if (!w) return set_err(ctx, TD_ERR_ARG, n + ": want is NULL");
    if (w->noff < 1 || w->noff > kResMaxOffsets) return set_err(ctx, TD_ERR_ARG, n + ": noff must be 1 .. 4096");
    if (!w->off) return set_err(ctx, TD_ERR_ARG, n + ": off is NULL");
    if (const char *bad = res_offsets_check(w->off, w->noff)) return set_err(ctx, TD_ERR_ARG, n + ": " + bad);
    if (w->threshold != w->threshold) return set_err(ctx, TD_ERR_ARG, n + ": threshold is NaN");
    if (!w->cov_out && !w->corr_out && !w->footprint_out && !w->run_out && !w->extent_out && !w->censored_out && !w->mean_out &&
        !w->std_out)
        return set_err(ctx, TD_ERR_ARG, n + ": no output asked for");
    const int64_t nq = res_nodes(w);
    for (int64_t q = 0; w->weights && q < nq; ++q)
        if (!std::isfinite(w->weights[q])) return set_err(ctx, TD_ERR_ARG, n + ": weights is not finite");
    if (w->nx < 1 || w->ny < 1 || w->nz < 1) return set_err(ctx, TD_ERR_ARG, n + ": nx, ny and nz must be >= 1");
    if (!w->xs || !w->ys || !w->zs) return set_err(ctx, TD_ERR_ARG, n + ": xs, ys and zs must be given");
    const double *vec[3] = {w->xs, w->ys, w->zs};
    const int64_t len[3] = {w->nx, w->ny, w->nz};
    const char *name[3] = {"xs", "ys", "zs"};
    for (int a = 0; a < 3; ++a)
        for (int64_t i = 0; i < len[a]; ++i) {
            if (!std::isfinite(vec[a][i])) return set_err(ctx, TD_ERR_ARG, n + ": " + name[a] + " is not finite");
            if (i > 0 && !(vec[a][i] > vec[a][i - 1]))
                return set_err(ctx, TD_ERR_ARG, n + ": " + name[a] + " is not strictly increasing");
        }
    if (nq == 0) return set_err(ctx, TD_ERR_ARG, n + ": nx ny nz does not fit 64 bits");
    if (!w->mean_out != !w->std_out) return set_err(ctx, TD_ERR_ARG, n + ": mean_out and std_out must be given together");
    return TD_OK;
}

int64_t res_ceiling(int64_t M) { return volume_plan(M, 0, 0, kVolMaxSlabNodes).nodes; }  // the most nodes one sweep takes

// Both entry points; E and w have been checked (ensemble.h, res_check).
int res_core(td_ctx *ctx, const char *who, const Ensemble &E, const td_resolution *w) {
    constexpr int G = kResGroup;
    const std::string name(who);
    const int64_t M = E.nmodels, nx = w->nx, ny = w->ny, nz = w->nz, nq = nx * ny * nz, noff = w->noff;
    const bool summary = w->footprint_out || w->run_out || w->extent_out || w->censored_out;
    const bool runs = w->run_out || w->extent_out || w->censored_out;
    const bool pairs = summary || w->cov_out || w->corr_out, want_cov = w->cov_out != nullptr;
    if (M > kResMaxModels) return set_err(ctx, TD_ERR_ARG, name + ": more than 2^25 models");
    if (nx > INT32_MAX / 2 || ny > INT32_MAX / 2 || nz > INT32_MAX / 2)
        return set_err(ctx, TD_ERR_ARG, name + ": an axis of more than 2^30 nodes");
    if (pairs && nq > kResMaxRowBytes / 8 / noff)
        return set_err(ctx, TD_ERR_ARG, name + ": rows [noff][nq] of more than 1 GiB (8 noff nq bytes; they stay on the device)");
    int64_t reach = 0;
    const std::vector<ResOffset> tab = res_offsets_on(w->off, noff, nx, ny, nz, &reach);
    if (!pairs) reach = 0;
    const ResSetting setting = res_setting(ctx);
    const int64_t budget = setting.budget > 0 ? setting.budget : kResDefaultBudget;
    const ResPlan plan = res_plan(M, nq, reach, budget, ctx->vol_slab_nodes, res_ceiling(M));
    if (plan.ns == 0)
        return set_err(ctx, TD_ERR_ARG, name + ": no block of 64 nodes fits the window budget of " + std::to_string(budget) +
                                            " bytes (M = " + std::to_string(M) + " models, reach = " + std::to_string(reach) + " nodes)");
    std::vector<int32_t> act;  // the offsets with pairs on the lattice, in the x-runs' order
    std::vector<ResRun> xr;  // the x-runs of act
    if (pairs) xr = res_xruns(tab, &act);
    const std::array<std::vector<int32_t>, 3> axl = res_axis_lists(w->off, noff);
    std::vector<int> ax;
    ResAxes nax;
    for (int a = 0; a < 3; ++a) {
        nax.n[a] = (int)axl[(size_t)a].size();
        ax.insert(ax.end(), axl[(size_t)a].begin(), axl[(size_t)a].end());
    }
    std::vector<int2> leaves;
    if (pairs) res_leaves(0, (int)M - 1, &leaves);
    const int64_t ns = plan.ns, R = plan.R, nblocks = plan.nblocks, nleaves = (int64_t)leaves.size(), nact = (int64_t)act.size();
    // the chunks of offsets: whole runs whose leaf sums stay within kResLeafBytes (one run at the least), each
    // chunk's runs in the order of their kernels -- class 0: k_res_pairs on the positions sel, classes 1 .. 3: the
    // instances of k_res_xruns for up to 4, 8 and 12 offsets
    struct Chunk {
        int64_t a0, na, r0, nr[4], s0, nsel;
    };
    std::vector<Chunk> chunks;
    std::vector<int> sel;  // the chunks' positions for k_res_pairs, behind one another
    int64_t chunk = 0;     // the most offsets of a chunk
    if (pairs) {
        const int64_t most = std::max<int64_t>(kResLeafBytes / 8 / (nleaves * ns), kResRunMax);
        const int form = setting.form;
        auto cls = [form](const ResRun &r) {
            if (form == 1 || (form == 0 && r.cnt <= kResShortRun)) return 0;
            return r.cnt <= 4 ? 1 : r.cnt <= 8 ? 2 : 3;
        };
        for (size_t r = 0; r < xr.size(); ++r) {
            if (chunks.empty() || chunks.back().na + xr[r].cnt > most) chunks.push_back({xr[r].first, 0, (int64_t)r, {0, 0, 0, 0}, 0, 0});
            chunks.back().na += xr[r].cnt;
            ++chunks.back().nr[cls(xr[r])];
        }
        for (Chunk &c : chunks) {
            chunk = std::max(chunk, c.na);
            std::stable_sort(xr.begin() + c.r0, xr.begin() + c.r0 + c.nr[0] + c.nr[1] + c.nr[2] + c.nr[3],
                             [&](const ResRun &x, const ResRun &y) { return cls(x) < cls(y); });
            c.s0 = (int64_t)sel.size();
            for (int64_t r = c.r0; r < c.r0 + c.nr[0]; ++r)
                for (int g = 0; g < xr[(size_t)r].cnt; ++g) sel.push_back((int)(xr[(size_t)r].first - c.a0) + g);
            c.nsel = (int64_t)sel.size() - c.s0;
        }
    }

    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    hipStream_t s = ctx->stream;
    // ctx->raster (8-byte words): the lattice's vectors | weights [nq] | queries [3][ns] | ring [R][M][ns] | mean, std
    // [nblocks ns] | leaf sums [leaves][chunk][ns] | corr, cov [noff][nq] | footprint [nq] | the offsets' table |
    // the runs | leaves | 32-bit: run [6][nq], censored [nq] | act | sel | axis lists
    const size_t n_xyz = (size_t)(nx + ny + nz), n_w = summary && w->weights ? (size_t)nq : 0, n_q = 3 * (size_t)ns,
                 n_ring = (size_t)R * (size_t)M * (size_t)ns, n_ms = (size_t)nblocks * (size_t)ns,
                 n_ps = pairs ? (size_t)nleaves * (size_t)chunk * (size_t)ns : 0, n_C = pairs ? (size_t)noff * (size_t)nq : 0,
                 n_cov = want_cov ? n_C : 0, n_foot = summary ? (size_t)nq : 0, n_tab = 3 * (size_t)noff, n_runs = 2 * xr.size(), n_leaf = (size_t)nleaves,
                 n_run = summary ? (7 * (size_t)nq + 1) / 2 : 0, n_act = ((size_t)nact + 1) / 2, n_sel = (sel.size() + 1) / 2, n_ax = (ax.size() + 1) / 2;
    if (int rc = raster_reserve(ctx, n_xyz + n_w + n_q + n_ring + 2 * n_ms + n_ps + n_C + n_cov + n_foot + n_tab + n_runs + n_leaf +
                                         n_run + n_act + n_sel + n_ax,
                                1))
        return rc;
    double *dxyz = ctx->raster.as<double>(), *dw = dxyz + n_xyz, *dq = dw + n_w, *dring = dq + n_q, *dm = dring + n_ring,
           *dsd = dm + n_ms, *dps = dsd + n_ms, *dcorr = dps + n_ps, *dcov = dcorr + n_C, *dfoot = dcov + n_cov;
    ResOffset *dtab = reinterpret_cast<ResOffset *>(dfoot + n_foot);
    ResRun *druns = reinterpret_cast<ResRun *>(dfoot + n_foot + n_tab);
    int2 *dleaf = reinterpret_cast<int2 *>(dfoot + n_foot + n_tab + n_runs);
    int *drun = reinterpret_cast<int *>(dfoot + n_foot + n_tab + n_runs + n_leaf), *dcens = drun + 6 * nq;
    int *dact = reinterpret_cast<int *>(dfoot + n_foot + n_tab + n_runs + n_leaf + n_run);
    int *dsel = reinterpret_cast<int *>(dfoot + n_foot + n_tab + n_runs + n_leaf + n_run + n_act);
    int *dax = reinterpret_cast<int *>(dfoot + n_foot + n_tab + n_runs + n_leaf + n_run + n_act + n_sel);
    const ResLattice L{(int)nx, (int)ny, (int)nz, (long)nq};
    TD_HIP(ctx, hipStreamSynchronize(s));  // (the workspace is free)
    TD_HIP(ctx, hipMemcpyAsync(dxyz, w->xs, sizeof(double) * (size_t)nx, hipMemcpyHostToDevice, s));
    TD_HIP(ctx, hipMemcpyAsync(dxyz + nx, w->ys, sizeof(double) * (size_t)ny, hipMemcpyHostToDevice, s));
    TD_HIP(ctx, hipMemcpyAsync(dxyz + nx + ny, w->zs, sizeof(double) * (size_t)nz, hipMemcpyHostToDevice, s));
    if (n_w > 0) TD_HIP(ctx, hipMemcpyAsync(dw, w->weights, sizeof(double) * n_w, hipMemcpyHostToDevice, s));
    if (pairs) {
        TD_HIP(ctx, hipMemcpyAsync(dtab, tab.data(), sizeof(ResOffset) * (size_t)noff, hipMemcpyHostToDevice, s));
        TD_HIP(ctx, hipMemcpyAsync(dleaf, leaves.data(), sizeof(int2) * (size_t)nleaves, hipMemcpyHostToDevice, s));
        if (nact > 0) {
            TD_HIP(ctx, hipMemcpyAsync(dact, act.data(), sizeof(int) * (size_t)nact, hipMemcpyHostToDevice, s));
            TD_HIP(ctx, hipMemcpyAsync(druns, xr.data(), sizeof(ResRun) * xr.size(), hipMemcpyHostToDevice, s));
            if (!sel.empty()) TD_HIP(ctx, hipMemcpyAsync(dsel, sel.data(), sizeof(int) * sel.size(), hipMemcpyHostToDevice, s));
        }
        if (!ax.empty()) TD_HIP(ctx, hipMemcpyAsync(dax, ax.data(), sizeof(int) * ax.size(), hipMemcpyHostToDevice, s));
    }
    int64_t brute_pairs = 0, swept = 0;
    const size_t lds = sizeof(double) * 256 * (size_t)cov_levels(M);
    for (int64_t b = 0; b < nblocks; ++b) {
        for (; swept < std::min(nblocks, b + R); ++swept) {  // every block once: sweep, statistics, centre
            double *dv = dring + (size_t)(swept % R) * (size_t)M * (size_t)ns;
            hipLaunchKernelGGL(k_res_nodes, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, s, dxyz, L, (long)(swept * ns), (int)ns, dq);
            TD_HIP(ctx, hipGetLastError());
            if (int rc = volume_sweep(ctx, S, 0, M, dq, ns, dv)) return rc;
            if (!S.grid) brute_pairs += M * ns;
            TD_HIP(ctx, timed_launch(ctx, "raster_stats", [&] {
                       return launch_raster_stats(dv, (int)M, (int)ns, dm + swept * ns, dsd + swept * ns, s);
                   }));
            if (pairs) {
                const long total = (long)M * ns;
                TD_HIP(ctx, timed_launch(ctx, "res_center", [&] {
                           hipLaunchKernelGGL(k_res_center, dim3((unsigned)std::min<long>((total + 255) / 256, 1L << 20)), dim3(256), 0, s,
                                              dv, total, (int)ns, dm + swept * ns);
                       }));
            }
        }
        for (const Chunk &c : chunks) {
            const int64_t a0 = c.a0, na = c.na;
            const unsigned nl = (unsigned)nleaves, tiles = (unsigned)(ns / kResThreads);
            TD_HIP(ctx, timed_launch(ctx, "res_pairs", [&] {  // (both forms' launches under the one name)
                       if (c.nsel > 0)
                           hipLaunchKernelGGL(k_res_pairs<G>, dim3((unsigned)((c.nsel + G - 1) / G), nl, tiles), dim3(kResThreads), 0, s,
                                              dring, (int)M, (int)ns, (long)R, (long)b, L, dleaf, dtab, dact + a0, (int)na, dsel + c.s0,
                                              (int)c.nsel, dps);
                       const ResRun *r = druns + c.r0 + c.nr[0];
                       if (c.nr[1] > 0)
                           hipLaunchKernelGGL(k_res_xruns<4>, dim3((unsigned)c.nr[1], nl, tiles), dim3(kResThreads), 0, s, dring, (int)M,
                                              (int)ns, (long)R, (long)b, L, dleaf, r, (int)a0, (int)na, dps);
                       if (c.nr[2] > 0)
                           hipLaunchKernelGGL(k_res_xruns<8>, dim3((unsigned)c.nr[2], nl, tiles), dim3(kResThreads), 0, s, dring, (int)M,
                                              (int)ns, (long)R, (long)b, L, dleaf, r + c.nr[1], (int)a0, (int)na, dps);
                       if (c.nr[3] > 0)
                           hipLaunchKernelGGL(k_res_xruns<kResRunMax>, dim3((unsigned)c.nr[3], nl, tiles), dim3(kResThreads), 0, s, dring,
                                              (int)M, (int)ns, (long)R, (long)b, L, dleaf, r + c.nr[1] + c.nr[2], (int)a0, (int)na, dps);
                   }));
            TD_HIP(ctx, timed_launch(ctx, "res_combine", [&] {
                       hipLaunchKernelGGL(k_res_combine, dim3((unsigned)((ns + 255) / 256), (unsigned)na), dim3(256), lds, s, dps,
                                          (int)nleaves, (int)M, (int)ns, (long)b, L, dtab, dact + a0, (int)na, dsd,
                                          want_cov ? dcov : nullptr, dcorr);
                   }));
        }
    }
    if (w->mean_out) {
        TD_HIP(ctx, hipMemcpyAsync(w->mean_out, dm, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, s));
        TD_HIP(ctx, hipMemcpyAsync(w->std_out, dsd, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, s));
    }
    std::vector<int32_t> run_host;
    if (summary) {
        TD_HIP(ctx, timed_launch(ctx, "res_summary", [&] {
                   hipLaunchKernelGGL(k_res_summary, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, dcorr, L, dtab, (int)noff, dax,
                                      nax, w->threshold, n_w > 0 ? dw : nullptr, w->footprint_out ? dfoot : nullptr,
                                      runs ? drun : nullptr, w->censored_out ? dcens : nullptr);
               }));
        if (w->footprint_out)
            TD_HIP(ctx, hipMemcpyAsync(w->footprint_out, dfoot, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, s));
        if (w->censored_out)
            TD_HIP(ctx, hipMemcpyAsync(w->censored_out, dcens, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
        if (runs) {
            run_host.resize(6 * (size_t)nq);
            TD_HIP(ctx, hipMemcpyAsync(run_host.data(), drun, sizeof(int32_t) * 6 * (size_t)nq, hipMemcpyDeviceToHost, s));
        }
    }
    // the rows of the offsets with pairs on the lattice; the others are NaN throughout
    for (int pass = 0; pass < 2; ++pass) {
        double *out = pass ? w->corr_out : w->cov_out;
        const double *dev = pass ? dcorr : dcov;
        if (!out) continue;
        for (int64_t o = 0; o < noff; ++o) {
            if (tab[(size_t)o].f > 0)
                TD_HIP(ctx, hipMemcpyAsync(out + o * nq, dev + o * nq, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, s));
            else
                std::fill(out + o * nq, out + (o + 1) * nq, std::nan(""));
        }
    }
    TD_HIP(ctx, hipStreamSynchronize(s));
    if (runs) {
        if (w->run_out) std::memcpy(w->run_out, run_host.data(), sizeof(int32_t) * run_host.size());
        const double *vec[3] = {w->xs, w->ys, w->zs};
        const int64_t stride[3] = {1, nx, nx * ny}, len[3] = {nx, ny, nz};
        for (int a = 0; w->extent_out && a < 3; ++a)
            for (int64_t q = 0; q < nq; ++q) {
                const int64_t idx = (q / stride[a]) % len[a];
                w->extent_out[a * nq + q] = vec[a][idx + run_host[(size_t)((2 * a) * nq + q)]] - vec[a][idx - run_host[(size_t)((2 * a + 1) * nq + q)]];
            }
    }
    return volume_counters_finish(ctx, S, brute_pairs);  // (tdt_volume_counters: this call's sweeps)
}

}  // namespace

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_resolution(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                       const double *yCell, const double *zCell, const double *zeta,
                                       const td_resolution *want) {
    const char *who = "td_rasterize_resolution";
    return ensemble_entry_arrays(
        ctx, who, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta), nullptr, [&] { return res_check(ctx, want, who); },
        [&](const Ensemble &E) { return res_core(ctx, who, E, want); });
}

extern "C" int td_history_resolution(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_resolution *want) {
    const char *who = "td_history_resolution";
    return ensemble_entry_histories(
        ctx, who, hs, nh, nullptr, [&] { return res_check(ctx, want, who); },
        [&](const Ensemble &E) { return res_core(ctx, who, E, want); });
}

extern "C" int tdt_resolution_plan(int64_t nmodels, int64_t nq, int64_t reach, int64_t budget, int64_t forced, int64_t out[3]) {
    if (!out || nmodels < 1 || nq < 1 || nq > ((int64_t)1 << 56) || reach < 0 || reach >= nq || budget < 0 || forced < 0)
        return TD_ERR_ARG;
    const ResPlan p = res_plan(nmodels, nq, reach, budget, forced, res_ceiling(nmodels));
    if (p.ns == 0) return TD_ERR_ARG;
    out[0] = p.ns;
    out[1] = p.R;
    out[2] = p.nblocks;
    return TD_OK;
}

extern "C" int tdt_set_resolution(td_ctx *ctx, int64_t budget, int form) {
    if (!ctx || budget < 0 || form < 0 || form > 2) return TD_ERR_ARG;
    std::lock_guard<std::mutex> hold(g_setting_lock);
    if (budget == 0 && form == 0)
        g_setting.erase(ctx);
    else
        g_setting[ctx] = ResSetting{budget, form};
    return TD_OK;
}
