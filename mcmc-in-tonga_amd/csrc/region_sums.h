// region_sums.h -- what regions.hip and recovery.hip share: per model the weighted sum of a function of a slab's
// values over each region of a point list, in td_rasterize's association counted over the index within the
// region.  The unit of that association is the leaf: a block of at most 1024 consecutive points of one region
// (region_leaves: the split of iface_leaves applied to the region's point count).  The leaves of all regions tile
// the point list in order.  Everything here has internal linkage: each unit that includes the header holds kernels
// of its own.
//   k_region_sums<Op> work item = (a leaf's columns in this slab, 64 models), one wave, one lane per model.
//                     V_slab is row-major, so a lane walking its own row would stride by 8 ns bytes: the wave
//                     reads a tile of 64 models x 64 columns row by row instead -- each row one coalesced
//                     512-byte load, kRegAhead of them in flight per lane -- into LDS (rows padded to 65
//                     doubles: lane m's ds_read_b64 of column c hits the bank pair 2 (m + c) mod 64, none twice
//                     in a half wave), with the tile's weights as one more LDS row; then each lane walks its row
//                     left to right, t = Op(w, v) rounded, then acc = acc + t.  A leaf is summed left to right, so
//                     a slab boundary inside it is carried: the accumulators acc[leaf][M] live in the workspace
//                     across the slabs, started at -0.0 (-0.0 + t is t for every t, the sign of a zero
//                     included) where the leaf begins.
//   k_region_combine  one lane per (model, region): the region's leaf sums are added in the tree's order (the
//                     walk of k_iface_combine with a leaf as the unit, the waiting left halves in LDS), divided
//                     by W[r] when asked, and written to F[m][r].  W is formed on the host in the same
//                     association (region_weight).
// The including unit is compiled without contraction, so an Op's multiplies are rounded one by one.
//
// The host side of both units is here too, behind the kernels: the checks of a point list cut into regions
// (RegionList, region_list_check), its leaves and a call's limits (RegionPlan, region_layout, region_limits,
// region_plan), and the steps of a call in the order a unit takes them -- region_upload once; per slab
// region_stage_weights before the sweep and region_sums_slab<Op> after it; then region_combine, region_tail and
// region_finish.  What a unit keeps is its workspace layout, its own kernels and its own outputs.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "covariance.h"
#include "ctx.h"
#include "ensemble.h"
#include "volume.h"

namespace tdstar {

namespace {

constexpr int kRegTile = 64;          // models and columns of an LDS tile; one wave
constexpr int kRegPad = kRegTile + 1; // doubles per LDS row
constexpr int kRegAhead = 16;         // rows of the tile a lane keeps in flight

// V = V_slab[M][ns], the points [c0, c0 + ns) of the list.  Leaf l is the points [leafp[l], leafp[l + 1]);
// workgroup b takes the leaf la + b / mgroups and the models 64 (b % mgroups) ...  wcol [ns]: the slab's weights
// (null: 1.0).  acc [leaves][M].  Op::term(w, v): the term of the sum.
template <class Op>
__global__ __launch_bounds__(kRegTile) void k_region_sums(const double *__restrict__ V, long ns, int M, long c0,
                                                          const long long *__restrict__ leafp, long la, int mgroups,
                                                          const double *__restrict__ wcol, double *__restrict__ acc) {
    __shared__ double tile[kRegTile * kRegPad];
    __shared__ double wrow[kRegTile];
    const int lane = threadIdx.x;
    const long leaf = la + blockIdx.x / mgroups;
    const int m0 = (int)(blockIdx.x % mgroups) * kRegTile;
    const long p0 = leafp[leaf], p1 = leafp[leaf + 1];
    const long s0 = max(p0, c0) - c0, s1 = min(p1, c0 + ns) - c0;  // the leaf's columns of this slab: [s0, s1)
    const int m = min(m0 + lane, M - 1);
    double a = p0 >= c0 ? -0.0 : acc[leaf * M + m];  // the leaf begins here, or is carried from the slab before
    const double *__restrict__ mine = tile + lane * kRegPad;
    for (long t0 = s0; t0 < s1; t0 += kRegTile) {
        const int nc = (int)min((long)kRegTile, s1 - t0);
        const long col = t0 + min(lane, nc - 1);  // (past the leaf's end: its last column again, not used)
        wrow[lane] = wcol ? wcol[col] : 1.0;
#pragma unroll
        for (int j0 = 0; j0 < kRegTile; j0 += kRegAhead) {
            double r[kRegAhead];
#pragma unroll
            for (int j = 0; j < kRegAhead; ++j) r[j] = V[(long)min(m0 + j0 + j, M - 1) * ns + col];
#pragma unroll
            for (int j = 0; j < kRegAhead; ++j) tile[(j0 + j) * kRegPad + lane] = r[j];
        }
        __syncthreads();
        if (nc == kRegTile) {
#pragma unroll 16
            for (int c = 0; c < kRegTile; ++c) {
                const double t = Op::term(wrow[c], mine[c]);
                a = a + t;
            }
        } else {
            for (int c = 0; c < nc; ++c) {
                const double t = Op::term(wrow[c], mine[c]);
                a = a + t;
            }
        }
        __syncthreads();  // (the tile is filled again)
    }
    if (m0 + lane < M) acc[leaf * M + m0 + lane] = a;
}

// Region r's leaves are regleaf[r] .. regleaf[r + 1] - 1.  Workgroup b: region b / mblocks, models 256 (b % mblocks) ...
__global__ __launch_bounds__(256) void k_region_combine(const double *__restrict__ acc, int M, int mblocks,
                                                        const long long *__restrict__ regleaf,
                                                        const long long *__restrict__ leafp,
                                                        const double *__restrict__ W, int normalize, long R,
                                                        double *__restrict__ F) {
    extern __shared__ double pend[];  // the waiting left halves [cov_levels(the most points of a region)][256]
    const long r = blockIdx.x / mblocks;
    const int m = (int)(blockIdx.x % mblocks) * 256 + threadIdx.x;
    if (m >= M) return;
    const long l0 = regleaf[r], nl = regleaf[r + 1] - l0;
    const long n = leafp[l0 + nl] - leafp[l0];  // the region's points
    const double *__restrict__ ps = acc + l0 * M + m;
    double total;
    if (nl == 1) {
        total = ps[0];
    } else {  // k_iface_combine's walk of the pairwise tree over the region's n points, a block of <= 1024 being a leaf
        unsigned path = 0;  // bit d: the right child at depth d
        int depth = 0, nv = 0;
        long leaf = 0;
        for (;;) {
            long lo = 0, hi = n - 1;
            for (int d = 0; d < depth; ++d) {
                const long mid = lo + ((hi - lo) >> 1);
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
            total = ps[leaf * M];
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
    F[(long)m * R + r] = normalize ? total / W[r] : total;
}

// The leaves of a region of n points whose first point is `base`, in order: the first points, appended to out.
inline void region_leaves(int64_t base, int64_t lo, int64_t hi, std::vector<long long> *out) {
    if (hi - lo < 1024) {
        out->push_back(base + lo);
        return;
    }
    const int64_t mid = (lo + hi) >> 1;
    region_leaves(base, lo, mid, out);
    region_leaves(base, mid + 1, hi, out);
}

// W of one region: the sum of w[lo .. hi] (null: of ones) in the tree's order, a block left to right.
inline double region_weight(const double *w, int64_t lo, int64_t hi) {
    if (hi - lo < 1024) {
        double s = w ? w[lo] : 1.0;
        for (int64_t k = lo + 1; k <= hi; ++k) s = s + (w ? w[k] : 1.0);
        return s;
    }
    const int64_t mid = (lo + hi) >> 1;
    const double a = region_weight(w, lo, mid), b = region_weight(w, mid + 1, hi);
    return a + b;
}

constexpr int64_t kRegMaxRegions = kVolMaxSlabNodes;  // the statistics take one slab's columns

// The point list of a td_regions or a td_recovery (the two lay these fields out differently).
struct RegionList {
    const double *px, *py, *pz, *w;  // w null: 1.0 everywhere
    int64_t np;
    const int64_t *reg_off;  // [nreg + 1], region r = the points [reg_off[r], reg_off[r + 1])
    int64_t nreg, normalize;
};

// One more vector [np] that a unit's list must carry (recovery: truth).
struct RegionVector {
    const double *v;
    const char *name;
};

// The checks of a list that need no context and no HIP call (ctx only receives the message); extra nullable.
inline int region_list_check(td_ctx *ctx, const char *who, const RegionList &l, const RegionVector *extra) {
    const std::string n(who);
    if (l.np < 1 || l.nreg < 1) return set_err(ctx, TD_ERR_ARG, n + ": np and nreg must be >= 1");
    if (!l.px || !l.py || !l.pz || !l.reg_off || (extra && !extra->v))
        return set_err(ctx, TD_ERR_ARG,
                       n + (extra ? std::string(": px, py, pz, reg_off and ") + extra->name : ": px, py, pz and reg_off") +
                           " must be given");
    if (l.reg_off[0] != 0) return set_err(ctx, TD_ERR_ARG, n + ": reg_off[0] must be 0");
    for (int64_t r = 0; r < l.nreg; ++r) {
        if (l.reg_off[r + 1] < l.reg_off[r]) return set_err(ctx, TD_ERR_ARG, n + ": reg_off is not monotone");
        if (l.reg_off[r + 1] == l.reg_off[r]) return set_err(ctx, TD_ERR_ARG, n + ": a region without points");
        if (l.reg_off[r + 1] > l.np) return set_err(ctx, TD_ERR_ARG, n + ": reg_off[nreg] must be np");
    }
    if (l.reg_off[l.nreg] != l.np) return set_err(ctx, TD_ERR_ARG, n + ": reg_off[nreg] must be np");
    const double *vec[5] = {l.px, l.py, l.pz, l.w, extra ? extra->v : nullptr};
    const char *name[5] = {"px", "py", "pz", "w", extra ? extra->name : ""};
    for (int a = 0; a < 5; ++a)
        for (int64_t i = 0; vec[a] && i < l.np; ++i)
            if (!std::isfinite(vec[a][i])) return set_err(ctx, TD_ERR_ARG, n + ": " + name[a] + " is not finite");
    if (l.normalize != 0 && l.normalize != 1) return set_err(ctx, TD_ERR_ARG, n + ": normalize must be 0 or 1");
    return TD_OK;
}

// A checked list's leaves and a call's launch shapes.
struct RegionPlan {
    int64_t M = 0, R = 0, np = 0;
    std::vector<long long> leafp;    // [L + 1]: leaf l = the points [leafp[l], leafp[l + 1]), all regions' behind one another
    std::vector<long long> regleaf;  // [R + 1]: region r's leaves are regleaf[r] .. regleaf[r + 1] - 1
    std::vector<double> W;           // [R]
    int64_t most = 1, L = 0;         // the most points of a region; the leaves
    int mgroups = 0, mblocks = 0;    // the models in 64s (k_region_sums) and in 256s (k_region_combine)
    int64_t cap = 0;                 // the most points of a slab
    VolPlan vol;
};

// leafp, regleaf, W, most and L of a checked list: pure host code.
inline void region_layout(const RegionList &l, RegionPlan *p) {
    const int64_t R = l.nreg;
    p->R = R;
    p->np = l.np;
    p->leafp.clear();
    p->regleaf.assign((size_t)R + 1, 0);
    p->W.assign((size_t)R, 0.0);
    p->most = 1;
    for (int64_t r = 0; r < R; ++r) {
        const int64_t lo = l.reg_off[r], cnt = l.reg_off[r + 1] - lo;
        p->regleaf[(size_t)r] = (long long)p->leafp.size();
        region_leaves(lo, 0, cnt - 1, &p->leafp);
        p->W[(size_t)r] = region_weight(l.w ? l.w + lo : nullptr, 0, cnt - 1);
        p->most = std::max(p->most, cnt);
    }
    p->L = (int64_t)p->leafp.size();
    p->regleaf[(size_t)R] = p->L;
    p->leafp.push_back(l.np);
}

// What a call refuses before its layout is made; a unit's own limits follow (regions: the pair counters), then
// region_plan.
inline int region_limits(td_ctx *ctx, const char *who, int64_t M, int64_t R) {
    const std::string n(who);
    if (R > kRegMaxRegions) return set_err(ctx, TD_ERR_ARG, n + ": more than 2^18 regions");
    if (M > kVolDefaultBudget / 8 / R) return set_err(ctx, TD_ERR_ARG, n + ": the series [nmodels][nreg] exceed 1 GiB");
    return TD_OK;
}

// The layout, what is refused after it, and the launch shapes.  Needs a context for its slab setting; issues nothing.
inline int region_plan(td_ctx *ctx, const char *who, int64_t M, const RegionList &l, const td_marginals *marg, RegionPlan *p) {
    const std::string n(who);
    region_layout(l, p);
    p->M = M;
    if (M > kVolDefaultBudget / 8 / p->L)
        return set_err(ctx, TD_ERR_ARG, n + ": the leaf sums [leaves][nmodels] exceed 1 GiB");
    if (int rc = marg_check_models(ctx, marg, M)) return rc;  // (before anything is issued)
    p->vol = volume_plan(M, l.np, kVolDefaultBudget, ctx->vol_slab_nodes);
    p->cap = std::min(p->vol.nodes, l.np);
    p->mgroups = (int)((M + kRegTile - 1) / kRegTile);
    p->mblocks = (int)((M + 255) / 256);
    if ((p->cap + 1) * (int64_t)p->mgroups > INT32_MAX || p->R * (int64_t)p->mblocks > INT32_MAX)
        return set_err(ctx, TD_ERR_ARG, n + ": too many models for one launch");
    return TD_OK;
}

// leafp, regleaf and W to the workspace (dlp [L + 1], drl [R + 1], dW [R]) on ctx->stream.
inline int region_upload(td_ctx *ctx, const RegionPlan &p, long long *dlp, long long *drl, double *dW) {
    hipStream_t s = ctx->stream;
    TD_HIP(ctx, hipMemcpyAsync(dlp, p.leafp.data(), sizeof(long long) * p.leafp.size(), hipMemcpyHostToDevice, s));
    TD_HIP(ctx, hipMemcpyAsync(drl, p.regleaf.data(), sizeof(long long) * p.regleaf.size(), hipMemcpyHostToDevice, s));
    TD_HIP(ctx, hipMemcpyAsync(dW, p.W.data(), sizeof(double) * p.W.size(), hipMemcpyHostToDevice, s));
    return TD_OK;
}

// The slab's weights through the pinned hw to dw (nothing for w == NULL).  The stream has been waited for since
// hw's last use.
inline int region_stage_weights(td_ctx *ctx, const RegionList &l, int64_t c0, int64_t ns, double *hw, double *dw) {
    if (!l.w) return TD_OK;
    std::memcpy(hw, l.w + c0, sizeof(double) * (size_t)ns);
    TD_HIP(ctx, hipMemcpyAsync(dw, hw, sizeof(double) * (size_t)ns, hipMemcpyHostToDevice, ctx->stream));
    return TD_OK;
}

// k_region_sums<Op> on the slab [c0, c0 + ns) of dv over the leaves with a point in it.  *la: the first such
// leaf, carried from slab to slab (0 before the first).  dw null: 1.0.
template <class Op>
int region_sums_slab(td_ctx *ctx, const char *timer_name, const RegionPlan &p, int64_t c0, int64_t ns, const double *dv,
                     const double *dw, const long long *dlp, double *dacc, int64_t *la) {
    while (p.leafp[(size_t)*la + 1] <= c0) ++*la;
    int64_t lb = *la;  // the last leaf with a point in the slab
    while (p.leafp[(size_t)lb + 1] < c0 + ns) ++lb;
    TD_HIP(ctx, timed_launch(ctx, timer_name, [&] {
               hipLaunchKernelGGL(k_region_sums<Op>, dim3((unsigned)((lb - *la + 1) * p.mgroups)), dim3(kRegTile), 0, ctx->stream,
                                  dv, (long)ns, (int)p.M, (long)c0, dlp, (long)*la, p.mgroups, dw, dacc);
           }));
    return TD_OK;
}

// k_region_combine after the last slab: F [M][R] from the leaf sums.
inline int region_combine(td_ctx *ctx, const char *timer_name, const RegionPlan &p, const double *dacc, const long long *drl,
                          const long long *dlp, const double *dW, int normalize, double *dF) {
    TD_HIP(ctx, timed_launch(ctx, timer_name, [&] {
               hipLaunchKernelGGL(k_region_combine, dim3((unsigned)(p.R * p.mblocks)), dim3(256),
                                  sizeof(double) * 256 * (size_t)cov_levels(p.most), ctx->stream, dacc, (int)p.M, p.mblocks, drl,
                                  dlp, dW, normalize, (long)p.R, dF);
           }));
    return TD_OK;
}

// The tail: the regions in the place of a slab's columns, the slab being the whole matrix F (want.row regions).
inline int region_tail(td_ctx *ctx, const Ensemble &E, const SlabWant &want, const double *dF, double *dm, double *dsd) {
    Timer *tm = ctx->timer.on ? &ctx->timer : nullptr;
    hipEvent_t t0 = tm ? tm->begin(ctx->stream) : nullptr;
    const int rc = slab_statistics(ctx, E, want, dF, 0, want.row, dm, dsd, false, nullptr);
    if (tm) tm->end("raster_stats", t0, ctx->stream);
    return rc;
}

// The end of a call: the stream waited for, W to the caller (nullable), tdt_volume_counters: this call's sweeps.
inline int region_finish(td_ctx *ctx, const RegionPlan &p, const VolSearch &S, int64_t brute_pairs, double *weight_out) {
    TD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (weight_out) std::memcpy(weight_out, p.W.data(), sizeof(double) * p.W.size());
    return volume_counters_finish(ctx, S, brute_pairs);
}

}  // namespace

}  // namespace tdstar
