// regions.hip -- posterior region averages: per model the weighted sum (or average) of the nearest-cell value
// over each region of a point list, and on that matrix F[M][regions] the statistics of a posterior volume with
// the regions in the place of the nodes (include/tdstar_regions.h holds the contract).
//
// The search structure is the volume's (volume_build).  The point list is swept slab by slab of volume_plan's
// columns; a slab's V_slab[M][ns] (volume_sweep) is reduced over its COLUMNS, per model, in td_rasterize's
// association counted over the index within the region.  The unit of that association is the leaf: a block of
// at most 1024 consecutive points of one region (region_leaves: the split of iface_leaves applied to the
// region's point count).  The leaves of all regions tile the point list in order.
//   k_region_sums, k_region_combine (region_sums.h, shared with recovery.hip): the term is t = w * v, one multiply.
//   k_region_greater greater[a][b] over the rows of F: a workgroup takes 16 x 16 pairs and a chunk of models
//                     through LDS, one lane per pair, and adds its 32-bit count with one 64-bit atomic (integer
//                     sums: any order gives the same number).
// The tail is slab_statistics on (F, M, regions): k_raster_stats, marginals_run and convergence_run as a volume
// runs them.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/tdstar_regions.h"
#include "covariance.h"
#include "ctx.h"
#include "ensemble.h"
#include "history.h"
#include "region_sums.h"
#include "volume.h"

namespace tdstar {

namespace {

struct RegionTerm {  // t[m][p] = w[p] * V[m][p]
    static __device__ double term(double w, double v) { return w * v; }
};

constexpr int kRegPairs = 16;         // k_region_greater: 16 x 16 pairs per workgroup
constexpr int kRegChunk = 1024;       // ... and this many models, 64 at a time through LDS
constexpr int64_t kRegMaxCounters = kVolDefaultBudget / 8;       // greater_out: 1 GiB of 64-bit counters

// cnt [R][R], zeroed.  Workgroup (x: chunk of kRegChunk models, y: 16 regions b, z: 16 regions a).
__global__ __launch_bounds__(256) void k_region_greater(const double *__restrict__ F, int M, long R,
                                                        unsigned long long *__restrict__ cnt) {
    __shared__ double sa[64 * (kRegPairs + 1)], sb[64 * (kRegPairs + 1)];
    const int t = threadIdx.x, i = t / kRegPairs, j = t % kRegPairs;
    const long ra = (long)blockIdx.z * kRegPairs, rb = (long)blockIdx.y * kRegPairs;
    const long mbeg = (long)blockIdx.x * kRegChunk, mend = min(mbeg + kRegChunk, (long)M);
    unsigned count = 0;
    for (long mm = mbeg; mm < mend; mm += 64) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // 64 rows x 16 columns of each side; what lies outside is NaN (> is false)
            const int e = t + 256 * k, row = e / kRegPairs, c = e % kRegPairs;
            const bool in = mm + row < mend;
            sa[row * (kRegPairs + 1) + c] = in && ra + c < R ? F[(mm + row) * R + ra + c] : __builtin_nan("");
            sb[row * (kRegPairs + 1) + c] = in && rb + c < R ? F[(mm + row) * R + rb + c] : __builtin_nan("");
        }
        __syncthreads();
#pragma unroll 8
        for (int row = 0; row < 64; ++row) count += sa[row * (kRegPairs + 1) + i] > sb[row * (kRegPairs + 1) + j];
        __syncthreads();
    }
    if (count > 0 && ra + i < R && rb + j < R) atomicAdd(&cnt[(ra + i) * R + rb + j], (unsigned long long)count);
}

RegionList region_list(const td_regions *w) { return {w->px, w->py, w->pz, w->w, w->np, w->reg_off, w->nreg, w->normalize}; }

// the checks of both entry points that need no context and no HIP call, in the header's order
int regions_check(td_ctx *ctx, const td_regions *w, const char *who) {
    const std::string n(who);
    if (!w) return set_err(ctx, TD_ERR_ARG, n + ": want is NULL");
    if (int rc = region_list_check(ctx, who, region_list(w), nullptr)) return rc;
    if (!w->series_out && !w->weight_out && !w->mean_out && !w->std_out && !w->greater_out && !w->marg && !w->conv)
        return set_err(ctx, TD_ERR_ARG, n + ": no output asked for");
    if (!w->mean_out != !w->std_out) return set_err(ctx, TD_ERR_ARG, n + ": mean_out and std_out must be given together");
    if (w->marg)
        if (int rc = marg_check_want(ctx, w->marg, who)) return rc;
    if (w->conv)
        if (int rc = conv_check_want(ctx, w->conv, who)) return rc;
    return TD_OK;
}

// Both entry points; E and w have been checked (ensemble.h, regions_check).
int regions_core(td_ctx *ctx, const char *who, const Ensemble &E, const td_regions *w) {
    const int64_t M = E.nmodels, np = w->np, R = w->nreg;
    const RegionList list = region_list(w);
    RegionPlan P;
    if (int rc = region_limits(ctx, who, M, R)) return rc;
    if (w->greater_out && R * R > kRegMaxCounters)
        return set_err(ctx, TD_ERR_ARG, std::string(who) + ": greater_out of more than 2^27 counters (1 GiB)");
    if (int rc = region_plan(ctx, who, M, list, w->marg, &P)) return rc;
    const int64_t cap = P.cap, L = P.L;
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    hipStream_t s = ctx->stream;
    // ctx->raster (8-byte words): queries [3][cap] | weights [cap] | V_slab [M][cap] | mean, std [R] | leaf sums
    // [L][M] | F [M][R] | W [R] | counters [R][R] | leafp [L + 1] | regleaf [R + 1]; pinned: queries | weights
    const size_t n_q = 3 * (size_t)cap, n_w = (size_t)cap, n_v = (size_t)M * (size_t)cap, n_ms = 2 * (size_t)R,
                 n_acc = (size_t)L * (size_t)M, n_F = (size_t)M * (size_t)R, n_W = (size_t)R,
                 n_cnt = w->greater_out ? (size_t)R * (size_t)R : 0, n_lp = (size_t)L + 1, n_rl = (size_t)R + 1;
    if (int rc = raster_reserve(ctx, n_q + n_w + n_v + n_ms + n_acc + n_F + n_W + n_cnt + n_lp + n_rl, n_q + n_w)) return rc;
    double *dq = ctx->raster.as<double>(), *dw = dq + n_q, *dv = dw + n_w, *dm = dv + n_v, *dsd = dm + R, *dacc = dsd + R,
           *dF = dacc + n_acc, *dW = dF + n_F;
    unsigned long long *dcnt = reinterpret_cast<unsigned long long *>(dW + n_W);
    long long *dlp = reinterpret_cast<long long *>(dW + n_W + n_cnt), *drl = dlp + n_lp;
    double *hw = ctx->h_raster.as<double>() + n_q;
    TD_HIP(ctx, hipStreamSynchronize(s));  // (the pinned block and the workspace are free)
    if (int rc = region_upload(ctx, P, dlp, drl, dW)) return rc;
    int64_t brute_pairs = 0, la = 0;
    for (int64_t c0 = 0; c0 < np; c0 += P.vol.nodes) {
        const int64_t ns = std::min(P.vol.nodes, np - c0);
        if (int rc = stage_queries(ctx, w->px, w->py, w->pz, c0, ns, dq)) return rc;
        if (int rc = region_stage_weights(ctx, list, c0, ns, hw, dw)) return rc;
        if (int rc = volume_sweep(ctx, S, 0, M, dq, ns, dv)) return rc;
        if (!S.grid) brute_pairs += M * ns;
        if (int rc = region_sums_slab<RegionTerm>(ctx, "region_sums", P, c0, ns, dv, w->w ? dw : nullptr, dlp, dacc, &la)) return rc;
        TD_HIP(ctx, hipStreamSynchronize(s));  // the pinned block is packed again for the next slab
    }
    if (int rc = region_combine(ctx, "region_combine", P, dacc, drl, dlp, dW, (int)w->normalize, dF)) return rc;
    if (w->greater_out) {
        TD_HIP(ctx, hipMemsetAsync(dcnt, 0, sizeof(unsigned long long) * n_cnt, s));
        const unsigned tiles = (unsigned)((R + kRegPairs - 1) / kRegPairs);
        TD_HIP(ctx, timed_launch(ctx, "region_greater", [&] {
                   hipLaunchKernelGGL(k_region_greater, dim3((unsigned)((M + kRegChunk - 1) / kRegChunk), tiles, tiles), dim3(256), 0,
                                      s, dF, (int)M, (long)R, dcnt);
               }));
        TD_HIP(ctx, hipMemcpyAsync(w->greater_out, dcnt, sizeof(int64_t) * n_cnt, hipMemcpyDeviceToHost, s));
    }
    if (int rc = region_tail(ctx, E, SlabWant{R, w->mean_out, w->std_out, w->series_out, w->marg, w->conv}, dF, dm, dsd)) return rc;
    return region_finish(ctx, P, S, brute_pairs, w->weight_out);
}

}  // namespace

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_regions(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                    const double *yCell, const double *zCell, const double *zeta, int64_t nchains,
                                    const int64_t *chain_len, const td_regions *want) {
    const char *who = "td_rasterize_regions";
    return ensemble_entry_arrays(
        ctx, who, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta, nchains, chain_len), want ? want->conv : nullptr,
        [&] { return regions_check(ctx, want, who); }, [&](const Ensemble &E) { return regions_core(ctx, who, E, want); });
}

extern "C" int td_history_regions(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_regions *want) {
    const char *who = "td_history_regions";
    return ensemble_entry_histories(
        ctx, who, hs, nh, want ? want->conv : nullptr, [&] { return regions_check(ctx, want, who); },
        [&](const Ensemble &E) { return regions_core(ctx, who, E, want); });
}

extern "C" int tdt_regions_plan(int64_t nmodels, int64_t np, int64_t budget, int64_t forced, int64_t out[2]) {
    if (!out || nmodels < 1 || np < 1 || budget < 0 || forced < 0) return TD_ERR_ARG;
    const VolPlan p = volume_plan(nmodels, np, budget, forced);
    out[0] = p.nodes;
    out[1] = p.nslabs;
    return TD_OK;
}
