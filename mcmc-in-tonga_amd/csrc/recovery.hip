// recovery.hip -- posterior recovery: an ensemble against a known model.  Per point of a point list the rank of the
// truth in the sample (below / equal / above) and the mean and sigma of the error, per model and region the
// weighted mean square of the error, and on that matrix F[M][regions] the statistics of a posterior volume with the
// regions in the place of the nodes (include/tdstar_recovery.h holds the contract).
//
// The search structure is the volume's (volume_build) and the point list is swept slab by slab of volume_plan's
// columns, as regions.hip sweeps it.  Per slab V_slab[M][ns] (volume_sweep):
//   k_recovery_counts one lane per column, the models in model order (a row of the slab per step, coalesced, eight
//                     rows in flight per lane): the three counts against truth[p] as 32-bit sums written as int64
//                     (integer sums: any order gives the same number), and D = V - truth written IN PLACE -- V is
//                     not read again, so the slab needs no second block.
//   k_raster_stats    (raster.hip, unchanged) on D: dmean, dstd.
//   k_region_sums     (region_sums.h, shared with regions.hip) with the term u = d * d; t = w * u, two rounded
//                     multiplies, into the leaf accumulators acc[leaf][M] carried across the slabs.
// After the last slab k_region_combine (region_sums.h) adds the leaf sums in the tree's order and divides by W[r]
// when asked, and the tail is slab_statistics on (F, M, regions), as in regions.hip.
// The counts do not go through the LDS tile of the sums kernel: D has to be written for k_raster_stats whatever
// counts it, the pass that writes it has each value in a register already, and counting there costs three
// compares and no atomics, no zeroed counters and no second reading of the slab.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tdstar_recovery.h"
#include "covariance.h"
#include "ctx.h"
#include "ensemble.h"
#include "history.h"
#include "region_sums.h"
#include "volume.h"

namespace tdstar {

namespace {

constexpr int kRecThreads = 256;
constexpr int kRecAhead = 8;  // rows of the slab a lane of k_recovery_counts keeps in flight
constexpr int64_t kRecMaxRegions = kVolMaxSlabNodes;  // the statistics take one slab's columns

struct RecoveryTerm {  // u = d * d; t = w * u
    static __device__ double term(double w, double d) {
        const double u = d * d;
        return w * u;
    }
};

// V = V_slab[M][ns], overwritten by D = V - truth when write_d; truth [ns]; cnt [3][ns]: below | equal | above.
__global__ __launch_bounds__(kRecThreads) void k_recovery_counts(double *__restrict__ V, int M, long ns,
                                                                 const double *__restrict__ truth, int write_d,
                                                                 long long *__restrict__ cnt) {
    const long q = (long)blockIdx.x * kRecThreads + threadIdx.x;
    if (q >= ns) return;
    const double tr = truth[q];
    double *__restrict__ col = V + q;
    unsigned below = 0, equal = 0, above = 0;
    int m = 0;
    for (; m + kRecAhead <= M; m += kRecAhead) {
        double v[kRecAhead];
#pragma unroll
        for (int j = 0; j < kRecAhead; ++j) v[j] = col[(long)(m + j) * ns];
#pragma unroll
        for (int j = 0; j < kRecAhead; ++j) {
            below += v[j] < tr;
            equal += v[j] == tr;
            above += v[j] > tr;
            if (write_d) col[(long)(m + j) * ns] = v[j] - tr;
        }
    }
    for (; m < M; ++m) {
        const double v = col[(long)m * ns];
        below += v < tr;
        equal += v == tr;
        above += v > tr;
        if (write_d) col[(long)m * ns] = v - tr;
    }
    cnt[q] = (long long)below;
    cnt[ns + q] = (long long)equal;
    cnt[2 * ns + q] = (long long)above;
}

// what a call needs beyond the counts
bool wants_series(const td_recovery *w) { return w->series_out || w->mean_out || w->std_out || w->marg || w->conv; }
bool wants_counts(const td_recovery *w) { return w->below_out || w->equal_out || w->above_out; }

// the checks of both entry points that need no context and no HIP call, in the header's order
int recovery_check(td_ctx *ctx, const td_recovery *w, const char *who) {
    const std::string n(who);
    if (!w) return set_err(ctx, TD_ERR_ARG, n + ": want is NULL");
    if (w->np < 1 || w->nreg < 1) return set_err(ctx, TD_ERR_ARG, n + ": np and nreg must be >= 1");
    if (!w->px || !w->py || !w->pz || !w->reg_off || !w->truth)
        return set_err(ctx, TD_ERR_ARG, n + ": px, py, pz, reg_off and truth must be given");
    if (w->reg_off[0] != 0) return set_err(ctx, TD_ERR_ARG, n + ": reg_off[0] must be 0");
    for (int64_t r = 0; r < w->nreg; ++r) {
        if (w->reg_off[r + 1] < w->reg_off[r]) return set_err(ctx, TD_ERR_ARG, n + ": reg_off is not monotone");
        if (w->reg_off[r + 1] == w->reg_off[r]) return set_err(ctx, TD_ERR_ARG, n + ": a region without points");
        if (w->reg_off[r + 1] > w->np) return set_err(ctx, TD_ERR_ARG, n + ": reg_off[nreg] must be np");
    }
    if (w->reg_off[w->nreg] != w->np) return set_err(ctx, TD_ERR_ARG, n + ": reg_off[nreg] must be np");
    const double *vec[5] = {w->px, w->py, w->pz, w->w, w->truth};
    const char *name[5] = {"px", "py", "pz", "w", "truth"};
    for (int a = 0; a < 5; ++a)
        for (int64_t i = 0; vec[a] && i < w->np; ++i)
            if (!std::isfinite(vec[a][i])) return set_err(ctx, TD_ERR_ARG, n + ": " + name[a] + " is not finite");
    if (w->normalize != 0 && w->normalize != 1) return set_err(ctx, TD_ERR_ARG, n + ": normalize must be 0 or 1");
    if (!wants_counts(w) && !w->dmean_out && !w->dstd_out && !w->weight_out && !wants_series(w))
        return set_err(ctx, TD_ERR_ARG, n + ": no output asked for");
    if (!w->dmean_out != !w->dstd_out) return set_err(ctx, TD_ERR_ARG, n + ": dmean_out and dstd_out must be given together");
    if (!w->mean_out != !w->std_out) return set_err(ctx, TD_ERR_ARG, n + ": mean_out and std_out must be given together");
    if (w->marg)
        if (int rc = marg_check_want(ctx, w->marg, who)) return rc;
    if (w->conv)
        if (int rc = conv_check_want(ctx, w->conv, who)) return rc;
    return TD_OK;
}

// Both entry points; E and w have been checked (ensemble.h, recovery_check).
int recovery_core(td_ctx *ctx, const char *who, const Ensemble &E, const td_recovery *w) {
    const std::string n(who);
    const int64_t M = E.nmodels, np = w->np, R = w->nreg;
    if (R > kRecMaxRegions) return set_err(ctx, TD_ERR_ARG, n + ": more than 2^18 regions");
    if (M > kVolDefaultBudget / 8 / R)
        return set_err(ctx, TD_ERR_ARG, n + ": the series [nmodels][nreg] exceed 1 GiB");
    // the leaves of all regions behind one another: leaf l = the points [leafp[l], leafp[l + 1])
    std::vector<long long> leafp, regleaf((size_t)R + 1);
    std::vector<double> W((size_t)R);
    int64_t most = 1;
    for (int64_t r = 0; r < R; ++r) {
        const int64_t lo = w->reg_off[r], cnt = w->reg_off[r + 1] - lo;
        regleaf[(size_t)r] = (long long)leafp.size();
        region_leaves(lo, 0, cnt - 1, &leafp);
        W[(size_t)r] = region_weight(w->w ? w->w + lo : nullptr, 0, cnt - 1);
        most = std::max(most, cnt);
    }
    const int64_t L = (int64_t)leafp.size();
    regleaf[(size_t)R] = L;
    leafp.push_back(np);
    if (M > kVolDefaultBudget / 8 / L)
        return set_err(ctx, TD_ERR_ARG, n + ": the leaf sums [leaves][nmodels] exceed 1 GiB");
    if (int rc = marg_check_models(ctx, w->marg, M)) return rc;  // (before anything is issued)
    const VolPlan plan = volume_plan(M, np, kVolDefaultBudget, ctx->vol_slab_nodes);
    const int64_t cap = std::min(plan.nodes, np);
    const int mgroups = (int)((M + kRegTile - 1) / kRegTile), mblocks = (int)((M + 255) / 256);
    if ((cap + 1) * (int64_t)mgroups > INT32_MAX || R * (int64_t)mblocks > INT32_MAX)
        return set_err(ctx, TD_ERR_ARG, n + ": too many models for one launch");
    const bool series = wants_series(w), dstats = w->dmean_out != nullptr;
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    hipStream_t s = ctx->stream;
    Timer *tm = ctx->timer.on ? &ctx->timer : nullptr;
    // ctx->raster (8-byte words): queries [3][cap] | weights [cap] | truth [cap] | V_slab, then D [M][cap] | dmean, dstd
    // [cap] | counts [3][cap] | mean, std [R] | leaf sums [L][M] | F [M][R] | W [R] | leafp [L + 1] | regleaf [R + 1];
    // pinned: queries | weights | truth
    const size_t n_q = 3 * (size_t)cap, n_w = (size_t)cap, n_t = (size_t)cap, n_v = (size_t)M * (size_t)cap,
                 n_d = 2 * (size_t)cap, n_c = 3 * (size_t)cap, n_ms = 2 * (size_t)R, n_acc = (size_t)L * (size_t)M,
                 n_F = (size_t)M * (size_t)R, n_W = (size_t)R, n_lp = (size_t)L + 1, n_rl = (size_t)R + 1;
    if (int rc = raster_reserve(ctx, n_q + n_w + n_t + n_v + n_d + n_c + n_ms + n_acc + n_F + n_W + n_lp + n_rl, n_q + n_w + n_t))
        return rc;
    double *dq = ctx->raster.as<double>(), *dw = dq + n_q, *dt = dw + n_w, *dv = dt + n_t, *ddm = dv + n_v, *ddsd = ddm + cap;
    long long *dcnt = reinterpret_cast<long long *>(ddm + n_d);
    double *dm = ddm + n_d + n_c, *dsd = dm + R, *dacc = dm + n_ms, *dF = dacc + n_acc, *dW = dF + n_F;
    long long *dlp = reinterpret_cast<long long *>(dW + n_W), *drl = dlp + n_lp;
    double *hw = ctx->h_raster.as<double>() + n_q, *ht = hw + n_w;
    TD_HIP(ctx, hipStreamSynchronize(s));  // (the pinned block and the workspace are free)
    TD_HIP(ctx, hipMemcpyAsync(dlp, leafp.data(), sizeof(long long) * n_lp, hipMemcpyHostToDevice, s));
    TD_HIP(ctx, hipMemcpyAsync(drl, regleaf.data(), sizeof(long long) * n_rl, hipMemcpyHostToDevice, s));
    TD_HIP(ctx, hipMemcpyAsync(dW, W.data(), sizeof(double) * n_W, hipMemcpyHostToDevice, s));
    int64_t *const cnt_out[3] = {w->below_out, w->equal_out, w->above_out};
    int64_t brute_pairs = 0, la = 0;  // la: the first leaf with a point in the slab
    for (int64_t c0 = 0; c0 < np; c0 += plan.nodes) {
        const int64_t ns = std::min(plan.nodes, np - c0);
        if (int rc = stage_queries(ctx, w->px, w->py, w->pz, c0, ns, dq)) return rc;
        if (w->w) {
            std::memcpy(hw, w->w + c0, sizeof(double) * (size_t)ns);
            TD_HIP(ctx, hipMemcpyAsync(dw, hw, sizeof(double) * (size_t)ns, hipMemcpyHostToDevice, s));
        }
        std::memcpy(ht, w->truth + c0, sizeof(double) * (size_t)ns);
        TD_HIP(ctx, hipMemcpyAsync(dt, ht, sizeof(double) * (size_t)ns, hipMemcpyHostToDevice, s));
        if (int rc = volume_sweep(ctx, S, 0, M, dq, ns, dv)) return rc;
        if (!S.grid) brute_pairs += M * ns;
        {
            hipEvent_t t0 = tm ? tm->begin(s) : nullptr;
            hipLaunchKernelGGL(k_recovery_counts, dim3((unsigned)((ns + kRecThreads - 1) / kRecThreads)), dim3(kRecThreads), 0, s, dv,
                               (int)M, (long)ns, dt, (int)(series || dstats), dcnt);
            if (tm) tm->end("recovery_counts", t0, s);
            TD_HIP(ctx, hipGetLastError());
        }
        for (int k = 0; k < 3; ++k)
            if (cnt_out[k])
                TD_HIP(ctx, hipMemcpyAsync(cnt_out[k] + c0, dcnt + k * ns, sizeof(int64_t) * (size_t)ns, hipMemcpyDeviceToHost, s));
        if (dstats) {
            hipEvent_t t0 = tm ? tm->begin(s) : nullptr;
            const hipError_t e = launch_raster_stats(dv, (int)M, (int)ns, ddm, ddsd, s);
            if (tm) tm->end("recovery_dstats", t0, s);
            TD_HIP(ctx, e);
            TD_HIP(ctx, hipMemcpyAsync(w->dmean_out + c0, ddm, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
            TD_HIP(ctx, hipMemcpyAsync(w->dstd_out + c0, ddsd, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
        }
        if (series) {
            while (leafp[(size_t)la + 1] <= c0) ++la;
            int64_t lb = la;  // the last leaf with a point in the slab
            while (leafp[(size_t)lb + 1] < c0 + ns) ++lb;
            hipEvent_t t0 = tm ? tm->begin(s) : nullptr;
            hipLaunchKernelGGL(k_region_sums<RecoveryTerm>, dim3((unsigned)((lb - la + 1) * mgroups)), dim3(kRegTile), 0, s, dv,
                               (long)ns, (int)M, (long)c0, dlp, (long)la, mgroups, w->w ? dw : nullptr, dacc);
            if (tm) tm->end("recovery_sums", t0, s);
            TD_HIP(ctx, hipGetLastError());
        }
        TD_HIP(ctx, hipStreamSynchronize(s));  // the pinned block is packed again for the next slab
    }
    if (series) {
        {
            hipEvent_t t0 = tm ? tm->begin(s) : nullptr;
            hipLaunchKernelGGL(k_region_combine, dim3((unsigned)(R * mblocks)), dim3(256), sizeof(double) * 256 * (size_t)cov_levels(most),
                               s, dacc, (int)M, mblocks, drl, dlp, dW, (int)w->normalize, (long)R, dF);
            if (tm) tm->end("recovery_combine", t0, s);
            TD_HIP(ctx, hipGetLastError());
        }
        // the regions in the place of a slab's columns: the slab is the whole matrix
        const SlabWant want{R, w->mean_out, w->std_out, w->series_out, w->marg, w->conv};
        hipEvent_t t0 = tm ? tm->begin(s) : nullptr;
        const int rc = slab_statistics(ctx, E, want, dF, 0, R, dm, dsd, false, nullptr);
        if (tm) tm->end("raster_stats", t0, s);
        if (rc) return rc;
    }
    TD_HIP(ctx, hipStreamSynchronize(s));
    if (w->weight_out) std::memcpy(w->weight_out, W.data(), sizeof(double) * n_W);
    return volume_counters_finish(ctx, S, brute_pairs);  // (tdt_volume_counters: this call's sweeps)
}

}  // namespace

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_recovery(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                     const double *yCell, const double *zCell, const double *zeta, int64_t nchains,
                                     const int64_t *chain_len, const td_recovery *want) {
    const char *who = "td_rasterize_recovery";
    if (int rc = recovery_check(ctx, want, who)) return rc;
    if (want->conv)
        if (int rc = conv_check_chains(ctx, nchains, chain_len, nmodels, who)) return rc;
    if (int rc = ensemble_check_arrays(ctx, who, nmodels, cell_off, xCell, yCell, zCell, zeta)) return rc;
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    return recovery_core(ctx, who, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta, nchains, chain_len), want);
}

extern "C" int td_history_recovery(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_recovery *want) {
    const char *who = "td_history_recovery";
    if (int rc = recovery_check(ctx, want, who)) return rc;
    Ensemble E;
    if (int rc = ensemble_from_histories(ctx, who, hs, nh, HistoryRule::SameDevice, &E)) return rc;
    if (want->conv)  // (one history with samples is one chain)
        if (int rc = conv_check_chains(ctx, E.nchains, E.chain_len, E.nmodels, who)) return rc;
    if (int rc = ensemble_check_device(ctx, who, E)) return rc;  // (of the first history's device without a context)
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    if (int rc = ensemble_sync_foreign(ctx, E)) return rc;
    return recovery_core(ctx, who, E, want);
}
