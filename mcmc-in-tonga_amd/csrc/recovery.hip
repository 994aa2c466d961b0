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
#include <cstring>
#include <string>

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

RegionList region_list(const td_recovery *w) { return {w->px, w->py, w->pz, w->w, w->np, w->reg_off, w->nreg, w->normalize}; }

// the checks of both entry points that need no context and no HIP call, in the header's order
int recovery_check(td_ctx *ctx, const td_recovery *w, const char *who) {
    const std::string n(who);
    if (!w) return set_err(ctx, TD_ERR_ARG, n + ": want is NULL");
    const RegionVector truth{w->truth, "truth"};
    if (int rc = region_list_check(ctx, who, region_list(w), &truth)) return rc;
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
    const int64_t M = E.nmodels, np = w->np, R = w->nreg;
    const RegionList list = region_list(w);
    RegionPlan P;
    if (int rc = region_limits(ctx, who, M, R)) return rc;
    if (int rc = region_plan(ctx, who, M, list, w->marg, &P)) return rc;
    const int64_t cap = P.cap, L = P.L;
    const bool series = wants_series(w), dstats = w->dmean_out != nullptr;
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    hipStream_t s = ctx->stream;
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
    if (int rc = region_upload(ctx, P, dlp, drl, dW)) return rc;
    int64_t *const cnt_out[3] = {w->below_out, w->equal_out, w->above_out};
    int64_t brute_pairs = 0, la = 0;
    for (int64_t c0 = 0; c0 < np; c0 += P.vol.nodes) {
        const int64_t ns = std::min(P.vol.nodes, np - c0);
        if (int rc = stage_queries(ctx, w->px, w->py, w->pz, c0, ns, dq)) return rc;
        if (int rc = region_stage_weights(ctx, list, c0, ns, hw, dw)) return rc;
        std::memcpy(ht, w->truth + c0, sizeof(double) * (size_t)ns);
        TD_HIP(ctx, hipMemcpyAsync(dt, ht, sizeof(double) * (size_t)ns, hipMemcpyHostToDevice, s));
        if (int rc = volume_sweep(ctx, S, 0, M, dq, ns, dv)) return rc;
        if (!S.grid) brute_pairs += M * ns;
        TD_HIP(ctx, timed_launch(ctx, "recovery_counts", [&] {
                   hipLaunchKernelGGL(k_recovery_counts, dim3((unsigned)((ns + kRecThreads - 1) / kRecThreads)), dim3(kRecThreads), 0,
                                      s, dv, (int)M, (long)ns, dt, (int)(series || dstats), dcnt);
               }));
        for (int k = 0; k < 3; ++k)
            if (cnt_out[k])
                TD_HIP(ctx, hipMemcpyAsync(cnt_out[k] + c0, dcnt + k * ns, sizeof(int64_t) * (size_t)ns, hipMemcpyDeviceToHost, s));
        if (dstats) {
            TD_HIP(ctx, timed_launch(ctx, "recovery_dstats", [&] { return launch_raster_stats(dv, (int)M, (int)ns, ddm, ddsd, s); }));
            TD_HIP(ctx, hipMemcpyAsync(w->dmean_out + c0, ddm, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
            TD_HIP(ctx, hipMemcpyAsync(w->dstd_out + c0, ddsd, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
        }
        if (series)
            if (int rc = region_sums_slab<RecoveryTerm>(ctx, "recovery_sums", P, c0, ns, dv, w->w ? dw : nullptr, dlp, dacc, &la))
                return rc;
        TD_HIP(ctx, hipStreamSynchronize(s));  // the pinned block is packed again for the next slab
    }
    if (series) {
        if (int rc = region_combine(ctx, "recovery_combine", P, dacc, drl, dlp, dW, (int)w->normalize, dF)) return rc;
        if (int rc = region_tail(ctx, E, SlabWant{R, w->mean_out, w->std_out, w->series_out, w->marg, w->conv}, dF, dm, dsd)) return rc;
    }
    return region_finish(ctx, P, S, brute_pairs, w->weight_out);
}

}  // namespace

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_recovery(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                     const double *yCell, const double *zCell, const double *zeta, int64_t nchains,
                                     const int64_t *chain_len, const td_recovery *want) {
    const char *who = "td_rasterize_recovery";
    return ensemble_entry_arrays(
        ctx, who, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta, nchains, chain_len), want ? want->conv : nullptr,
        [&] { return recovery_check(ctx, want, who); }, [&](const Ensemble &E) { return recovery_core(ctx, who, E, want); });
}

extern "C" int td_history_recovery(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_recovery *want) {
    const char *who = "td_history_recovery";
    return ensemble_entry_histories(
        ctx, who, hs, nh, want ? want->conv : nullptr, [&] { return recovery_check(ctx, want, who); },
        [&](const Ensemble &E) { return recovery_core(ctx, who, E, want); });
}
