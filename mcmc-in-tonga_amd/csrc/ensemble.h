// ensemble.h -- what the posterior entry points (raster.hip, volume.hip, predict.hip, covariance.hip,
// interfaces.hip, regions.hip, support.hip, recovery.hip, and region_sums.h for the last three's shared part)
// share on the host: the ensemble of models a call is about, its checks, the fold of histories into one, the
// order of an entry point's steps (ensemble_entry_arrays, ensemble_entry_histories), and the tail of a slab of
// the value matrix.  Every core function takes a `const Ensemble &` whose every member has been checked by the
// functions here.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "convergence.h"
#include "ctx.h"
#include "history.h"
#include "marginals.h"
#include "volume.h"

namespace tdstar {

struct Ensemble {
    int64_t nmodels = 0;
    const int64_t *cell_off = nullptr;  // host prefix, cell_off[nmodels] = total
    const double *x = nullptr, *y = nullptr, *z = nullptr, *zeta = nullptr;  // host arrays, or all null when segs is set
    const std::vector<td_history *> *segs = nullptr;  // device-resident samples (no empty history), or null
    int64_t nchains = 0;                // 0 / null when the call has none
    const int64_t *chain_len = nullptr;
    // what cell_off / segs / chain_len point to when ensemble_from_histories built it
    std::vector<int64_t> own_off, own_len;
    std::vector<td_history *> own_segs;

    Ensemble() = default;
    Ensemble(int64_t nmodels_, const int64_t *cell_off_, const double *x_, const double *y_, const double *z_,
             const double *zeta_, int64_t nchains_ = 0, const int64_t *chain_len_ = nullptr)
        : nmodels(nmodels_), cell_off(cell_off_), x(x_), y(y_), z(z_), zeta(zeta_), nchains(nchains_), chain_len(chain_len_) {}
    Ensemble(const Ensemble &) = delete;  // (the pointers into its own vectors)
    Ensemble &operator=(const Ensemble &) = delete;
    int64_t total() const { return cell_off[nmodels]; }
};

// The host arrays of a td_rasterize_* call; needs no context and no HIP call (ctx only receives the message).
inline int ensemble_check_arrays(td_ctx *ctx, const char *who, int64_t nmodels, const int64_t *cell_off, const double *x,
                                 const double *y, const double *z, const double *zeta) {
    const std::string w(who);
    if (nmodels < 1 || !cell_off) return set_err(ctx, TD_ERR_ARG, w + ": need nmodels >= 1 and cell_off");
    const int64_t total = cell_off[nmodels];
    if (cell_off[0] != 0 || total < 0 || (total > 0 && (!x || !y || !z || !zeta)))
        return set_err(ctx, TD_ERR_ARG, w + ": bad cell offsets or arrays");
    for (int64_t k = 0; k < nmodels; ++k)
        if (cell_off[k + 1] < cell_off[k]) return set_err(ctx, TD_ERR_ARG, w + ": offsets not monotone");
    return TD_OK;
}

enum class HistoryRule {
    // td_history_rasterize, td_history_marginals, td_history_convergence, td_history_volume: a context and at
    // least one history, every history non-NULL and of that context (refused in this order, before the fold)
    SameContext,
    // td_history_predict, td_history_covariance: any context's histories on the context's device, of which only
    // the cells and offsets are read.  The fold needs no context; the entry point then calls
    // ensemble_check_device and, with a context, ensemble_sync_foreign: every device is checked before any
    // foreign stream is waited for, so a refused call has waited for none.
    SameDevice,
};

// The histories' samples behind one another as one ensemble: the offsets' prefix from the host mirrors, the
// histories that hold samples (an empty one is skipped) and their lengths as the chains.
inline int ensemble_from_histories(td_ctx *ctx, const char *who, td_history *const *hs, int64_t nh, HistoryRule rule,
                                   Ensemble *out) {
    const std::string w(who);
    const bool same = rule == HistoryRule::SameContext;
    if (same && !ctx) return set_err(nullptr, TD_ERR_ARG, w + ": ctx is NULL");
    if (same && (!hs || nh < 1)) return set_err(ctx, TD_ERR_ARG, w + ": no history");
    std::vector<int64_t> &off = out->own_off;
    off.assign(1, 0);
    for (int64_t i = 0; hs && i < nh; ++i) {
        td_history *h = hs[i];
        if (same && (!h || h->ctx != ctx))
            return set_err(ctx, TD_ERR_ARG, w + ": every history must be non-NULL and of this context");
        if (!h) return set_err(ctx, TD_ERR_ARG, w + ": a history is NULL");
        const int64_t base = off.back();
        for (int64_t k = 1; k <= h->samples; ++k) off.push_back(base + h->off[(size_t)k]);
        if (h->samples > 0) {
            out->own_segs.push_back(h);
            out->own_len.push_back(h->samples);
        }
    }
    out->nmodels = (int64_t)off.size() - 1;
    if (out->nmodels < 1) return set_err(ctx, TD_ERR_ARG, w + ": the histories hold no sample");
    out->cell_off = off.data();
    out->segs = &out->own_segs;
    out->nchains = (int64_t)out->own_len.size();
    out->chain_len = out->own_len.data();
    return TD_OK;
}

// HistoryRule::SameDevice: the context's device, or without a context the first history's
inline int ensemble_check_device(td_ctx *ctx, const char *who, const Ensemble &E) {
    const int device = ctx ? ctx->device : (*E.segs)[0]->ctx->device;
    for (const td_history *h : *E.segs)
        if (h->ctx->device != device)
            return set_err(ctx, TD_ERR_ARG, std::string(who) + ": every history must live on the context's device");
    return TD_OK;
}

// HistoryRule::SameDevice: what recorded another context's history has ended
inline int ensemble_sync_foreign(td_ctx *ctx, const Ensemble &E) {
    for (const td_history *h : *E.segs)
        if (h->ctx != ctx) TD_HIP(ctx, hipStreamSynchronize(h->ctx->stream));
    return TD_OK;
}

// The td_rasterize_X / td_history_X pair of covariance, interfaces, regions, support and recovery: the steps of
// an entry point in the order the callers rely on (which refusal comes first is part of the contract).  The array
// form takes the caller's arrays as an unchecked Ensemble.
//   check()  the request's own checks, which need no context
//   conv     the request's convergence part (null: none, or the request itself is NULL): the chains are checked
//   core(E)  the work, on a checked ensemble and a non-NULL context
// Three entry points keep an order of their own and do not come through here: td_rasterize_predict and
// td_history_predict (arrays before chains when models are given, ctx before the device) and td_history_volume
// (HistoryRule::SameContext).
template <class Check, class Core>
int ensemble_entry_arrays(td_ctx *ctx, const char *who, const Ensemble &E, const td_convergence *conv, Check check, Core core) {
    if (int rc = check()) return rc;
    if (conv)
        if (int rc = conv_check_chains(ctx, E.nchains, E.chain_len, E.nmodels, who)) return rc;
    if (int rc = ensemble_check_arrays(ctx, who, E.nmodels, E.cell_off, E.x, E.y, E.z, E.zeta)) return rc;
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    return core(E);
}
template <class Check, class Core>
int ensemble_entry_histories(td_ctx *ctx, const char *who, td_history *const *hs, int64_t nh, const td_convergence *conv,
                             Check check, Core core) {
    if (int rc = check()) return rc;
    Ensemble E;
    if (int rc = ensemble_from_histories(ctx, who, hs, nh, HistoryRule::SameDevice, &E)) return rc;
    if (conv)  // (one history with samples is one chain)
        if (int rc = conv_check_chains(ctx, E.nchains, E.chain_len, E.nmodels, who)) return rc;
    if (int rc = ensemble_check_device(ctx, who, E)) return rc;  // (of the first history's device without a context)
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    if (int rc = ensemble_sync_foreign(ctx, E)) return rc;
    return core(E);
}

// E.segs: each history's packed samples behind the ones before, component by component, into the SoA block dc
// of stride cs
inline int ensemble_copy_segments(td_ctx *ctx, const Ensemble &E, double *dc, int64_t cs, hipStream_t s) {
    int64_t pos = 0;
    for (const td_history *h : *E.segs) {
        const int64_t cnt = h->off[(size_t)h->samples];
        for (int comp = 0; comp < 4 && cnt > 0; ++comp)
            TD_HIP(ctx, hipMemcpyAsync(dc + comp * cs + pos, h->d.cells + comp * h->d.stride, sizeof(double) * (size_t)cnt,
                                       hipMemcpyDeviceToDevice, s));
        pos += cnt;
    }
    return TD_OK;
}

// Points q0 .. q0 + ns of (qx, qy, qz) as the block [3][ns] at the start of the pinned ctx->h_raster, and its
// copy to dq on ctx->stream.  The stream has been waited for since the block's last use.
inline void pack_queries(td_ctx *ctx, const double *qx, const double *qy, const double *qz, int64_t q0, int64_t ns) {
    double *h = ctx->h_raster.as<double>();
    std::memcpy(h, qx + q0, sizeof(double) * (size_t)ns);
    std::memcpy(h + ns, qy + q0, sizeof(double) * (size_t)ns);
    std::memcpy(h + 2 * ns, qz + q0, sizeof(double) * (size_t)ns);
}
inline int stage_queries(td_ctx *ctx, const double *qx, const double *qy, const double *qz, int64_t q0, int64_t ns,
                         double *dq) {
    pack_queries(ctx, qx, qy, qz, q0, ns);
    TD_HIP(ctx, hipMemcpyAsync(dq, ctx->h_raster.p, sizeof(double) * 3 * (size_t)ns, hipMemcpyHostToDevice, ctx->stream));
    return TD_OK;
}

// What a slab's tail writes: the caller's arrays, whose rows hold `row` columns (null: not asked for).
struct SlabWant {
    int64_t row;
    double *mean_out, *std_out, *values_out;
    const td_marginals *marg;
    const td_convergence *conv;
};

// The tail of one slab: the device value matrix vals[E.nmodels][ns] holds the columns q0 .. q0 + ns of the
// caller's outputs.  Mean and standard deviation through dm, dsd [ns]; marginals (hist_out is contiguous per
// column; staged: the quantile rows go through the pinned hquant [nprob][ns] and are scattered after a wait
// for the stream -- not staged: the slab is the whole matrix, they go straight to the caller and nothing is
// waited for); convergence; the matrix itself.
inline int slab_statistics(td_ctx *ctx, const Ensemble &E, const SlabWant &w, const double *vals, int64_t q0, int64_t ns,
                           double *dm, double *dsd, bool staged, double *hquant) {
    hipStream_t s = ctx->stream;
    const int64_t M = E.nmodels;
    const int nprob = w.marg ? (int)w.marg->nprob : 0;
    if (w.mean_out) {
        TD_HIP(ctx, launch_raster_stats(vals, (int)M, (int)ns, dm, dsd, s));
        TD_HIP(ctx, hipMemcpyAsync(w.mean_out + q0, dm, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
        TD_HIP(ctx, hipMemcpyAsync(w.std_out + q0, dsd, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
    }
    if (w.marg) {
        td_marginals mw = *w.marg;
        if (staged) mw.quant_out = nprob > 0 ? hquant : nullptr;
        mw.hist_out = mw.nbins > 0 ? w.marg->hist_out + q0 * (mw.nbins + 3) : nullptr;
        if (int rc = marginals_run(ctx, vals, M, ns, &mw)) return rc;
    }
    if (w.conv) {
        td_convergence cw = *w.conv;
        if (cw.rhat_out) cw.rhat_out += q0;
        if (cw.ess_out) cw.ess_out += q0;
        if (cw.lags_out) cw.lags_out += q0;
        if (int rc = convergence_run(ctx, vals, M, ns, E.nchains, E.chain_len, &cw)) return rc;
    }
    if (w.values_out)
        TD_HIP(ctx, hipMemcpy2DAsync(w.values_out + q0, sizeof(double) * (size_t)w.row, vals, sizeof(double) * (size_t)ns,
                                     sizeof(double) * (size_t)ns, (size_t)M, hipMemcpyDeviceToHost, s));
    if (!staged) return TD_OK;
    TD_HIP(ctx, hipStreamSynchronize(s));  // the pinned block is filled again by the next slab
    for (int p = 0; p < nprob; ++p)
        std::memcpy(w.marg->quant_out + (int64_t)p * w.row + q0, hquant + (int64_t)p * ns, sizeof(double) * (size_t)ns);
    return TD_OK;
}

}  // namespace tdstar
