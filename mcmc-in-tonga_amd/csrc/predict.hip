// predict.hip -- posterior predictive data: td_evaluate's t* of every model of an ensemble on the rays of a
// context, its chi^2, and the statistics of the matrix ptS[nmodels][n] over the models.
//
// The search structure is the volume's (volume_build: one bucket grid per model, built once for all models
// where they lie), the queries are the context's ray points, which are on the device already:
//   per slab (a run of whole consecutive rays, predict_plan) the points' [3][ns] block is filled by device
//   to device copies, and per chunk of models
//     volume_sweep      V_slab[models of the chunk][ns]: zeta of the nearest cell (td_evaluate's rule: the
//                       lexicographic minimum of (FP64 squared distance, index) below the sentinel);
//     k_pred_ray_sums   work item = (model, ray of the slab), one wave each: wave_ray_sum (ray_sum.h, Julia's
//                       Base.sum association) on the model's row of V_slab -> ptS[model][ray];
//   k_pred_chi2         one lane per model: C = C + ((ptS - tS)^2 * 1.0) / sig^2 in ray order, td_evaluate's
//                       host loop (api.cpp host_chi2) operation for operation.
// ptS[nmodels][n] is the one matrix kept whole; k_raster_stats, marginals_run and convergence_run take it
// as a value matrix (in ray slabs gathered by strided copies where volume_plan allows no single one).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "convergence.h"
#include "ctx.h"
#include "ensemble.h"
#include "history.h"
#include "marginals.h"
#include "predict.h"
#include "ray_sum.h"
#include "volume.h"

namespace tdstar {

namespace {

constexpr int kPredWaves = 4;            // rays per workgroup of k_pred_ray_sums
constexpr int kPredPending = 16;         // left halves a pairwise sum of <= 2^18 terms holds at most (9)
constexpr int kPredScratch = 96 + kPredPending;  // wave_ray_sum's 96 doubles | the pending left halves
constexpr int kPredXcds = 8;

// wave_ray_sum for a ray of any length without a per-lane stack: up to 1024 segments it IS wave_ray_sum;
// beyond, Julia's pairwise split (mapreduce_impl: [f, l] at f + ((l - f) >> 1) while l - f >= 1024) is
// walked leaf by leaf, each leaf of 512 .. 1024 segments summed by wave_ray_sum itself (the association of
// julia_block_lane, 32 accumulators wide), the finished left halves waiting in LDS.  The node is found
// again from the root along `path` (bit d: the right child at depth d), at most 9 steps per leaf.
// Result on lane 0.
template <class Z>
__device__ __forceinline__ double pred_ray_sum(int lane, const double *__restrict__ w, const Z &zeta, int s0, int np,
                                               double *scratch) {
    const int L = np > 0 ? np - 1 : 0;
    if (L <= 1024) return wave_ray_sum(lane, w, zeta, s0, min(np, 1025), scratch);
    double *pend = scratch + 96;
    unsigned path = 0;
    int depth = 0, nv = 0;
    double v;
    for (;;) {
        int f = 0, l = L - 1;
        for (int d = 0; d < depth; ++d) {
            const int mid = f + ((l - f) >> 1);
            if ((path >> d) & 1u)
                f = mid + 1;
            else
                l = mid;
        }
        while (l - f >= 1024) {  // down the left children to a leaf
            l = f + ((l - f) >> 1);
            path &= ~(1u << depth);
            ++depth;
        }
        v = wave_ray_sum(lane, w, zeta, s0 + f, min(l - f + 2, 1025), scratch);  // segments f .. l
        while (depth > 0 && ((path >> (depth - 1)) & 1u)) {  // a right child: its parent is left + right
            --nv;
            if (lane == 0) v = pend[nv] + v;
            --depth;
        }
        if (depth == 0) break;
        if (lane == 0) pend[nv] = v;  // a left child waits for its sibling
        ++nv;
        path |= 1u << (depth - 1);
    }
    return v;
}

// V = V_slab[nm][ns] (the slab's points p0 .. p0 + ns of every model of the chunk), rays r0 .. r0 + nr of
// the context; rb = ceil(nr / 4) workgroups per model.  XCD: the workgroups of model m run on XCD m % 8
// (k_vol_search's mapping, which wrote the row into that XCD's L2); else a model's workgroups follow each
// other.  ptS: row 0 = the chunk's first model, n doubles a row.
template <bool XCD>
__global__ __launch_bounds__(64 * kPredWaves) void k_pred_ray_sums(const int *__restrict__ ray_off, int r0, int nr, int p0,
                                                                   const double *__restrict__ w,
                                                                   const double *__restrict__ V, int ns, int nm, int rb,
                                                                   double *__restrict__ ptS, long n) {
    __shared__ double scratch[kPredWaves][kPredScratch];
    int m, rblk;
    if (XCD) {
        const int Lb = blockIdx.x, xcd = Lb % kPredXcds, j = Lb / kPredXcds;
        m = xcd + kPredXcds * (j / rb);
        rblk = j % rb;
        if (m >= nm) return;
    } else {
        m = blockIdx.x / rb;
        rblk = blockIdx.x % rb;
    }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ray = rblk * kPredWaves + wv;
    if (ray >= nr) return;  // wave-uniform; no block barrier below
    const int a = ray_off[r0 + ray];
    const int np = ray_off[r0 + ray + 1] - a;
    const double r = pred_ray_sum(lane, w + p0, PlainZeta{V + (long)m * ns}, a - p0, np, scratch[wv]);
    if (lane == 0) ptS[(long)m * n + r0 + ray] = r;  // rays of 0 and 1 points: 0.0
}

// MCsub.jl:169-172 per model, one lane each: strictly sequential in k, every operation an IEEE double one.
__global__ __launch_bounds__(64) void k_pred_chi2(const double *__restrict__ ptS, const double *__restrict__ tS,
                                                  const double *__restrict__ sig, int n, long nmodels,
                                                  double *__restrict__ phi) {
    const long m = (long)blockIdx.x * 64 + threadIdx.x;
    if (m >= nmodels) return;
    const double *__restrict__ p = ptS + m * n;
    double C = 0.0;
    for (int k = 0; k < n; ++k) {
        const double d = p[k] - tS[k];
        const double s = sig[k];
        C = C + ((d * d) * 1.0) / (s * s);  // MCsub.jl:171
    }
    phi[m] = C;
}

// the checks of both entry points that need no context and no HIP call
int predict_check(td_ctx *ctx, const td_predict *out, const char *who) {
    const std::string w(who);
    if (!out) return set_err(ctx, TD_ERR_ARG, w + ": out is NULL");
    if (!out->ptS_out && !out->phi_out && !out->mean_out && !out->std_out && !out->marg && !out->conv)
        return set_err(ctx, TD_ERR_ARG, w + ": nothing asked for");
    if (!out->mean_out != !out->std_out) return set_err(ctx, TD_ERR_ARG, w + ": mean_out and std_out must be given together");
    if (out->marg)
        if (int rc = marg_check_want(ctx, out->marg, who)) return rc;
    if (out->conv)
        if (int rc = conv_check_want(ctx, out->conv, who)) return rc;
    return TD_OK;
}

// Both entry points; E and out have been checked (ensemble.h, predict_check).
int predict_core(td_ctx *ctx, const char *who, const Ensemble &E, const td_predict *out) {
    const std::string w(who);
    const int64_t nmodels = E.nmodels;
    const int64_t n = ctx->g.n;
    const std::vector<int> &roff = ctx->ray_off_host;
    std::vector<int64_t> ray_points((size_t)n);
    for (int64_t i = 0; i < n; ++i) ray_points[(size_t)i] = roff[(size_t)i + 1] - roff[(size_t)i];
    PredPlan plan;
    if (!predict_plan(nmodels, n, ray_points.data(), kVolDefaultBudget, ctx->pred_slab_points, ctx->pred_model_chunk, &plan))
        return set_err(ctx, TD_ERR_ARG, w + ": a ray of more than 2^18 points");
    if (n == 0) {  // td_evaluate_batch on no rays: chi^2 = 0 (MCsub.jl:169), nothing else to say
        if (out->phi_out) std::fill(out->phi_out, out->phi_out + nmodels, 0.0);
        return TD_OK;
    }
    if (int rc = marg_check_models(ctx, out->marg, nmodels)) return rc;  // (before anything is issued)
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    hipStream_t s = ctx->stream;
    Timer *tm = ctx->timer.on ? &ctx->timer : nullptr;
    const auto &g = ctx->g;
    // the statistics' slabs of rays (one, the matrix itself, wherever volume_plan allows it)
    const bool stats = out->mean_out || out->marg || out->conv;
    const VolPlan sp = volume_plan(nmodels, n, kVolDefaultBudget, ctx->vol_slab_nodes);
    const bool gather = stats && sp.nodes < n;
    const int nprob = out->marg ? (int)out->marg->nprob : 0;
    // ctx->pred: ptS [nmodels][n] | phi [nmodels] | mean, std [n]
    if (int rc = grow(ctx, ctx->pred, sizeof(double) * ((size_t)nmodels * (size_t)n + (size_t)nmodels + 2 * (size_t)n))) return rc;
    double *dptS = ctx->pred.as<double>(), *dphi = dptS + nmodels * n, *dm = dphi + nmodels, *dsd = dm + n;
    // ctx->raster: the slab's points [3][points] | V_slab [chunk][points] | a gathered slab of ptS
    int64_t maxpts = 0;
    for (size_t k = 0; k + 1 < plan.edges.size(); ++k)
        maxpts = std::max<int64_t>(maxpts, roff[(size_t)plan.edges[k + 1]] - roff[(size_t)plan.edges[k]]);
    const size_t n_sweep = (size_t)maxpts * (3 + (size_t)plan.chunk), n_gather = gather ? (size_t)nmodels * (size_t)sp.nodes : 0;
    if (int rc = raster_reserve(ctx, std::max<size_t>(n_sweep + n_gather, 1), gather ? (size_t)nprob * (size_t)sp.nodes : 0))
        return rc;
    double *dq = ctx->raster.as<double>(), *dv = dq + 3 * maxpts, *dg = dq + n_sweep;
    int64_t brute_pairs = 0;
    for (size_t k = 0; k + 1 < plan.edges.size(); ++k) {
        const int64_t r0 = plan.edges[k], nr = plan.edges[k + 1] - r0;
        const int64_t p0 = roff[(size_t)r0], ns = roff[(size_t)(r0 + nr)] - p0;
        if (ns > 0) {
            const double *src[3] = {g.px, g.py, g.pz};
            for (int d = 0; d < 3; ++d)
                TD_HIP(ctx, hipMemcpyAsync(dq + d * ns, src[d] + p0, sizeof(double) * (size_t)ns, hipMemcpyDeviceToDevice, s));
        }
        const int64_t rb = (nr + kPredWaves - 1) / kPredWaves;
        for (int64_t m0 = 0; m0 < nmodels; m0 += plan.chunk) {
            const int64_t nm = std::min(plan.chunk, nmodels - m0);
            if (ns > 0) {  // (a slab of rays without points has nothing to search: its sums are 0.0)
                if (int rc = volume_sweep(ctx, S, m0, nm, dq, ns, dv)) return rc;
                if (!S.grid) brute_pairs += nm * ns;
            }
            // one launch's workgroups fit 32 bits: as many models of the chunk at a time
            const int64_t per = std::max<int64_t>(kPredXcds, ((int64_t)1 << 30) / rb / kPredXcds * kPredXcds);
            for (int64_t a = 0; a < nm; a += per) {
                const int64_t na = std::min(per, nm - a);
                hipEvent_t t0 = tm ? tm->begin(s) : nullptr;
                if (ctx->pred_placement)
                    hipLaunchKernelGGL(k_pred_ray_sums<true>, dim3((unsigned)(kPredXcds * ((na + kPredXcds - 1) / kPredXcds) * rb)),
                                       dim3(64 * kPredWaves), 0, s, g.ray_off, (int)r0, (int)nr, (int)p0, g.w, dv + a * ns,
                                       (int)ns, (int)na, (int)rb, dptS + (m0 + a) * n, (long)n);
                else
                    hipLaunchKernelGGL(k_pred_ray_sums<false>, dim3((unsigned)(na * rb)), dim3(64 * kPredWaves), 0, s, g.ray_off,
                                       (int)r0, (int)nr, (int)p0, g.w, dv + a * ns, (int)ns, (int)na, (int)rb,
                                       dptS + (m0 + a) * n, (long)n);
                if (tm) tm->end("pred_ray_sums", t0, s);
                TD_HIP(ctx, hipGetLastError());
            }
        }
    }
    if (out->phi_out) {
        hipEvent_t t0 = tm ? tm->begin(s) : nullptr;
        hipLaunchKernelGGL(k_pred_chi2, dim3((unsigned)((nmodels + 63) / 64)), dim3(64), 0, s, dptS, g.tS, g.sig, (int)n,
                           (long)nmodels, dphi);
        if (tm) tm->end("pred_chi2", t0, s);
        TD_HIP(ctx, hipGetLastError());
        TD_HIP(ctx, hipMemcpyAsync(out->phi_out, dphi, sizeof(double) * (size_t)nmodels, hipMemcpyDeviceToHost, s));
    }
    if (out->ptS_out)
        TD_HIP(ctx, hipMemcpyAsync(out->ptS_out, dptS, sizeof(double) * (size_t)nmodels * (size_t)n, hipMemcpyDeviceToHost, s));
    // a gathered slab's quantile rows go through the pinned block
    const SlabWant want{n, out->mean_out, out->std_out, nullptr, out->marg, out->conv};
    for (int64_t q0 = 0; stats && q0 < n; q0 += sp.nodes) {
        const int64_t ns = std::min(sp.nodes, n - q0);
        const double *vals = dptS;
        if (gather) {  // columns q0 .. q0 + ns of ptS as a matrix of their own
            TD_HIP(ctx, hipMemcpy2DAsync(dg, sizeof(double) * (size_t)ns, dptS + q0, sizeof(double) * (size_t)n,
                                         sizeof(double) * (size_t)ns, (size_t)nmodels, hipMemcpyDeviceToDevice, s));
            vals = dg;
        }
        if (int rc = slab_statistics(ctx, E, want, vals, q0, ns, dm, dsd, gather, ctx->h_raster.as<double>())) return rc;
    }
    TD_HIP(ctx, hipStreamSynchronize(s));
    return volume_counters_finish(ctx, S, brute_pairs);  // (tdt_volume_counters: the last call's, this one's sweeps too)
}

}  // namespace

bool predict_plan(int64_t nmodels, int64_t n, const int64_t *ray_points, int64_t budget, int64_t forced_points,
                  int64_t forced_chunk, PredPlan *plan) {
    const int64_t nm = std::max<int64_t>(nmodels, 1), b = budget > 0 ? budget : kVolDefaultBudget;
    int64_t longest = 0;
    for (int64_t i = 0; i < n; ++i) longest = std::max(longest, ray_points[i]);
    if (longest > kPredMaxSlabPoints) return false;
    int64_t pts = forced_points > 0 ? forced_points / kPredTile * kPredTile : b / 8 / nm / kPredTile * kPredTile;
    pts = std::max(pts, kPredTile);
    pts = std::max(pts, (longest + kPredTile - 1) / kPredTile * kPredTile);
    pts = std::min(pts, kPredMaxSlabPoints);
    int64_t chunk = forced_chunk > 0 ? forced_chunk : (nm <= b / 8 / pts ? nm : std::max<int64_t>(1, b / (8 * pts)));
    chunk = std::min(std::min(chunk, nm), kPredMaxChunk);
    plan->points = pts;
    plan->chunk = chunk;
    plan->edges.assign(1, 0);
    int64_t used = 0;
    for (int64_t i = 0; i < n; ++i) {  // greedily: a slab ends before the ray that would overfill it
        if (i > plan->edges.back() && (used + ray_points[i] > pts || i - plan->edges.back() == kPredMaxSlabRays)) {
            plan->edges.push_back(i);
            used = 0;
        }
        used += ray_points[i];
    }
    if (n > 0) plan->edges.push_back(n);
    return true;
}

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_predict(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                    const double *yCell, const double *zCell, const double *zeta, int64_t nchains,
                                    const int64_t *chain_len, const td_predict *out) {
    const char *who = "td_rasterize_predict";
    if (int rc = predict_check(ctx, out, who)) return rc;
    const bool given = nmodels >= 1 && cell_off;  // (the chains are checked before the refusal of no models)
    if (given)  // models and offsets are there: the arrays' refusals come before the chains'
        if (int rc = ensemble_check_arrays(ctx, who, nmodels, cell_off, xCell, yCell, zCell, zeta)) return rc;
    if (out->conv)
        if (int rc = conv_check_chains(ctx, nchains, chain_len, std::max<int64_t>(nmodels, 0), who)) return rc;
    // no models or no offsets: refused after the chains, in ensemble_check_arrays' words
    if (!given) return ensemble_check_arrays(ctx, who, nmodels, cell_off, xCell, yCell, zCell, zeta);
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    return predict_core(ctx, who, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta, nchains, chain_len), out);
}

extern "C" int td_history_predict(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_predict *out) {
    const char *who = "td_history_predict";
    if (int rc = predict_check(ctx, out, who)) return rc;
    Ensemble E;
    if (int rc = ensemble_from_histories(ctx, who, hs, nh, HistoryRule::SameDevice, &E)) return rc;
    if (out->conv)
        if (int rc = conv_check_chains(ctx, E.nchains, E.chain_len, E.nmodels, who)) return rc;
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    if (int rc = ensemble_check_device(ctx, who, E)) return rc;
    if (int rc = ensemble_sync_foreign(ctx, E)) return rc;
    return predict_core(ctx, who, E, out);
}

extern "C" int tdt_predict_plan(int64_t nmodels, int64_t n, const int64_t *ray_points, int64_t budget,
                                int64_t forced_points, int64_t forced_chunk, int64_t out[3], int64_t *edges) {
    if (!out || nmodels < 1 || n < 0 || (n > 0 && !ray_points) || budget < 0 || forced_points < 0 || forced_chunk < 0)
        return TD_ERR_ARG;
    for (int64_t i = 0; i < n; ++i)
        if (ray_points[i] < 0) return TD_ERR_ARG;
    PredPlan p;
    if (!predict_plan(nmodels, n, ray_points, budget, forced_points, forced_chunk, &p)) return TD_ERR_ARG;
    out[0] = p.points;
    out[1] = p.chunk;
    out[2] = (int64_t)p.edges.size() - 1;
    if (edges) std::memcpy(edges, p.edges.data(), sizeof(int64_t) * p.edges.size());
    return TD_OK;
}

extern "C" int tdt_set_predict_plan(td_ctx *ctx, int64_t slab_points, int64_t model_chunk) {
    if (!ctx || slab_points < 0 || model_chunk < 0) return TD_ERR_ARG;
    ctx->pred_slab_points = slab_points;
    ctx->pred_model_chunk = model_chunk;
    return TD_OK;
}

extern "C" int tdt_set_predict_placement(td_ctx *ctx, int xcd) {
    if (!ctx || xcd < 0 || xcd > 1) return TD_ERR_ARG;
    ctx->pred_placement = xcd;
    return TD_OK;
}
