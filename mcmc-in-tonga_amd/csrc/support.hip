// support.hip -- posterior data support: per model and cell the (weighted) ray points of the context the cell
// owns, and that number painted back on a node list through the owning cell, with the statistics of a posterior
// volume on the painted matrix (include/tdstar_support.h holds the contract).
//
// The volume's sweep returns, per (model, query), component 3 of the winning cell of the volume's cell block, so
// both directions use the search unchanged (volume_build once, volume_sweep per slab): with the cell's index
// there it says who owns a ray point, with the cell's support there it paints the support on the nodes.  The
// search rule is td_rasterize's by construction.
//   k_sup_index    one workgroup per model: component 3 = (double)(local index + 1); 0.0 stays "no owner".
//   (ray-point slabs: volume_plan with the context's P points in the place of the nodes, the block [3][ns] filled
//    device to device as predict.hip fills it; volume_sweep -> I[M][ns])
//   k_sup_scatter  one workgroup per model and slab: K[cell] += k[p], count[cell] += 1 for the slab's points.  The
//                  weights were quantised to int64 on the host (support_quantise), so every sum is an integer sum:
//                  any order, either path and any slab size give the same bits.  While the model's cells fit
//                  kSupLdsCells the adds are LDS atomics (ds_add_u64 / ds_add_u32: consecutive points of a ray
//                  share their owner, so the lanes of a wave meet on few words, which must not be global ones)
//                  and the workgroup flushes once per slab with plain read-add-write stores: no other workgroup
//                  touches the model's range, and the slabs follow each other on the stream.  Above the cap the
//                  atomics go to the global arrays.  Orphans (points without owner) are counted per wave by ballot.
//   k_sup_finish   one workgroup per model: sup = ldexp((double)K, -e) into component 3, barren[m], and count as
//                  int64 where asked.
//   (node slabs: the volume's own; volume_sweep -> U_slab[M][ns], then slab_statistics)
//   k_sup_exceed   one lane per node and four thresholds, the models in model order (a row of U_slab per step,
//                  coalesced): int64 counters [nthr][ns].
// The scatter mode of tdt_set_support_scatter is kept beside the context in this unit: a field of td_ctx would
// change the layout every other unit is compiled against.
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

#include "../../include/tdstar_support.h"
#include "ctx.h"
#include "ensemble.h"
#include "history.h"
#include "volume.h"

namespace tdstar {

namespace {

constexpr int kSupThreads = 256;
// 8 + 4 bytes of LDS per cell: 60 KiB, so that two workgroups share the 160 KiB of a CU
constexpr int kSupLdsCells = 5120;
constexpr int kSupThr = 4;  // thresholds a lane of k_sup_exceed counts at once
constexpr int64_t kSupMaxAccumulators = kVolDefaultBudget;  // bytes of K and count over all models' cells

std::mutex g_mode_lock;
std::unordered_map<const td_ctx *, int> g_mode;  // contexts whose scatter mode is not 0

int scatter_mode(const td_ctx *ctx) {
    std::lock_guard<std::mutex> hold(g_mode_lock);
    const auto it = g_mode.find(ctx);
    return it == g_mode.end() ? 0 : it->second;
}

__global__ __launch_bounds__(kSupThreads) void k_sup_index(const int64_t *__restrict__ off, double *__restrict__ comp3) {
    const int64_t a = off[blockIdx.x];
    const int nc = (int)(off[blockIdx.x + 1] - a);
    for (int i = threadIdx.x; i < nc; i += kSupThreads) comp3[a + i] = (double)(i + 1);
}

// I = I[M][ns]: (the owner's local index + 1) of the slab's points, 0.0: none.  kq [ns]: the slab's quantised
// weights (null: 1).  Dynamic LDS: K [lds_cells] | count [lds_cells]; a model of more cells adds globally.
__global__ __launch_bounds__(kSupThreads) void k_sup_scatter(const double *__restrict__ I, int ns,
                                                             const int64_t *__restrict__ off,
                                                             const long long *__restrict__ kq, int lds_cells,
                                                             unsigned long long *__restrict__ Kg,
                                                             unsigned *__restrict__ Cg,
                                                             unsigned long long *__restrict__ orphans) {
    extern __shared__ unsigned long long sK[];
    __shared__ unsigned s_lost;
    unsigned *sC = reinterpret_cast<unsigned *>(sK + lds_cells);
    const int m = blockIdx.x, t = threadIdx.x;
    const int64_t a = off[m];
    const int nc = (int)(off[m + 1] - a);
    const bool lds = nc <= lds_cells;  // (uniform over the workgroup)
    if (lds)
        for (int i = t; i < nc; i += kSupThreads) {
            sK[i] = 0;
            sC[i] = 0;
        }
    if (t == 0) s_lost = 0;
    __syncthreads();
    const double *__restrict__ row = I + (long)m * ns;
    unsigned lost = 0;  // the wave's orphans, the same number on every lane
    for (int p0 = 0; p0 < ns; p0 += kSupThreads) {  // (the same trips for every lane: the ballot sees whole waves)
        const int p = p0 + t;
        const bool live = p < ns;
        const int idx = live ? (int)row[p] - 1 : -1;
        const bool owned = idx >= 0 && idx < nc;
        if (owned) {
            const unsigned long long k = kq ? (unsigned long long)kq[p] : 1ull;  // (two's complement: a negative weight subtracts)
            if (lds) {
                atomicAdd(&sK[idx], k);
                atomicAdd(&sC[idx], 1u);
            } else {
                atomicAdd(&Kg[a + idx], k);
                atomicAdd(&Cg[a + idx], 1u);
            }
        }
        lost += (unsigned)__popcll(__ballot(live && !owned));
    }
    if ((t & 63) == 0 && lost) atomicAdd(&s_lost, lost);
    __syncthreads();
    if (lds)
        for (int i = t; i < nc; i += kSupThreads) {
            const unsigned c = sC[i];
            if (c) {  // (this workgroup alone holds the model's range during the launch)
                Kg[a + i] += sK[i];
                Cg[a + i] += c;
            }
        }
    if (t == 0 && s_lost) orphans[m] += s_lost;
}

__global__ __launch_bounds__(kSupThreads) void k_sup_finish(const int64_t *__restrict__ off,
                                                            const long long *__restrict__ Kg,
                                                            const unsigned *__restrict__ Cg, int e,
                                                            double *__restrict__ comp3, long long *__restrict__ count64,
                                                            long long *__restrict__ barren) {
    __shared__ unsigned s_barren;
    const int m = blockIdx.x, t = threadIdx.x;
    const int64_t a = off[m];
    const int nc = (int)(off[m + 1] - a);
    if (t == 0) s_barren = 0;
    __syncthreads();
    unsigned nb = 0;
    for (int i = t; i < nc; i += kSupThreads) {
        const unsigned c = Cg[a + i];
        comp3[a + i] = ldexp((double)Kg[a + i], -e);
        if (count64) count64[a + i] = (long long)c;
        nb += c == 0;
    }
    if (nb) atomicAdd(&s_barren, nb);
    __syncthreads();
    if (t == 0) barren[m] = (long long)s_barren;
}

// U = U_slab[M][ns]; out [nthr][ns].  Workgroup (x: 256 nodes, y: groups of kSupThr thresholds).
__global__ __launch_bounds__(kSupThreads) void k_sup_exceed(const double *__restrict__ U, int M, int ns,
                                                            const double *__restrict__ thr, int nthr,
                                                            long long *__restrict__ out) {
    const int q = blockIdx.x * kSupThreads + threadIdx.x;
    if (q >= ns) return;
    for (int t0 = blockIdx.y * kSupThr; t0 < nthr; t0 += gridDim.y * kSupThr) {
        double th[kSupThr];
        unsigned c[kSupThr];
#pragma unroll
        for (int j = 0; j < kSupThr; ++j) {
            th[j] = t0 + j < nthr ? thr[t0 + j] : HUGE_VAL;  // (nothing exceeds it)
            c[j] = 0;
        }
#pragma unroll 8
        for (int m = 0; m < M; ++m) {
            const double v = U[(long)m * ns + q];
#pragma unroll
            for (int j = 0; j < kSupThr; ++j) c[j] += v > th[j];
        }
#pragma unroll
        for (int j = 0; j < kSupThr; ++j)
            if (t0 + j < nthr) out[(long)(t0 + j) * ns + q] = (long long)c[j];
    }
}

// The quantisation of the header, pure host code: k [n] and e.  -> null, or what is not finite.
const char *support_quantise(const double *w, int64_t n, long long *k, int *e_out) {
    double A = 0.0;
    for (int64_t p = 0; p < n; ++p) {
        if (!std::isfinite(w[p])) return "w is not finite";
        A = A + std::fabs(w[p]);
    }
    if (!std::isfinite(A)) return "the sum of |w| is not finite";
    int E = 0;
    (void)std::frexp(A, &E);
    const int e = A == 0.0 ? 0 : 61 - E;
    for (int64_t p = 0; p < n; ++p) k[p] = std::llrint(std::ldexp(w[p], e));  // (to nearest even: the default mode)
    *e_out = e;
    return nullptr;
}

bool wants_nodes(const td_support *w) {
    return w->values_out || w->mean_out || w->std_out || w->nthr > 0 || w->marg || w->conv;
}

// The checks of both entry points that need no HIP call, in the header's order; with a context the weights are
// quantised on the way (kq, e; kq stays empty for w == NULL).
int support_check(td_ctx *ctx, const td_support *w, const char *who, std::vector<long long> *kq, int *e) {
    const std::string n(who);
    if (!w) return set_err(ctx, TD_ERR_ARG, n + ": want is NULL");
    if (w->nq < 0) return set_err(ctx, TD_ERR_ARG, n + ": nq must be >= 0");
    if (w->nq > 0 && (!w->qx || !w->qy || !w->qz)) return set_err(ctx, TD_ERR_ARG, n + ": qx, qy and qz must be given for nq > 0");
    if (w->nthr < 0) return set_err(ctx, TD_ERR_ARG, n + ": nthr must be >= 0");
    if (w->nthr > 0 && (!w->thr || !w->exceed_out))
        return set_err(ctx, TD_ERR_ARG, n + ": thr and exceed_out must be given for nthr > 0");
    const double *vec[4] = {w->qx, w->qy, w->qz, w->thr};
    const int64_t len[4] = {w->nq, w->nq, w->nq, w->nthr};
    const char *name[4] = {"qx", "qy", "qz", "thr"};
    for (int a = 0; a < 4; ++a)
        for (int64_t i = 0; i < len[a]; ++i)
            if (!std::isfinite(vec[a][i])) return set_err(ctx, TD_ERR_ARG, n + ": " + name[a] + " is not finite");
    *e = 0;
    if (ctx && w->w) {
        kq->resize((size_t)ctx->g.P);
        if (const char *bad = support_quantise(w->w, ctx->g.P, kq->data(), e)) return set_err(ctx, TD_ERR_ARG, n + ": " + bad);
    }
    if (!w->cell_out && !w->count_out && !w->barren_out && !w->orphans_out && !wants_nodes(w))
        return set_err(ctx, TD_ERR_ARG, n + ": no output asked for");
    if (w->nq == 0 && wants_nodes(w)) return set_err(ctx, TD_ERR_ARG, n + ": an output that needs nodes with nq == 0");
    if (!w->mean_out != !w->std_out) return set_err(ctx, TD_ERR_ARG, n + ": mean_out and std_out must be given together");
    if (w->marg)
        if (int rc = marg_check_want(ctx, w->marg, who)) return rc;
    if (w->conv)
        if (int rc = conv_check_want(ctx, w->conv, who)) return rc;
    return TD_OK;
}

// Both entry points; E and w have been checked (ensemble.h, support_check).
int support_core(td_ctx *ctx, const char *who, const Ensemble &E, const td_support *w, const std::vector<long long> &kq, int e) {
    const std::string n(who);
    const int64_t M = E.nmodels, total = E.total(), P = ctx->g.P, nthr = w->nthr;
    const int64_t nq = wants_nodes(w) ? w->nq : 0;  // (nodes nobody reads are not swept)
    if (total > kSupMaxAccumulators / 12)
        return set_err(ctx, TD_ERR_ARG, n + ": the accumulators of all cells (12 bytes each) exceed 1 GiB");
    if (int rc = marg_check_models(ctx, w->marg, M)) return rc;  // (before anything is issued)
    int64_t most = 0;  // the most cells of a model
    for (int64_t m = 0; m < M; ++m) most = std::max(most, E.cell_off[m + 1] - E.cell_off[m]);
    const int mode = scatter_mode(ctx);
    const int lds_cells = mode == 2 ? 0 : (int)std::min<int64_t>(most, kSupLdsCells);
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    hipStream_t s = ctx->stream;
    const VolPlan pp = volume_plan(M, P, kVolDefaultBudget, ctx->vol_slab_nodes);
    const VolPlan qp = volume_plan(M, nq, kVolDefaultBudget, ctx->vol_slab_nodes);
    const int64_t capp = std::min(pp.nodes, P), capq = std::min(qp.nodes, nq), cap = std::max<int64_t>(std::max(capp, capq), 1);
    const int nprob = w->marg ? (int)w->marg->nprob : 0;
    // ctx->raster (8-byte words): queries [3][cap] | I or U_slab [M][cap] | mean, std [capq] | k [P] | K [total] |
    // count [total] (32 bits each) | count as int64 [total] | barren, orphans [M] | counters [nthr][capq] | thr [nthr];
    // pinned: queries | quantile rows
    const size_t n_q = 3 * (size_t)cap, n_v = (size_t)M * (size_t)cap, n_ms = 2 * (size_t)capq, n_k = kq.size(),
                 n_K = (size_t)total, n_C = ((size_t)total + 1) / 2, n_c64 = w->count_out ? (size_t)total : 0,
                 n_bo = 2 * (size_t)M, n_ex = (size_t)nthr * (size_t)capq, n_thr = (size_t)nthr;
    if (int rc = raster_reserve(ctx, n_q + n_v + n_ms + n_k + n_K + n_C + n_c64 + n_bo + n_ex + n_thr,
                                (size_t)cap * 3 + (size_t)capq * (size_t)nprob))
        return rc;
    double *dq = ctx->raster.as<double>(), *dv = dq + n_q, *dm = dv + n_v, *dsd = dm + capq;
    long long *dk = reinterpret_cast<long long *>(dm + n_ms), *dK = dk + n_k;
    unsigned *dC = reinterpret_cast<unsigned *>(dK + n_K);
    long long *dc64 = dK + n_K + n_C, *dbar = dc64 + n_c64, *dorph = dbar + M, *dex = dorph + M;
    double *dthr = reinterpret_cast<double *>(dex + n_ex);
    double *comp3 = S.cells + 3 * S.cs;
    TD_HIP(ctx, hipStreamSynchronize(s));  // (the pinned block and the workspace are free)
    if (n_k) TD_HIP(ctx, hipMemcpyAsync(dk, kq.data(), sizeof(long long) * n_k, hipMemcpyHostToDevice, s));
    if (n_thr) TD_HIP(ctx, hipMemcpyAsync(dthr, w->thr, sizeof(double) * n_thr, hipMemcpyHostToDevice, s));
    if (total > 0) TD_HIP(ctx, hipMemsetAsync(dK, 0, sizeof(long long) * (n_K + n_C), s));
    TD_HIP(ctx, hipMemsetAsync(dorph, 0, sizeof(long long) * (size_t)M, s));
    TD_HIP(ctx, timed_launch(ctx, "sup_index",
                             [&] { hipLaunchKernelGGL(k_sup_index, dim3((unsigned)M), dim3(kSupThreads), 0, s, S.off, comp3); }));
    int64_t brute_pairs = 0;
    const auto &g = ctx->g;
    for (int64_t p0 = 0; p0 < P; p0 += pp.nodes) {  // who owns the ray points
        const int64_t ns = std::min(pp.nodes, P - p0);
        const double *src[3] = {g.px, g.py, g.pz};
        for (int d = 0; d < 3; ++d)
            TD_HIP(ctx, hipMemcpyAsync(dq + d * ns, src[d] + p0, sizeof(double) * (size_t)ns, hipMemcpyDeviceToDevice, s));
        if (int rc = volume_sweep(ctx, S, 0, M, dq, ns, dv)) return rc;
        if (!S.grid) brute_pairs += M * ns;
        TD_HIP(ctx, timed_launch(ctx, "sup_scatter", [&] {
                   hipLaunchKernelGGL(k_sup_scatter, dim3((unsigned)M), dim3(kSupThreads), 12 * (size_t)lds_cells, s, dv, (int)ns, S.off,
                                      n_k ? dk + p0 : nullptr, lds_cells, reinterpret_cast<unsigned long long *>(dK), dC,
                                      reinterpret_cast<unsigned long long *>(dorph));
               }));
    }
    TD_HIP(ctx, timed_launch(ctx, "sup_finish", [&] {
               hipLaunchKernelGGL(k_sup_finish, dim3((unsigned)M), dim3(kSupThreads), 0, s, S.off, dK, dC, e, comp3,
                                  w->count_out ? dc64 : nullptr, dbar);
           }));
    if (w->cell_out && total > 0)
        TD_HIP(ctx, hipMemcpyAsync(w->cell_out, comp3, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, s));
    if (w->count_out && total > 0)
        TD_HIP(ctx, hipMemcpyAsync(w->count_out, dc64, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToHost, s));
    if (w->barren_out) TD_HIP(ctx, hipMemcpyAsync(w->barren_out, dbar, sizeof(int64_t) * (size_t)M, hipMemcpyDeviceToHost, s));
    if (w->orphans_out) TD_HIP(ctx, hipMemcpyAsync(w->orphans_out, dorph, sizeof(int64_t) * (size_t)M, hipMemcpyDeviceToHost, s));
    double *hquant = ctx->h_raster.as<double>() + 3 * cap;
    const SlabWant want{nq, w->mean_out, w->std_out, w->values_out, w->marg, w->conv};
    for (int64_t q0 = 0; q0 < nq; q0 += qp.nodes) {  // the support painted on the nodes
        const int64_t ns = std::min(qp.nodes, nq - q0);
        if (int rc = stage_queries(ctx, w->qx, w->qy, w->qz, q0, ns, dq)) return rc;
        if (int rc = volume_sweep(ctx, S, 0, M, dq, ns, dv)) return rc;
        if (!S.grid) brute_pairs += M * ns;
        if (nthr > 0) {
            const unsigned groups = (unsigned)std::min<int64_t>((nthr + kSupThr - 1) / kSupThr, 65535);
            TD_HIP(ctx, timed_launch(ctx, "sup_exceed", [&] {
                       hipLaunchKernelGGL(k_sup_exceed, dim3((unsigned)((ns + kSupThreads - 1) / kSupThreads), groups),
                                          dim3(kSupThreads), 0, s, dv, (int)M, (int)ns, dthr, (int)nthr, dex);
                   }));
            TD_HIP(ctx, hipMemcpy2DAsync(w->exceed_out + q0, sizeof(int64_t) * (size_t)nq, dex, sizeof(int64_t) * (size_t)ns,
                                         sizeof(int64_t) * (size_t)ns, (size_t)nthr, hipMemcpyDeviceToHost, s));
        }
        // (waits for the stream: the pinned block is packed again for the next slab)
        if (int rc = slab_statistics(ctx, E, want, dv, q0, ns, dm, dsd, true, hquant)) return rc;
    }
    TD_HIP(ctx, hipStreamSynchronize(s));
    return volume_counters_finish(ctx, S, brute_pairs);  // (tdt_volume_counters: this call's sweeps)
}

}  // namespace

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_support(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                    const double *yCell, const double *zCell, int64_t nchains, const int64_t *chain_len,
                                    const td_support *want) {
    const char *who = "td_rasterize_support";
    std::vector<long long> kq;
    int e = 0;
    // (zeta is no input: the x array stands in its place, and k_sup_index overwrites the copy)
    return ensemble_entry_arrays(
        ctx, who, Ensemble(nmodels, cell_off, xCell, yCell, zCell, xCell, nchains, chain_len), want ? want->conv : nullptr,
        [&] { return support_check(ctx, want, who, &kq, &e); },
        [&](const Ensemble &E) { return support_core(ctx, who, E, want, kq, e); });
}

extern "C" int td_history_support(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_support *want) {
    const char *who = "td_history_support";
    std::vector<long long> kq;
    int e = 0;
    return ensemble_entry_histories(
        ctx, who, hs, nh, want ? want->conv : nullptr, [&] { return support_check(ctx, want, who, &kq, &e); },
        [&](const Ensemble &E) { return support_core(ctx, who, E, want, kq, e); });
}

extern "C" int64_t tdt_support_lds_cells(void) { return kSupLdsCells; }

extern "C" int tdt_set_support_scatter(td_ctx *ctx, int mode) {
    if (!ctx || mode < 0 || mode > 2) return TD_ERR_ARG;
    std::lock_guard<std::mutex> hold(g_mode_lock);
    if (mode == 0)
        g_mode.erase(ctx);
    else
        g_mode[ctx] = mode;
    return TD_OK;
}

extern "C" int tdt_support_quantise(const double *w, int64_t n, int64_t *k_out, int64_t *e_out) {
    if (n < 0 || (n > 0 && (!w || !k_out)) || !e_out) return TD_ERR_ARG;
    std::vector<long long> k((size_t)n);
    int e = 0;
    if (support_quantise(w, n, k.data(), &e)) return TD_ERR_ARG;
    for (int64_t p = 0; p < n; ++p) k_out[p] = k[(size_t)p];
    *e_out = e;
    return TD_OK;
}
