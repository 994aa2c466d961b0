// raster.hip -- posterior maps of plot_model_hist (MCsub.jl:753-825) without
// the plotting: the nearest-cell value of every saved model at every node of
// a cross-section (v_nearest, MCsub.jl:765-768 / 799-802), then per node the
// mean and the standard deviation over the models (MCsub.jl:774-775) in the
// association Julia's Statistics uses for a Vector of matrices:
//   mean = sum(A) / n          sum: mapreduce(+) -- n < 16 left to right,
//                              else pairwise halves down to <= 1024-element
//                              blocks added left to right (no SIMD
//                              reassociation: the elements are arrays)
//   std  = sqrt.(sum(abs2.(A .- mean)) / (n - 1))      (same association)
// The model sweep reuses the evaluate path's nearest search (bucket grid or
// brute force per model size), one launch group per model.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "convergence.h"
#include "ctx.h"
#include "ensemble.h"
#include "history.h"
#include "marginals.h"
#include "volume.h"

namespace tdstar {

namespace {

// Julia's mapreduce association over k = 0..n-1 of f(k) (n >= 1).
template <class F>
__device__ double julia_mapreduce_seq_blocks(F f, int n) {
    if (n == 1) return f(0);
    if (n < 16) {
        double s = f(0) + f(1);
        for (int k = 2; k < n; ++k) s = s + f(k);
        return s;
    }
    // pairwise: blocks of <= 1024 elements are summed left to right
    int lo_s[40], hi_s[40], st_s[40];
    double vals[40];
    int top = 1, nv = 0;
    lo_s[0] = 0;
    hi_s[0] = n - 1;
    st_s[0] = 0;
    while (top > 0) {
        const int lo = lo_s[top - 1], hi = hi_s[top - 1];
        if (hi - lo < 1024) {
            double s = f(lo) + f(lo + 1);
            for (int k = lo + 2; k <= hi; ++k) s = s + f(k);
            vals[nv++] = s;
            --top;
            continue;
        }
        const int mid = (lo + hi) >> 1;
        if (st_s[top - 1] == 0) {
            st_s[top - 1] = 1;
            lo_s[top] = lo; hi_s[top] = mid; st_s[top] = 0; ++top;
        } else if (st_s[top - 1] == 1) {
            st_s[top - 1] = 2;
            lo_s[top] = mid + 1; hi_s[top] = hi; st_s[top] = 0; ++top;
        } else {
            const double v2 = vals[--nv];
            const double v1 = vals[--nv];
            vals[nv++] = v1 + v2;
            --top;
        }
    }
    return vals[0];
}

// Every model at every node in ONE launch (the section's nodes are few; one
// launch group per model cost ~80 us of launches and host work per model).
// A work item = (model, chunk of kRasterNodes nodes); a 512-thread workgroup
// is 8 waves = 8 slices of the model's cells, each lane 2 nodes of the chunk
// (100 models x 16 chunks x 8 waves: 13 waves per SIMD, no partial last wave).
// The cells a wave reads are the same in every lane, so they come through the
// scalar cache (wave-uniform addresses: s_load, SGPR operands) -- no LDS
// staging, no barrier but the final one.  Each lane keeps its nodes' running
// (distance, index) with v_nearest's strict '<' in index order (MCsub.jl:
// 250-258: the first minimum wins, only distances below the 1e9 sentinel
// count; NaN never wins); groups of 8 cells take one v_min per distance and
// look the index up only when the group beats the running best.  The slices
// are merged in slice order (a tie keeps the lower slice, hence the lower
// index).  The value is zeta of the winner, or 0.0 when none (MCsub.jl:249).
// XCD-aware mapping: the dispatcher deals workgroups round-robin over the 8
// XCDs, so block L runs on XCD L % 8; every chunk of model m is given to a
// block of XCD m % 8, and each model's cells are fetched from HBM into ONE L2.
constexpr int kRasterThreads = 512;
constexpr int kRasterSlices = kRasterThreads / 64;
constexpr int kRasterPPL = 2;
constexpr int kRasterNodes = 64 * kRasterPPL;
constexpr int kXcds = 8;
__global__ __launch_bounds__(kRasterThreads) void k_raster_brute(const int64_t *__restrict__ cell_off,
                                                                 const double *__restrict__ cells, int64_t cs,
                                                                 const double *__restrict__ q, int nq, int nmodels,
                                                                 int nchunks, double *__restrict__ values) {
    __shared__ double md[kRasterSlices][kRasterNodes];
    __shared__ int mi[kRasterSlices][kRasterNodes];
    const int L = blockIdx.x, xcd = L % kXcds, j = L / kXcds;
    const int m = xcd + kXcds * (j / nchunks), chunk = j % nchunks;
    if (m >= nmodels) return;  // the whole workgroup: no barrier reached
    const long a = (long)cell_off[m];
    const int nc = (int)(cell_off[m + 1] - a);
    const int lane = threadIdx.x & 63;
    const int sl = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int per = (nc + kRasterSlices - 1) / kRasterSlices;
    const int c_lo = min(sl * per, nc), c_hi = min(c_lo + per, nc);
    const double *__restrict__ cx = cells + a, *__restrict__ cy = cells + cs + a, *__restrict__ cz = cells + 2 * cs + a;
    double x[kRasterPPL], y[kRasterPPL], z[kRasterPPL], bd[kRasterPPL];
    int bi[kRasterPPL];
#pragma unroll
    for (int k = 0; k < kRasterPPL; ++k) {
        const int nd = min(chunk * kRasterNodes + k * 64 + lane, nq - 1);
        x[k] = q[nd];
        y[k] = q[nq + nd];
        z[k] = q[2 * (long)nq + nd];
        bd[k] = kSentinel;
        bi[k] = -1;
    }
    int c = c_lo;
    // the next group's cells are loaded (scalar loads, wave-uniform) while this group is scanned
    double ux[8], uy[8], uz[8];
    if (c + 8 <= c_hi) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            ux[u] = cx[c + u];
            uy[u] = cy[c + u];
            uz[u] = cz[c + u];
        }
    }
    for (; c + 8 <= c_hi; c += 8) {
        double vx[8], vy[8], vz[8];
        const int cn = c + 8 + 8 <= c_hi ? c + 8 : c;  // (the last group reloads itself: no branch)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            vx[u] = cx[cn + u];
            vy[u] = cy[cn + u];
            vz[u] = cz[cn + u];
        }
        double dg[kRasterPPL][8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
#pragma unroll
            for (int k = 0; k < kRasterPPL; ++k) {
                // (mx[i]-x)^2 + (my[i]-y)^2 + (mz[i]-z)^2, MCsub.jl:254, left to right, unfused
                const double dx = ux[u] - x[k], dy = uy[u] - y[k], dz = uz[u] - z[k];
                double d = dx * dx;
                d = d + dy * dy;
                d = d + dz * dz;
                dg[k][u] = d;
            }
        }
        group8_update<kRasterPPL>(dg, bd, bi, c);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            ux[u] = vx[u];
            uy[u] = vy[u];
            uz[u] = vz[u];
        }
    }
    for (; c < c_hi; ++c) {
        const double ux = cx[c], uy = cy[c], uz = cz[c];
#pragma unroll
        for (int k = 0; k < kRasterPPL; ++k) {
            const double dx = ux - x[k], dy = uy - y[k], dz = uz - z[k];
            double d = dx * dx;
            d = d + dy * dy;
            d = d + dz * dz;
            if (d < bd[k]) {
                bd[k] = d;
                bi[k] = c;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kRasterPPL; ++k) {
        md[sl][k * 64 + lane] = bd[k];
        mi[sl][k * 64 + lane] = bi[k];
    }
    __syncthreads();
    if (threadIdx.x < kRasterNodes) {
        const int t = threadIdx.x, node = chunk * kRasterNodes + t;
        double d = md[0][t];
        int i = mi[0][t];
#pragma unroll
        for (int s2 = 1; s2 < kRasterSlices; ++s2)
            if (md[s2][t] < d) {  // strict: the lower slice keeps a tie
                d = md[s2][t];
                i = mi[s2][t];
            }
        if (node < nq) values[(long)m * nq + node] = i >= 0 ? cells[3 * cs + a + i] : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_raster_stats(const double *__restrict__ values, int nmodels, int nq,
                                                      double *__restrict__ mean, double *__restrict__ sd) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const double *v = values + q;
    const long st = nq;
    const double m = julia_mapreduce_seq_blocks([&](int k) { return v[k * st]; }, nmodels) / (double)nmodels;
    const double ss = julia_mapreduce_seq_blocks(
        [&](int k) {
            const double d = v[k * st] - m;
            return d * d;  // abs2
        },
        nmodels);
    mean[q] = m;
    sd[q] = sqrt(ss / (double)(nmodels - 1));  // corrected; n == 1 gives 0/0 = NaN as in Julia
}

}  // namespace

}  // namespace tdstar

using namespace tdstar;

int tdstar::raster_reserve(td_ctx *ctx, size_t nd, size_t nh) {
    if (int rc = grow(ctx, ctx->raster, sizeof(double) * nd)) return rc;
    return grow(ctx, ctx->h_raster, sizeof(double) * nh);
}

// volume.hip sweeps a slab of nodes with the same two kernels (volume.h)
bool tdstar::raster_brute_fits(int64_t nmodels, int64_t nq) {
    return (int64_t)kXcds * ((nmodels + kXcds - 1) / kXcds) * ((nq + kRasterNodes - 1) / kRasterNodes) <= INT32_MAX;
}

hipError_t tdstar::launch_raster_brute(const int64_t *cell_off_dev, const double *cells, int64_t cs, const double *q,
                                       int nq, int nmodels, double *values, hipStream_t s, Timer *tm) {
    hipEvent_t t0 = tm ? tm->begin(s) : nullptr;
    const int nchunks = (nq + kRasterNodes - 1) / kRasterNodes;
    const int64_t blocks = (int64_t)kXcds * ((nmodels + kXcds - 1) / kXcds) * nchunks;
    hipLaunchKernelGGL(k_raster_brute, dim3((unsigned)blocks), dim3(kRasterThreads), 0, s, cell_off_dev, cells, cs, q,
                       nq, nmodels, nchunks, values);
    if (tm) tm->end("raster_brute", t0, s);
    return hipGetLastError();
}

hipError_t tdstar::launch_raster_stats(const double *values, int nmodels, int nq, double *mean, double *sd,
                                       hipStream_t s) {
    hipLaunchKernelGGL(k_raster_stats, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, values, nmodels, nq, mean,
                       sd);
    return hipGetLastError();
}

namespace {

// a section's few nodes: every model in one brute-force launch; many nodes: per model,
// the evaluate path's search (the bucket grid from kGridMinCells cells)
bool raster_batched(int64_t nmodels, int64_t total, int64_t nq) {
    return nq * (total / std::max<int64_t>(nmodels, 1)) <= (int64_t)1 << 28 &&
           (int64_t)kXcds * ((nmodels + kXcds - 1) / kXcds) * ((nq + kRasterNodes - 1) / kRasterNodes) <= INT32_MAX;
}

// The request of every section entry point: the nodes, the caller's outputs, and what is computed of the
// value matrix besides its mean and standard deviation
struct SectionRequest {
    const double *qx, *qy, *qz;
    int64_t nq;
    double *mean_out, *std_out, *values_out;
    const td_marginals *want;    // td_rasterize_marginals / td_history_marginals, else nullptr
    const td_convergence *conv;  // td_rasterize_convergence / td_history_convergence, else nullptr
};

// (the td_rasterize wording, whichever of them was called)
int raster_check_request(td_ctx *ctx, const SectionRequest &r) {
    if (r.nq < 0 || (r.nq > 0 && (!r.qx || !r.qy || !r.qz || !r.mean_out || !r.std_out)))
        return set_err(ctx, TD_ERR_ARG, "td_rasterize: bad arguments");
    return TD_OK;
}

// The section entry points; E and the request have been checked (ensemble.h, raster_check_request).  Host
// arrays are packed into the pinned block behind the queries and reach the device in one copy; E.segs
// (td_history_rasterize, the batched launch only) are copied device to device behind the queries.
// r.want: quantiles and histograms of the value matrix as well (marginals.hip), already checked by
// marg_check_want.
// r.conv: R-hat and ESS of the value matrix's columns over E's chains as well (convergence.hip), already
// checked by conv_check_want / conv_check_chains.
int rasterize_core(td_ctx *ctx, const Ensemble &E, const SectionRequest &r) {
    const int64_t nmodels = E.nmodels, total = E.total(), *cell_off = E.cell_off, nq = r.nq;
    if (nq == 0) return TD_OK;
    if (nq > 0x7fffffff / std::max<int64_t>(nmodels, 1) || total > 0x7fffffff)
        return set_err(ctx, TD_ERR_ARG, "td_rasterize: too large");
    // marginals_run's own refusal, made here before anything is issued: there the search kernels and the
    // copies into mean_out / std_out are already under way, and the call would return while they run
    if (int rc = marg_check_models(ctx, r.want, nmodels)) return rc;
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    // one device block: queries (3 nq), all cells SoA (4 total), values (nmodels nq), mean, std (2 nq)
    const size_t nd = 3 * (size_t)nq + 4 * (size_t)std::max<int64_t>(total, 1) + (size_t)nmodels * nq + 2 * (size_t)nq;
    const int64_t cs = std::max<int64_t>(total, 1);  // SoA stride of the cells
    // packed into a pinned staging block (reused across calls), then one DMA copy: pageable
    // copies of these sizes run at ~1 GB/s here
    const size_t nh = 3 * (size_t)nq + (E.segs ? 0 : 4 * (size_t)cs);
    if (int rc = raster_reserve(ctx, nd, nh)) return rc;
    double *dq = ctx->raster.as<double>(), *dc = dq + 3 * nq, *dv = dc + 4 * cs, *dm = dv + nmodels * nq, *ds = dm + nq;
    TD_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the staging block may still feed a previous copy
    double *h = ctx->h_raster.as<double>(), *hc = h + 3 * nq;
    pack_queries(ctx, r.qx, r.qy, r.qz, 0, nq);
    if (total > 0 && !E.segs) {
        std::memcpy(hc, E.x, sizeof(double) * (size_t)total);
        std::memcpy(hc + cs, E.y, sizeof(double) * (size_t)total);
        std::memcpy(hc + 2 * cs, E.z, sizeof(double) * (size_t)total);
        std::memcpy(hc + 3 * cs, E.zeta, sizeof(double) * (size_t)total);
    }
    TD_HIP(ctx, hipMemcpyAsync(dq, h, sizeof(double) * nh, hipMemcpyHostToDevice, ctx->stream));
    if (E.segs)
        if (int rc = ensemble_copy_segments(ctx, E, dc, cs, ctx->stream)) return rc;
    if (int rc = grow(ctx, ctx->raster_i, sizeof(int) * (size_t)nq)) return rc;  // nearest-cell indices (not returned)
    Timer *tm = ctx->timer.on ? &ctx->timer : nullptr;
    const bool batched = raster_batched(nmodels, total, nq);
    if (E.segs && !batched) return set_err(ctx, TD_ERR_ARG, "td_history_rasterize: internal: per-model path");
    if (batched) {
        if (int rc = grow(ctx, ctx->raster_off, sizeof(int64_t) * (size_t)(nmodels + 1))) return rc;
        int64_t *doff = ctx->raster_off.as<int64_t>();
        TD_HIP(ctx, hipMemcpyAsync(doff, cell_off, sizeof(int64_t) * (size_t)(nmodels + 1), hipMemcpyHostToDevice,
                                   ctx->stream));
        TD_HIP(ctx, launch_raster_brute(doff, dc, cs, dq, (int)nq, (int)nmodels, dv, ctx->stream, tm));
    }
    for (int64_t k = 0; k < (batched ? 0 : nmodels); ++k) {
        const int64_t a = cell_off[k], nc = cell_off[k + 1] - a;
        double *out = dv + k * nq;
        hipError_t e;
        if (nc >= kGridMinCells && ctx->nn_method != 1) {
            double lo[3], hi[3];
            const double *src[3] = {E.x + a, E.y + a, E.z + a};
            for (int d = 0; d < 3; ++d) {
                double l = HUGE_VAL, u = -HUGE_VAL;
                for (int64_t i = 0; i < nc; ++i) {
                    l = src[d][i] < l ? src[d][i] : l;
                    u = src[d][i] > u ? src[d][i] : u;
                }
                lo[d] = l <= u ? l : 0.0;
                hi[d] = l <= u ? u : 0.0;
            }
            const CellGrid G = make_cell_grid(lo, hi, (double)nc / 2.0, 4096, kGridMaxBuckets);
            e = launch_nearest_grid(dq, dq + nq, dq + 2 * nq, nq, 1, 1, dc + a, cs, nc, G, ctx->nn, ctx->num_cus,
                                    ctx->raster_i.as<int>(), nullptr, out, ctx->stream, tm);
        } else {
            e = launch_nearest(dq, dq + nq, dq + 2 * nq, nq, 1, 1, dc + a, cs, nc, ctx->nn, ctx->num_cus,
                               ctx->raster_i.as<int>(), nullptr, out, ctx->stream, tm);
        }
        if (e != hipSuccess) return hip_err(ctx, e, "td_rasterize: nearest kernels");
    }
    TD_HIP(ctx, launch_raster_stats(dv, (int)nmodels, (int)nq, dm, ds, ctx->stream));
    TD_HIP(ctx, hipMemcpyAsync(r.mean_out, dm, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    TD_HIP(ctx, hipMemcpyAsync(r.std_out, ds, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    if (r.want)
        if (int rc = marginals_run(ctx, dv, nmodels, nq, r.want)) return rc;
    if (r.conv)
        if (int rc = convergence_run(ctx, dv, nmodels, nq, E.nchains, E.chain_len, r.conv)) return rc;
    if (r.values_out)
        TD_HIP(ctx, hipMemcpyAsync(r.values_out, dv, sizeof(double) * (size_t)nq * nmodels, hipMemcpyDeviceToHost,
                                   ctx->stream));
    TD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TD_OK;
}

// td_rasterize, td_rasterize_marginals and td_rasterize_convergence; E holds the caller's arguments, unchecked
int rasterize_arrays(td_ctx *ctx, const Ensemble &E, const SectionRequest &r) {
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, "td_rasterize: ctx is NULL");
    if (E.nmodels < 1 || !E.cell_off) return set_err(ctx, TD_ERR_ARG, "td_rasterize: bad arguments");
    if (int rc = raster_check_request(ctx, r)) return rc;
    if (int rc = ensemble_check_arrays(ctx, "td_rasterize", E.nmodels, E.cell_off, E.x, E.y, E.z, E.zeta)) return rc;
    return rasterize_core(ctx, E, r);
}

// td_history_rasterize, td_history_marginals and td_history_convergence (one history with samples = one chain)
int history_rasterize(td_ctx *ctx, td_history *const *hs, int64_t nh, const SectionRequest &r) {
    Ensemble E;
    if (int rc = ensemble_from_histories(ctx, "td_history_rasterize", hs, nh, HistoryRule::SameContext, &E)) return rc;
    if (r.conv)
        if (int rc = conv_check_chains(ctx, E.nchains, E.chain_len, E.nmodels, "td_history_convergence")) return rc;
    if (int rc = raster_check_request(ctx, r)) return rc;
    if (raster_batched(E.nmodels, E.total(), r.nq)) return rasterize_core(ctx, E, r);
    // the per-model search computes each model's bounding box on the host: fetch the cells
    const size_t total = (size_t)std::max<int64_t>(E.total(), 1);
    std::vector<double> c(4 * total);
    size_t pos = 0;
    for (td_history *h : *E.segs) {
        const int64_t cnt = h->off[(size_t)h->samples];
        int rc = td_history_read(h, 0, h->samples, nullptr, c.data() + pos, c.data() + total + pos,
                                 c.data() + 2 * total + pos, c.data() + 3 * total + pos, cnt, nullptr, nullptr, nullptr,
                                 nullptr, nullptr);
        if (rc) return rc;
        pos += (size_t)cnt;
    }
    const Ensemble F(E.nmodels, E.cell_off, c.data(), c.data() + total, c.data() + 2 * total, c.data() + 3 * total,
                     E.nchains, E.chain_len);
    return rasterize_core(ctx, F, r);
}

}  // namespace

extern "C" int td_rasterize(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                            const double *yCell, const double *zCell, const double *zeta, const double *qx,
                            const double *qy, const double *qz, int64_t nq, double *mean_out, double *std_out,
                            double *values_out) {
    return rasterize_arrays(ctx, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta),
                            {qx, qy, qz, nq, mean_out, std_out, values_out, nullptr, nullptr});
}

extern "C" int td_history_rasterize(td_ctx *ctx, td_history *const *hs, int64_t nh, const double *qx,
                                    const double *qy, const double *qz, int64_t nq, double *mean_out,
                                    double *std_out, double *values_out) {
    return history_rasterize(ctx, hs, nh, {qx, qy, qz, nq, mean_out, std_out, values_out, nullptr, nullptr});
}

extern "C" int td_rasterize_marginals(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                      const double *yCell, const double *zCell, const double *zeta, const double *qx,
                                      const double *qy, const double *qz, int64_t nq, double *mean_out,
                                      double *std_out, const td_marginals *want) {
    if (int rc = marg_check_want(ctx, want, "td_rasterize_marginals")) return rc;
    return rasterize_arrays(ctx, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta),
                            {qx, qy, qz, nq, mean_out, std_out, nullptr, want, nullptr});
}

extern "C" int td_history_marginals(td_ctx *ctx, td_history *const *hs, int64_t nh, const double *qx,
                                    const double *qy, const double *qz, int64_t nq, double *mean_out,
                                    double *std_out, const td_marginals *want) {
    if (int rc = marg_check_want(ctx, want, "td_history_marginals")) return rc;
    return history_rasterize(ctx, hs, nh, {qx, qy, qz, nq, mean_out, std_out, nullptr, want, nullptr});
}

extern "C" int td_rasterize_convergence(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                        const double *yCell, const double *zCell, const double *zeta, const double *qx,
                                        const double *qy, const double *qz, int64_t nq, int64_t nchains,
                                        const int64_t *chain_len, double *mean_out, double *std_out,
                                        const td_convergence *want) {
    if (int rc = conv_check_want(ctx, want, "td_rasterize_convergence")) return rc;
    if (int rc = conv_check_chains(ctx, nchains, chain_len, nmodels, "td_rasterize_convergence")) return rc;
    return rasterize_arrays(ctx, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta, nchains, chain_len),
                            {qx, qy, qz, nq, mean_out, std_out, nullptr, nullptr, want});
}

extern "C" int td_history_convergence(td_ctx *ctx, td_history *const *hs, int64_t nh, const double *qx,
                                      const double *qy, const double *qz, int64_t nq, double *mean_out,
                                      double *std_out, const td_convergence *want) {
    if (int rc = conv_check_want(ctx, want, "td_history_convergence")) return rc;
    return history_rasterize(ctx, hs, nh, {qx, qy, qz, nq, mean_out, std_out, nullptr, nullptr, want});
}
