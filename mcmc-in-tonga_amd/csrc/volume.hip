// volume.hip -- posterior volumes: what td_rasterize and its marginal and convergence siblings compute for
// a cross-section, at every node of a lattice (or any node list) of any size.
//
// One pass builds a search structure for ALL models, then the nodes are swept in slabs, so the value
// matrix V[nmodels][nq] never exists whole:
//   k_vol_boxes       one block per model: min / max of x, y, z where the cells lie (NaN ignored, the
//                     comparisons of rasterize_core's host loop); 6 doubles per model come back in one
//                     copy and the host makes each model's CellGrid (make_cell_grid, nc / 2 buckets);
//   k_vol_grid_build  one block per model: count per bucket, exclusive scan, scatter -- a counting sort
//                     of BucketEntry{x, y, z, index in the model} into ONE compact array (32 B per cell;
//                     bucket b of model m is entries [start[b], start[b + 1]) of the model's segment; no
//                     capacity, hence no overflow case).  The order inside a bucket is whatever the
//                     atomics give; the answer does not depend on it (lexicographic minimum);
//   k_vol_search      work item = (model, 256 nodes of the slab), one lane per node.  Buckets that
//                     follow each other along x are contiguous in the compact array, so the 3x3x3 block
//                     is 9 runs of entries; the result counts if it is strictly closer than
//                     grid_block_lb(G, x, y, z, 1), k_nn_grid's rule; else the 5x5x5 block (25 runs),
//                     else every cell of the model in index order.
// Per slab the section entry points' own kernels run on (V_slab, nmodels, nodes): k_raster_stats,
// marginals_run, convergence_run -- a volume's numbers are theirs bit for bit.  Where the models are
// small, k_raster_brute sweeps the slab instead (kVolGridMinMeanCells).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "convergence.h"
#include "ctx.h"
#include "ensemble.h"
#include "history.h"
#include "marginals.h"
#include "volume.h"

namespace tdstar {

namespace {

// Mean cells per model from which the bucket grids sweep a slab faster than k_raster_brute.  Measured on
// one slab of 13 376 lattice nodes x 1000 models (tools/volume_rate.py --crossover), ms:
//   cells per model        50    100    200    400    800   2000   5000
//   k_raster_brute        0.41   0.56   0.97   1.83   3.44   8.11  19.06
//   k_vol_search + build  0.56   0.64   0.84   0.96   1.08   1.27   1.61    (the build over 5 slabs)
// the lines cross between 100 and 200 cells, at about 140 by linear interpolation.
constexpr int64_t kVolGridMinMeanCells = 140;

constexpr int kVolThreads = 256;  // k_vol_search: nodes per work item; the per-model kernels' block
constexpr int kVolXcds = 8;

__device__ __forceinline__ double vol_dist2(double cx, double cy, double cz, double x, double y, double z) {
    // (mx-x)^2 + (my-y)^2 + (mz-z)^2, MCsub.jl:254, left to right, unfused
    const double dx = cx - x, dy = cy - y, dz = cz - z;
    double d = dx * dx;
    d = d + dy * dy;
    d = d + dz * dz;
    return d;
}

// lexicographic (distance, index) update; distances >= the sentinel never count, a NaN never wins
__device__ __forceinline__ void vol_take(double d, int i, double &bd, int &bi) {
    if (d < bd || (d == bd && d < kSentinel && i < bi)) {
        bd = d;
        bi = i;
    }
}

__global__ __launch_bounds__(kVolThreads) void k_vol_boxes(const int64_t *__restrict__ off,
                                                           const double *__restrict__ cells, int64_t cs,
                                                           double *__restrict__ boxes) {
    __shared__ double red[6][kVolThreads];
    const int m = blockIdx.x, t = threadIdx.x;
    const int64_t a = off[m];
    const int nc = (int)(off[m + 1] - a);
    double l[3], u[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        l[d] = HUGE_VAL;
        u[d] = -HUGE_VAL;
        const double *__restrict__ src = cells + d * cs + a;
        for (int i = t; i < nc; i += kVolThreads) {
            const double v = src[i];
            l[d] = v < l[d] ? v : l[d];  // (a NaN is neither below nor above)
            u[d] = v > u[d] ? v : u[d];
        }
        red[d][t] = l[d];
        red[3 + d][t] = u[d];
    }
    __syncthreads();
    for (int w = kVolThreads / 2; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double lo = red[d][t + w], hi = red[3 + d][t + w];
                red[d][t] = lo < red[d][t] ? lo : red[d][t];
                red[3 + d][t] = hi > red[3 + d][t] ? hi : red[3 + d][t];
            }
        }
        __syncthreads();
    }
    if (t < 3) {  // an empty or all-NaN axis: 0, 0
        const double lo = red[t][0], hi = red[3 + t][0];
        boxes[6 * (int64_t)m + t] = lo <= hi ? lo : 0.0;
        boxes[6 * (int64_t)m + 3 + t] = lo <= hi ? hi : 0.0;
    }
}

// The counters are read and written by different lanes of the block across its barriers: every access
// is an agent-scope atomic, so none is served from a stale line of the vector L1.
__device__ __forceinline__ int cur_load(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cur_store(int *p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Model m's buckets are start/cur[boff[m] .. boff[m] + nb] (nb + 1 ints: start[nb] = the model's cells),
// its entries ent[off[m] .. off[m + 1]).
__global__ __launch_bounds__(kVolThreads) void k_vol_grid_build(const int64_t *__restrict__ off,
                                                                const double *__restrict__ cells, int64_t cs,
                                                                const CellGrid *__restrict__ grids,
                                                                const int64_t *__restrict__ boff,
                                                                int *__restrict__ start, int *__restrict__ cur,
                                                                BucketEntry *__restrict__ ent) {
    __shared__ int part[kVolThreads];
    const int m = blockIdx.x, t = threadIdx.x;
    const int64_t a = off[m];
    const int nc = (int)(off[m + 1] - a);
    const CellGrid G = grids[m];
    const int nb = G.gx * G.gy * G.gz;
    int *__restrict__ st = start + boff[m], *__restrict__ cu = cur + boff[m];
    const double *__restrict__ cx = cells + a, *__restrict__ cy = cells + cs + a, *__restrict__ cz = cells + 2 * cs + a;
    for (int b = t; b <= nb; b += kVolThreads) cur_store(&cu[b], 0);
    __syncthreads();
    for (int i = t; i < nc; i += kVolThreads) atomicAdd(&cu[grid_bucket(G, cx[i], cy[i], cz[i])], 1);
    __syncthreads();
    // exclusive scan: each thread a run of consecutive buckets, the runs' sums scanned in LDS
    const int per = (nb + kVolThreads - 1) / kVolThreads;
    const int b_lo = min(t * per, nb), b_hi = min(b_lo + per, nb);
    int sum = 0;
    for (int b = b_lo; b < b_hi; ++b) sum += cur_load(&cu[b]);
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < kVolThreads; ++k) {
            const int c = part[k];
            part[k] = run;
            run += c;
        }
        st[nb] = nc;
    }
    __syncthreads();
    int run = part[t];
    for (int b = b_lo; b < b_hi; ++b) {
        const int c = cur_load(&cu[b]);
        st[b] = run;
        cur_store(&cu[b], run);
        run += c;
    }
    __syncthreads();
    for (int i = t; i < nc; i += kVolThreads) {
        const double x = cx[i], y = cy[i], z = cz[i];
        const int pos = atomicAdd(&cu[grid_bucket(G, x, y, z)], 1);  // < nc: the counts sum to it
        ent[a + pos] = BucketEntry{x, y, z, i, 0};
    }
}

// One lane per node.  The 4-lane form of k_nn_grid4 (lane s of a quad walking the runs s, s + 4, ... and a
// DPP minimum over the quad) was built and measured on the same slab, both without the counters: 1.00 -
// 2.08 ms for 50 - 5000 cells per model against 0.55 - 1.52 ms for this one; not kept.
// COUNT: counters[0..2] += the (model, node) pairs decided by the 3x3x3 block, the 5x5x5 block and a full
// scan, one atomic per wave and path taken.  Every wave adds to the same three words, and that alone
// makes the sweep of a slab 2.8 - 3.3 ms whatever the models' size: the product runs the instance
// without them, the hook tdt_set_volume_counting selects this one.
template <bool COUNT>
__global__ __launch_bounds__(kVolThreads) void k_vol_search(const int64_t *__restrict__ off,
                                                            const double *__restrict__ cells, int64_t cs,
                                                            const CellGrid *__restrict__ grids,
                                                            const int64_t *__restrict__ boff,
                                                            const int *__restrict__ start,
                                                            const BucketEntry *__restrict__ ent,
                                                            const double *__restrict__ q, int nq, int nmodels,
                                                            int nchunks, double *__restrict__ values,
                                                            unsigned long long *__restrict__ counters) {
    // model m on XCD m % 8 (k_raster_brute's mapping): a model's entries are fetched into one L2
    const int L = blockIdx.x, xcd = L % kVolXcds, j = L / kVolXcds;
    const int m = xcd + kVolXcds * (j / nchunks), chunk = j % nchunks;
    if (m >= nmodels) return;
    const int64_t a = off[m];
    const int nc = (int)(off[m + 1] - a);
    const CellGrid G = grids[m];
    const int *__restrict__ st = start + boff[m];
    const BucketEntry *__restrict__ en = ent + a;
    const int node = chunk * kVolThreads + (int)threadIdx.x;
    const bool live = node < nq;
    const int nd = min(node, nq - 1);
    const double x = q[nd], y = q[(long)nq + nd], z = q[2 * (long)nq + nd];
    const int bi = grid_axis(x, G.x0, G.ix, G.gx), bj = grid_axis(y, G.y0, G.iy, G.gy),
              bk = grid_axis(z, G.z0, G.iz, G.gz);
    double bd = kSentinel;
    int bx = INT_MAX;
    int path = 0;
    {  // the 3x3x3 block: 9 runs, their bounds in one round of loads
        const int ilo = max(bi - 1, 0), ihi = min(bi + 1, G.gx - 1);
        int s9[9], e9[9];
#pragma unroll
        for (int u = 0; u < 9; ++u) {
            const int jj = bj + u % 3 - 1, kk = bk + u / 3 - 1;
            const bool in = jj >= 0 && jj < G.gy && kk >= 0 && kk < G.gz;
            const int row = in ? (kk * G.gy + jj) * G.gx : 0;
            s9[u] = in ? st[row + ilo] : 0;
            e9[u] = in ? st[row + ihi + 1] : 0;
        }
        const double lb = grid_block_lb(G, x, y, z, 1);  // independent of the loads: computed while they fly
#pragma unroll
        for (int u = 0; u < 9; ++u)
            for (int t = s9[u]; t < e9[u]; ++t) {
                const BucketEntry e = en[t];
                vol_take(vol_dist2(e.x, e.y, e.z, x, y, z), e.slot, bd, bx);
            }
        if (!(bd < lb)) path = 1;  // something outside could tie or win
    }
    if (path == 1) {  // the 5x5x5 block (the entries seen again change nothing)
        const int ilo = max(bi - 2, 0), ihi = min(bi + 2, G.gx - 1);
        for (int r = 0; r < 25; ++r) {
            const int jj = bj + r % 5 - 2, kk = bk + r / 5 - 2;
            if (jj < 0 || jj >= G.gy || kk < 0 || kk >= G.gz) continue;
            const int row = (kk * G.gy + jj) * G.gx;
            const int s = st[row + ilo], e2 = st[row + ihi + 1];
            for (int t = s; t < e2; ++t) {
                const BucketEntry e = en[t];
                vol_take(vol_dist2(e.x, e.y, e.z, x, y, z), e.slot, bd, bx);
            }
        }
        if (!(bd < grid_block_lb(G, x, y, z, 2))) path = 2;
    }
    if (path == 2) {  // rare: every cell in index order, v_nearest's own scan
        const double *__restrict__ cx = cells + a, *__restrict__ cy = cells + cs + a, *__restrict__ cz = cells + 2 * cs + a;
        bd = kSentinel;
        bx = INT_MAX;
        for (int i = 0; i < nc; ++i) {
            const double d = vol_dist2(cx[i], cy[i], cz[i], x, y, z);
            if (d < bd) {
                bd = d;
                bx = i;
            }
        }
    }
    if (live) values[(long)m * nq + node] = bd < kSentinel ? cells[3 * cs + a + bx] : 0.0;  // MCsub.jl:249
    if (COUNT) {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const unsigned long long b = __ballot(live && path == p);
            if (lane == 0 && b) atomicAdd(&counters[p], (unsigned long long)__popcll(b));
        }
    }
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// A model whose box is not finite (a cell at infinity, an extent that overflows): one bucket, no box
// bound -- its search is the scan of that bucket, which is every cell.
CellGrid one_bucket_grid() {
    CellGrid G{};
    G.gx = G.gy = G.gz = 1;
    return G;
}

}  // namespace

// The search structure of the volume, predictive and covariance calls, in ctx's volume workspaces.  E has
// been checked (ensemble.h).
int volume_build(td_ctx *ctx, const char *who, const Ensemble &E, VolSearch *out) {
    const std::string w(who);
    const int64_t nmodels = E.nmodels, *cell_off = E.cell_off;
    const int64_t total = E.total(), cs = std::max<int64_t>(total, 1);
    if (nmodels > INT32_MAX - 64) return set_err(ctx, TD_ERR_ARG, w + ": too many models");
    for (int64_t k = 0; k < nmodels; ++k)
        if (cell_off[k + 1] - cell_off[k] > INT32_MAX) return set_err(ctx, TD_ERR_ARG, w + ": a model of too many cells");
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);  // (both volume entry points; the predictive and covariance calls have stopped them already)
    hipStream_t s = ctx->stream;
    const bool grid = ctx->vol_method == 1 || (ctx->vol_method == 0 && total / nmodels >= kVolGridMinMeanCells);
    // the models: cells SoA | offsets | boxes | grids | bucket prefix | counters
    const size_t b_cells = up256(sizeof(double) * 4 * (size_t)cs), b_off = up256(sizeof(int64_t) * (size_t)(nmodels + 1)),
                 b_box = up256(sizeof(double) * 6 * (size_t)nmodels), b_grid = up256(sizeof(CellGrid) * (size_t)nmodels);
    if (int rc = grow(ctx, ctx->vol, b_cells + 2 * b_off + b_box + b_grid + 256)) return rc;
    char *base = ctx->vol.as<char>();
    double *dc = reinterpret_cast<double *>(base);
    int64_t *doff = reinterpret_cast<int64_t *>(base + b_cells);
    double *dbox = reinterpret_cast<double *>(base + b_cells + b_off);
    CellGrid *dgrid = reinterpret_cast<CellGrid *>(base + b_cells + b_off + b_box);
    int64_t *dboff = reinterpret_cast<int64_t *>(base + b_cells + b_off + b_box + b_grid);
    unsigned long long *dcount = reinterpret_cast<unsigned long long *>(base + b_cells + 2 * b_off + b_box + b_grid);
    TD_HIP(ctx, hipStreamSynchronize(s));
    if (E.segs) {
        if (int rc = ensemble_copy_segments(ctx, E, dc, cs, s)) return rc;
    } else if (total > 0) {  // (four copies from the caller's arrays; the sections pack theirs into the pinned block)
        const double *src[4] = {E.x, E.y, E.z, E.zeta};
        for (int comp = 0; comp < 4; ++comp)
            TD_HIP(ctx, hipMemcpyAsync(dc + comp * cs, src[comp], sizeof(double) * (size_t)total, hipMemcpyHostToDevice, s));
    }
    TD_HIP(ctx, hipMemcpyAsync(doff, cell_off, sizeof(int64_t) * (size_t)(nmodels + 1), hipMemcpyHostToDevice, s));
    TD_HIP(ctx, hipMemsetAsync(dcount, 0, 4 * sizeof(unsigned long long), s));
    int *dstart = nullptr;
    BucketEntry *dent = nullptr;
    std::vector<double> boxes;
    std::vector<CellGrid> &grids = out->grids_host;  // (the sources of asynchronous copies: they live as long as the sweeps)
    std::vector<int64_t> &boff = out->boff_host;
    if (grid) {
        TD_HIP(ctx, timed_launch(ctx, "vol_boxes", [&] {
                   hipLaunchKernelGGL(k_vol_boxes, dim3((unsigned)nmodels), dim3(kVolThreads), 0, s, doff, dc, cs, dbox);
               }));
        boxes.resize(6 * (size_t)nmodels);
        TD_HIP(ctx, hipMemcpyAsync(boxes.data(), dbox, sizeof(double) * boxes.size(), hipMemcpyDeviceToHost, s));
        TD_HIP(ctx, hipStreamSynchronize(s));
        grids.resize((size_t)nmodels);
        boff.assign((size_t)nmodels + 1, 0);
        for (int64_t m = 0; m < nmodels; ++m) {
            const double *lo = &boxes[6 * (size_t)m], *hi = lo + 3;
            bool finite = true;
            for (int d = 0; d < 3; ++d) finite = finite && std::isfinite(lo[d]) && std::isfinite(hi[d]) && std::isfinite(hi[d] - lo[d]);
            const int64_t nc = cell_off[m + 1] - cell_off[m];
            grids[(size_t)m] = finite ? make_cell_grid(lo, hi, (double)nc / 2.0, 4096, kGridMaxBuckets) : one_bucket_grid();
            const CellGrid &G = grids[(size_t)m];
            boff[(size_t)m + 1] = boff[(size_t)m] + (int64_t)G.gx * G.gy * G.gz + 1;
        }
        const size_t nbp = (size_t)boff[(size_t)nmodels], b_start = up256(sizeof(int) * nbp);
        if (int rc = grow(ctx, ctx->vol_grid, 2 * b_start + sizeof(BucketEntry) * (size_t)cs)) return rc;
        char *gb = ctx->vol_grid.as<char>();
        dstart = reinterpret_cast<int *>(gb);
        int *dcur = reinterpret_cast<int *>(gb + b_start);
        dent = reinterpret_cast<BucketEntry *>(gb + 2 * b_start);
        TD_HIP(ctx, hipMemcpyAsync(dgrid, grids.data(), sizeof(CellGrid) * (size_t)nmodels, hipMemcpyHostToDevice, s));
        TD_HIP(ctx, hipMemcpyAsync(dboff, boff.data(), sizeof(int64_t) * (size_t)(nmodels + 1), hipMemcpyHostToDevice, s));
        TD_HIP(ctx, timed_launch(ctx, "vol_grid_build", [&] {
                   hipLaunchKernelGGL(k_vol_grid_build, dim3((unsigned)nmodels), dim3(kVolThreads), 0, s, doff, dc, cs, dgrid, dboff,
                                      dstart, dcur, dent);
               }));
    }
    out->nmodels = nmodels;
    out->cs = cs;
    out->grid = grid;
    out->cells = dc;
    out->off = doff;
    out->grids = dgrid;
    out->boff = dboff;
    out->start = dstart;
    out->ent = dent;
    out->counters = dcount;
    return TD_OK;
}

// One slab's sweep: values[nm][ns] of the models [m0, m0 + nm) at the device query block q = [3][ns].
int volume_sweep(td_ctx *ctx, const VolSearch &S, int64_t m0, int64_t nm, const double *q, int64_t ns, double *values) {
    hipStream_t s = ctx->stream;
    Timer *tm = ctx->timer.on ? &ctx->timer : nullptr;
    if (S.grid) {
        const int nchunks = (int)((ns + kVolThreads - 1) / kVolThreads);
        const int64_t blocks = (int64_t)kVolXcds * ((nm + kVolXcds - 1) / kVolXcds) * nchunks;
        TD_HIP(ctx, timed_launch(ctx, "vol_search", [&] {
                   if (ctx->vol_counting)
                       hipLaunchKernelGGL(k_vol_search<true>, dim3((unsigned)blocks), dim3(kVolThreads), 0, s, S.off + m0, S.cells,
                                          S.cs, S.grids + m0, S.boff + m0, S.start, S.ent, q, (int)ns, (int)nm, nchunks, values,
                                          S.counters);
                   else
                       hipLaunchKernelGGL(k_vol_search<false>, dim3((unsigned)blocks), dim3(kVolThreads), 0, s, S.off + m0, S.cells,
                                          S.cs, S.grids + m0, S.boff + m0, S.start, S.ent, q, (int)ns, (int)nm, nchunks, values,
                                          S.counters);
               }));
    } else {
        TD_HIP(ctx, launch_raster_brute(S.off + m0, S.cells, S.cs, q, (int)ns, (int)nm, values, s, tm));
    }
    return TD_OK;
}

int volume_counters_finish(td_ctx *ctx, const VolSearch &S, int64_t brute_pairs) {
    unsigned long long cnt[4] = {0, 0, 0, 0};
    TD_HIP(ctx, hipMemcpy(cnt, S.counters, sizeof cnt, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; ++k) ctx->vol_counters[k] = S.grid && !ctx->vol_counting ? -1 : (int64_t)cnt[k];
    ctx->vol_counters[3] = brute_pairs;
    return TD_OK;
}

namespace {

// td_rasterize_volume and td_history_volume; E and vol have been checked (ensemble.h, volume_check).
int volume_core(td_ctx *ctx, const char *who, const Ensemble &E, const td_volume *vol) {
    const int64_t nmodels = E.nmodels, nq = vol->nq;
    if (nq == 0) return TD_OK;
    if (int rc = marg_check_models(ctx, vol->marg, nmodels)) return rc;  // (before anything is issued)
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    // the slabs: queries [3][ns] | V_slab [nmodels][ns] | mean, std [ns]; pinned: queries | quantile rows
    const VolPlan plan = volume_plan(nmodels, nq, kVolDefaultBudget, ctx->vol_slab_nodes);
    const int64_t cap = std::min(plan.nodes, nq);
    const int nprob = vol->marg ? (int)vol->marg->nprob : 0;
    if (int rc = raster_reserve(ctx, (size_t)cap * (5 + (size_t)nmodels), (size_t)cap * (3 + (size_t)nprob))) return rc;
    double *dq = ctx->raster.as<double>(), *dv = dq + 3 * cap, *dm = dv + nmodels * cap, *dsd = dm + cap;
    double *hquant = ctx->h_raster.as<double>() + 3 * cap;
    const SlabWant want{nq, vol->mean_out, vol->std_out, vol->values_out, vol->marg, vol->conv};
    int64_t brute_pairs = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += plan.nodes) {
        const int64_t ns = std::min(plan.nodes, nq - q0);
        if (int rc = stage_queries(ctx, vol->qx, vol->qy, vol->qz, q0, ns, dq)) return rc;
        if (int rc = volume_sweep(ctx, S, 0, nmodels, dq, ns, dv)) return rc;
        if (!S.grid) brute_pairs += nmodels * ns;
        // (waits for the stream: the pinned block is packed again for the next slab)
        if (int rc = slab_statistics(ctx, E, want, dv, q0, ns, dm, dsd, true, hquant)) return rc;
    }
    return volume_counters_finish(ctx, S, brute_pairs);
}

// the checks of both entry points that need no context and no HIP call
int volume_check(td_ctx *ctx, const td_volume *vol, const char *who) {
    const std::string w(who);
    if (!vol) return set_err(ctx, TD_ERR_ARG, w + ": vol is NULL");
    if (vol->nq < 0) return set_err(ctx, TD_ERR_ARG, w + ": nq must be >= 0");
    if (vol->nq > 0 && (!vol->qx || !vol->qy || !vol->qz || !vol->mean_out || !vol->std_out))
        return set_err(ctx, TD_ERR_ARG, w + ": qx, qy, qz, mean_out and std_out must be given for nq > 0");
    if (vol->marg)
        if (int rc = marg_check_want(ctx, vol->marg, who)) return rc;
    if (vol->conv)
        if (int rc = conv_check_want(ctx, vol->conv, who)) return rc;
    return TD_OK;
}

}  // namespace

VolPlan volume_plan(int64_t nmodels, int64_t nq, int64_t budget, int64_t forced) {
    const int64_t nm = std::max<int64_t>(nmodels, 1), b = budget > 0 ? budget : kVolDefaultBudget;
    int64_t nodes = forced > 0 ? forced / kVolTile * kVolTile : b / 8 / nm / kVolTile * kVolTile;
    nodes = std::min(std::max(nodes, kVolTile), kVolMaxSlabNodes);
    // one launch's blocks, for the sweep with the fewest nodes per block (k_raster_brute: 128)
    const int64_t groups = kVolXcds * ((nm + kVolXcds - 1) / kVolXcds), chunks = (int64_t)INT32_MAX / groups;
    nodes = std::min(nodes, std::max(kVolTile, chunks * 128));
    VolPlan p;
    p.nodes = nodes;
    p.nslabs = (std::max<int64_t>(nq, 0) + nodes - 1) / nodes;
    return p;
}

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_volume(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                   const double *yCell, const double *zCell, const double *zeta, int64_t nchains,
                                   const int64_t *chain_len, const td_volume *vol) {
    const char *who = "td_rasterize_volume";
    if (int rc = volume_check(ctx, vol, who)) return rc;
    if (vol->conv)
        if (int rc = conv_check_chains(ctx, nchains, chain_len, nmodels, who)) return rc;
    if (int rc = ensemble_check_arrays(ctx, who, nmodels, cell_off, xCell, yCell, zCell, zeta)) return rc;
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    return volume_core(ctx, who, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta, nchains, chain_len), vol);
}

extern "C" int td_history_volume(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_volume *vol) {
    const char *who = "td_history_volume";
    if (int rc = volume_check(ctx, vol, who)) return rc;
    Ensemble E;
    if (int rc = ensemble_from_histories(ctx, who, hs, nh, HistoryRule::SameContext, &E)) return rc;
    if (vol->conv)
        if (int rc = conv_check_chains(ctx, E.nchains, E.chain_len, E.nmodels, who)) return rc;
    return volume_core(ctx, who, E, vol);
}

extern "C" int tdt_volume_plan(int64_t nmodels, int64_t nq, int64_t budget, int64_t forced, int64_t out[2]) {
    if (!out || nmodels < 1 || nq < 0 || budget < 0 || forced < 0) return TD_ERR_ARG;
    const VolPlan p = volume_plan(nmodels, nq, budget, forced);
    out[0] = p.nodes;
    out[1] = p.nslabs;
    return TD_OK;
}

extern "C" int tdt_set_volume_slab_nodes(td_ctx *ctx, int64_t n) {
    if (!ctx || n < 0) return TD_ERR_ARG;
    ctx->vol_slab_nodes = n;
    return TD_OK;
}

extern "C" int tdt_set_volume_method(td_ctx *ctx, int method) {
    if (!ctx || method < 0 || method > 2) return TD_ERR_ARG;
    ctx->vol_method = method;
    return TD_OK;
}

extern "C" int tdt_volume_counters(td_ctx *ctx, int64_t out[4]) {
    if (!ctx || !out) return TD_ERR_ARG;
    for (int k = 0; k < 4; ++k) out[k] = ctx->vol_counters[k];
    return TD_OK;
}

extern "C" int tdt_set_volume_counting(td_ctx *ctx, int on) {
    if (!ctx || on < 0 || on > 1) return TD_ERR_ARG;
    ctx->vol_counting = on;
    return TD_OK;
}
