// covariance.hip -- posterior covariance: the covariance and the correlation, over the models of an
// ensemble, between zeta at a few targets and zeta at every node of a lattice (or of any node list).
//
// A target is a point, whose series a[k] is model k's nearest-cell zeta there (the volume's own sweep), or a
// series the caller hands in (a ray's predicted t*, the phi trace, ...).  With v_q[k] the value at node q,
//   cov[t][q]  = S / (M - 1),  S = mapreduce over k of (v_q[k] - m_q) * (a_t[k] - m_t)
//   corr[t][q] = cov[t][q] / (s_q * s_t)
// m and s being k_raster_stats' mean and sigma of those columns, and the association of S
// julia_mapreduce_seq_blocks' (raster.hip): M < 16 left to right, else pairwise halves at (lo + hi) >> 1 down
// to blocks of at most 1024, each block left to right.  No FMA: each difference and product is rounded once.
//
// The search structure is the volume's (volume_build), the target points are swept as query blocks into
// A[M][T] (the caller's series are copied beside them), k_raster_stats gives A's means and sigmas, and
//   k_cov_center    Ac[group][k][0..G) = A[k][t] - m_t for the G targets of a group (zeros past T): the G
//                   numbers a wave needs for model k lie in one 64-byte line, and 64 models' lines are one
//                   4 KiB LDS tile, fetched a line per lane and read at one address by all lanes (the lines
//                   taken one at a time as wave-uniform scalar loads were measured 3.6 times slower: DESIGN 4.6g);
// then per slab of volume_plan: volume_sweep -> V_slab[M][ns], k_raster_stats -> mean, sigma [ns], and
//   k_cov_targets   work item = (64 nodes of the slab, group of G targets), one wave, one lane per node: a
//                   row of V_slab is one coalesced 512-byte load per wave and is loaded ONCE per group, not
//                   once per target; G running sums per lane in registers; the left halves of the pairwise
//                   split that wait for their sibling lie in LDS ([level][g][lane], conflict free), as many
//                   levels as cov_levels(M) says.  The tree is walked leaf by leaf by wave-uniform scalars
//                   (predict.hip's pred_ray_sum: the node is found again from the root along `path`).
//                   cov and corr are formed and stored by the same lane.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tdstar_testing.h"
#include "convergence.h"
#include "covariance.h"
#include "ctx.h"
#include "ensemble.h"
#include "history.h"
#include "volume.h"

namespace tdstar {

namespace {

constexpr int kCovMaxGroupsY = 32768;  // groups per launch (grid.y)
constexpr int kCovAhead = 16;          // rows of the slab a wave keeps in flight

__global__ __launch_bounds__(256) void k_cov_center(const double *__restrict__ A, const double *__restrict__ mean_t,
                                                    int M, int T, long total, double *__restrict__ Ac) {
    constexpr int G = kCovGroup;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int g = (int)(i % G);
        const long r = i / G;
        const long k = r % M, grp = r / M;
        const long t = grp * G + g;
        Ac[i] = t < T ? A[k * T + t] - mean_t[t] : 0.0;
    }
}

// s[g] = the terms lo .. hi (hi > lo) of the group's rows ac, left to right: (f(lo) + f(lo + 1)) + f(lo + 2) ...
// A slab has fewer waves than the device has SIMDs (one per 64 nodes), so a wave hides the latency of its
// own loads: the lane's next kCovAhead values of the column are in flight in registers while one is used
// (past the block's end the last row is loaded again, and not used), and the centred targets come 64 rows at
// a time through the LDS tile -- lane j fetches row j's 64 bytes, the next tile's while this one is used,
// and every lane reads the same address of the tile (a broadcast).
template <int G>
__device__ __forceinline__ void cov_block(const double *__restrict__ v, long st, double m,
                                          const double *__restrict__ ac, int lo, int hi, int lane,
                                          double *__restrict__ tile, double (&s)[G]) {
    const double *__restrict__ p = v + (long)lo * st;
    const double *__restrict__ a = ac + (long)lo * G;
    const double d0 = p[0] - m;
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = d0 * a[g];
    p += st;
    a += G;
    const int n = hi - lo;  // the terms after the first, >= 1
    double buf[kCovAhead], nxt[G];
#pragma unroll
    for (int j = 0; j < kCovAhead; ++j) buf[j] = p[(long)min(j, n - 1) * st];
    {
        const double *__restrict__ r = a + (long)min(lane, n - 1) * G;
#pragma unroll
        for (int g = 0; g < G; ++g) nxt[g] = r[g];
    }
    for (int c = 0; c < n; c += kCovThreads) {
        __syncthreads();  // (one wave: the tile's readers are done)
#pragma unroll
        for (int g = 0; g < G; ++g) tile[lane * G + g] = nxt[g];
        {
            const double *__restrict__ r = a + (long)min(c + kCovThreads + lane, n - 1) * G;
#pragma unroll
            for (int g = 0; g < G; ++g) nxt[g] = r[g];
        }
        __syncthreads();
        const int cnt = min(kCovThreads, n - c);
        int jj = 0;
        for (; jj + kCovAhead <= cnt; jj += kCovAhead) {
            double cur[G], nx[G];  // the tile's row in use, and the next one on its way
#pragma unroll
            for (int g = 0; g < G; ++g) cur[g] = tile[jj * G + g];
#pragma unroll
            for (int j = 0; j < kCovAhead; ++j) {
                const double d = buf[j] - m;
                buf[j] = p[(long)min(c + jj + kCovAhead + j, n - 1) * st];
#pragma unroll
                for (int g = 0; g < G; ++g) nx[g] = tile[min(jj + j + 1, kCovThreads - 1) * G + g];
#pragma unroll
                for (int g = 0; g < G; ++g) s[g] = s[g] + d * cur[g];
#pragma unroll
                for (int g = 0; g < G; ++g) cur[g] = nx[g];
            }
        }
#pragma unroll
        for (int j = 0; j < kCovAhead; ++j)  // (the block's last rows: nothing is loaded after them)
            if (jj + j < cnt) {
                const double d = buf[j] - m;
#pragma unroll
                for (int g = 0; g < G; ++g) s[g] = s[g] + d * tile[(jj + j) * G + g];
            }
    }
}

// V = V_slab[M][ns]; Ac = the centred targets [groups][M][G]; cov, corr [T][ns] (each nullable).
template <int G>
__global__ __launch_bounds__(kCovThreads) void k_cov_targets(const double *__restrict__ V, int M, int ns,
                                                             const double *__restrict__ mean,
                                                             const double *__restrict__ sd,
                                                             const double *__restrict__ Ac,
                                                             const double *__restrict__ sd_t, int T, int g0,
                                                             double *__restrict__ cov, double *__restrict__ corr) {
    extern __shared__ __attribute__((aligned(16))) double lds[];  // the tile [64][G] | the waiting left halves [level][G][64]
    double *__restrict__ tile = lds, *__restrict__ pend = lds + kCovThreads * G;
    const int lane = threadIdx.x;
    const int node = blockIdx.x * kCovThreads + lane;
    const int q = min(node, ns - 1);
    const int grp = g0 + (int)blockIdx.y;
    const double *__restrict__ v = V + q;
    const double *__restrict__ ac =
        static_cast<const double *>(__builtin_assume_aligned(Ac, 64)) + (long)grp * M * G;  // (cov_core aligns it)
    const long st = ns;
    const double m = mean[q];
    double s[G];
    if (M == 1) {
        const double d = v[0] - m;
#pragma unroll
        for (int g = 0; g < G; ++g) s[g] = d * ac[g];
    } else {
        unsigned path = 0;  // bit d: the right child at depth d
        int depth = 0, nv = 0;
        for (;;) {
            int f = 0, l = M - 1;
            for (int d = 0; d < depth; ++d) {
                const int mid = f + ((l - f) >> 1);
                if ((path >> d) & 1u)
                    f = mid + 1;
                else
                    l = mid;
            }
            while (l - f >= 1024) {  // down the left children to a block
                l = f + ((l - f) >> 1);
                path &= ~(1u << depth);
                ++depth;
            }
            cov_block<G>(v, st, m, ac, f, l, lane, tile, s);
            while (depth > 0 && ((path >> (depth - 1)) & 1u)) {  // a right child: its parent is left + right
                --nv;
#pragma unroll
                for (int g = 0; g < G; ++g) s[g] = pend[(nv * G + g) * kCovThreads + lane] + s[g];
                --depth;
            }
            if (depth == 0) break;
#pragma unroll
            for (int g = 0; g < G; ++g) pend[(nv * G + g) * kCovThreads + lane] = s[g];  // a left child waits
            ++nv;
            path |= 1u << (depth - 1);
        }
    }
    if (node >= ns) return;
    const double sq = sd[q], nm1 = (double)(M - 1);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int t = grp * G + g;
        if (t < T) {
            const double c = s[g] / nm1;  // M == 1: 0 / 0 = NaN, as sigma
            if (cov) cov[(long)t * ns + node] = c;
            if (corr) corr[(long)t * ns + node] = c / (sq * sd_t[t]);
        }
    }
}

// the checks of both entry points that need no context and no HIP call, in the header's order
int cov_check(td_ctx *ctx, const td_covariance *cv, const char *who) {
    const std::string w(who);
    if (!cv) return set_err(ctx, TD_ERR_ARG, w + ": cov is NULL");
    if (cv->nq < 0 || cv->nt < 0 || cv->nseries < 0) return set_err(ctx, TD_ERR_ARG, w + ": nq, nt and nseries must be >= 0");
    if (cv->nt + cv->nseries == 0) return set_err(ctx, TD_ERR_ARG, w + ": no target (nt + nseries == 0)");
    if (!cv->cov_out && !cv->corr_out) return set_err(ctx, TD_ERR_ARG, w + ": cov_out and corr_out are both NULL");
    if (cv->nq > 0 && (!cv->qx || !cv->qy || !cv->qz)) return set_err(ctx, TD_ERR_ARG, w + ": qx, qy and qz must be given for nq > 0");
    if (cv->nt > 0 && (!cv->tx || !cv->ty || !cv->tz)) return set_err(ctx, TD_ERR_ARG, w + ": tx, ty and tz must be given for nt > 0");
    if (cv->nseries > 0 && !cv->series) return set_err(ctx, TD_ERR_ARG, w + ": series is NULL");
    if (!cv->mean_out != !cv->std_out) return set_err(ctx, TD_ERR_ARG, w + ": mean_out and std_out must be given together");
    if (!cv->tmean_out != !cv->tstd_out)
        return set_err(ctx, TD_ERR_ARG, w + ": tmean_out and tstd_out must be given together");
    return TD_OK;
}

hipError_t timed_stats(td_ctx *ctx, const double *values, int nmodels, int n, double *mean, double *sd) {
    return timed_launch(ctx, "raster_stats", [&] { return launch_raster_stats(values, nmodels, n, mean, sd, ctx->stream); });
}

// Both entry points; E and cv have been checked (ensemble.h, cov_check).
int cov_core(td_ctx *ctx, const char *who, const Ensemble &E, const td_covariance *cv) {
    constexpr int G = kCovGroup;
    const std::string w(who);
    const int64_t M = E.nmodels, nq = cv->nq, nt = cv->nt, T = cv->nt + cv->nseries;
    if (T > INT32_MAX - 64) return set_err(ctx, TD_ERR_ARG, w + ": too many targets");
    const size_t lds = sizeof(double) * (size_t)(1 + cov_levels(M)) * G * kCovThreads;  // the tile | the levels
    if (lds > 64 * 1024) return set_err(ctx, TD_ERR_ARG, w + ": more than 2^25 models");  // (15 levels: 64 KiB of LDS)
    if (nq == 0 && !cv->tmean_out) return TD_OK;
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    hipStream_t s = ctx->stream;
    const VolPlan plan = volume_plan(M, nq, kVolDefaultBudget, ctx->vol_slab_nodes);
    const int64_t cap = std::max<int64_t>(std::min(plan.nodes, std::max(nq, nt)), 1), capq = std::min(plan.nodes, nq);
    const int64_t ngroups = (T + G - 1) / G;
    const bool want_cov = cv->cov_out != nullptr, want_corr = cv->corr_out != nullptr;
    // ctx->raster: Ac [groups][M][G] (first: its rows are 64-byte aligned) | queries [3][cap] | V_slab [M][cap] |
    // mean, std [cap] | A [M][T] | mean, std [T] | cov, corr [T][capq]; pinned: queries [3][cap] | cov, corr rows
    const size_t n_slab = (size_t)cap * (5 + (size_t)M), n_A = (size_t)M * (size_t)T,
                 n_Ac = nq > 0 ? (size_t)ngroups * (size_t)M * G : 0, n_out = (size_t)T * (size_t)capq;
    if (int rc = raster_reserve(ctx, n_slab + n_A + 2 * (size_t)T + n_Ac + 2 * n_out, 3 * (size_t)cap + 2 * n_out)) return rc;
    double *dAc = ctx->raster.as<double>(), *dq = dAc + n_Ac, *dv = dq + 3 * cap, *dm = dv + M * cap, *dsd = dm + cap;
    double *dA = dsd + cap, *dmt = dA + n_A, *dst = dmt + T, *dcov = dst + T, *dcorr = dcov + n_out;
    double *hcov = ctx->h_raster.as<double>() + 3 * cap, *hcorr = hcov + n_out;
    int64_t brute_pairs = 0;
    // the targets: the points swept as query blocks into A[:, 0:nt], the caller's series beside them
    for (int64_t t0 = 0; t0 < nt; t0 += plan.nodes) {
        const int64_t nts = std::min(plan.nodes, nt - t0);
        if (int rc = stage_queries(ctx, cv->tx, cv->ty, cv->tz, t0, nts, dq)) return rc;
        if (int rc = volume_sweep(ctx, S, 0, M, dq, nts, dv)) return rc;
        if (!S.grid) brute_pairs += M * nts;
        TD_HIP(ctx, hipMemcpy2DAsync(dA + t0, sizeof(double) * (size_t)T, dv, sizeof(double) * (size_t)nts,
                                     sizeof(double) * (size_t)nts, (size_t)M, hipMemcpyDeviceToDevice, s));
        TD_HIP(ctx, hipStreamSynchronize(s));  // the pinned block is packed again
    }
    if (cv->nseries > 0)
        TD_HIP(ctx, hipMemcpy2DAsync(dA + nt, sizeof(double) * (size_t)T, cv->series, sizeof(double) * (size_t)cv->nseries,
                                     sizeof(double) * (size_t)cv->nseries, (size_t)M, hipMemcpyHostToDevice, s));
    TD_HIP(ctx, timed_stats(ctx, dA, (int)M, (int)T, dmt, dst));
    if (cv->tmean_out) {
        TD_HIP(ctx, hipMemcpyAsync(cv->tmean_out, dmt, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, s));
        TD_HIP(ctx, hipMemcpyAsync(cv->tstd_out, dst, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, s));
    }
    if (nq > 0) {
        const long total = (long)n_Ac;
        const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 1L << 20);
        TD_HIP(ctx, timed_launch(ctx, "cov_center", [&] {
                   hipLaunchKernelGGL(k_cov_center, dim3(blocks), dim3(256), 0, s, dA, dmt, (int)M, (int)T, total, dAc);
               }));
    }
    for (int64_t q0 = 0; q0 < nq; q0 += plan.nodes) {
        const int64_t ns = std::min(plan.nodes, nq - q0);
        if (int rc = stage_queries(ctx, cv->qx, cv->qy, cv->qz, q0, ns, dq)) return rc;
        if (int rc = volume_sweep(ctx, S, 0, M, dq, ns, dv)) return rc;
        if (!S.grid) brute_pairs += M * ns;
        TD_HIP(ctx, timed_stats(ctx, dv, (int)M, (int)ns, dm, dsd));
        if (cv->mean_out) {
            TD_HIP(ctx, hipMemcpyAsync(cv->mean_out + q0, dm, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
            TD_HIP(ctx, hipMemcpyAsync(cv->std_out + q0, dsd, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
        }
        TD_HIP(ctx, timed_launch(ctx, "cov_targets", [&] {
                   for (int64_t g0 = 0; g0 < ngroups; g0 += kCovMaxGroupsY) {
                       const int64_t ng = std::min<int64_t>(kCovMaxGroupsY, ngroups - g0);
                       hipLaunchKernelGGL(k_cov_targets<G>, dim3((unsigned)((ns + kCovThreads - 1) / kCovThreads), (unsigned)ng),
                                          dim3(kCovThreads), lds, s, dv, (int)M, (int)ns, dm, dsd, dAc, dst, (int)T, (int)g0,
                                          want_cov ? dcov : nullptr, want_corr ? dcorr : nullptr);
                   }
               }));
        // the [T][ns] rows go out through the pinned block, as the volume's quantile rows do
        if (want_cov) TD_HIP(ctx, hipMemcpyAsync(hcov, dcov, sizeof(double) * (size_t)T * (size_t)ns, hipMemcpyDeviceToHost, s));
        if (want_corr)
            TD_HIP(ctx, hipMemcpyAsync(hcorr, dcorr, sizeof(double) * (size_t)T * (size_t)ns, hipMemcpyDeviceToHost, s));
        TD_HIP(ctx, hipStreamSynchronize(s));  // the pinned block is packed again for the next slab
        for (int64_t t = 0; t < T; ++t) {
            if (want_cov) std::memcpy(cv->cov_out + t * nq + q0, hcov + t * ns, sizeof(double) * (size_t)ns);
            if (want_corr) std::memcpy(cv->corr_out + t * nq + q0, hcorr + t * ns, sizeof(double) * (size_t)ns);
        }
    }
    TD_HIP(ctx, hipStreamSynchronize(s));
    return volume_counters_finish(ctx, S, brute_pairs);  // (tdt_volume_counters: the last call's, this one's sweeps too)
}

}  // namespace

int cov_levels(int64_t nmodels) {
    int levels = 0;
    for (int64_t len = nmodels; len - 1 >= 1024; len = (len + 1) / 2) ++levels;  // the left half is the longer one
    return levels;
}

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_covariance(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                       const double *yCell, const double *zCell, const double *zeta,
                                       const td_covariance *cov) {
    const char *who = "td_rasterize_covariance";
    return ensemble_entry_arrays(
        ctx, who, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta), nullptr, [&] { return cov_check(ctx, cov, who); },
        [&](const Ensemble &E) { return cov_core(ctx, who, E, cov); });
}

extern "C" int td_history_covariance(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_covariance *cov) {
    const char *who = "td_history_covariance";
    return ensemble_entry_histories(
        ctx, who, hs, nh, nullptr, [&] { return cov_check(ctx, cov, who); },
        [&](const Ensemble &E) { return cov_core(ctx, who, E, cov); });
}

extern "C" int tdt_covariance_group(void) { return kCovGroup; }
