// compare.hip -- posterior comparison: one ensemble against another.  Per column (a node of a node list, or a
// column of two host matrices) the two-sample rank statistics of side A's MA values against side B's MB values:
// the pair counts less / equal / greater, the exceedance counts of a scaled and shifted B, and the
// Kolmogorov-Smirnov numbers, all exact integers (include/tdstar_compare.h holds the contract).
//
// The two sides are ONE ensemble of MA + MB models, A first: one search structure (volume_build) and one sweep per
// slab of volume_plan's columns, as recovery.hip sweeps its point list.  A slab V[MA + MB][ns] is row-major, so
// side B is V + MA ns with the same row length, and k_raster_stats and marginals_run (slab_statistics, ensemble.h)
// take either side as it lies.  Per slab:
//   slab_statistics   side A's rows, then side B's: mean, sigma, quantiles, histograms -- the volume's kernels on the
//                     rows a volume of that side alone would hold.  Each call ends with a wait for the stream:
//                     marginals_run's host parameter block (ctx->marg_par_h) is the source of an asynchronous
//                     copy and the second call rewrites it.
//   k_compare_sort    one workgroup per (column, side): the column into LDS (-0.0 -> +0.0, a NaN counted and
//                     replaced by +inf: the first M - #NaN of the sorted column are the numbers), a bitonic network
//                     whose comparators all point upwards, so that a pair reaching past M is a pair with a virtual
//                     +inf and is skipped: M values take 8 M bytes of LDS, not the next power of two's.  The sorted
//                     column goes to the workspace S[ns][MA + MB], contiguous per column.
//   k_compare_count   one workgroup per column.  Sorted B in LDS, every a_i binary-searched: lower and upper bound
//                     give greater, equal and less, a search on fl(fl(s b) + t) (non-decreasing in b for s > 0, so
//                     the sorted order survives) gives exceed[k], and the upper bound is cB(a_i) for KS.  Then
//                     sorted A in LDS and every b_j's upper bound: cA(b_j).  T is evaluated at the last element of
//                     every run of equal values of either side, which covers X.  int64 sums and maxima, reduced over
//                     the wave and the block.
// The counts of a slab go to the caller through the pinned staging of ctx->h_raster.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tdstar_compare.h"
#include "ctx.h"
#include "ensemble.h"
#include "history.h"
#include "marginals.h"
#include "volume.h"

namespace tdstar {

namespace {

constexpr int kCmpMaxThreads = 1024;
constexpr int64_t kCmpMaxModels = TD_COMPARE_MAX_MODELS;
static_assert(kCmpMaxModels == kMargResidentMax, "a side is what the resident quantile regime holds");
constexpr int kCmpRows = 5;  // less | equal | greater | ks_plus | ks_minus, then exceed[k], then ks_at
int g_cmp_placement = 0;     // tdt_set_compare_form: 1 plain columns; the threads of the two kernels, 0 auto
int g_cmp_sort_threads = 0, g_cmp_count_threads = 0;

struct CmpPairs {
    int n;
    double s[TD_COMPARE_MAX_EXCEED], t[TD_COMPARE_MAX_EXCEED];
};

// The column a workgroup of k_compare_sort takes.  Workgroups go round the 8 XCDs; within a group of 64 columns
// the 8 workgroups that follow each other on one XCD take 8 neighbouring columns, which share the 64-byte
// segments of every row of V in that XCD's L2.  (plain: the workgroup's own index.)
__device__ __forceinline__ long cmp_column(long b, long ns, int plain) {
    const long g = b >> 6;
    if (plain || (g + 1) * 64 > ns) return b;
    const int r = (int)(b & 63);
    return g * 64 + (r & 7) * 8 + (r >> 3);
}

__device__ __forceinline__ void cmp_exchange(double *col, int i, int l) {
    const double a = col[i], b = col[l];
    if (a > b) {
        col[i] = b;
        col[l] = a;
    }
}

// V [MA + MB][ns]; S [ns][MA + MB]: the column's side A sorted, then side B sorted (behind the numbers: +inf, one per
// NaN); nv [ns][2] the numbers of each side.  col[M] doubles of dynamic LDS.  blockDim a multiple of 64.
__global__ __launch_bounds__(kCmpMaxThreads) void k_compare_sort(const double *__restrict__ V, int MA, int MB, long ns,
                                                                  int plain, double *__restrict__ S, int *__restrict__ nv) {
    extern __shared__ double col[];
    __shared__ int nan_count;
    const int side = (int)blockIdx.y, M = side ? MB : MA, row0 = side ? MA : 0;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const long q = cmp_column((long)blockIdx.x, ns, plain);
    if (tid == 0) nan_count = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < M; i += nt) {
        double v = V[(long)(row0 + i) * ns + q];
        if (v != v) {
            ++mine;
            v = __builtin_inf();
        } else if (v == 0.0) {
            v = 0.0;
        }
        col[i] = v;
    }
    if (mine) atomicAdd(&nan_count, mine);
    __syncthreads();
    int Mp = 1;
    while (Mp < M) Mp <<= 1;
    const int npairs = Mp >> 1;
    for (int k = 2; k <= Mp; k <<= 1) {
        const int half = k >> 1;
        for (int p = tid; p < npairs; p += nt) {  // the flip: i with its mirror image in the block of k
            const int base = (p / half) * k, o = p & (half - 1);
            const int i = base + o, l = base + k - 1 - o;
            if (l < M) cmp_exchange(col, i, l);
        }
        __syncthreads();
        for (int j = half >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < npairs; p += nt) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                if (l < M) cmp_exchange(col, i, l);
            }
            __syncthreads();
        }
    }
    double *__restrict__ out = S + q * (long)(MA + MB) + row0;
    for (int i = tid; i < M; i += nt) out[i] = col[i];
    if (tid == 0) nv[2 * q + side] = M - nan_count;
}

// the first index in [lo, n) of the sorted s whose element is not below a / is above a
__device__ __forceinline__ int cmp_lower(const double *s, int lo, int n, double a) {
    int hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] < a)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int cmp_upper(const double *s, int lo, int n, double a) {
    int hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] <= a)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// #{j : fl(fl(sc s[j]) + sh) < a}; the map is non-decreasing for sc > 0
__device__ __forceinline__ int cmp_lower_affine(const double *s, int n, double a, double sc, double sh) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double u = sc * s[mid];
        const double f = u + sh;
        if (f < a)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// every thread of the block gets the result; sc [kCmpMaxThreads / 64]
template <bool kMax>
__device__ __forceinline__ long long cmp_block_ll(long long v, long long *sc) {
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_down(v, off, 64);
        v = kMax ? (o > v ? o : v) : v + o;
    }
    __syncthreads();  // (sc is free again)
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = sc[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = kMax ? (sc[w] > r ? sc[w] : r) : r + sc[w];
    return r;
}
__device__ __forceinline__ double cmp_block_min(double v, double *sc) {
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off, 64);
        v = o < v ? o : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sc[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = sc[w] < r ? sc[w] : r;
    return r;
}

struct KsBest {
    long long plus = 0, minus = 0, best = 0;  // max T, max -T, max |T| (all >= 0)
    double at = __builtin_inf();              // the smallest x with |T(x)| == best, among this thread's
    __device__ __forceinline__ void take(long long T, double x) {
        const long long a = T < 0 ? -T : T;
        if (T > plus) plus = T;
        if (-T > minus) minus = -T;
        if (a > best || (a == best && x < at)) {
            best = a;
            at = x;
        }
    }
};

// S, nv: k_compare_sort's.  out: rows of ns int64 (less | equal | greater | ks_plus | ks_minus | exceed[k] ...), then
// ns doubles ks_at.  lds[max(MA, MB)] doubles of dynamic LDS.  blockDim a multiple of 64.
__global__ __launch_bounds__(kCmpMaxThreads) void k_compare_count(const double *__restrict__ S, const int *__restrict__ nv,
                                                                   int MA, int MB, long ns, int want_counts, int want_ks,
                                                                   CmpPairs pairs, long long *__restrict__ out) {
    extern __shared__ double lds[];
    __shared__ long long sc[kCmpMaxThreads / 64];
    __shared__ double scd[kCmpMaxThreads / 64];
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const long q = blockIdx.x;
    const double *__restrict__ sa = S + q * (long)(MA + MB), *__restrict__ sb = sa + MA;
    const int nA = nv[2 * q], nB = nv[2 * q + 1];
    for (int j = tid; j < nB; j += nt) lds[j] = sb[j];
    __syncthreads();
    KsBest ks;
    if (want_counts || want_ks) {
        long long less = 0, equal = 0, greater = 0;
        for (int i = tid; i < nA; i += nt) {
            const double a = sa[i];
            const int lb = cmp_lower(lds, 0, nB, a), ub = cmp_upper(lds, lb, nB, a);
            greater += lb;
            equal += ub - lb;
            less += nB - ub;
            if (want_ks && (i == nA - 1 || sa[i + 1] > a)) ks.take((long long)(i + 1) * MB - (long long)ub * MA, a);
        }
        if (want_counts) {
            less = cmp_block_ll<false>(less, sc);
            equal = cmp_block_ll<false>(equal, sc);
            greater = cmp_block_ll<false>(greater, sc);
            if (tid == 0) {
                out[q] = less;
                out[ns + q] = equal;
                out[2 * ns + q] = greater;
            }
        }
    }
    for (int k = 0; k < pairs.n; ++k) {
        const double scale = pairs.s[k], shift = pairs.t[k];
        long long n = 0;
        for (int i = tid; i < nA; i += nt) n += cmp_lower_affine(lds, nB, sa[i], scale, shift);
        n = cmp_block_ll<false>(n, sc);
        if (tid == 0) out[(long)(kCmpRows + k) * ns + q] = n;
    }
    if (!want_ks) return;
    __syncthreads();  // (every search in B has ended)
    for (int i = tid; i < nA; i += nt) lds[i] = sa[i];
    __syncthreads();
    for (int j = tid; j < nB; j += nt) {
        const double b = sb[j];
        if (j == nB - 1 || sb[j + 1] > b) ks.take((long long)cmp_upper(lds, 0, nA, b) * MB - (long long)(j + 1) * MA, b);
    }
    const long long plus = cmp_block_ll<true>(ks.plus, sc), minus = cmp_block_ll<true>(ks.minus, sc);
    const long long best = plus > minus ? plus : minus;
    const double at = cmp_block_min(best > 0 && ks.best == best ? ks.at : __builtin_inf(), scd);
    if (tid == 0) {
        out[3 * ns + q] = plus;
        out[4 * ns + q] = minus;
        reinterpret_cast<double *>(out)[(long)(kCmpRows + pairs.n) * ns + q] =
            best > 0 ? at : __longlong_as_double(0x7ff8000000000000ll);
    }
}

int cmp_allow_lds(td_ctx *ctx, const void *kern, size_t lds) {
    if (lds > 48 * 1024) TD_HIP(ctx, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return TD_OK;
}

bool wants_counts(const td_compare *w) { return w->less_out || w->equal_out || w->greater_out; }
bool wants_ranks(const td_compare *w) { return wants_counts(w) || w->nexceed > 0 || w->ks_plus_out; }
bool wants_side(const double *mean_out, const td_marginals *marg) { return mean_out || marg; }

// The checks of the three entry points that need no context and no HIP call, in the header's order.  sizes_ok,
// inputs_ok: the entry point's own part of the second and third refusal.
int compare_check(td_ctx *ctx, const td_compare *w, const char *who, bool sizes_ok, bool inputs_ok) {
    const std::string n(who);
    if (!w) return set_err(ctx, TD_ERR_ARG, n + ": want is NULL");
    if (!sizes_ok || w->nexceed < 0 || w->nexceed > TD_COMPARE_MAX_EXCEED)
        return set_err(ctx, TD_ERR_ARG, n + ": counts must be >= 0 and nexceed at most 16");
    if (!inputs_ok) return set_err(ctx, TD_ERR_ARG, n + ": the columns' inputs must be given");
    if (w->nexceed > 0 && (!w->scale || !w->shift || !w->exceed_out))
        return set_err(ctx, TD_ERR_ARG, n + ": scale, shift and exceed_out must be given for nexceed > 0");
    for (int64_t k = 0; k < w->nexceed; ++k)
        if (!(std::isfinite(w->scale[k]) && w->scale[k] > 0.0) || !std::isfinite(w->shift[k]))
            return set_err(ctx, TD_ERR_ARG, n + ": every scale must be finite and > 0, every shift finite");
    if (!wants_ranks(w) && !w->ks_minus_out && !w->ks_at_out && !w->mean_a_out && !w->std_a_out && !w->mean_b_out &&
        !w->std_b_out && !w->marg_a && !w->marg_b)
        return set_err(ctx, TD_ERR_ARG, n + ": no output asked for");
    if (!w->ks_plus_out != !w->ks_minus_out)
        return set_err(ctx, TD_ERR_ARG, n + ": ks_plus_out and ks_minus_out must be given together");
    if (w->ks_at_out && !w->ks_plus_out) return set_err(ctx, TD_ERR_ARG, n + ": ks_at_out needs ks_plus_out and ks_minus_out");
    if (!w->mean_a_out != !w->std_a_out) return set_err(ctx, TD_ERR_ARG, n + ": mean_a_out and std_a_out must be given together");
    if (!w->mean_b_out != !w->std_b_out) return set_err(ctx, TD_ERR_ARG, n + ": mean_b_out and std_b_out must be given together");
    if (w->marg_a)
        if (int rc = marg_check_want(ctx, w->marg_a, who)) return rc;
    if (w->marg_b)
        if (int rc = marg_check_want(ctx, w->marg_b, who)) return rc;
    return TD_OK;
}

int compare_check_size(td_ctx *ctx, const char *who, int64_t MA, int64_t MB) {
    for (int side = 0; side < 2; ++side)
        if ((side ? MB : MA) > kCmpMaxModels)
            return set_err(ctx, TD_ERR_ARG, std::string(who) + ": side " + (side ? "B" : "A") + " holds " +
                                                std::to_string(side ? MB : MA) + " models, at most 16384 a side");
    return TD_OK;
}

int pow2_threads(int64_t n) {
    int nt = 64;
    while (nt < n && nt < kCmpMaxThreads) nt <<= 1;
    return nt;
}

// The slabs of both forms.  n columns in slabs of `nodes`; front: the doubles per column at the start of the pinned
// block that fill() packs (3: the queries; MA + MB: the values).  fill(c0, ns, dq, dv) issues on ctx->stream what
// leaves the slab's V[MA + MB][ns] in dv (dq: room for [3][ns] queries); the pinned front block is free when it is
// called.
template <class Fill>
int compare_slabs(td_ctx *ctx, const td_compare *w, int64_t MA, int64_t MB, int64_t n, int64_t nodes, int64_t front, Fill fill) {
    const int64_t M = MA + MB, cap = std::min(nodes, n), ne = w->nexceed, rows = kCmpRows + ne + 1;
    const bool ranks = wants_ranks(w), side_a = wants_side(w->mean_a_out, w->marg_a), side_b = wants_side(w->mean_b_out, w->marg_b);
    if (int rc = marg_check_models(ctx, w->marg_a, MA)) return rc;  // (before anything is issued)
    if (int rc = marg_check_models(ctx, w->marg_b, MB)) return rc;
    const int64_t nprob = std::max<int64_t>(w->marg_a ? w->marg_a->nprob : 0, w->marg_b ? w->marg_b->nprob : 0);
    // ctx->raster (8-byte words): queries [3][cap] | V_slab [M][cap] | S [cap][M] | mean, std [cap] | out rows [rows][cap]
    // | nv [cap] (two ints); pinned: front [front][cap] | quantile rows [nprob][cap] | out rows [rows][cap]
    const size_t n_q = 3 * (size_t)cap, n_v = (size_t)M * (size_t)cap, n_s = ranks ? n_v : 0, n_ms = 2 * (size_t)cap,
                 n_o = (size_t)rows * (size_t)cap, n_nv = (size_t)cap;
    const size_t h_f = (size_t)front * (size_t)cap, h_q = (size_t)nprob * (size_t)cap;
    if (int rc = raster_reserve(ctx, n_q + n_v + n_s + n_ms + n_o + n_nv, h_f + h_q + n_o)) return rc;
    double *dq = ctx->raster.as<double>(), *dv = dq + n_q, *ds = dv + n_v, *dm = ds + n_s, *dsd = dm + cap;
    long long *dout = reinterpret_cast<long long *>(dm + n_ms);
    int *dnv = reinterpret_cast<int *>(dout + n_o);
    double *hquant = ctx->h_raster.as<double>() + h_f;
    int64_t *hout = reinterpret_cast<int64_t *>(hquant + h_q);
    hipStream_t s = ctx->stream;
    TD_HIP(ctx, hipStreamSynchronize(s));  // (the pinned block and the workspace are free)
    Ensemble EA, EB;  // (slab_statistics reads the number of rows)
    EA.nmodels = MA;
    EB.nmodels = MB;
    CmpPairs pairs;
    std::memset(&pairs, 0, sizeof pairs);
    pairs.n = (int)ne;
    for (int64_t k = 0; k < ne; ++k) {
        pairs.s[k] = w->scale[k];
        pairs.t[k] = w->shift[k];
    }
    const int nt_sort = g_cmp_sort_threads ? g_cmp_sort_threads : pow2_threads(std::max(MA, MB) / 2),
              nt_count = g_cmp_count_threads ? g_cmp_count_threads : pow2_threads(std::max(MA, MB) / 4);
    const size_t lds = sizeof(double) * (size_t)std::max(MA, MB);
    if (ranks) {
        if (int rc = cmp_allow_lds(ctx, (const void *)k_compare_sort, lds)) return rc;
        if (int rc = cmp_allow_lds(ctx, (const void *)k_compare_count, lds)) return rc;
    }
    int64_t *const row_out[kCmpRows] = {w->less_out, w->equal_out, w->greater_out, w->ks_plus_out, w->ks_minus_out};
    for (int64_t c0 = 0; c0 < n; c0 += nodes) {
        const int64_t ns = std::min(nodes, n - c0);
        if (int rc = fill(c0, ns, dq, dv)) return rc;
        // (each ends with a wait for the stream: marginals_run's host parameter block is rewritten by the next call)
        for (int side = 0; side < 2; ++side) {
            if (!(side ? side_b : side_a)) continue;
            const SlabWant sw{n, side ? w->mean_b_out : w->mean_a_out, side ? w->std_b_out : w->std_a_out, nullptr,
                              side ? w->marg_b : w->marg_a, nullptr};
            Timer *tm = ctx->timer.on ? &ctx->timer : nullptr;  // (a side's statistics and their copies under one name)
            hipEvent_t t0 = tm ? tm->begin(s) : nullptr;
            const int rc = slab_statistics(ctx, side ? EB : EA, sw, side ? dv + MA * ns : dv, c0, ns, dm, dsd, true, hquant);
            if (tm) tm->end("compare_side_stats", t0, s);
            if (rc) return rc;
        }
        if (ranks) {
            TD_HIP(ctx, timed_launch(ctx, "compare_sort", [&] {
                       hipLaunchKernelGGL(k_compare_sort, dim3((unsigned)ns, 2), dim3(nt_sort), lds, s, dv, (int)MA, (int)MB,
                                          (long)ns, g_cmp_placement, ds, dnv);
                   }));
            TD_HIP(ctx, timed_launch(ctx, "compare_count", [&] {
                       hipLaunchKernelGGL(k_compare_count, dim3((unsigned)ns), dim3(nt_count), lds, s, ds, dnv, (int)MA, (int)MB,
                                          (long)ns, (int)wants_counts(w), (int)(w->ks_plus_out != nullptr), pairs, dout);
                   }));
            TD_HIP(ctx, hipMemcpyAsync(hout, dout, sizeof(int64_t) * (size_t)rows * (size_t)ns, hipMemcpyDeviceToHost, s));
        }
        TD_HIP(ctx, hipStreamSynchronize(s));  // the pinned block is packed again for the next slab
        if (!ranks) continue;
        const size_t row_b = sizeof(int64_t) * (size_t)ns;
        for (int r = 0; r < kCmpRows; ++r)
            if (row_out[r]) std::memcpy(row_out[r] + c0, hout + r * ns, row_b);
        for (int64_t k = 0; k < ne; ++k) std::memcpy(w->exceed_out + k * n + c0, hout + (kCmpRows + k) * ns, row_b);
        if (w->ks_at_out) std::memcpy(w->ks_at_out + c0, hout + (kCmpRows + ne) * ns, row_b);
    }
    return TD_OK;
}

// td_rasterize_compare and td_history_compare; E (MA + MB models, A first) and w have been checked.
int compare_core(td_ctx *ctx, const char *who, const Ensemble &E, int64_t MA, int64_t MB, const td_compare *w) {
    const int64_t M = MA + MB, nq = w->nq;
    if (nq == 0) return TD_OK;
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    // (the volumes' slab; the sorted columns take as many bytes again: with half a slab each, k_raster_stats, one lane
    // per column, has half the lanes and the call is slower by more than the two new kernels take)
    const VolPlan plan = volume_plan(M, nq, kVolDefaultBudget, ctx->vol_slab_nodes);
    int64_t brute_pairs = 0;
    const int rc = compare_slabs(ctx, w, MA, MB, nq, plan.nodes, 3, [&](int64_t c0, int64_t ns, double *dq, double *dv) {
        if (int r = stage_queries(ctx, w->qx, w->qy, w->qz, c0, ns, dq)) return r;
        if (int r = volume_sweep(ctx, S, 0, M, dq, ns, dv)) return r;
        if (!S.grid) brute_pairs += M * ns;
        return (int)TD_OK;
    });
    if (rc) return rc;
    return volume_counters_finish(ctx, S, brute_pairs);
}

}  // namespace

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_compare(td_ctx *ctx, int64_t nA, const int64_t *offA, const double *xA, const double *yA,
                                    const double *zA, const double *zetaA, int64_t nB, const int64_t *offB, const double *xB,
                                    const double *yB, const double *zB, const double *zetaB, const td_compare *want) {
    const char *who = "td_rasterize_compare";
    if (int rc = compare_check(ctx, want, who, !want || want->nq >= 0, !want || want->nq <= 0 || (want->qx && want->qy && want->qz)))
        return rc;
    if (int rc = ensemble_check_arrays(ctx, "td_rasterize_compare (side A)", nA, offA, xA, yA, zA, zetaA)) return rc;
    if (int rc = ensemble_check_arrays(ctx, "td_rasterize_compare (side B)", nB, offB, xB, yB, zB, zetaB)) return rc;
    if (int rc = compare_check_size(ctx, who, nA, nB)) return rc;
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    if (want->nq == 0) return TD_OK;
    // one ensemble, A first
    const int64_t tA = offA[nA], tB = offB[nB];
    std::vector<int64_t> off((size_t)(nA + nB) + 1);
    std::copy(offA, offA + nA + 1, off.begin());
    for (int64_t k = 1; k <= nB; ++k) off[(size_t)(nA + k)] = tA + offB[k];
    std::vector<double> cat[4];
    const double *srcA[4] = {xA, yA, zA, zetaA}, *srcB[4] = {xB, yB, zB, zetaB};
    for (int c = 0; c < 4; ++c) {
        cat[c].resize((size_t)(tA + tB));
        if (tA > 0) std::memcpy(cat[c].data(), srcA[c], sizeof(double) * (size_t)tA);
        if (tB > 0) std::memcpy(cat[c].data() + tA, srcB[c], sizeof(double) * (size_t)tB);
    }
    return compare_core(ctx, who, Ensemble(nA + nB, off.data(), cat[0].data(), cat[1].data(), cat[2].data(), cat[3].data()), nA,
                        nB, want);
}

extern "C" int td_history_compare(td_ctx *ctx, td_history *const *hsA, int64_t nhA, td_history *const *hsB, int64_t nhB,
                                  const td_compare *want) {
    const char *who = "td_history_compare";
    if (int rc = compare_check(ctx, want, who, !want || want->nq >= 0, !want || want->nq <= 0 || (want->qx && want->qy && want->qz)))
        return rc;
    std::vector<td_history *> all;
    int64_t MA = 0, MB = 0;
    for (int side = 0; side < 2; ++side) {
        td_history *const *hs = side ? hsB : hsA;
        const int64_t nh = side ? nhB : nhA;
        for (int64_t i = 0; hs && i < nh; ++i) {
            if (!hs[i]) return set_err(ctx, TD_ERR_ARG, std::string(who) + ": a history is NULL");
            all.push_back(hs[i]);
            (side ? MB : MA) += hs[i]->samples;
        }
    }
    for (int side = 0; side < 2; ++side)
        if ((side ? MB : MA) < 1)
            return set_err(ctx, TD_ERR_ARG, std::string(who) + ": the histories of side " + (side ? "B" : "A") + " hold no sample");
    if (int rc = compare_check_size(ctx, who, MA, MB)) return rc;
    Ensemble E;
    if (int rc = ensemble_from_histories(ctx, who, all.data(), (int64_t)all.size(), HistoryRule::SameDevice, &E)) return rc;
    if (int rc = ensemble_check_device(ctx, who, E)) return rc;  // (of the first history's device without a context)
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    if (int rc = ensemble_sync_foreign(ctx, E)) return rc;
    return compare_core(ctx, who, E, MA, MB, want);
}

extern "C" int td_compare_values(td_ctx *ctx, const double *A, int64_t MA, const double *B, int64_t MB, int64_t ncol,
                                 const td_compare *want) {
    const char *who = "td_compare_values";
    if (int rc = compare_check(ctx, want, who, MA >= 0 && MB >= 0 && ncol >= 0, ncol <= 0 || MA <= 0 || MB <= 0 || (A && B)))
        return rc;
    for (int side = 0; side < 2; ++side)
        if ((side ? MB : MA) < 1)
            return set_err(ctx, TD_ERR_ARG, std::string(who) + ": side " + (side ? "B" : "A") + " holds no row");
    if (int rc = compare_check_size(ctx, who, MA, MB)) return rc;
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    if (ncol == 0) return TD_OK;
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    const int64_t M = MA + MB;
    // (an eighth of the volumes' bytes: the slab is staged in pinned memory)
    const VolPlan plan = volume_plan(M, ncol, kVolDefaultBudget / 8, ctx->vol_slab_nodes);
    return compare_slabs(ctx, want, MA, MB, ncol, plan.nodes, M, [&](int64_t c0, int64_t ns, double *, double *dv) {
        double *h = ctx->h_raster.as<double>();
        for (int64_t r = 0; r < MA; ++r) std::memcpy(h + r * ns, A + r * ncol + c0, sizeof(double) * (size_t)ns);
        for (int64_t r = 0; r < MB; ++r) std::memcpy(h + (MA + r) * ns, B + r * ncol + c0, sizeof(double) * (size_t)ns);
        TD_HIP(ctx, hipMemcpyAsync(dv, h, sizeof(double) * (size_t)(M * ns), hipMemcpyHostToDevice, ctx->stream));
        return (int)TD_OK;
    });
}

extern "C" int tdt_set_compare_form(int plain, int sort_threads, int count_threads) {
    for (int t : {sort_threads, count_threads})
        if (t != 0 && (t < 64 || t > kCmpMaxThreads || (t & (t - 1)))) return TD_ERR_ARG;
    if (plain < 0 || plain > 1) return TD_ERR_ARG;
    g_cmp_placement = plain;
    g_cmp_sort_threads = sort_threads;
    g_cmp_count_threads = count_threads;
    return TD_OK;
}
