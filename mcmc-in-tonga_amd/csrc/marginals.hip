// marginals.hip -- posterior marginals on the device: per-node quantiles and histograms of the value
// matrix V[k][q] td_rasterize computes (model k at node q, model-major), and the pooled zeta histogram
// of recorded samples (plot_distribution.jl:66-80).
//
// Quantiles are Julia's Statistics.quantile(V[:, q], p) with alpha = beta = 1: the host turns (M, p)
// into two order statistics and a weight (quantile_rank), the kernels select the order statistics
// exactly and form a + g * (b - a), unfused.  A value becomes an order-preserving 64-bit key (sign
// bit flipped for positives, all bits for negatives), so selection is integer work; a NaN gets the
// all-ones key (after every number) and is counted: a column with a NaN gives NaN.
//   k_node_quantiles_resident: a tile of W nodes x all M models in LDS ([Mp][W] keys, Mp = M rounded up
//     to a power of two, padded with all-ones keys), loaded row by row (W consecutive nodes of a model
//     are contiguous), a bitonic network over every column at once, then the ranks are read off.
//   k_node_quantiles_stream: M beyond the LDS: one workgroup per node, a radix select over the column
//     in global memory (8-bit digits, most significant first, one LDS digit histogram per wanted order
//     statistic, integer atomics only: the counts, hence the result, do not depend on the order).
//     V is only read; no device memory beyond the outputs.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "history.h"
#include "marginals.h"

namespace tdstar {

namespace {

constexpr unsigned long long kKeyMax = ~0ull;  // NaN and padding: after +inf

__device__ __forceinline__ unsigned long long key_of(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// what the host worked out per probability (device memory): the 0-based rows of a and b in the sorted
// column and the weight of b
struct QuantPar {
    double g[kMargMaxProbs];
    int ja[kMargMaxProbs], jb[kMargMaxProbs];
};

// keys[Mp][W] in LDS (dynamic), W and Mp powers of two, Mp * W <= 16384; blockDim a power of two.
__global__ __launch_bounds__(1024) void k_node_quantiles_resident(const double *__restrict__ V, int M, int nq, int Mp,
                                                                  int logW, const QuantPar *__restrict__ par,
                                                                  int nprob, double *__restrict__ quant) {
    extern __shared__ unsigned long long keys[];
    __shared__ int has_nan[64];
    const int W = 1 << logW, tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const long q0 = (long)blockIdx.x << logW;
    if (tid < 64) has_nan[tid] = 0;
    __syncthreads();
    for (int e = tid; e < Mp << logW; e += nt) {
        const int row = e >> logW, c = e & (W - 1);
        unsigned long long k = kKeyMax;
        if (row < M && q0 + c < nq) {
            const double v = V[(long)row * nq + q0 + c];
            if (v != v)
                has_nan[c] = 1;  // (every writer stores the same value)
            else
                k = key_of(v);
        }
        keys[e] = k;
    }
    __syncthreads();
    const int npairs = (Mp >> 1) << logW;
    for (int k = 2; k <= Mp; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < npairs; p += nt) {
                const int c = p & (W - 1), pi = p >> logW;
                const int i = ((pi & ~(j - 1)) << 1) | (pi & (j - 1)), l = i | j;
                const unsigned long long a = keys[(i << logW) + c], b = keys[(l << logW) + c];
                if ((a > b) == ((i & k) == 0)) {
                    keys[(i << logW) + c] = b;
                    keys[(l << logW) + c] = a;
                }
            }
            __syncthreads();
        }
    for (int e = tid; e < nprob << logW; e += nt) {
        const int p = e >> logW, c = e & (W - 1);
        if (q0 + c >= nq) continue;
        const double a = value_of(keys[(par->ja[p] << logW) + c]), b = value_of(keys[(par->jb[p] << logW) + c]);
        const double d = b - a;
        const double r = a + par->g[p] * d;
        quant[(long)p * nq + q0 + c] = has_nan[c] ? __builtin_nan("") : r;
    }
}

// One workgroup per node; hist[2 nprob][256] ints in LDS (dynamic).
constexpr int kStreamThreads = 512;
__global__ __launch_bounds__(kStreamThreads) void k_node_quantiles_stream(const double *__restrict__ V, int M, int nq,
                                                                          const QuantPar *__restrict__ par, int nprob,
                                                                          double *__restrict__ quant) {
    extern __shared__ int hist[];
    __shared__ unsigned long long prefix[2 * kMargMaxProbs];
    __shared__ int rem[2 * kMargMaxProbs];
    __shared__ int nan_count;
    const int tid = (int)threadIdx.x, R = 2 * nprob;
    const long q = blockIdx.x;
    if (tid < R) {
        prefix[tid] = 0;
        rem[tid] = tid < nprob ? par->ja[tid] : par->jb[tid - nprob];
    }
    if (tid == 0) nan_count = 0;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int e = tid; e < R * 256; e += kStreamThreads) hist[e] = 0;
        __syncthreads();
        for (int k = tid; k < M; k += kStreamThreads) {
            const double v = V[(long)k * nq + q];
            const bool isn = v != v;
            const unsigned long long key = isn ? kKeyMax : key_of(v);
            if (pass == 0 && isn) atomicAdd(&nan_count, 1);
            const int digit = (int)((key >> shift) & 255);
            const unsigned long long head = pass == 0 ? 0 : key >> (shift + 8);
            for (int r = 0; r < R; ++r)
                if (head == prefix[r]) atomicAdd(&hist[r * 256 + digit], 1);
        }
        __syncthreads();
        if (tid < R) {  // the digit that holds this order statistic among the keys that share its prefix
            int left = rem[tid], d = 0;
            for (; d < 255; ++d) {
                const int n = hist[tid * 256 + d];
                if (left < n) break;
                left -= n;
            }
            rem[tid] = left;
            prefix[tid] = (prefix[tid] << 8) | (unsigned long long)d;
        }
        __syncthreads();
    }
    if (tid < nprob) {
        const double a = value_of(prefix[tid]), b = value_of(prefix[nprob + tid]);
        const double d = b - a;
        const double r = a + par->g[tid] * d;
        quant[(long)tid * nq + q] = nan_count ? __builtin_nan("") : r;
    }
}

// Per-node counts: a wave takes 64 consecutive nodes (coalesced rows of V) and the models
// [y * per, (y + 1) * per); a lane adds a run of equal slots with one atomic (consecutive samples of a
// chain mostly repeat).  hist is zeroed before the launch; integer atomics: any order, same counts.
__global__ __launch_bounds__(64) void k_node_hist(const double *__restrict__ V, int M, int nq, int per, int nbins,
                                                  double lo, double hi, double w,
                                                  unsigned long long *__restrict__ hist) {
    const long q = (long)blockIdx.x * 64 + threadIdx.x;
    if (q >= nq) return;
    const int k0 = (int)blockIdx.y * per, k1 = min(k0 + per, M);
    unsigned long long *row = hist + q * (long)(nbins + 3);
    int cur = -1;
    unsigned long long run = 0;
    for (int k = k0; k < k1; ++k) {
        const int s = marg_slot(V[(long)k * nq + q], lo, hi, w, nbins);
        if (s != cur) {
            if (run) atomicAdd(&row[cur], run);
            cur = s;
            run = 0;
        }
        ++run;
    }
    if (run) atomicAdd(&row[cur], run);
}

// The pooled histogram of a packed zeta segment: a workgroup counts its grid-stride share in LDS, then
// adds its non-zero counts to the global ones.
__global__ __launch_bounds__(256) void k_zeta_hist(const double *__restrict__ zeta, long n, int nbins, double lo,
                                                   double hi, double w, unsigned long long *__restrict__ hist) {
    extern __shared__ unsigned int cnt[];
    for (int s = (int)threadIdx.x; s < nbins + 3; s += 256) cnt[s] = 0;
    __syncthreads();
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        atomicAdd(&cnt[marg_slot(zeta[i], lo, hi, w, nbins)], 1u);
    __syncthreads();
    for (int s = (int)threadIdx.x; s < nbins + 3; s += 256)
        if (cnt[s]) atomicAdd(&hist[s], (unsigned long long)cnt[s]);
}

int allow_lds(td_ctx *ctx, const void *kern, size_t lds) {
    if (lds > 48 * 1024)
        TD_HIP(ctx, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return TD_OK;
}

}  // namespace

void quantile_rank(int64_t M, double p, int64_t *j, double *g) {
    const double aleph = (double)M * p + (1.0 - p);
    const int64_t top = std::max<int64_t>(M - 1, 1);
    int64_t jj = (int64_t)std::trunc(aleph);
    jj = std::min(std::max<int64_t>(jj, 1), top);
    double gg = aleph - (double)jj;
    gg = gg < 0.0 ? 0.0 : (gg > 1.0 ? 1.0 : gg);
    *j = jj;
    *g = gg;
}

int marg_check_bins(td_ctx *ctx, int64_t nbins, double lo, double hi, const char *who) {
    const std::string w(who);
    if (nbins < 0 || nbins > kMargMaxBins) return set_err(ctx, TD_ERR_ARG, w + ": nbins must be 0..4096");
    if (nbins > 0 && !(std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo)))
        return set_err(ctx, TD_ERR_ARG, w + ": need finite lo < hi");
    return TD_OK;
}

int marg_check_want(td_ctx *ctx, const td_marginals *want, const char *who) {
    const std::string w(who);
    if (!want) return set_err(ctx, TD_ERR_ARG, w + ": want is NULL");
    if (want->nprob < 0 || want->nprob > kMargMaxProbs) return set_err(ctx, TD_ERR_ARG, w + ": nprob must be 0..64");
    if (want->nprob > 0 && (!want->probs || !want->quant_out))
        return set_err(ctx, TD_ERR_ARG, w + ": probs and quant_out must be given for nprob > 0");
    for (int64_t i = 0; i < want->nprob; ++i)
        if (!(want->probs[i] >= 0.0 && want->probs[i] <= 1.0))
            return set_err(ctx, TD_ERR_ARG, w + ": every probability must lie in [0, 1]");
    if (int rc = marg_check_bins(ctx, want->nbins, want->lo, want->hi, who)) return rc;
    if (want->nbins > 0 && !want->hist_out) return set_err(ctx, TD_ERR_ARG, w + ": hist_out must be given for nbins > 0");
    return TD_OK;
}

bool marginals_plan(int64_t M, int64_t nq, int num_cus, int method, int nprob, MargPlan *plan) {
    MargPlan p;
    p.resident = method == 1 || (method == 0 && M <= kMargResidentMax);
    if (p.resident) {
        if (M > kMargResidentMax) return false;
        while (p.Mp < M) p.Mp <<= 1;
        // the widest tile the LDS holds, narrowed (down to 8 nodes: 64-byte rows) until the tiles
        // are two per CU
        p.W = (int)std::min<int64_t>(64, kMargResidentMax / p.Mp);
        while (p.W > 8 && (nq + p.W - 1) / p.W < 2 * (int64_t)num_cus) p.W >>= 1;
        while ((1 << p.logW) < p.W) ++p.logW;
        const int npairs = (p.Mp / 2) * p.W;
        p.threads = 64;
        while (p.threads < npairs && p.threads < 1024) p.threads <<= 1;
        p.lds = sizeof(unsigned long long) * (size_t)p.Mp * p.W;
    } else {
        p.Mp = 0;
        p.threads = kStreamThreads;
        p.lds = sizeof(int) * 256 * 2 * (size_t)nprob;
    }
    *plan = p;
    return true;
}

int marg_check_models(td_ctx *ctx, const td_marginals *want, int64_t M) {
    if (want && (want->nprob > 0 || want->nbins > 0) && ctx->marg_method == 1 && M > kMargResidentMax)
        return set_err(ctx, TD_ERR_ARG, "td_marginals: the resident regime cannot hold this many models");
    return TD_OK;
}

int marginals_run(td_ctx *ctx, const double *values, int64_t M, int64_t nq, const td_marginals *want) {
    const int nprob = (int)want->nprob, nbins = (int)want->nbins;
    if (nq == 0 || (nprob == 0 && nbins == 0)) return TD_OK;
    const int64_t slots = nbins + 3;
    if (nbins > 0 && nq > INT64_C(0x7fffffff) / slots) return set_err(ctx, TD_ERR_ARG, "td_marginals: nq * (nbins + 3) too large");
    if (int rc = marg_check_models(ctx, want, M)) return rc;  // (the entry points have made it already)
    const size_t par_b = sizeof(QuantPar), quant_b = sizeof(double) * (size_t)nprob * nq,
                 hist_b = nbins > 0 ? sizeof(int64_t) * (size_t)nq * slots : 0;
    if (int rc = grow(ctx, ctx->marg, par_b + quant_b + hist_b)) return rc;
    QuantPar *dpar = ctx->marg.as<QuantPar>();
    double *dquant = reinterpret_cast<double *>(ctx->marg.as<char>() + par_b);
    unsigned long long *dhist = reinterpret_cast<unsigned long long *>(ctx->marg.as<char>() + par_b + quant_b);
    Timer *tm = ctx->timer.on ? &ctx->timer : nullptr;
    if (nprob > 0) {
        ctx->marg_par_h.resize(par_b);  // (outlives the copy: the caller synchronises before returning)
        QuantPar *hp = reinterpret_cast<QuantPar *>(ctx->marg_par_h.data());
        std::memset(hp, 0, par_b);
        for (int i = 0; i < nprob; ++i) {
            int64_t j;
            quantile_rank(M, want->probs[i], &j, &hp->g[i]);
            hp->ja[i] = (int)(j - 1);
            hp->jb[i] = M == 1 ? 0 : (int)j;
        }
        TD_HIP(ctx, hipMemcpyAsync(dpar, hp, par_b, hipMemcpyHostToDevice, ctx->stream));
        MargPlan plan;
        if (!marginals_plan(M, nq, ctx->num_cus, ctx->marg_method, nprob, &plan))
            return set_err(ctx, TD_ERR_ARG, "td_marginals: the resident regime cannot hold this many models");
        hipEvent_t t0 = tm ? tm->begin(ctx->stream) : nullptr;
        if (plan.resident) {
            if (int rc = allow_lds(ctx, (const void *)k_node_quantiles_resident, plan.lds)) return rc;
            hipLaunchKernelGGL(k_node_quantiles_resident, dim3((unsigned)((nq + plan.W - 1) / plan.W)), dim3(plan.threads),
                               plan.lds, ctx->stream, values, (int)M, (int)nq, plan.Mp, plan.logW, dpar, nprob, dquant);
        } else {
            if (int rc = allow_lds(ctx, (const void *)k_node_quantiles_stream, plan.lds)) return rc;
            hipLaunchKernelGGL(k_node_quantiles_stream, dim3((unsigned)nq), dim3(plan.threads), plan.lds, ctx->stream,
                               values, (int)M, (int)nq, dpar, nprob, dquant);
        }
        if (tm) tm->end("raster_quantile", t0, ctx->stream);
        TD_HIP(ctx, hipGetLastError());
        TD_HIP(ctx, hipMemcpyAsync(want->quant_out, dquant, quant_b, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (nbins > 0) {
        const double w = (want->hi - want->lo) / (double)nbins;
        TD_HIP(ctx, hipMemsetAsync(dhist, 0, hist_b, ctx->stream));
        const int64_t ntiles = (nq + 63) / 64;
        // about 4096 waves in all, at least 16 models each
        const int64_t nsl = std::min<int64_t>(std::max<int64_t>((4096 + ntiles - 1) / ntiles, 1), (M + 15) / 16);
        const int per = (int)((M + nsl - 1) / nsl);
        hipEvent_t t0 = tm ? tm->begin(ctx->stream) : nullptr;
        hipLaunchKernelGGL(k_node_hist, dim3((unsigned)ntiles, (unsigned)((M + per - 1) / per)), dim3(64), 0, ctx->stream,
                           values, (int)M, (int)nq, per, nbins, want->lo, want->hi, w, dhist);
        if (tm) tm->end("raster_node_hist", t0, ctx->stream);
        TD_HIP(ctx, hipGetLastError());
        TD_HIP(ctx, hipMemcpyAsync(want->hist_out, dhist, hist_b, hipMemcpyDeviceToHost, ctx->stream));
    }
    return TD_OK;
}

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_history_zeta_hist(td_ctx *ctx, td_history *const *hs, int64_t nh, int64_t nbins, double lo, double hi,
                                    int64_t *hist_out, int64_t *ncells_out) {
    if (int rc = marg_check_bins(ctx, nbins, lo, hi, "td_history_zeta_hist")) return rc;
    if (nbins < 1 || !hist_out) return set_err(ctx, TD_ERR_ARG, "td_history_zeta_hist: need nbins >= 1 and hist_out");
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, "td_history_zeta_hist: ctx is NULL");
    if (!hs || nh < 1) return set_err(ctx, TD_ERR_ARG, "td_history_zeta_hist: no history");
    for (int64_t i = 0; i < nh; ++i)
        if (!hs[i] || hs[i]->ctx != ctx)
            return set_err(ctx, TD_ERR_ARG, "td_history_zeta_hist: every history must be non-NULL and of this context");
    const double w = (hi - lo) / (double)nbins;
    const size_t hist_b = sizeof(int64_t) * (size_t)(nbins + 3);
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    if (int rc = grow(ctx, ctx->marg, hist_b)) return rc;
    unsigned long long *dhist = ctx->marg.as<unsigned long long>();
    TD_HIP(ctx, hipMemsetAsync(dhist, 0, hist_b, ctx->stream));
    Timer *tm = ctx->timer.on ? &ctx->timer : nullptr;
    int64_t pos = 0;
    for (int64_t i = 0; i < nh; ++i) {
        const td_history *h = hs[i];
        if (ncells_out)  // the samples' nCells: the host mirror of the offsets
            for (int64_t k = 0; k < h->samples; ++k) ncells_out[pos + k] = h->off[(size_t)k + 1] - h->off[(size_t)k];
        pos += h->samples;
        const int64_t cnt = h->samples > 0 ? h->off[(size_t)h->samples] : 0;
        if (cnt <= 0) continue;
        const int64_t blocks = std::min<int64_t>((cnt + 255) / 256, 4 * (int64_t)std::max(ctx->num_cus, 1));
        hipEvent_t t0 = tm ? tm->begin(ctx->stream) : nullptr;
        hipLaunchKernelGGL(k_zeta_hist, dim3((unsigned)blocks), dim3(256), sizeof(unsigned int) * (size_t)(nbins + 3),
                           ctx->stream, h->d.cells + 3 * h->d.stride, (long)cnt, (int)nbins, lo, hi, w, dhist);
        if (tm) tm->end("zeta_hist", t0, ctx->stream);
        TD_HIP(ctx, hipGetLastError());
    }
    TD_HIP(ctx, hipMemcpyAsync(hist_out, dhist, hist_b, hipMemcpyDeviceToHost, ctx->stream));
    TD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TD_OK;
}

extern "C" int tdt_quantile_rank(int64_t M, double p, int64_t *j, double *g) {
    if (M < 1 || !(p >= 0.0 && p <= 1.0) || !j || !g) return TD_ERR_ARG;
    quantile_rank(M, p, j, g);
    return TD_OK;
}

extern "C" int tdt_marginals_plan(int64_t M, int64_t nq, int num_cus, int method, int nprob, int64_t out[5]) {
    if (M < 1 || M > INT64_C(0x7fffffff) || nq < 1 || num_cus < 0 || method < 0 || method > 2 || nprob < 0 ||
        nprob > kMargMaxProbs || !out)
        return TD_ERR_ARG;
    MargPlan p;
    if (!marginals_plan(M, nq, num_cus, method, nprob, &p)) return TD_ERR_ARG;
    out[0] = p.resident ? 1 : 0;
    out[1] = p.Mp;
    out[2] = p.W;
    out[3] = p.threads;
    out[4] = (int64_t)p.lds;
    return TD_OK;
}

extern "C" int tdt_set_marginals_method(td_ctx *ctx, int method) {
    if (!ctx || method < 0 || method > 2) return TD_ERR_ARG;
    ctx->marg_method = method;
    return TD_OK;
}

extern "C" int tdt_marginals_resident_max(td_ctx *ctx, int64_t *M) {
    if (!ctx || !M) return TD_ERR_ARG;
    *M = kMargResidentMax;
    return TD_OK;
}
