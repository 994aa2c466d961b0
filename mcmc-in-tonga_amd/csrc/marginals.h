// marginals.h -- posterior marginals of the value matrix td_rasterize computes (marginals.hip):
// per-node quantiles (Julia's Statistics.quantile, alpha = beta = 1), per-node histograms and the
// pooled zeta histogram of recorded samples.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ctx.h"

namespace tdstar {

constexpr int kMargMaxProbs = 64;    // td_marginals.nprob
constexpr int kMargMaxBins = 4096;   // td_marginals.nbins, td_history_zeta_hist
// the resident regime sorts a column of Mp = 2^ceil(log2 M) 64-bit keys in LDS: 16384 keys = 128 KiB
constexpr int64_t kMargResidentMax = 16384;

// Julia's quantile position for a column of M values (1-based j, weight g of v[j+1]); host only.
void quantile_rank(int64_t M, double p, int64_t *j, double *g);

// Slot of v in a histogram of nbins bins of width w over [lo, hi): 0 below, 1 + b in range,
// nbins + 1 at or above hi, nbins + 2 NaN.  The same three FP64 operations on host and device.
__host__ __device__ inline int marg_slot(double v, double lo, double hi, double w, int nbins) {
    if (v != v) return nbins + 2;
    if (v < lo) return 0;
    if (v >= hi) return nbins + 1;
    const int b = (int)floor((v - lo) / w);
    return 1 + (b < nbins - 1 ? b : nbins - 1);
}

// The argument checks of td_rasterize_marginals / td_history_marginals that need no context and no
// HIP call (ctx only receives the message).
int marg_check_want(td_ctx *ctx, const td_marginals *want, const char *who);
int marg_check_bins(td_ctx *ctx, int64_t nbins, double lo, double hi, const char *who);

// The one refusal that depends on the number of models M (the resident regime forced on a column it
// cannot hold), for the entry points to make before they issue anything: marginals_run itself runs
// behind their search kernels and copies.  want may be NULL.
int marg_check_models(td_ctx *ctx, const td_marginals *want, int64_t M);

// The launch of the quantile kernel for a value matrix of M models x nq nodes on num_cus compute units
// under method (0 auto, 1 resident, 2 streaming) with nprob probabilities; pure host code.  Resident: a
// tile of W nodes (a power of two, at most 64: the kernel's has_nan) x Mp keys (M rounded up to a power
// of two), Mp * W <= kMargResidentMax.  Streaming: Mp 0, W 1 (a workgroup per node), the 2 nprob digit
// histograms as lds.  false: the resident regime forced on more models than it holds.
struct MargPlan {
    bool resident = false;
    int Mp = 1, W = 1, logW = 0, threads = 64;
    size_t lds = 0;  // dynamic LDS, bytes
};
bool marginals_plan(int64_t M, int64_t nq, int num_cus, int method, int nprob, MargPlan *plan);

// Quantiles and histograms of the device value matrix values[M][nq] (left unchanged), enqueued on
// ctx->stream with the copies to want's host arrays; the caller synchronises.
int marginals_run(td_ctx *ctx, const double *values, int64_t M, int64_t nq, const td_marginals *want);

}  // namespace tdstar
