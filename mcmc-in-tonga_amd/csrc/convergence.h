// convergence.h -- convergence diagnostics of the value matrix td_rasterize computes (convergence.hip):
// per column the split Gelman-Rubin R-hat over the chains' half sequences and the effective sample size
// from Geyer's initial monotone positive sequence (include/tdstar.h "Convergence diagnostics").
#pragma once
#include <cstdint>
#include <vector>

#include "ctx.h"

namespace tdstar {

constexpr size_t kConvScratchBudget = (size_t)64 << 20;  // bytes of acov[m][R][ncol]; R shrinks to fit, not below 2

// What the chain lengths and max_lag decide (host only): every chain's last 2n rows, split in two.
struct ConvPlan {
    int64_t n = 0, m = 0, T = 0;     // rows per sequence, sequences, largest lag
    std::vector<int64_t> seq_start;  // [m] first row of each sequence in the value matrix
    double tau_floor = 0.0;          // 1 / log10(m n)
};

// The lengths must already have passed conv_check_chains.
void conv_plan(int64_t nchains, const int64_t *chain_len, int64_t max_lag, ConvPlan *plan);

// The argument checks that need no context and no HIP call (ctx only receives the message).
int conv_check_want(td_ctx *ctx, const td_convergence *want, const char *who);
int conv_check_chains(td_ctx *ctx, int64_t nchains, const int64_t *chain_len, int64_t M, const char *who);

// R-hat, ESS and lags of the device value matrix values[M][ncol] (left unchanged) on ctx->stream, with the
// copies to want's host arrays enqueued; waits for the stream once per round of lags, the caller
// synchronises at the end.
int convergence_run(td_ctx *ctx, const double *values, int64_t M, int64_t ncol, int64_t nchains,
                    const int64_t *chain_len, const td_convergence *want);

}  // namespace tdstar
