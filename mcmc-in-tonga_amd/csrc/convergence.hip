// convergence.hip -- convergence diagnostics on the device: per column of the value matrix V[k][q]
// td_rasterize computes (model k at node q, model-major) the split Gelman-Rubin R-hat and the effective
// sample size from Geyer's initial monotone positive sequence; the formulas are in include/tdstar.h.
//
// Every sum is sequential in a stated order (the results are compared bit for bit with a restatement), so
// a sum is one dependent chain and the parallelism is columns x sequences x lags:
//   k_seq_moments: a lane is a column (64 consecutive columns: 512-byte rows of V), blockIdx.y the
//     sequence; two passes: mean_s, var_s.
//   k_rhat: a lane is a column; walks the m sequences in order: W, vp, rhat; arms the round state.
//   k_autocov<LB>: a wave is 64 columns x one sequence x LB consecutive lags: LB accumulators and a window
//     of the LB deviations d_{i+t}, t in the block, in registers; a step loads the row that enters the
//     window and row i, subtracts the mean from each, and does LB multiplies and LB adds.  The main loop
//     is unrolled by the window length, so the shifting window costs no moves; the last steps, where the
//     longer lags have run out of rows, are predicated per lag.
//   k_geyer: a lane is a column; A(t) over the sequences in order, then the round's pairs
//     (rho(2k), rho(2k+1)) into {S, Pprev, last, stopped}; finishes a column that stops (or, in the last
//     round, every column left), clears its tile's flag when no column of the tile goes on, and takes the
//     columns it finished off the global count.
// The host runs rounds of R lags, [rR, (r+1)R) without lag 0 (R even: a pair never straddles two rounds),
// until the count is zero or the lags are covered; the count comes back as one 4-byte pinned read per
// round.  Only stores, loads and integer atomics on the count: nothing depends on scheduling.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "convergence.h"
#include "volume.h"

namespace tdstar {

namespace {

__global__ __launch_bounds__(64) void k_seq_moments(const double *__restrict__ V, int ncol, int n,
                                                    const long long *__restrict__ seq_start,
                                                    double *__restrict__ mean, double *__restrict__ var) {
    const int col = (int)blockIdx.x * 64 + (int)threadIdx.x, s = (int)blockIdx.y;
    if (col >= ncol) return;
    const double *x = V + (long)seq_start[s] * ncol + col;
    const long st = ncol;
    double a = 0.0;
#pragma unroll 8
    for (int i = 0; i < n; ++i) a = a + x[i * st];
    const double mu = a / (double)n;
    double q = 0.0;
#pragma unroll 8
    for (int i = 0; i < n; ++i) {
        const double d = x[i * st] - mu;
        q = q + d * d;
    }
    mean[(long)s * ncol + col] = mu;
    var[(long)s * ncol + col] = q / (double)(n - 1);
}

// the per-column round state of k_geyer
struct ConvState {
    double *W, *vp, *S, *Pprev;
    int *last, *stopped, *tile_active, *count;
};

__global__ __launch_bounds__(64) void k_rhat(const double *__restrict__ mean, const double *__restrict__ var, int ncol,
                                             int n, int m, ConvState st, double *__restrict__ rhat) {
    const int col = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (threadIdx.x == 0) {
        st.tile_active[blockIdx.x] = 1;
        if (blockIdx.x == 0) *st.count = ncol;
    }
    if (col >= ncol) return;
    double w = 0.0, mu = 0.0;
    for (int s = 0; s < m; ++s) {
        w = w + var[(long)s * ncol + col];
        mu = mu + mean[(long)s * ncol + col];
    }
    w = w / (double)m;
    mu = mu / (double)m;
    double b = 0.0;
    for (int s = 0; s < m; ++s) {
        const double d = mean[(long)s * ncol + col] - mu;
        b = b + d * d;
    }
    b = b / (double)(m - 1);
    const double f = (double)(n - 1) / (double)n;
    const double vp = f * w + b;
    st.W[col] = w;
    st.vp[col] = vp;
    st.stopped[col] = 0;
    rhat[col] = sqrt(vp / w);
}

// Lags [tb, tb + LB) with tb = t_lo + blockIdx.z * LB, those below t_hi stored at slot t - base of
// acov[m][R][ncol].  t_hi <= n: a stored lag has at least one term.
template <int LB>
__global__ __launch_bounds__(64) void k_autocov(const double *__restrict__ V, int ncol, int n,
                                                const long long *__restrict__ seq_start,
                                                const double *__restrict__ mean, int t_lo, int t_hi, int base, int R,
                                                double *__restrict__ acov, const int *__restrict__ tile_active) {
    if (!tile_active[blockIdx.x]) return;  // (the same word in every lane)
    const int col = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (col >= ncol) return;
    const int s = (int)blockIdx.y, tb = t_lo + (int)blockIdx.z * LB;
    const double *x = V + (long)seq_start[s] * ncol + col;
    const long st = ncol;
    const double mu = mean[(long)s * ncol + col];
    double acc[LB], w[LB];  // w[j] = d_{i + tb + j}
#pragma unroll
    for (int j = 0; j < LB; ++j) acc[j] = 0.0;
#pragma unroll
    for (int j = 0; j < LB - 1; ++j) w[j] = tb + j < n ? x[(tb + j) * st] - mu : 0.0;
    int i = 0;
    const int nfull = n - tb - LB + 1;  // the steps at which every lag of the block still has its row
    for (; i + LB <= nfull; i += LB) {
#pragma unroll
        for (int u = 0; u < LB; ++u) {
            w[LB - 1] = x[(i + u + tb + LB - 1) * st] - mu;
            const double d = x[(i + u) * st] - mu;
#pragma unroll
            for (int j = 0; j < LB; ++j) acc[j] = acc[j] + d * w[j];
#pragma unroll
            for (int j = 0; j < LB - 1; ++j) w[j] = w[j + 1];
        }
    }
    for (; i < n - tb; ++i) {
        const int r = i + tb + LB - 1;
        w[LB - 1] = r < n ? x[r * st] - mu : 0.0;
        const double d = x[i * st] - mu;
#pragma unroll
        for (int j = 0; j < LB; ++j)
            if (i + tb + j < n) acc[j] = acc[j] + d * w[j];
#pragma unroll
        for (int j = 0; j < LB - 1; ++j) w[j] = w[j + 1];
    }
#pragma unroll
    for (int j = 0; j < LB; ++j)
        if (tb + j < t_hi) acov[((long)s * R + (tb + j - base)) * ncol + col] = acc[j] / (double)n;
}

// The round's lags [t_lo, t_hi) (t_lo is 1 or even, t_hi even) of acov, slot t - base.
__global__ __launch_bounds__(64) void k_geyer(const double *__restrict__ acov, int ncol, int m, int R, int t_lo, int t_hi,
                                              int base, int final_round, ConvState st, double mn, double tau_floor,
                                              double *__restrict__ ess, int *__restrict__ lags) {
    const int tile = (int)blockIdx.x;
    if (!st.tile_active[tile]) return;  // (the same word in every lane)
    const int col = tile * 64 + (int)threadIdx.x;
    const bool live = col < ncol && !st.stopped[col];
    bool done = false;
    if (live) {
        const double w = st.W[col], vp = st.vp[col];
        auto rho = [&](int t) {
            double a = 0.0;
#pragma unroll 8  // (the loads of eight sequences in flight; the adds stay in order)
            for (int s = 0; s < m; ++s) a = a + acov[((long)s * R + (t - base)) * ncol + col];
            a = a / (double)m;
            return 1.0 - (w - a) / vp;
        };
        double S, pp;
        int la, t = t_lo;
        if (t_lo == 1) {
            pp = 1.0 + rho(1);
            S = pp;
            la = 1;
            t = 2;
        } else {
            S = st.S[col];
            pp = st.Pprev[col];
            la = st.last[col];
        }
        bool stop = false;
        for (; t + 1 < t_hi; t += 2) {
            double P = rho(t) + rho(t + 1);
            if (!(P > 0.0)) {  // NaN stops here too
                stop = true;
                break;
            }
            if (P > pp) P = pp;
            S = S + P;
            pp = P;
            la = t + 1;
        }
        if (stop || final_round) {
            double tau = -1.0 + 2.0 * S;
            if (tau < tau_floor) tau = tau_floor;  // a NaN tau stays NaN
            ess[col] = mn / tau;
            lags[col] = stop ? la : -la;
            st.stopped[col] = 1;
            done = true;
        } else {
            st.S[col] = S;
            st.Pprev[col] = pp;
            st.last[col] = la;
        }
    }
    const unsigned long long go_on = __ballot(live && !done), finished = __ballot(done);
    if (threadIdx.x == 0) {
        if (!go_on) st.tile_active[tile] = 0;
        if (finished) atomicSub(st.count, __popcll(finished));
    }
}

template <int LB>
void launch_autocov(td_ctx *ctx, dim3 grid, const double *V, int ncol, int n, const long long *seq, const double *mean,
                    int t_lo, int t_hi, int base, int R, double *acov, const int *tile_active) {
    hipLaunchKernelGGL(k_autocov<LB>, grid, dim3(64), 0, ctx->stream, V, ncol, n, seq, mean, t_lo, t_hi, base, R, acov,
                       tile_active);
}

}  // namespace

void conv_plan(int64_t nchains, const int64_t *chain_len, int64_t max_lag, ConvPlan *plan) {
    int64_t N = chain_len[0];
    for (int64_t c = 1; c < nchains; ++c) N = std::min(N, chain_len[c]);
    const int64_t n = N / 2, m = 2 * nchains;
    plan->n = n;
    plan->m = m;
    plan->T = max_lag == 0 ? n - 1 : std::min(n - 1, max_lag);
    plan->seq_start.resize((size_t)m);
    int64_t pos = 0;
    for (int64_t c = 0; c < nchains; ++c) {
        plan->seq_start[(size_t)(2 * c)] = pos + chain_len[c] - 2 * n;
        plan->seq_start[(size_t)(2 * c + 1)] = pos + chain_len[c] - n;
        pos += chain_len[c];
    }
    plan->tau_floor = 1.0 / std::log10((double)(m * n));
}

int conv_check_want(td_ctx *ctx, const td_convergence *want, const char *who) {
    const std::string w(who);
    if (!want) return set_err(ctx, TD_ERR_ARG, w + ": want is NULL");
    if (want->max_lag < 0) return set_err(ctx, TD_ERR_ARG, w + ": max_lag must be >= 0");
    if (!want->rhat_out && !want->ess_out && !want->lags_out)
        return set_err(ctx, TD_ERR_ARG, w + ": rhat_out, ess_out and lags_out are all NULL");
    return TD_OK;
}

int conv_check_chains(td_ctx *ctx, int64_t nchains, const int64_t *chain_len, int64_t M, const char *who) {
    const std::string w(who);
    if (nchains < 1) return set_err(ctx, TD_ERR_ARG, w + ": nchains must be >= 1");
    if (!chain_len) return set_err(ctx, TD_ERR_ARG, w + ": chain_len is NULL");
    int64_t sum = 0, N = INT64_MAX;
    for (int64_t c = 0; c < nchains; ++c) {
        if (chain_len[c] < 4) return set_err(ctx, TD_ERR_ARG, w + ": every chain needs at least 4 rows");
        if (chain_len[c] > INT64_MAX - sum) return set_err(ctx, TD_ERR_ARG, w + ": the chain lengths overflow");
        sum += chain_len[c];
        N = std::min(N, chain_len[c]);
    }
    if (sum != M) return set_err(ctx, TD_ERR_ARG, w + ": the chain lengths do not sum to the number of rows");
    if (nchains > INT32_MAX / 2 || (N / 2) > (int64_t)INT32_MAX / (2 * nchains))
        return set_err(ctx, TD_ERR_ARG, w + ": m * n exceeds INT32_MAX");
    return TD_OK;
}

int convergence_run(td_ctx *ctx, const double *values, int64_t M, int64_t ncol64, int64_t nchains,
                    const int64_t *chain_len, const td_convergence *want) {
    (void)M;
    if (ncol64 == 0) return TD_OK;
    ConvPlan p;
    conv_plan(nchains, chain_len, want->max_lag, &p);
    if (ncol64 > INT32_MAX - 64 || p.m > 65535)
        return set_err(ctx, TD_ERR_ARG, "td_convergence: too many columns or chains (at most 32767)");
    const int ncol = (int)ncol64, n = (int)p.n, m = (int)p.m;
    const bool lagged = want->ess_out || want->lags_out;
    const int ntiles = (ncol + 63) / 64;
    const int t_need = (p.T & 1) ? (int)p.T : (int)p.T - 1;  // the last lag a pair (2k, 2k+1) or rho(1) uses
    const int LB = ctx->conv_lb ? ctx->conv_lb : 8;  // measured: DESIGN 4.6c
    int64_t R = ctx->conv_round;
    if (R == 0) {  // enough lag blocks for about two waves per SIMD, at most 512 lags a round
        const int64_t waves = (int64_t)ntiles * m, target = 8 * (int64_t)std::max(ctx->num_cus, 1);
        R = std::min<int64_t>(512, LB * ((target + waves - 1) / waves));
    }
    R = std::min<int64_t>(R, t_need + 1);
    const int64_t fit = (int64_t)(kConvScratchBudget / (sizeof(double) * (size_t)m * (size_t)ncol)) & ~(int64_t)1;
    R = std::max<int64_t>(2, std::min(R, fit));
    if (!lagged) R = 0;
    // doubles: mean, var [m][ncol] | W, vp, S, Pprev, rhat, ess [ncol] | acov [m][R][ncol];
    // then seq_start [m] (64-bit); then last, stopped, lags [ncol], tile_active [ntiles], count (32-bit)
    const size_t mc = (size_t)m * ncol, nd = 2 * mc + 6 * (size_t)ncol + mc * (size_t)R;
    const size_t ni = 3 * (size_t)ncol + (size_t)ntiles + 1;
    const size_t host_b = 8 + sizeof(int64_t) * (size_t)m;
    if (int rc = grow(ctx, ctx->conv, sizeof(double) * nd + sizeof(int64_t) * (size_t)m + sizeof(int) * ni)) return rc;
    if (int rc = grow(ctx, ctx->h_conv, host_b)) return rc;
    double *dmean = ctx->conv.as<double>(), *dvar = dmean + mc, *dW = dvar + mc, *dvp = dW + ncol,
           *dS = dvp + ncol, *dPp = dS + ncol, *drhat = dPp + ncol, *dess = drhat + ncol, *dacov = dess + ncol;
    long long *dseq = reinterpret_cast<long long *>(dacov + mc * (size_t)R);
    int *dlast = reinterpret_cast<int *>(dseq + m), *dstopped = dlast + ncol, *dlags = dstopped + ncol,
        *dtile = dlags + ncol, *dcount = dtile + ntiles;
    TD_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the pinned block may still feed a previous copy
    int *hcount = ctx->h_conv.as<int>();
    int64_t *hseq = reinterpret_cast<int64_t *>(ctx->h_conv.as<char>() + 8);
    std::memcpy(hseq, p.seq_start.data(), sizeof(int64_t) * (size_t)m);
    TD_HIP(ctx, hipMemcpyAsync(dseq, hseq, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    Timer *tm = ctx->timer.on ? &ctx->timer : nullptr;
    const ConvState st{dW, dvp, dS, dPp, dlast, dstopped, dtile, dcount};
    hipEvent_t t0 = tm ? tm->begin(ctx->stream) : nullptr;
    hipLaunchKernelGGL(k_seq_moments, dim3((unsigned)ntiles, (unsigned)m), dim3(64), 0, ctx->stream, values, ncol, n, dseq,
                       dmean, dvar);
    hipLaunchKernelGGL(k_rhat, dim3((unsigned)ntiles), dim3(64), 0, ctx->stream, dmean, dvar, ncol, n, m, st, drhat);
    if (tm) tm->end("conv_moments", t0, ctx->stream);
    TD_HIP(ctx, hipGetLastError());
    if (want->rhat_out)
        TD_HIP(ctx, hipMemcpyAsync(want->rhat_out, drhat, sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost, ctx->stream));
    if (!lagged) return TD_OK;
    const int Ri = (int)R;
    for (int base = 0; base <= t_need; base += Ri) {
        const int t_lo = std::max(base, 1), t_hi = std::min(base + Ri, t_need + 1);
        const int final_round = t_hi > t_need;
        const dim3 grid((unsigned)ntiles, (unsigned)m, (unsigned)((t_hi - t_lo + LB - 1) / LB));
        t0 = tm ? tm->begin(ctx->stream) : nullptr;
        if (LB == 8)
            launch_autocov<8>(ctx, grid, values, ncol, n, dseq, dmean, t_lo, t_hi, base, Ri, dacov, dtile);
        else
            launch_autocov<16>(ctx, grid, values, ncol, n, dseq, dmean, t_lo, t_hi, base, Ri, dacov, dtile);
        if (tm) tm->end("conv_autocov", t0, ctx->stream);
        TD_HIP(ctx, hipGetLastError());
        t0 = tm ? tm->begin(ctx->stream) : nullptr;
        hipLaunchKernelGGL(k_geyer, dim3((unsigned)ntiles), dim3(64), 0, ctx->stream, dacov, ncol, m, Ri, t_lo, t_hi, base,
                           final_round, st, (double)(p.m * p.n), p.tau_floor, dess, dlags);
        if (tm) tm->end("conv_geyer", t0, ctx->stream);
        TD_HIP(ctx, hipGetLastError());
        if (final_round) break;
        TD_HIP(ctx, hipMemcpyAsync(hcount, dcount, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        TD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (*hcount == 0) break;  // every column has stopped
    }
    if (want->ess_out)
        TD_HIP(ctx, hipMemcpyAsync(want->ess_out, dess, sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost, ctx->stream));
    if (want->lags_out)
        TD_HIP(ctx, hipMemcpyAsync(want->lags_out, dlags, sizeof(int32_t) * (size_t)ncol, hipMemcpyDeviceToHost, ctx->stream));
    return TD_OK;
}

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_convergence_values(td_ctx *ctx, const double *values, int64_t M, int64_t ncol, int64_t nchains,
                                     const int64_t *chain_len, const td_convergence *want) {
    const char *who = "td_convergence_values";
    if (int rc = conv_check_want(ctx, want, who)) return rc;
    if (int rc = conv_check_chains(ctx, nchains, chain_len, M, who)) return rc;
    if (ncol < 0 || (ncol > 0 && !values)) return set_err(ctx, TD_ERR_ARG, std::string(who) + ": bad values or ncol");
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, std::string(who) + ": ctx is NULL");
    if (ncol == 0) return TD_OK;
    if (ncol > INT32_MAX || (uint64_t)M > (uint64_t)INT64_MAX / 8 / (uint64_t)ncol)
        return set_err(ctx, TD_ERR_ARG, std::string(who) + ": too large");
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    const size_t nv = (size_t)M * (size_t)ncol;
    if (int rc = raster_reserve(ctx, nv, nv)) return rc;
    TD_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the staging block may still feed a previous copy
    std::memcpy(ctx->h_raster.p, values, sizeof(double) * nv);
    TD_HIP(ctx, hipMemcpyAsync(ctx->raster.p, ctx->h_raster.p, sizeof(double) * nv, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = convergence_run(ctx, ctx->raster.as<double>(), M, ncol, nchains, chain_len, want)) return rc;
    TD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TD_OK;
}

extern "C" int tdt_convergence_plan(int64_t nchains, const int64_t *chain_len, int64_t max_lag, int64_t out[4],
                                    int64_t *seq_start, double *tau_floor) {
    if (!out || max_lag < 0) return TD_ERR_ARG;
    int64_t sum = 0;
    for (int64_t c = 0; chain_len && c < nchains; ++c) sum += chain_len[c] >= 4 ? chain_len[c] : 0;
    if (int rc = conv_check_chains(nullptr, nchains, chain_len, sum, "tdt_convergence_plan")) return rc;
    ConvPlan p;
    conv_plan(nchains, chain_len, max_lag, &p);
    out[0] = p.n;
    out[1] = p.m;
    out[2] = p.T;
    out[3] = p.seq_start[0];
    if (seq_start) std::memcpy(seq_start, p.seq_start.data(), sizeof(int64_t) * (size_t)p.m);
    if (tau_floor) *tau_floor = p.tau_floor;
    return TD_OK;
}

extern "C" int tdt_set_convergence_round(td_ctx *ctx, int64_t R) {
    if (!ctx || R < 0 || (R & 1) || R > INT32_MAX / 2) return TD_ERR_ARG;
    ctx->conv_round = R;
    return TD_OK;
}

extern "C" int tdt_set_convergence_lag_block(td_ctx *ctx, int LB) {
    if (!ctx || (LB != 0 && LB != 8 && LB != 16)) return TD_ERR_ARG;
    ctx->conv_lb = LB;
    return TD_OK;
}
