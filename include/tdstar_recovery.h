/*
 * tdstar_recovery.h -- posterior recovery: an ensemble held against a model
 * that is KNOWN (a checkerboard or spike test, a synthetic recovery, another
 * study's volume).  Every other posterior entry point describes an ensemble by
 * itself.  The questions of a recovery test are per-sample or per-rank
 * quantities that the per-node maps cannot answer: where in the sample at a
 * node the true value falls (ties with the truth decide it, so interpolated
 * quantiles cannot give it), and how far every single sample is from the truth
 * over a region (a mean SQUARE, non-linear in zeta, so td_regions, which is
 * linear, cannot form it).  The reference has the intent
 * (load_synthetic_data_Tonga, load_data_Tonga.jl:86-166) and no scoring: the
 * definition below is the contract.
 *
 * A header of its own, which tdstar.h does not include, for the reason
 * tdstar_regions.h gives: the catalogue of tests/context_ops.py lists every
 * td_* of tdstar.h, and the two entry points below have cross-call tests of
 * their own (tests/test_gpu_recovery_state.py).  Folding this header into
 * tdstar.h, with catalogue entries, is a later change.
 * TDSTAR_ABI_VERSION is unchanged: nothing existing moved.
 *
 *   td_rasterize_recovery takes td_rasterize's models and, as
 * td_rasterize_volume does, the chains as (nchains, chain_len) behind them
 * (0 / NULL: none; they are read only for want->conv); td_history_recovery
 * takes the samples of the histories, history by history, where they lie, one
 * history being one chain (one without samples is skipped; a history need not
 * belong to ctx, it must only live on ctx's device).
 *
 *   Contract (M = the number of models, R = nreg >= 1).
 *   The point list and the regions are td_regions' exactly: region r is the
 * points p in [reg_off[r], reg_off[r + 1]) of px, py, pz [np] and w [np];
 * reg_off[0] = 0, reg_off is monotone, every region holds at least one point,
 * reg_off[nreg] = np; a point may appear in several regions by being listed
 * again; w may be NULL: 1.0 everywhere, bit-identical to an array of ones;
 * every weight is finite.  truth [np] is the known model's value at each
 * listed point, finite.
 *   V[m][p] is model m's nearest-cell zeta at point p, td_rasterize's value
 * under td_rasterize's rules (the lexicographic minimum of (FP64 squared
 * distance, cell index) below the 1e9 sentinel, a NaN distance never wins, no
 * answer gives 0.0, a NaN zeta is a value like any other).
 *     D[m][p]     = V[m][p] - truth[p]              one FP64 subtraction
 *     below[p]    = #{m : V[m][p] <  truth[p]}      IEEE comparisons: a NaN V
 *     equal[p]    = #{m : V[m][p] == truth[p]}      counts in none of the three;
 *     above[p]    = #{m : V[m][p] >  truth[p]}      -0.0 == 0.0
 *     dmean, dstd = td_rasterize's mean and sigma (the same kernel) of column p
 *                   of D
 *     u[m][p]     = D * D;  t[m][p] = w[p] * u[m][p]   two FP64 multiplies,
 *                   each rounded, no FMA
 *     S[m][r]     = sum over the region's points of t[m][p]
 *     W[r]        = sum over the region's points of w[p]
 *     F[m][r]     = normalize ? S[m][r] / W[r] : S[m][r]
 *                   one FP64 division, nothing clamped
 *   Both sums run in td_rasterize's association over the index WITHIN the
 * region: fewer than 16 terms left to right; else pairwise halves at
 * (lo + hi) >> 1 down to blocks of at most 1024, each left to right.
 *   below_out, equal_out, above_out: int64 [np].  dmean_out, dstd_out [np].
 * series_out = F [M][nreg], weight_out = W.  On the matrix F, with the regions
 * in the place of a volume's nodes, exactly as td_regions does on its F:
 * mean_out / std_out are td_rasterize's (the same kernel), marg the quantile
 * rows [nprob][nreg] and histograms [nreg][nbins + 3] of a td_marginals, conv
 * the R-hat, ESS and lags [nreg] of a td_convergence over the chains.  The
 * square root of F (the RMS distance) is the caller's to take.
 *   The search structure and the slabs (of the point list's columns) are the
 * posterior volumes' (the value matrix never exists whole;
 * tdt_set_volume_slab_nodes, _method and _counting are honoured,
 * tdt_volume_counters reports this call's sweeps, tdt_regions_plan gives the
 * plan), and the results depend on none of them.
 *   TD_ERR_ARG, before any HIP call (the message, which names the entry
 * point, through td_last_error(NULL) without a context), in this order: want
 * NULL; np < 1 or nreg < 1; px, py, pz, reg_off or truth NULL; reg_off[0] != 0,
 * not monotone, an empty region, or reg_off[nreg] != np; a coordinate, a weight
 * or a truth value that is not finite (px, py, pz, w, truth in this order);
 * normalize not 0 or 1; no output asked for; only one of dmean_out / dstd_out;
 * only one of mean_out / std_out; a marg or conv that td_rasterize_marginals /
 * td_convergence_values would refuse; conv given without chains (or with
 * chains that td_rasterize_volume would refuse); offsets not monotone; no
 * model or no sample in all; a history on another device; ctx NULL.  Then,
 * with a message and never attempted: more than 2^18 regions (one slab's
 * columns of the statistics), 8 M nreg bytes of F or 8 M leaves bytes of the
 * sums' workspace (a leaf: a block of at most 1024 points of a region) beyond
 * 1 GiB.  A refused call changes nothing.  (csrc/recovery.hip)
 */
#ifndef TDSTAR_RECOVERY_H
#define TDSTAR_RECOVERY_H
#include <stdint.h>

#include "tdstar.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct td_recovery {
    const double *px, *py, *pz, *w;  int64_t np;   /* the points; w nullable (1.0 everywhere)               */
    const int64_t *reg_off;          int64_t nreg; /* [nreg + 1], region r = [reg_off[r], reg_off[r + 1])    */
    const double *truth;                            /* [np] the known model's value at each point             */
    int64_t normalize;                              /* 0: the weighted sum of squares, 1: divided by W[r]     */
    int64_t *below_out, *equal_out, *above_out;     /* [np], each nullable                                    */
    double *dmean_out, *dstd_out;                   /* [np], nullable (both or neither)                       */
    double *series_out;                             /* [M][nreg] F, nullable                                  */
    double *weight_out;                             /* [nreg] W, nullable                                     */
    double *mean_out, *std_out;                     /* [nreg], nullable (both or neither)                     */
    const td_marginals *marg;                       /* nullable; rows of nreg columns                         */
    const td_convergence *conv;                     /* nullable; needs chains                                 */
} td_recovery;
int td_rasterize_recovery(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                          const double *yCell, const double *zCell, const double *zeta, int64_t nchains,
                          const int64_t *chain_len, const td_recovery *want);
int td_history_recovery(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_recovery *want);

#ifdef __cplusplus
}
#endif
#endif /* TDSTAR_RECOVERY_H */
