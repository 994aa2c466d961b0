/*
 * tdstar_regions.h -- posterior region averages: one number per sample and
 * region.  The other posterior entry points answer questions about single
 * points; the average of a region is a functional of EACH sample, whose
 * distribution over the samples depends on how the nodes co-vary, so neither
 * its sigma nor P(A > B) can be read off the per-node maps.  The reference
 * has no counterpart (its allaveatten, MCsub.jl:162, is one such path
 * average per trace): the definition below is the contract.
 *
 * A header of its own, which tdstar.h does not include, for the reason
 * tdstar_interfaces.h gives: the catalogue of tests/context_ops.py lists
 * every td_* of tdstar.h, and the two entry points below have cross-call
 * tests of their own (tests/test_gpu_regions_state.py).  Folding this header
 * into tdstar.h, with catalogue entries, is a later change.
 * TDSTAR_ABI_VERSION is unchanged: nothing existing moved.
 *
 *   td_rasterize_regions takes td_rasterize's models and, as
 * td_rasterize_volume does, the chains as (nchains, chain_len) behind them
 * (0 / NULL: none; they are read only for want->conv); td_history_regions
 * takes the samples of the histories, history by history, where they lie, one
 * history being one chain (one without samples is skipped; a history need not
 * belong to ctx, it must only live on ctx's device).
 *
 *   Contract (M = the number of models, R = nreg >= 1).
 *   Region r is the points p in [reg_off[r], reg_off[r + 1]) of px, py, pz
 * [np] and w [np]: reg_off[0] = 0, reg_off is monotone, every region holds at
 * least one point, reg_off[nreg] = np.  A point may appear in several regions
 * by being listed again.  w may be NULL: 1.0 everywhere, bit-identical to an
 * array of ones.  Every weight is finite; negative weights are legal (a region
 * may be a contrast).
 *   V[m][p] is model m's nearest-cell zeta at point p, td_rasterize's value
 * under td_rasterize's rules (the lexicographic minimum of (FP64 squared
 * distance, cell index) below the 1e9 sentinel, a NaN distance never wins, no
 * answer gives 0.0, a NaN zeta is a value like any other).
 *     t[m][p]       = w[p] * V[m][p]                 one FP64 multiply, no FMA
 *     S[m][r]       = sum over the region's points of t[m][p]
 *     W[r]          = sum over the region's points of w[p]
 *     F[m][r]       = normalize ? S[m][r] / W[r] : S[m][r]
 *                     one FP64 division, nothing clamped (W[r] == 0 gives what
 *                     the division gives)
 *     greater[a][b] = #{m : F[m][a] > F[m][b]}       IEEE: NaN > x is false;
 *                     the diagonal is 0
 *   Both sums run in td_rasterize's association over the index WITHIN the
 * region: fewer than 16 terms left to right; else pairwise halves at
 * (lo + hi) >> 1 down to blocks of at most 1024, each left to right.
 *   series_out = F [M][nreg], weight_out = W.  On the matrix F, with the
 * regions in the place of a volume's nodes: mean_out / std_out are
 * td_rasterize's (the same kernel), marg the quantile rows [nprob][nreg] and
 * histograms [nreg][nbins + 3] of a td_marginals, conv the R-hat, ESS and lags
 * [nreg] of a td_convergence over the chains.
 *   The search structure and the slabs (of the point list's columns) are the
 * posterior volumes' (the value matrix never exists whole;
 * tdt_set_volume_slab_nodes, _method and _counting are honoured,
 * tdt_volume_counters reports this call's sweeps), and the results depend on
 * none of them.
 *   TD_ERR_ARG, before any HIP call (the message, which names the entry
 * point, through td_last_error(NULL) without a context), in this order: want
 * NULL; np < 1 or nreg < 1; px, py, pz or reg_off NULL; reg_off[0] != 0, not
 * monotone, an empty region, or reg_off[nreg] != np; a coordinate or a weight
 * that is not finite; normalize not 0 or 1; no output asked for; only one of
 * mean_out / std_out; a marg or conv that td_rasterize_marginals /
 * td_convergence_values would refuse; conv given without chains (or with
 * chains that td_rasterize_volume would refuse); offsets not monotone; no
 * model or no sample in all; a history on another device; ctx NULL.  Then,
 * with a message and never attempted: more than 2^18 regions (one slab's
 * columns of the statistics), 8 M nreg bytes of F or 8 M leaves bytes of the
 * sums' workspace (a leaf: a block of at most 1024 points of a region) beyond
 * 1 GiB, and greater_out of more than 2^27 counters (1 GiB).  A refused call
 * changes nothing.  (csrc/regions.hip)
 */
#ifndef TDSTAR_REGIONS_H
#define TDSTAR_REGIONS_H
#include <stdint.h>

#include "tdstar.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct td_regions {
    const double *px, *py, *pz, *w;  int64_t np;   /* the points; w nullable (1.0 everywhere)               */
    const int64_t *reg_off;          int64_t nreg; /* [nreg + 1], region r = [reg_off[r], reg_off[r + 1])    */
    int64_t normalize;                              /* 0: the weighted sum, 1: divided by W[r]                */
    double *series_out;                             /* [M][nreg] F, nullable                                  */
    double *weight_out;                             /* [nreg] W, nullable                                     */
    double *mean_out, *std_out;                     /* [nreg], nullable (both or neither)                     */
    int64_t *greater_out;                           /* [nreg][nreg], nullable                                 */
    const td_marginals *marg;                       /* nullable; rows of nreg columns                         */
    const td_convergence *conv;                     /* nullable; needs chains                                 */
} td_regions;
int td_rasterize_regions(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                         const double *yCell, const double *zCell, const double *zeta, int64_t nchains,
                         const int64_t *chain_len, const td_regions *want);
int td_history_regions(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_regions *want);

/* Testing hook, pure host code.  What (nmodels, np points), the budget in bytes of a slab's value matrix (0: the
 * default, 1 GiB) and a forced slab size (0: none; tdt_set_volume_slab_nodes sets it for a context) decide, out =
 * {the columns (points) of a slab, slabs}: tdt_volume_plan's numbers with the point list in the place of the
 * nodes. */
int tdt_regions_plan(int64_t nmodels, int64_t np, int64_t budget, int64_t forced, int64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* TDSTAR_REGIONS_H */
