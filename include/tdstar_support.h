/*
 * tdstar_support.h -- posterior data support: which cells, and through them
 * which nodes, the rays of a context constrain, per sample.  Every other
 * posterior product says what the ensemble holds about zeta at a node; this
 * one says whether the data said anything there.  A Voronoi cell that owns no
 * ray point does not enter td_evaluate at all: its zeta is a prior draw in
 * every sample, and a node it owns shows the prior.  The reference's only
 * guard is poststd > 5 -> NaN (MCsub.jl:776-782), which a node that the data
 * constrain to a bimodal answer fails as well.  The reference has no
 * counterpart: the definition below is the contract.
 *
 * A header of its own, which tdstar.h does not include, for the reason
 * tdstar_regions.h gives: the catalogue of tests/context_ops.py lists every
 * td_* of tdstar.h, and the two entry points below have cross-call tests of
 * their own (tests/test_gpu_support_state.py).  TDSTAR_ABI_VERSION is
 * unchanged: nothing existing moved.
 *
 *   td_rasterize_support takes td_rasterize_volume's models WITHOUT zeta (it
 * is not an input) and the chains as (nchains, chain_len) behind them (0 /
 * NULL: none; read only for want->conv); td_history_support takes the samples
 * of the histories, history by history, where they lie, one history being one
 * chain (one without samples is skipped; a history need not belong to ctx, it
 * must only live on ctx's device).  ctx is required: its rays are the data.
 *
 *   Contract (M = the number of models, P = td_info.npoints of ctx, the valid
 * ray points ray-major: td_evaluate's nearest_out order).
 *   Owner.  owner[m][p] is the cell td_evaluate picks for ray point p in model
 * m: the lexicographic minimum of (FP64 squared distance, cell index) below
 * the 1e9 sentinel, a NaN distance never wins.  Where no cell is below the
 * sentinel (a metre frame, a model of 0 cells) the point has no owner.
 *   Quantised weights, fixed once per call on the host, so that every sum
 * below is an exact integer sum and therefore independent of its order:
 *     A    = sum over p of |w[p]|, left to right in FP64
 *     A    = f 2^E with 0.5 <= f < 1 (frexp);  e = 61 - E, and e = 0 when A == 0
 *     k[p] = llrint(ldexp(w[p], e))            round to nearest, ties to even
 *   w == NULL means k[p] = 1 and e = 0, which gives outputs bit-identical to
 * an array of ones (A = P = f 2^E, k[p] = 2^(61 - E), K = count 2^(61 - E),
 * sup = count exactly in both).  Negative and zero weights are legal.  A
 * positive weight below 2^(-e-1), that is below about A 2^-62, quantises to 0
 * and supports nothing; so does a negative one above -2^(-e-1).
 *   Per cell c (ensemble order: the models' cells behind one another):
 *     K[c]       = sum over the points c owns of k[p]       int64; cannot
 *                  overflow: sum |k| < 2^61 + P when A is exact, and A,
 *                  a rounded sum, is exact to P 2^-53 relative (P < 2^31)
 *     count[c]   = the number of points c owns
 *     sup[c]     = ldexp((double)K[c], -e)                   one conversion,
 *                  round to nearest even; the scaling is exact
 *     barren[m]  = #{c of model m : count[c] == 0}
 *     orphans[m] = the number of points without owner in model m
 *   Per node q (nq of them; nq == 0: only the outputs above):
 *     U[m][q]    = sup[the cell td_rasterize picks for node q in model m], and
 *                  0.0 where it picks none
 *     exceed[t][q] = #{m : U[m][q] > thr[t]}                 IEEE, strict
 *   mean_out / std_out are td_rasterize's of the matrix U (the same kernel),
 * marg the quantile rows [nprob][nq] and histograms [nq][nbins + 3] of a
 * td_marginals, conv the R-hat, ESS and lags [nq] of a td_convergence over the
 * chains.
 *   The search structure and the slabs (of the ray points, then of the nodes)
 * are the posterior volumes' (tdt_set_volume_slab_nodes, _method and _counting
 * are honoured, tdt_volume_counters reports this call's sweeps), and the
 * results depend on none of them, nor on tdt_set_support_scatter.
 *   TD_ERR_ARG, before any HIP call (the message, which names the entry
 * point, through td_last_error(NULL) without a context), in this order: want
 * NULL; nq < 0, or nq > 0 with qx, qy or qz NULL; nthr < 0, or nthr > 0 with
 * thr or exceed_out NULL; a node coordinate (qx, then qy, then qz), then a
 * threshold, then a weight that is not finite, then A not finite (w is read
 * only with a context: it holds P numbers, and without a context the call is
 * refused at the end of this list whatever w holds); no output asked for; with
 * nq == 0 an output that needs nodes (values_out, mean_out, std_out, marg,
 * conv; thresholds need nq > 0 too); only one of mean_out / std_out; a marg or
 * conv that td_rasterize_marginals / td_convergence_values would refuse; conv
 * given without chains (or with chains that td_rasterize_volume would
 * refuse); offsets not monotone; no model or no sample in all; a history on
 * another device; ctx NULL.  Then, with a message and never attempted: what
 * the volume call refuses (too many models, a model of too many cells), and
 * accumulators (8 + 4 bytes per cell of all models) beyond 1 GiB.  A refused
 * call changes nothing.  (csrc/support.hip)
 */
#ifndef TDSTAR_SUPPORT_H
#define TDSTAR_SUPPORT_H
#include <stdint.h>

#include "tdstar.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct td_support {
    const double *w;                        /* [P] per ray point, ray-major valid points; NULL: 1.0   */
    const double *qx, *qy, *qz; int64_t nq; /* nodes; nq == 0: only the per-cell / per-model outputs  */
    const double *thr; int64_t nthr;        /* thresholds on the node support, nullable / 0           */
    double *cell_out;                       /* [total cells] sup, ensemble order, nullable            */
    int64_t *count_out;                     /* [total cells] ray points owned, nullable               */
    int64_t *barren_out;                    /* [M] cells with count == 0, nullable                    */
    int64_t *orphans_out;                   /* [M] ray points no cell owns, nullable                  */
    double *values_out;                     /* [M][nq] U, nullable                                    */
    double *mean_out, *std_out;             /* [nq], nullable (both or neither)                       */
    int64_t *exceed_out;                    /* [nthr][nq] #{m : U[m][q] > thr[t]}                     */
    const td_marginals *marg;               /* nullable; rows of nq columns                           */
    const td_convergence *conv;             /* nullable; needs chains                                 */
} td_support;
int td_rasterize_support(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                         const double *yCell, const double *zCell, int64_t nchains, const int64_t *chain_len,
                         const td_support *want);
int td_history_support(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_support *want);

/* Testing hooks.  The most cells of a model whose sums the scatter kernel keeps in LDS (pure host code). */
int64_t tdt_support_lds_cells(void);
/* How the scatter kernel adds: 0 auto, 1 in LDS where the model's cells fit, 2 with atomics on the global arrays
 * always.  Same answer.  Kept beside the context until set again: set it back to 0 before td_destroy. */
int tdt_set_support_scatter(td_ctx *ctx, int mode);
/* The quantisation above on n weights (pure host code): k_out [n] and *e_out; TD_ERR_ARG where a weight or A is not
 * finite, and then nothing is written. */
int tdt_support_quantise(const double *w, int64_t n, int64_t *k_out, int64_t *e_out);

#ifdef __cplusplus
}
#endif
#endif /* TDSTAR_SUPPORT_H */
