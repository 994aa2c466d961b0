/*
 * tdstar_gram.h -- ensemble Gram and distance matrices: the M x M inner
 * products, or squared distances, between the samples' rasterised volumes.
 * The other posterior entry points answer questions about nodes or about
 * regions named beforehand; the principal components of the ensemble (which
 * whole-volume patterns the data leave undetermined), its medoid (the sample
 * that represents it) and the distance between chains in model space all
 * come from this one matrix, which is formed here without the value matrix
 * ever reaching the host.  The reference has no counterpart: the definition
 * below is the contract.
 *
 * A header of its own, which tdstar.h does not include, for the reason
 * tdstar_interfaces.h gives: the catalogue of tests/context_ops.py lists
 * every td_* of tdstar.h, and the two entry points below have cross-call
 * tests of their own (tests/test_gpu_gram_state.py).  Folding this header
 * into tdstar.h, with catalogue entries, is a later change.
 * TDSTAR_ABI_VERSION is unchanged: nothing existing moved.
 *
 *   td_rasterize_gram takes td_rasterize's models; td_history_gram takes the
 * samples of the histories, history by history, where they lie (one without
 * samples is skipped; a history need not belong to ctx, it must only live on
 * ctx's device).
 *
 *   Contract (M = the number of models, np >= 1 points px, py, pz, w [np]).
 *   w may be NULL: 1.0 everywhere, bit-identical to an array of ones.  Every
 * weight is finite and >= 0: a Gram matrix and a distance need a norm, so a
 * contrast (a negative weight, which td_rasterize_regions accepts) is refused.
 *   V[m][p] is model m's nearest-cell zeta at point p, td_rasterize's value
 * under td_rasterize's rules (the lexicographic minimum of (FP64 squared
 * distance, cell index) below the 1e9 sentinel, a NaN distance never wins, no
 * answer gives 0.0, a NaN zeta is a value like any other).  mean[p] and std[p]
 * are td_rasterize's over the models, from the same kernel.
 *     r[p]        = sqrt(w[p])                       the correctly rounded IEEE
 *                   square root, taken once on the host
 *     X[m][p]     = r[p] * (V[m][p] - mean[p])       one subtraction, then one
 *                   multiply, no FMA
 *     gram[a][b]  = sum over p of X[a][p] * X[b][p]
 *     dist2[a][b] = sum over p of e * e, e = X[a][p] - X[b][p]
 *                   every operation rounded once, no FMA
 *     W           = sum over p of w[p] in td_rasterize's association (fewer
 *                   than 16 terms left to right; else pairwise halves at
 *                   (lo + hi) >> 1 down to blocks of at most 1024, each left
 *                   to right): td_rasterize_regions' W[r] of one region
 *   Both matrices are symmetric bit for bit by the arithmetic itself (IEEE
 * multiplication commutes, (a - b)^2 and (b - a)^2 round alike); dist2's
 * diagonal is +0.0 unless a NaN reaches it.  A NaN zeta is a value like any
 * other: it spreads along the rows and columns of its model, and, where its
 * cell owns a point, through mean[p] to every model's X there and so to
 * every entry.
 *   Association over p, of both sums: the points in list order in blocks of
 * 64.  A block's sum runs left to right from its first term; the block sums
 * are added in block order to an accumulator that starts at +0.0.  (The last
 * block holds what is left.)  This is the order a register-tiled kernel runs
 * in with p innermost, with one more addition per 64 points; it excludes the
 * FP64 matrix instruction, whose fused products and internal order this header
 * does not fix.
 *   gram_out and dist2_out are [M][M] row-major, mean_out and std_out [np],
 * wsum_out [1] = W.
 *   The search structure and the slabs (of the point list's columns, a
 * multiple of 64 so that no block straddles two) are the posterior volumes'
 * (the value matrix never exists whole; tdt_set_volume_slab_nodes, _method
 * and _counting are honoured, tdt_volume_counters reports this call's sweeps),
 * and the results depend on none of them, nor on the kernel's tiling
 * (tdt_set_gram_form).
 *   TD_ERR_ARG, before any HIP call (the message, which names the entry
 * point, through td_last_error(NULL) without a context), in this order: want
 * NULL; np < 1; px, py or pz NULL; a coordinate that is not finite; a weight
 * that is not finite or is negative; no output asked for; only one of
 * mean_out / std_out; offsets not monotone; no model or no sample in all; a
 * history on another device; ctx NULL.  Then, with a message and never
 * attempted: 8 M^2 bytes of a matrix that is asked for beyond 1 GiB (M >
 * 11585; each matrix has a GiB of its own, apart from the slab's).  A refused call changes
 * nothing.  (csrc/gram.hip)
 */
#ifndef TDSTAR_GRAM_H
#define TDSTAR_GRAM_H
#include <stdint.h>

#include "tdstar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TD_GRAM_MAX_MODELS 11585 /* 8 M^2 <= 1 GiB */

typedef struct td_gram {
    const double *px, *py, *pz, *w;  int64_t np;   /* the points; w nullable (1.0 everywhere) */
    double *gram_out;                               /* [M][M], nullable                        */
    double *dist2_out;                              /* [M][M], nullable                        */
    double *mean_out, *std_out;                     /* [np], nullable (both or neither)        */
    double *wsum_out;                               /* [1] W, nullable                         */
} td_gram;
int td_rasterize_gram(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell, const double *yCell,
                      const double *zCell, const double *zeta, const td_gram *want);
int td_history_gram(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_gram *want);

/* Testing hooks, pure host code.
 * tdt_gram_plan: what (nmodels, np points), the budget in bytes of a slab's value matrix (0: the default, 1 GiB)
 * and a forced slab size (0: none; tdt_set_volume_slab_nodes sets it for a context) decide, out = {the columns
 * (points) of a slab, slabs}: tdt_volume_plan's numbers with the point list in the place of the nodes.
 * tdt_set_gram_form: the pair kernel's register tile, process-wide; no answer depends on it.  0: the kept one,
 * 1: 4 x 4 pairs a lane (a workgroup owns 64 x 64), 2: 8 x 8 (128 x 128).  tdt_gram_tile: the rows of a workgroup's
 * tile under a form (0: the kept one's), -1 for a form that does not exist.
 * tdt_gram_tiles: the tiles of the lower triangle for M models under a form, and through out (nullable, [2]) the
 * (row tile, column tile) of tile `index`: the kernel's own bookkeeping, for tests. */
int tdt_gram_plan(int64_t nmodels, int64_t np, int64_t budget, int64_t forced, int64_t out[2]);
int tdt_set_gram_form(int form);
int tdt_gram_tile(int form);
int64_t tdt_gram_tiles(int64_t nmodels, int form, int64_t index, int64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* TDSTAR_GRAM_H */
