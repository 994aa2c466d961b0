/*
 * tdstar_compare.h -- posterior comparison: one ensemble held against ANOTHER
 * (posterior against a debug_prior = 1 ensemble, run against run, zeta_S
 * against zeta_P).  Every other posterior entry point describes one ensemble by
 * itself or against one fixed model (tdstar_recovery.h).  The statistics are
 * two-sample rank statistics -- the probability of superiority (Mann-Whitney
 * U), Kolmogorov-Smirnov, the exceedance of a scaled and shifted difference --
 * and every one of them is an exact integer: the contract is equality, bit for
 * bit.  The reference only plots the prior's histograms
 * (plot_distribution.jl:66-80) and has no two-sample statistic: the definition
 * below is the contract.
 *
 * A header of its own, which tdstar.h does not include, for the reason
 * tdstar_recovery.h gives: the catalogue of tests/context_ops.py lists every
 * td_* of tdstar.h, and the three entry points below have cross-call tests of
 * their own (tests/test_gpu_compare_state.py).  Folding this header into
 * tdstar.h, with catalogue entries, is a later change.
 * TDSTAR_ABI_VERSION is unchanged: nothing existing moved.
 *
 *   td_rasterize_compare takes td_rasterize's models twice, side A and side B;
 * td_history_compare takes the samples of two lists of histories where they
 * lie, history by history (one without samples is skipped; a history need not
 * belong to ctx, it must only live on ctx's device); td_compare_values takes
 * two host matrices A [MA][ncol], B [MB][ncol] (row-major) and runs the same
 * kernels with no search: want->qx, qy, qz and nq are ignored and every output
 * has ncol columns.
 *
 *   Contract (MA, MB = the models of the two sides, 1 .. 16384 each).
 *   Per column q (a node of any node list; a lattice is sent x fastest) a_i,
 * i < MA, is side A's value and b_j, j < MB, side B's: td_rasterize's
 * nearest-cell zeta under td_rasterize's rules (tdstar_recovery.h restates
 * them), or column q of the host matrix.  All comparisons are IEEE: a NaN
 * counts in nothing, -0.0 == 0.0, +-inf are values.
 *     less[q]      = #{(i, j) : a_i <  b_j}
 *     equal[q]     = #{(i, j) : a_i == b_j}
 *     greater[q]   = #{(i, j) : a_i >  b_j}
 *     exceed[k][q] = #{(i, j) : a_i >  fl(fl(scale[k] * b_j) + shift[k])}
 *                    two FP64 operations, each rounded once, no FMA; the pair
 *                    (1, 0) therefore gives greater
 *   Kolmogorov-Smirnov, in int64: cA(x) = #{i : a_i <= x}, cB(x) = #{j : b_j <=
 * x}, T(x) = cA(x) * MB - cB(x) * MA, X = the non-NaN values of both columns;
 *     ks_plus[q]   = max(0, max over X of  T)
 *     ks_minus[q]  = max(0, max over X of -T)
 *     ks_at[q]     = the smallest x of X (by IEEE <; a zero is reported as
 *                    +0.0) at which |T(x)| reaches max(ks_plus, ks_minus); NaN
 *                    (the quiet NaN 0x7ff8000000000000) when that maximum is 0
 * The KS distance is max(ks_plus, ks_minus) / (MA * MB) and the probability of
 * superiority (greater + equal / 2) / (MA * MB); dividing is the caller's.
 *   mean_a, std_a / mean_b, std_b are td_rasterize's mean and sigma (the same
 * kernel) of the side's rows; marg_a / marg_b the quantile rows [nprob][nq] and
 * histograms [nq][nbins + 3] of a td_marginals on the side's rows (the same
 * kernels): bit for bit what td_rasterize_volume / td_history_volume give for
 * that side alone.
 *   All count outputs are int64 [nq], exceed_out [nexceed][nq]; ks_at_out is
 * double [nq].
 *   The two sides are one ensemble of MA + MB models, A first: one search
 * structure and one sweep per slab of the posterior volumes'
 * (tdt_set_volume_slab_nodes, _method and _counting are honoured,
 * tdt_volume_counters reports this call's sweeps; the sorted columns take a
 * slab's bytes again, so the workspace is twice a volume's), and the results
 * depend on neither the slab size, the sweep method nor the order inside a
 * sort.
 *   TD_ERR_ARG, before any HIP call (the message, which names the entry point,
 * through td_last_error(NULL) without a context), in this order: want NULL;
 * nq < 0 (td_compare_values: MA, MB or ncol < 0), nexceed < 0 or > 16; nq > 0
 * without qx, qy, qz (td_compare_values: ncol > 0 and MA, MB > 0 without A or
 * B); nexceed > 0 without scale, shift or exceed_out; a scale that is not
 * finite and > 0, a shift that is not finite; no output asked for; only one of
 * ks_plus_out / ks_minus_out; ks_at_out without them; only one of mean_a_out /
 * std_a_out, then of mean_b_out / std_b_out; a marg_a, then a marg_b, that
 * td_rasterize_marginals would refuse; a NULL history; side A, then side B:
 * no model (nmodels < 1 or no cell_off; MA or MB < 1; histories without a
 * sample), bad or not monotone offsets; side A, then side B, beyond 16384
 * models (never attempted); a history on another device; ctx NULL.  nq == 0
 * (ncol == 0) is then TD_OK and nothing is written.  A refused call changes
 * nothing.  (csrc/compare.hip)
 */
#ifndef TDSTAR_COMPARE_H
#define TDSTAR_COMPARE_H
#include <stdint.h>

#include "tdstar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TD_COMPARE_MAX_EXCEED 16
#define TD_COMPARE_MAX_MODELS 16384

typedef struct td_compare {
    const double *qx, *qy, *qz;  int64_t nq;        /* any node list (unused by td_compare_values)            */
    int64_t nexceed; const double *scale, *shift;   /* 0..16 pairs (s_k, t_k), s_k finite and > 0, t_k finite */
    int64_t *less_out, *equal_out, *greater_out;    /* [nq], each nullable                                    */
    int64_t *exceed_out;                            /* [nexceed][nq]                                          */
    int64_t *ks_plus_out, *ks_minus_out;            /* [nq], nullable (both or neither)                       */
    double  *ks_at_out;                             /* [nq], nullable; needs the two above                    */
    double *mean_a_out, *std_a_out, *mean_b_out, *std_b_out;  /* [nq], per side both or neither               */
    const td_marginals *marg_a, *marg_b;            /* nullable; quant_out [nprob][nq], hist_out [nq][nbins+3] */
} td_compare;
int td_rasterize_compare(td_ctx *ctx, int64_t nA, const int64_t *offA, const double *xA, const double *yA,
                         const double *zA, const double *zetaA, int64_t nB, const int64_t *offB, const double *xB,
                         const double *yB, const double *zB, const double *zetaB, const td_compare *want);
int td_history_compare(td_ctx *ctx, td_history *const *hsA, int64_t nhA, td_history *const *hsB, int64_t nhB,
                       const td_compare *want);
int td_compare_values(td_ctx *ctx, const double *A, int64_t MA, const double *B, int64_t MB, int64_t ncol,
                      const td_compare *want);
/* testing, process-wide, same answer: plain = 1: a workgroup of the sort kernel takes the column of its
 * own index, 0 (default): eight neighbouring columns per XCD; the threads of a workgroup of the sort and of the
 * count kernel, a power of two 64 .. 1024, 0 (default): by the larger side. */
int tdt_set_compare_form(int plain, int sort_threads, int count_threads);

#ifdef __cplusplus
}
#endif
#endif /* TDSTAR_COMPARE_H */
