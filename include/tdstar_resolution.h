/*
 * tdstar_resolution.h -- posterior resolution: how far from every node of a
 * lattice the ensemble ties zeta together, in which direction, and where the
 * answer is unknown because the lattice or the window ends.  td_covariance
 * (include/tdstar.h) gives the correlation of a few targets with every node;
 * these entry points give, for EVERY node, its correlation with each neighbour
 * inside a window of lattice offsets, and reduce the rows on the device.
 *
 * A header of its own, which tdstar.h does not include: the catalogue of
 * tests/context_ops.py lists every td_* of tdstar.h, and the two entry points
 * below have cross-call tests of their own (tests/test_gpu_resolution_state.py;
 * DESIGN 4.6m, as 4.6h).  TDSTAR_ABI_VERSION is unchanged: nothing existing moved.
 *
 *   td_rasterize_resolution takes td_rasterize's models, td_history_resolution
 * the samples of the histories, history by history, where they lie (one
 * without samples is skipped; a history need not belong to ctx, it must only
 * live on ctx's device).
 *
 *   Contract (M = the number of models).
 *   Lattice: xs[nx] x ys[ny] x zs[nz], each vector finite and strictly
 * increasing, n* >= 1.  Node n = i + nx (j + ny k), x fastest; nq = nx ny nz.
 * V[m][n] is model m's nearest-cell zeta at node n, m_n and s_n the mean and
 * the corrected sigma of column n: td_rasterize_volume's values and statistics
 * (the same sweep, the same kernel), so mean_out and std_out are its.
 *   Offsets: off[noff][3] = int32 triples (di, dj, dk), 1 <= noff <= 4096,
 * every one forward (dk > 0, or dk == 0 and dj > 0, or dk == dj == 0 and
 * di > 0), none twice.  For |di| < nx, |dj| < ny, dk < nz the flat offset
 * f(o) = di + nx (dj + ny dk) is positive.  An offset outside those bounds is
 * legal: no pair of it lies on the lattice, its rows are NaN, it costs no
 * device work.  The pair (n, o) is on the lattice when 0 <= i + di < nx,
 * 0 <= j + dj < ny and k + dk < nz; its partner is n + f(o).
 *   Moments, per pair on the lattice:
 *     S[o][n]    = sum over m of (V[m][n] - m_n) * (V[m][n + f] - m_{n + f})
 *     cov[o][n]  = S / (double)(M - 1)
 *     corr[o][n] = cov / (s_n * s_{n + f})
 * in td_rasterize's association (M < 16: left to right; else pairwise halves
 * at (lo + hi) >> 1 down to blocks of at most 1024, each left to right), no
 * FMA, each factor one subtraction, the product of the sigmas formed first,
 * nothing clamped.  A pair off the lattice gives NaN in both rows, M = 1 gives
 * NaN (0 / 0), a zero sigma gives what the division gives.  corr[o][n] is, bit
 * for bit, td_covariance's corr[t][n + f] for a point target at node n, and
 * its corr[t'][n] for a point target at node n + f.
 *   Summaries.  pass(o, n): the pair is on the lattice and corr[o][n] >=
 * threshold (IEEE: a NaN fails).
 *   footprint[n]   acc = w[n]; for the offsets in list order: if pass(o, n),
 *                  acc += w[n + f]; then, if n - f is the owner of a pair of o
 *                  on the lattice whose partner is n, and pass(o, n - f),
 *                  acc += w[n - f].  FP64 additions, left to right.  w =
 *                  weights[nq] (finite), NULL: 1.0 everywhere.
 *   run[a][0][n]   axis a in {0: x, 1: y, 2: z}, e_a its unit offset: the
 *                  largest r >= 0 such that for every l in 1 .. r the offset
 *                  l e_a is in the list and pass(l e_a, n).
 *   run[a][1][n]   the same backwards: the pair (n - l e_a, l e_a) is on the
 *                  lattice and passes.
 *   extent[a][n]   coord_a[idx_a + run[a][0][n]] - coord_a[idx_a - run[a][1][n]],
 *                  one FP64 subtraction (idx_a: the node's index along a).
 *   censored[n]    bit 2a: the plus run along a ended because (r + 1) e_a is
 *                  not in the list or its pair is off the lattice, and not on a
 *                  failing correlation; bit 2a + 1: the same for the minus run.
 *                  An axis with no offset in the list gives run 0 and both
 *                  bits; M = 1 gives run 0 and the lattice-edge bits alone.
 *   The plan (tdt_resolution_plan; csrc/resolution.h).  Every partner lies
 * ahead of its owner in flat order, within reach = the largest f(o) of the
 * offsets inside the bounds above (0 when there is none).  The nodes are swept
 * once each, in blocks of ns consecutive flat nodes (a multiple of 64), each a
 * dense value matrix of its own; R = ceil(reach / ns) + 1 blocks are resident,
 * block b in slot b mod R, and block b's pairs are formed when the blocks up to
 * b + R - 1 have been swept.  ns = the largest multiple of 64, at most
 * tdt_volume_plan's ceiling of a slab and the lattice rounded up to 64, with
 * 8 M ns R <= budget (default 2 GiB); tdt_set_volume_slab_nodes forces ns
 * (rounded down to a multiple of 64, at least 64, at most the ceiling) whatever
 * the budget.  tdt_set_volume_method and _counting are honoured.  No result
 * depends on ns.
 *   TD_ERR_ARG, before any HIP call (the message, which names the entry
 * point, through td_last_error(NULL) without a context), in this order: want
 * NULL; noff < 1 or > 4096; off NULL; an offset that is not forward, or one
 * that appears twice; a NaN threshold; no output asked for; a weight that is
 * not finite (looked at when nx, ny, nz >= 1 and nx ny nz fits 64 bits: the
 * lattice's own refusals follow); nx, ny or nz < 1; xs, ys or zs NULL; a
 * vector that is not finite or not strictly increasing; nx ny nz beyond 64
 * bits; only one of mean_out / std_out; offsets not monotone; no model or no
 * sample in all; a history on another device; ctx NULL.  Then, still before
 * any HIP call: more than 2^25 models; an axis of more than 2^30 nodes; rows
 * cov or corr [noff][nq] of more than 1 GiB (8 noff nq bytes: they are kept on
 * the device for the whole call); no block of 64 nodes whose ring fits the
 * budget (the message names M and reach).  A refused call changes nothing.
 * (csrc/resolution.hip)
 */
#ifndef TDSTAR_RESOLUTION_H
#define TDSTAR_RESOLUTION_H
#include <stdint.h>

#include "tdstar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TD_RESOLUTION_MAX_OFFSETS 4096

typedef struct td_resolution {
    const double *xs, *ys, *zs; int64_t nx, ny, nz; /* the lattice, x fastest                              */
    const int32_t *off;         int64_t noff;       /* [noff][3] = (di, dj, dk), forward, none twice       */
    double threshold;                               /* c of pass(o, n); not NaN                            */
    const double *weights;                          /* [nq], finite; nullable: 1.0 everywhere              */
    double *cov_out, *corr_out;                     /* [noff][nq], each nullable                           */
    double *footprint_out;                          /* [nq], nullable                                      */
    int32_t *run_out;                               /* [3][2][nq], nullable                                */
    double *extent_out;                             /* [3][nq], nullable                                   */
    int32_t *censored_out;                          /* [nq], nullable                                      */
    double *mean_out, *std_out;                     /* [nq], nullable (both or neither)                    */
} td_resolution;
int td_rasterize_resolution(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                            const double *yCell, const double *zCell, const double *zeta, const td_resolution *want);
int td_history_resolution(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_resolution *want);

/* Testing hook, pure host code (it stands here, not in tdstar_testing.h, which the chain sources include).
 * What (nmodels, nq nodes, reach), the budget in bytes of the resident blocks' value matrices (0: the default,
 * 2 GiB) and a forced block size (0: none; tdt_set_volume_slab_nodes sets it for a context) decide, out = {ns:
 * the nodes of a block, R: the resident blocks, the blocks covering [0, nq)}.  TD_ERR_ARG: out NULL, nmodels < 1,
 * nq < 1 or > 2^56, reach < 0 or >= nq, budget < 0, forced < 0, or no block of 64 nodes fits the budget. */
int tdt_resolution_plan(int64_t nmodels, int64_t nq, int64_t reach, int64_t budget, int64_t forced, int64_t out[3]);
/* Testing hook: the budget in bytes of the resident blocks for ctx's calls (0: the default) and the form of the pair
 * kernel (0: the kept choice -- x-runs of two offsets and more, the plain form for the lone ones; 1: the plain form for
 * every offset -- one partner load per offset; 2: the x-run form for every run -- the offsets that differ in di alone
 * are served from one staged segment).  No result depends on either.  TD_ERR_ARG: ctx NULL,
 * budget < 0, form not 0 .. 2. */
int tdt_set_resolution(td_ctx *ctx, int64_t budget, int form);

#ifdef __cplusplus
}
#endif
#endif /* TDSTAR_RESOLUTION_H */
