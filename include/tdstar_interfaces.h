/*
 * tdstar_interfaces.h -- posterior interfaces: where the models of an ensemble
 * put their Voronoi boundaries on a lattice, how large the jump across them
 * is, and where the sampler spends its cells.  The other posterior entry
 * points (include/tdstar.h) read the value at every point and smooth over the
 * boundaries; these read the partition itself.
 *
 * A header of its own, which tdstar.h does not include: the catalogue of
 * tests/context_ops.py lists every td_* of tdstar.h, and the two entry points
 * below have cross-call tests of their own (tests/test_gpu_interfaces_state.py).
 * Folding this header into tdstar.h, with catalogue entries, is a later change
 * (DESIGN 4.6h).  TDSTAR_ABI_VERSION is unchanged: nothing existing moved.
 *
 *   td_rasterize_interfaces takes td_rasterize's models, td_history_interfaces
 * the samples of the histories, history by history, where they lie (one
 * without samples is skipped; a history need not belong to ctx, it must only
 * live on ctx's device).
 *
 *   Contract (M = the number of models).
 *   Lattice: xs[nx] x ys[ny] x zs[nz], each vector finite and strictly
 * increasing, n* >= 1.  Node n = i + nx (j + ny k), x fastest (the order of a
 * posterior volume); nq = nx ny nz is 64-bit and its overflow is refused.
 *   V[m][n] is model m's nearest-cell zeta at node n, td_rasterize's value
 * under td_rasterize's rules (the lexicographic minimum of (FP64 squared
 * distance, cell index) below the 1e9 sentinel, a NaN never wins, no answer
 * gives 0.0).
 *   Faces: axis a in {0: x, 1: y, 2: z} has stride s_a = (1, nx, nx ny); node
 * n has a forward face along a when its index along a is below n_a - 1.  On a
 * face d = V[m][n + s_a] - V[m][n], one FP64 subtraction, |d| = fabs(d); IEEE
 * semantics throughout (NaN != x is true, NaN > t is false).
 *   count[a][n]      the models with V[m][n] != V[m][n + s_a]; -1 without a face
 *   any[n]           the models whose value differs across at least one of n's
 *                    existing forward faces; -1 where n has none
 *   exceed[t][a][n]  the models with |d| > thr[t]; -1 without a face
 *   jump[a][n]       the sum over m of |d| in td_rasterize's association (M < 16:
 *                    left to right; else pairwise halves at (lo + hi) >> 1 down to
 *                    blocks of at most 1024, each left to right), divided by
 *                    (double)M; NaN without a face
 *   mean[n], std[n]  td_rasterize's own (td_rasterize_volume's, same kernel)
 *   density[n]       the cells, over all models, whose nucleus falls in node n's
 *                    voxel (zeta is not looked at): along x a cell's index is the
 *                    number of midpoints 0.5 * (xs[l] + xs[l + 1]), l = 0 .. nx - 2,
 *                    that are <= x -- every finite or infinite x lands somewhere,
 *                    the edge voxels take what lies beyond the hull, an axis of one
 *                    node gives 0.  A cell with a NaN coordinate is counted in
 *                    *skipped and nowhere else:
 *                    sum(density) + skipped == cell_off[nmodels].
 *   The search structure and the slabs are the posterior volumes' (the value
 * matrix never exists whole; tdt_set_volume_slab_nodes, _method and _counting
 * are honoured), a slab being swept with the halo of its forward neighbours
 * (tdt_interfaces_plan), and the results depend on none of them.  More than
 * 2^25 models, a lattice row that does not fit one slab's columns, and a
 * density of more than 2^27 nodes (its counters are one 1 GiB workspace) are
 * TD_ERR_ARG with a message.
 *   TD_ERR_ARG, before any HIP call (the message, which names the entry
 * point, through td_last_error(NULL) without a context), in this order: want
 * NULL; nx, ny or nz < 1; xs, ys or zs NULL; a vector that is not finite or
 * not strictly increasing; nx ny nz beyond 64 bits; nthr < 0 or > 8; thr NULL
 * with nthr > 0; a threshold that is not finite or < 0; exceed_out given
 * without thresholds or missing with them; no output asked for; only one of
 * mean_out / std_out; skipped_out without density_out; offsets not monotone;
 * no model or no sample in all; a history on another device; ctx NULL.  A
 * refused call changes nothing.  (csrc/interfaces.hip)
 */
#ifndef TDSTAR_INTERFACES_H
#define TDSTAR_INTERFACES_H
#include <stdint.h>

#include "tdstar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TD_INTERFACES_MAX_THR 8

typedef struct td_interfaces {
    const double *xs, *ys, *zs; int64_t nx, ny, nz; /* the lattice, x fastest                              */
    const double *thr;          int64_t nthr;       /* 0 .. 8 thresholds, nullable when nthr == 0          */
    int64_t *count_out;                             /* [3][nq], nullable                                   */
    int64_t *any_out;                               /* [nq], nullable                                      */
    int64_t *exceed_out;                            /* [nthr][3][nq]; required exactly when nthr > 0       */
    double *jump_out;                               /* [3][nq], nullable                                   */
    double *mean_out, *std_out;                     /* [nq], nullable (both or neither)                    */
    int64_t *density_out;                           /* [nq], nullable                                      */
    int64_t *skipped_out;                           /* [1], nullable; only with density_out                */
} td_interfaces;
int td_rasterize_interfaces(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                            const double *yCell, const double *zCell, const double *zeta, const td_interfaces *want);
int td_history_interfaces(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_interfaces *want);

/* Testing hook, pure host code (it stands here, not in tdstar_testing.h, which the chain sources include).
 * What (nmodels, the lattice nx x ny x nz), the budget in bytes of a slab's value matrix (0: the default,
 * 1 GiB) and a forced slab size (0: none; tdt_set_volume_slab_nodes sets it for a context) decide, out = {the
 * nodes a slab owns, slabs, the most columns of any slab}.  A slab owns the flat nodes [q0, q0 + nodes) and is
 * swept with the halo of its forward neighbours: the nodes up to q0 + nodes + h (h = nx; 1 when ny == 1; 0
 * when nx == 1 too) and [q0 + nx ny, q0 + nodes + nx ny), both clipped to the lattice, one range where they
 * meet -- at most 2 nodes + h columns.  nodes = the largest multiple of 64 with 8 nmodels (2 nodes + h) <=
 * budget (forced: rounded down to a multiple of 64), at least 64, and the columns at most tdt_volume_plan's
 * ceiling of a slab. */
int tdt_interfaces_plan(int64_t nmodels, int64_t nx, int64_t ny, int64_t nz, int64_t budget, int64_t forced,
                        int64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif /* TDSTAR_INTERFACES_H */
