// volume.h -- posterior volumes (volume.hip): td_rasterize's value matrix, statistics, marginals and
// convergence diagnostics at any number of nodes, one search structure for all models and the nodes swept
// slab by slab (include/tdstar.h "Posterior volumes").
#pragma once
#include <cstdint>

#include "ctx.h"

namespace tdstar {

constexpr int64_t kVolTile = 64;                         // a slab is a multiple of this many nodes
constexpr int64_t kVolDefaultBudget = (int64_t)1 << 30;  // bytes of V_slab[nmodels][slab nodes]
// the most nodes of a slab: every per-slab product of the marginal and convergence kernels
// (nodes x (4096 + 3) histogram slots, nodes + 64) stays below 2^31
constexpr int64_t kVolMaxSlabNodes = (int64_t)1 << 18;

// What (nmodels, nq) and the budget decide (host only): the nodes of a slab -- the largest multiple of
// kVolTile with 8 nmodels nodes <= budget, or `forced` rounded down to one, at least kVolTile, at most
// kVolMaxSlabNodes and what one launch's block count allows -- and the number of slabs covering [0, nq).
struct VolPlan {
    int64_t nodes = 0, nslabs = 0;
};
VolPlan volume_plan(int64_t nmodels, int64_t nq, int64_t budget, int64_t forced);

// raster.hip's kernels on a device value matrix of a slab (the section entry points' own statistics and
// brute-force sweep, so a volume's numbers are theirs): q = [3][nq] SoA, cells SoA of stride cs.
bool raster_brute_fits(int64_t nmodels, int64_t nq);
hipError_t launch_raster_brute(const int64_t *cell_off_dev, const double *cells, int64_t cs, const double *q, int nq,
                               int nmodels, double *values, hipStream_t s, Timer *tm);
hipError_t launch_raster_stats(const double *values, int nmodels, int nq, double *mean, double *sd, hipStream_t s);

// td_destroy: the volume workspaces of a context
void volume_free(td_ctx *ctx);

}  // namespace tdstar
