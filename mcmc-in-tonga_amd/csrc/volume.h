// volume.h -- posterior volumes (volume.hip): td_rasterize's value matrix, statistics, marginals and
// convergence diagnostics at any number of nodes, one search structure for all models and the nodes swept
// slab by slab (include/tdstar.h "Posterior volumes").
#pragma once
#include <cstdint>
#include <vector>

#include "ctx.h"

namespace tdstar {

struct Ensemble;  // ensemble.h

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

// The search structure of one call, built once for all models in ctx->vol / ctx->vol_grid (volume.hip:
// k_vol_boxes, the host's make_cell_grid per model, k_vol_grid_build; models of few cells are swept by
// k_raster_brute and get no grids), and the sweep of a device query block against it.  The volume entry
// points and the posterior predictive ones (predict.hip) share both.
struct VolSearch {
    int64_t nmodels = 0, cs = 1;  // cs: the SoA stride of cells
    bool grid = false;            // bucket grids (k_vol_search), else k_raster_brute
    double *cells = nullptr;      // x | y | z | zeta of every model behind one another
    int64_t *off = nullptr;       // [nmodels + 1] the models' first cells
    CellGrid *grids = nullptr;    // [nmodels]
    int64_t *boff = nullptr;      // [nmodels + 1] the models' first bucket starts
    int *start = nullptr;
    BucketEntry *ent = nullptr;
    unsigned long long *counters = nullptr;  // the paths k_vol_search<true> counts
    std::vector<CellGrid> grids_host;        // what grids and boff were copied from
    std::vector<int64_t> boff_host;
};
// The host arrays reach the device in four copies from the caller's arrays, a history's samples device to
// device (any context's, on ctx's device).
int volume_build(td_ctx *ctx, const char *who, const Ensemble &E, VolSearch *out);
// values[nm][ns] = the nearest cell's zeta of the models [m0, m0 + nm) at the device queries q = [3][ns],
// ns >= 1 (timers vol_search / raster_brute)
int volume_sweep(td_ctx *ctx, const VolSearch &S, int64_t m0, int64_t nm, const double *q, int64_t ns, double *values);
// The end of a call that swept S: tdt_volume_counters' numbers (brute_pairs: the pairs k_raster_brute took)
int volume_counters_finish(td_ctx *ctx, const VolSearch &S, int64_t brute_pairs);
// raster.hip: room for nd doubles in ctx->raster and nh doubles in the pinned ctx->h_raster
int raster_reserve(td_ctx *ctx, size_t nd, size_t nh);

}  // namespace tdstar
