// predict.h -- posterior predictive data (predict.hip): every model's predicted t* on the rays of a
// context, its chi^2, and the statistics of the matrix ptS[nmodels][n] over the models
// (include/tdstar.h "Posterior predictive data").
#pragma once
#include <cstdint>
#include <vector>

#include "ctx.h"

namespace tdstar {

constexpr int64_t kPredTile = 64;                  // a slab's capacity is a multiple of this many points
constexpr int64_t kPredMaxSlabPoints = (int64_t)1 << 18;  // and at most this: the longest ray a call takes
constexpr int64_t kPredMaxChunk = (int64_t)1 << 19;       // models per sweep: one launch's blocks fit 32 bits
constexpr int64_t kPredMaxSlabRays = (int64_t)1 << 20;    // rays per slab (rays without points add none)

// What (nmodels, the rays' point counts), the budget and the forced sizes decide (host only).  A slab is a
// run of whole consecutive rays of at most `points` points in all: points = the largest multiple of 64
// with 8 nmodels points <= budget (forced_points: rounded down to one), at least 64, raised to the longest
// ray rounded up to 64, at most 2^18.  Where 8 nmodels points is still above the budget the models are swept
// `chunk` = max(1, budget / (8 points)) at a time (forced_chunk: that many), at most nmodels and 2^19.
// edges[k] .. edges[k + 1] are slab k's rays (filled greedily, ray after ray, at most 2^20 rays each).
struct PredPlan {
    int64_t points = 0, chunk = 0;
    std::vector<int64_t> edges;  // [slabs + 1]; {0} without rays
};
// false: a ray of more than 2^18 points
bool predict_plan(int64_t nmodels, int64_t n, const int64_t *ray_points, int64_t budget, int64_t forced_points,
                  int64_t forced_chunk, PredPlan *plan);

}  // namespace tdstar
