// covariance.h -- posterior covariance (covariance.hip): the covariance and the correlation over the models
// between zeta at a few targets (points, or series the caller hands in) and zeta at every node of a lattice,
// swept slab by slab on the volume's search structure (include/tdstar.h "Posterior covariance").
#pragma once
#include <cstdint>

namespace tdstar {

// Targets per register group of k_cov_targets: each element of a slab is loaded once per group.
constexpr int kCovGroup = 8;
constexpr int kCovThreads = 64;  // one wave per workgroup, one lane per node

// The levels of Julia's pairwise split of nmodels terms (blocks of <= 1024): the most left halves that wait
// for their sibling at any time, hence the depth of k_cov_targets' combine stack (host only).
int cov_levels(int64_t nmodels);

}  // namespace tdstar
