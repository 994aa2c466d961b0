// interfaces.h -- the halo plan of the posterior interfaces (interfaces.hip; include/tdstar_interfaces.h): pure
// host arithmetic, shared by the entry points and the hook tdt_interfaces_plan.
#pragma once
#include <cstdint>

namespace tdstar {

// What (nmodels, the lattice) and the budget decide: the nodes a slab owns (a multiple of kVolTile, `forced`
// rounded down to one), the slabs covering [0, nq), and the most columns a slab's value matrix holds.
struct IfacePlan {
    int64_t nodes = 0, nslabs = 0, maxcols = 0;
};
IfacePlan iface_plan(int64_t nmodels, int64_t nx, int64_t ny, int64_t nz, int64_t budget, int64_t forced);

// One slab: it owns the flat nodes [q0, q0 + ns).  Its columns are the nodes [q0, q0 + r1n) followed by
// [r2lo, r2lo + r2n) (r2n == 0: one range).  The column of an owned node is its offset from q0, the column
// of its +x neighbour one on, of its +y neighbour nx on, of its +z neighbour zoff on.
struct IfaceSlab {
    int64_t q0 = 0, ns = 0, ncols = 0, r1n = 0, r2lo = 0, r2n = 0, zoff = 0;
};
IfaceSlab iface_slab(int64_t nx, int64_t ny, int64_t nz, int64_t q0, int64_t nodes);

}  // namespace tdstar
