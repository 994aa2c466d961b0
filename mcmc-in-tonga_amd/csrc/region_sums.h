// region_sums.h -- what regions.hip and recovery.hip share: per model the weighted sum of a function of a slab's
// values over each region of a point list, in td_rasterize's association counted over the index within the
// region.  The unit of that association is the leaf: a block of at most 1024 consecutive points of one region
// (region_leaves: the split of iface_leaves applied to the region's point count).  The leaves of all regions tile
// the point list in order.  Everything here has internal linkage: each unit that includes the header holds kernels
// of its own.
//   k_region_sums<Op> work item = (a leaf's columns in this slab, 64 models), one wave, one lane per model.
//                     V_slab is row-major, so a lane walking its own row would stride by 8 ns bytes: the wave
//                     reads a tile of 64 models x 64 columns row by row instead -- each row one coalesced
//                     512-byte load, kRegAhead of them in flight per lane -- into LDS (rows padded to 65
//                     doubles: lane m's ds_read_b64 of column c hits the bank pair 2 (m + c) mod 64, none twice
//                     in a half wave), with the tile's weights as one more LDS row; then each lane walks its row
//                     left to right, t = Op(w, v) rounded, then acc = acc + t.  A leaf is summed left to right, so
//                     a slab boundary inside it is carried: the accumulators acc[leaf][M] live in the workspace
//                     across the slabs, started at -0.0 (-0.0 + t is t for every t, the sign of a zero
//                     included) where the leaf begins.
//   k_region_combine  one lane per (model, region): the region's leaf sums are added in the tree's order (the
//                     walk of k_iface_combine with a leaf as the unit, the waiting left halves in LDS), divided
//                     by W[r] when asked, and written to F[m][r].  W is formed on the host in the same
//                     association (region_weight).
// The including unit is compiled without contraction, so an Op's multiplies are rounded one by one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace tdstar {

namespace {

constexpr int kRegTile = 64;          // models and columns of an LDS tile; one wave
constexpr int kRegPad = kRegTile + 1; // doubles per LDS row
constexpr int kRegAhead = 16;         // rows of the tile a lane keeps in flight

// V = V_slab[M][ns], the points [c0, c0 + ns) of the list.  Leaf l is the points [leafp[l], leafp[l + 1]);
// workgroup b takes the leaf la + b / mgroups and the models 64 (b % mgroups) ...  wcol [ns]: the slab's weights
// (null: 1.0).  acc [leaves][M].  Op::term(w, v): the term of the sum.
template <class Op>
__global__ __launch_bounds__(kRegTile) void k_region_sums(const double *__restrict__ V, long ns, int M, long c0,
                                                          const long long *__restrict__ leafp, long la, int mgroups,
                                                          const double *__restrict__ wcol, double *__restrict__ acc) {
    __shared__ double tile[kRegTile * kRegPad];
    __shared__ double wrow[kRegTile];
    const int lane = threadIdx.x;
    const long leaf = la + blockIdx.x / mgroups;
    const int m0 = (int)(blockIdx.x % mgroups) * kRegTile;
    const long p0 = leafp[leaf], p1 = leafp[leaf + 1];
    const long s0 = max(p0, c0) - c0, s1 = min(p1, c0 + ns) - c0;  // the leaf's columns of this slab: [s0, s1)
    const int m = min(m0 + lane, M - 1);
    double a = p0 >= c0 ? -0.0 : acc[leaf * M + m];  // the leaf begins here, or is carried from the slab before
    const double *__restrict__ mine = tile + lane * kRegPad;
    for (long t0 = s0; t0 < s1; t0 += kRegTile) {
        const int nc = (int)min((long)kRegTile, s1 - t0);
        const long col = t0 + min(lane, nc - 1);  // (past the leaf's end: its last column again, not used)
        wrow[lane] = wcol ? wcol[col] : 1.0;
#pragma unroll
        for (int j0 = 0; j0 < kRegTile; j0 += kRegAhead) {
            double r[kRegAhead];
#pragma unroll
            for (int j = 0; j < kRegAhead; ++j) r[j] = V[(long)min(m0 + j0 + j, M - 1) * ns + col];
#pragma unroll
            for (int j = 0; j < kRegAhead; ++j) tile[(j0 + j) * kRegPad + lane] = r[j];
        }
        __syncthreads();
        if (nc == kRegTile) {
#pragma unroll 16
            for (int c = 0; c < kRegTile; ++c) {
                const double t = Op::term(wrow[c], mine[c]);
                a = a + t;
            }
        } else {
            for (int c = 0; c < nc; ++c) {
                const double t = Op::term(wrow[c], mine[c]);
                a = a + t;
            }
        }
        __syncthreads();  // (the tile is filled again)
    }
    if (m0 + lane < M) acc[leaf * M + m0 + lane] = a;
}

// Region r's leaves are regleaf[r] .. regleaf[r + 1] - 1.  Workgroup b: region b / mblocks, models 256 (b % mblocks) ...
__global__ __launch_bounds__(256) void k_region_combine(const double *__restrict__ acc, int M, int mblocks,
                                                        const long long *__restrict__ regleaf,
                                                        const long long *__restrict__ leafp,
                                                        const double *__restrict__ W, int normalize, long R,
                                                        double *__restrict__ F) {
    extern __shared__ double pend[];  // the waiting left halves [cov_levels(the most points of a region)][256]
    const long r = blockIdx.x / mblocks;
    const int m = (int)(blockIdx.x % mblocks) * 256 + threadIdx.x;
    if (m >= M) return;
    const long l0 = regleaf[r], nl = regleaf[r + 1] - l0;
    const long n = leafp[l0 + nl] - leafp[l0];  // the region's points
    const double *__restrict__ ps = acc + l0 * M + m;
    double total;
    if (nl == 1) {
        total = ps[0];
    } else {  // k_iface_combine's walk of the pairwise tree over the region's n points, a block of <= 1024 being a leaf
        unsigned path = 0;  // bit d: the right child at depth d
        int depth = 0, nv = 0;
        long leaf = 0;
        for (;;) {
            long lo = 0, hi = n - 1;
            for (int d = 0; d < depth; ++d) {
                const long mid = lo + ((hi - lo) >> 1);
                if ((path >> d) & 1u)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            while (hi - lo >= 1024) {  // down the left children to a block
                hi = lo + ((hi - lo) >> 1);
                path &= ~(1u << depth);
                ++depth;
            }
            total = ps[leaf * M];
            ++leaf;
            while (depth > 0 && ((path >> (depth - 1)) & 1u)) {  // a right child: its parent is left + right
                --nv;
                total = pend[nv * 256 + threadIdx.x] + total;
                --depth;
            }
            if (depth == 0) break;
            pend[nv * 256 + threadIdx.x] = total;  // a left child waits (read again by this lane alone)
            ++nv;
            path |= 1u << (depth - 1);
        }
    }
    F[(long)m * R + r] = normalize ? total / W[r] : total;
}

// The leaves of a region of n points whose first point is `base`, in order: the first points, appended to out.
inline void region_leaves(int64_t base, int64_t lo, int64_t hi, std::vector<long long> *out) {
    if (hi - lo < 1024) {
        out->push_back(base + lo);
        return;
    }
    const int64_t mid = (lo + hi) >> 1;
    region_leaves(base, lo, mid, out);
    region_leaves(base, mid + 1, hi, out);
}

// W of one region: the sum of w[lo .. hi] (null: of ones) in the tree's order, a block left to right.
inline double region_weight(const double *w, int64_t lo, int64_t hi) {
    if (hi - lo < 1024) {
        double s = w ? w[lo] : 1.0;
        for (int64_t k = lo + 1; k <= hi; ++k) s = s + (w ? w[k] : 1.0);
        return s;
    }
    const int64_t mid = (lo + hi) >> 1;
    const double a = region_weight(w, lo, mid), b = region_weight(w, mid + 1, hi);
    return a + b;
}

}  // namespace

}  // namespace tdstar
