// interfaces.hip -- posterior interfaces: where the models of an ensemble put their Voronoi boundaries on a
// lattice, how large the jump across them is, and where the sampler spends its cells
// (include/tdstar_interfaces.h holds the contract).
//
// The search structure is the volume's (volume_build).  The lattice's nodes are swept slab by slab; a slab
// owns the contiguous flat nodes [q0, q0 + ns) and is swept together with the halo of its forward
// neighbours -- [q0, q0 + ns + nx) and [q0 + nx ny, q0 + ns + nx ny), clipped to the lattice, one range
// where they meet (iface_slab) -- so one volume_sweep gives V_slab[M][columns] with every value the slab's
// faces need, and a neighbour's column is the node's own plus a constant.
//   k_iface_faces    work item = (64 nodes of the slab, leaf of the sum's pairwise tree), one wave, one lane
//                    per node.  A row of V_slab is one coalesced 512-byte load per wave for the node, the
//                    same row one column on for +x, and two more coalesced loads at fixed column offsets
//                    for +y and +z; kIfaceAhead rows are in flight per lane.  count, any and exceed are
//                    32-bit counters in registers, the |d| sums of the three axes run left to right over
//                    the leaf's models.  The leaves (blocks of at most 1024 models) are independent, so 10^4
//                    models give 16 times the waves of a slab without rounding differently; no difference
//                    matrix is written (1.72 TB/s over the slabs of the shipped lattice: DESIGN 4.6h).
//   k_iface_combine  one lane per node: the leaves' sums are added in the tree's order (the walk of
//                    k_cov_targets with a leaf as the unit, the waiting left halves in LDS), the counters
//                    as integers, -1 / NaN where there is no face.
//   k_iface_density  one lane per cell of VolSearch::cells (all models behind one another): three binary
//                    searches over the voxel midpoints (formed on the host), one 64-bit atomic add into the
//                    node's counter, or into `skipped` for a NaN coordinate.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tdstar_interfaces.h"
#include "covariance.h"
#include "ctx.h"
#include "ensemble.h"
#include "history.h"
#include "interfaces.h"
#include "volume.h"

namespace tdstar {

namespace {

constexpr int kIfaceThreads = 64;  // one wave: a tile of the slab
constexpr int kIfaceAhead = 8;     // rows of the slab a lane keeps in flight (4 loads each)
constexpr int kIfaceMaxThr = TD_INTERFACES_MAX_THR;
constexpr int64_t kIfaceMaxModels = (int64_t)1 << 25;         // 2^15 leaves: one launch's grid.y
constexpr int64_t kIfaceMaxDensityNodes = (int64_t)1 << 27;  // 8-byte counters: 1 GiB (kVolDefaultBudget)

struct IfaceThr {
    double t[kIfaceMaxThr];
};

// which of a node's forward faces exist (g = the flat node)
__device__ __forceinline__ void iface_faces_of(long g, int nx, int ny, int nz, bool &fx, bool &fy, bool &fz) {
    const long sxy = (long)nx * ny;
    fx = (int)(g % nx) < nx - 1;
    fy = (int)((g / nx) % ny) < ny - 1;
    fz = g / sxy < (long)nz - 1;
}

// V = V_slab[M][ncols]; the slab owns the columns [0, ns) = the nodes q0 .. q0 + ns.  Leaf blockIdx.y is the
// models leaves[blockIdx.y].x .. .y.  psum [leaf][3][ns], pcnt [leaf][4 + 3 nthr][ns] (count x, y, z | any |
// exceed [t][a]).  NT >= nthr: the thresholds kept in registers, the ones past nthr +inf (nothing exceeds).
template <int NT>
__global__ __launch_bounds__(kIfaceThreads) void k_iface_faces(const double *__restrict__ V, long ncols, int ns, long q0,
                                                               int nx, int ny, int nz, long zoff,
                                                               const int2 *__restrict__ leaves, IfaceThr thr, int nthr,
                                                               double *__restrict__ psum, int *__restrict__ pcnt) {
    constexpr int NE = NT > 0 ? NT : 1;
    const int lane = threadIdx.x;
    const int node = blockIdx.x * kIfaceThreads + lane;
    const int c = min(node, ns - 1);
    bool fx, fy, fz;
    iface_faces_of(q0 + c, nx, ny, nz, fx, fy, fz);
    // (no face: the node's own column again, the result is not used)
    const long ox = fx ? 1 : 0, oy = fy ? (long)nx : 0, oz = fz ? zoff : 0;
    const int2 lf = leaves[blockIdx.y];
    const double *__restrict__ p = V + (long)lf.x * ncols + c;
    int cnt[3] = {0, 0, 0}, any = 0, ex[NE][3];
#pragma unroll
    for (int t = 0; t < NE; ++t) ex[t][0] = ex[t][1] = ex[t][2] = 0;
    double s[3] = {0.0, 0.0, 0.0};  // (0.0 + |d| is |d|: the first term starts the sum)
    auto take = [&](double v0, double vx, double vy, double vz) {
        const double nb[3] = {vx, vy, vz};
        const bool dx = v0 != vx, dy = v0 != vy, dz = v0 != vz;
        cnt[0] += dx;
        cnt[1] += dy;
        cnt[2] += dz;
        any += (fx && dx) || (fy && dy) || (fz && dz);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double d = fabs(nb[a] - v0);
            s[a] = s[a] + d;
#pragma unroll
            for (int t = 0; t < NT; ++t) ex[t][a] += d > thr.t[t];
        }
    };
    int k = lf.x;
    for (; k + kIfaceAhead <= lf.y + 1; k += kIfaceAhead) {
        double r[kIfaceAhead][4];
#pragma unroll
        for (int j = 0; j < kIfaceAhead; ++j) {
            const double *__restrict__ row = p + (long)j * ncols;
            r[j][0] = row[0];
            r[j][1] = row[ox];
            r[j][2] = row[oy];
            r[j][3] = row[oz];
        }
#pragma unroll
        for (int j = 0; j < kIfaceAhead; ++j) take(r[j][0], r[j][1], r[j][2], r[j][3]);
        p += (long)kIfaceAhead * ncols;
    }
    for (; k <= lf.y; ++k) {
        take(p[0], p[ox], p[oy], p[oz]);
        p += ncols;
    }
    if (node >= ns) return;
    const int ncnt = 4 + 3 * nthr;
    double *__restrict__ ps = psum + (long)blockIdx.y * 3 * ns + node;
    int *__restrict__ pc = pcnt + (long)blockIdx.y * ncnt * ns + node;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ps[(long)a * ns] = s[a];
        pc[(long)a * ns] = cnt[a];
    }
    pc[3L * ns] = any;
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (t < nthr) {
#pragma unroll
            for (int a = 0; a < 3; ++a) pc[(long)(4 + 3 * t + a) * ns] = ex[t][a];
        }
}

// out = [4 + 3 nthr][ns] int64 (count x, y, z | any | exceed [t][a]) then [3][ns] double (jump)
__global__ __launch_bounds__(256) void k_iface_combine(const double *__restrict__ psum, const int *__restrict__ pcnt,
                                                       int nleaves, int M, int ncnt, int ns, long q0, int nx, int ny,
                                                       int nz, long long *__restrict__ out) {
    extern __shared__ double pend[];  // the waiting left halves [cov_levels(M)][256]
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= ns) return;
    bool fx, fy, fz;
    iface_faces_of(q0 + node, nx, ny, nz, fx, fy, fz);
    const unsigned fm = (unsigned)fx | (unsigned)fy << 1 | (unsigned)fz << 2;  // bit a: the face along a exists
    for (int r = 0; r < ncnt; ++r) {
        long long sum = 0;
        for (int l = 0; l < nleaves; ++l) sum += pcnt[((long)l * ncnt + r) * ns + node];
        const bool has = r == 3 ? fm != 0 : ((fm >> (r < 3 ? r : (r - 4) % 3)) & 1u) != 0;
        out[(long)r * ns + node] = has ? sum : -1;
    }
    double *__restrict__ jump = reinterpret_cast<double *>(out + (long)ncnt * ns);
    for (int a = 0; a < 3; ++a) {
        const double *__restrict__ ps = psum + (long)a * ns + node;
        const long st = 3L * ns;  // from a leaf to the next
        double total;
        if (nleaves == 1) {
            total = ps[0];
        } else {  // k_cov_targets' walk of the pairwise tree, a block of at most 1024 models being the next leaf
            unsigned path = 0;  // bit d: the right child at depth d
            int depth = 0, nv = 0, leaf = 0;
            for (;;) {
                int lo = 0, hi = M - 1;
                for (int d = 0; d < depth; ++d) {
                    const int mid = lo + ((hi - lo) >> 1);
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
                total = ps[(long)leaf * st];
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
        jump[(long)a * ns + node] = ((fm >> a) & 1u) ? total / (double)M : __builtin_nan("");
    }
}

// the number of the n midpoints that are <= x (np.searchsorted(mid, x, side="right"))
__device__ __forceinline__ int iface_voxel(const double *__restrict__ mid, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (mid[m] <= x)
            lo = m + 1;
        else
            hi = m;
    }
    return lo;
}

// mid = the midpoints of x | y | z ([nx - 1 | ny - 1 | nz - 1]); dens [nx ny nz], skipped [1], zeroed
__global__ __launch_bounds__(256) void k_iface_density(const double *__restrict__ cells, long cs, long total,
                                                       const double *__restrict__ mid, int nx, int ny, int nz,
                                                       unsigned long long *__restrict__ dens,
                                                       unsigned long long *__restrict__ skipped) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const double x = cells[i], y = cells[cs + i], z = cells[2 * cs + i];
        if (x != x || y != y || z != z) {
            atomicAdd(skipped, 1ull);
            continue;
        }
        const long ix = iface_voxel(mid, nx - 1, x), iy = iface_voxel(mid + (nx - 1), ny - 1, y),
                   iz = iface_voxel(mid + (nx - 1) + (ny - 1), nz - 1, z);  // each <= n_a - 1
        atomicAdd(&dens[ix + (long)nx * (iy + (long)ny * iz)], 1ull);
    }
}

// the pairwise tree's leaves, in order: blocks of at most 1024 models (one leaf below 1025 models)
void iface_leaves(int lo, int hi, std::vector<int2> *out) {
    if (hi - lo < 1024) {
        out->push_back(make_int2(lo, hi));
        return;
    }
    const int mid = (lo + hi) >> 1;
    iface_leaves(lo, mid, out);
    iface_leaves(mid + 1, hi, out);
}

bool mul_fits(int64_t a, int64_t b, int64_t *out) { return !__builtin_mul_overflow(a, b, out); }

// the checks of both entry points that need no context and no HIP call, in the header's order
int iface_check(td_ctx *ctx, const td_interfaces *w, const char *who) {
    const std::string n(who);
    if (!w) return set_err(ctx, TD_ERR_ARG, n + ": want is NULL");
    if (w->nx < 1 || w->ny < 1 || w->nz < 1) return set_err(ctx, TD_ERR_ARG, n + ": nx, ny and nz must be >= 1");
    if (!w->xs || !w->ys || !w->zs) return set_err(ctx, TD_ERR_ARG, n + ": xs, ys and zs must be given");
    const double *vec[3] = {w->xs, w->ys, w->zs};
    const int64_t len[3] = {w->nx, w->ny, w->nz};
    const char *name[3] = {"xs", "ys", "zs"};
    for (int a = 0; a < 3; ++a)
        for (int64_t i = 0; i < len[a]; ++i) {
            if (!std::isfinite(vec[a][i])) return set_err(ctx, TD_ERR_ARG, n + ": " + name[a] + " is not finite");
            if (i > 0 && !(vec[a][i] > vec[a][i - 1]))
                return set_err(ctx, TD_ERR_ARG, n + ": " + name[a] + " is not strictly increasing");
        }
    int64_t nxy = 0, nq = 0;
    if (!mul_fits(w->nx, w->ny, &nxy) || !mul_fits(nxy, w->nz, &nq) || nq > INT64_MAX / 64)
        return set_err(ctx, TD_ERR_ARG, n + ": nx ny nz does not fit 64 bits");
    if (w->nthr < 0 || w->nthr > kIfaceMaxThr) return set_err(ctx, TD_ERR_ARG, n + ": nthr must be 0 .. 8");
    if (w->nthr > 0 && !w->thr) return set_err(ctx, TD_ERR_ARG, n + ": thr is NULL");
    for (int64_t t = 0; t < w->nthr; ++t)
        if (!std::isfinite(w->thr[t]) || w->thr[t] < 0.0)
            return set_err(ctx, TD_ERR_ARG, n + ": every threshold must be finite and >= 0");
    if ((w->nthr > 0) != (w->exceed_out != nullptr))
        return set_err(ctx, TD_ERR_ARG, n + ": exceed_out must be given exactly when nthr > 0");
    if (!w->count_out && !w->any_out && !w->exceed_out && !w->jump_out && !w->mean_out && !w->std_out && !w->density_out &&
        !w->skipped_out)
        return set_err(ctx, TD_ERR_ARG, n + ": no output asked for");
    if (!w->mean_out != !w->std_out) return set_err(ctx, TD_ERR_ARG, n + ": mean_out and std_out must be given together");
    if (w->skipped_out && !w->density_out) return set_err(ctx, TD_ERR_ARG, n + ": skipped_out needs density_out");
    return TD_OK;
}

template <int NT>
void launch_faces(hipStream_t s, unsigned tiles, unsigned nleaves, const double *V, const IfaceSlab &sl, int nx, int ny, int nz,
                  const int2 *leaves, const IfaceThr &thr, int nthr, double *psum, int *pcnt) {
    hipLaunchKernelGGL(k_iface_faces<NT>, dim3(tiles, nleaves), dim3(kIfaceThreads), 0, s, V, (long)sl.ncols, (int)sl.ns,
                       (long)sl.q0, nx, ny, nz, (long)sl.zoff, leaves, thr, nthr, psum, pcnt);
}

// Both entry points; E and w have been checked (ensemble.h, iface_check).
int iface_core(td_ctx *ctx, const char *who, const Ensemble &E, const td_interfaces *w) {
    const std::string n(who);
    const int64_t M = E.nmodels, nx = w->nx, ny = w->ny, nz = w->nz, nq = nx * ny * nz;
    const int nthr = (int)w->nthr, ncnt = 4 + 3 * nthr;
    const bool faces = w->count_out || w->any_out || w->exceed_out || w->jump_out, stats = w->mean_out != nullptr;
    const bool sweep = faces || stats, density = w->density_out != nullptr;
    if (M > kIfaceMaxModels) return set_err(ctx, TD_ERR_ARG, n + ": more than 2^25 models");
    if (nx > INT32_MAX / 2 || ny > INT32_MAX / 2 || nz > INT32_MAX / 2)
        return set_err(ctx, TD_ERR_ARG, n + ": an axis of more than 2^30 nodes");
    if (density && nq > kIfaceMaxDensityNodes)
        return set_err(ctx, TD_ERR_ARG, n + ": density_out of more than 2^27 nodes (its counters are one 1 GiB workspace)");
    const IfacePlan plan = iface_plan(M, nx, ny, nz, kVolDefaultBudget, ctx->vol_slab_nodes);
    const int64_t colcap = volume_plan(M, 0, 0, kVolMaxSlabNodes).nodes;  // the most nodes one sweep takes
    if (sweep && plan.maxcols > colcap)
        return set_err(ctx, TD_ERR_ARG, n + ": a lattice row of nx nodes does not fit one slab's columns");
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    hipStream_t s = ctx->stream;
    std::vector<int2> leaves;
    if (faces) iface_leaves(0, (int)M - 1, &leaves);
    const int64_t nleaves = (int64_t)leaves.size(), cap = std::min(plan.nodes, nq), cols = sweep ? plan.maxcols : 0;
    std::vector<double> mid;  // the voxel midpoints of x | y | z
    if (density) {
        const double *vec[3] = {w->xs, w->ys, w->zs};
        const int64_t len[3] = {nx, ny, nz};
        for (int a = 0; a < 3; ++a)
            for (int64_t l = 0; l + 1 < len[a]; ++l) mid.push_back(0.5 * (vec[a][l] + vec[a][l + 1]));
    }
    // ctx->raster (8-byte words): density counters [nq] | skipped [1] | midpoints | leaves | queries [3][cols] |
    // V_slab [M][cols] | mean, std [cols] | leaf sums [leaves][3][cap] | leaf counters [leaves][ncnt][cap] (32-bit) |
    // out [ncnt + 3][cap]; pinned: queries [3][cols] | out [ncnt + 3][cap]
    const size_t n_dens = density ? (size_t)nq + 1 : 0, n_mid = mid.size(), n_leaf = (size_t)nleaves,
                 n_q = 3 * (size_t)cols, n_v = (size_t)M * (size_t)cols, n_ms = 2 * (size_t)cols,
                 n_ps = faces ? (size_t)nleaves * 3 * (size_t)cap : 0,
                 n_pc = faces ? ((size_t)nleaves * (size_t)ncnt * (size_t)cap + 1) / 2 : 0,
                 n_out = faces ? (size_t)(ncnt + 3) * (size_t)cap : 0;
    if (int rc = raster_reserve(ctx, std::max<size_t>(n_dens + n_mid + n_leaf + n_q + n_v + n_ms + n_ps + n_pc + n_out, 1),
                                std::max<size_t>(n_q + n_out, 1)))
        return rc;
    double *base = ctx->raster.as<double>();
    unsigned long long *ddens = reinterpret_cast<unsigned long long *>(base);
    double *dmid = base + n_dens;
    int2 *dleaf = reinterpret_cast<int2 *>(dmid + n_mid);
    double *dq = dmid + n_mid + n_leaf, *dv = dq + n_q, *dm = dv + n_v, *dsd = dm + cols, *dps = dsd + cols;
    int *dpc = reinterpret_cast<int *>(dps + n_ps);
    long long *dout = reinterpret_cast<long long *>(dps + n_ps + n_pc);
    double *hq = ctx->h_raster.as<double>();
    long long *hout = reinterpret_cast<long long *>(hq + n_q);
    TD_HIP(ctx, hipStreamSynchronize(s));  // (the pinned block and the workspace are free)
    if (density) {
        TD_HIP(ctx, hipMemsetAsync(ddens, 0, sizeof(unsigned long long) * n_dens, s));
        if (n_mid > 0) TD_HIP(ctx, hipMemcpyAsync(dmid, mid.data(), sizeof(double) * n_mid, hipMemcpyHostToDevice, s));
        const int64_t total = E.total();
        if (total > 0) {
            const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 1 << 16);
            TD_HIP(ctx, timed_launch(ctx, "iface_density", [&] {
                       hipLaunchKernelGGL(k_iface_density, dim3(blocks), dim3(256), 0, s, S.cells, (long)S.cs, (long)total, dmid,
                                          (int)nx, (int)ny, (int)nz, ddens, ddens + nq);
                   }));
        }
        TD_HIP(ctx, hipMemcpyAsync(w->density_out, ddens, sizeof(int64_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
        if (w->skipped_out) TD_HIP(ctx, hipMemcpyAsync(w->skipped_out, ddens + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    }
    int64_t brute_pairs = 0;
    if (sweep) {
        if (faces)
            TD_HIP(ctx, hipMemcpyAsync(dleaf, leaves.data(), sizeof(int2) * (size_t)nleaves, hipMemcpyHostToDevice, s));
        IfaceThr thr;
        for (int t = 0; t < kIfaceMaxThr; ++t) thr.t[t] = t < nthr ? w->thr[t] : HUGE_VAL;
        for (int64_t q0 = 0; q0 < nq; q0 += plan.nodes) {
            const IfaceSlab sl = iface_slab(nx, ny, nz, q0, plan.nodes);
            const int64_t ns = sl.ns, nc = sl.ncols;
            // the columns' coordinates, [3][nc], through the pinned block
            for (int64_t c = 0; c < nc; ++c) {
                const int64_t g = c < sl.r1n ? q0 + c : sl.r2lo + (c - sl.r1n);
                hq[c] = w->xs[g % nx];
                hq[nc + c] = w->ys[(g / nx) % ny];
                hq[2 * nc + c] = w->zs[g / (nx * ny)];
            }
            TD_HIP(ctx, hipMemcpyAsync(dq, hq, sizeof(double) * 3 * (size_t)nc, hipMemcpyHostToDevice, s));
            if (int rc = volume_sweep(ctx, S, 0, M, dq, nc, dv)) return rc;
            if (!S.grid) brute_pairs += M * nc;
            if (stats) {  // k_raster_stats column by column: the owned nodes are the first ns
                TD_HIP(ctx, timed_launch(ctx, "raster_stats", [&] { return launch_raster_stats(dv, (int)M, (int)nc, dm, dsd, s); }));
                TD_HIP(ctx, hipMemcpyAsync(w->mean_out + q0, dm, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
                TD_HIP(ctx, hipMemcpyAsync(w->std_out + q0, dsd, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
            }
            if (faces) {
                const unsigned tiles = (unsigned)((ns + kIfaceThreads - 1) / kIfaceThreads), nl = (unsigned)nleaves;
                TD_HIP(ctx, timed_launch(ctx, "iface_faces", [&] {  // (both launches under the one name)
                           if (nthr == 0)
                               launch_faces<0>(s, tiles, nl, dv, sl, (int)nx, (int)ny, (int)nz, dleaf, thr, nthr, dps, dpc);
                           else if (nthr == 1)
                               launch_faces<1>(s, tiles, nl, dv, sl, (int)nx, (int)ny, (int)nz, dleaf, thr, nthr, dps, dpc);
                           else if (nthr == 2)
                               launch_faces<2>(s, tiles, nl, dv, sl, (int)nx, (int)ny, (int)nz, dleaf, thr, nthr, dps, dpc);
                           else if (nthr <= 4)
                               launch_faces<4>(s, tiles, nl, dv, sl, (int)nx, (int)ny, (int)nz, dleaf, thr, nthr, dps, dpc);
                           else
                               launch_faces<8>(s, tiles, nl, dv, sl, (int)nx, (int)ny, (int)nz, dleaf, thr, nthr, dps, dpc);
                           hipLaunchKernelGGL(k_iface_combine, dim3((unsigned)((ns + 255) / 256)), dim3(256),
                                              sizeof(double) * 256 * (size_t)cov_levels(M), s, dps, dpc, (int)nleaves, (int)M, ncnt,
                                              (int)ns, (long)q0, (int)nx, (int)ny, (int)nz, dout);
                       }));
                TD_HIP(ctx, hipMemcpyAsync(hout, dout, sizeof(int64_t) * (size_t)(ncnt + 3) * (size_t)ns, hipMemcpyDeviceToHost, s));
            }
            TD_HIP(ctx, hipStreamSynchronize(s));  // the pinned block is packed again for the next slab
            if (faces) {  // the rows [ns] of the slab into the caller's rows [nq]
                const size_t row = sizeof(int64_t) * (size_t)ns;
                for (int a = 0; a < 3; ++a) {
                    if (w->count_out) std::memcpy(w->count_out + a * nq + q0, hout + a * ns, row);
                    if (w->jump_out) std::memcpy(w->jump_out + a * nq + q0, hout + (ncnt + a) * ns, row);
                }
                if (w->any_out) std::memcpy(w->any_out + q0, hout + 3 * ns, row);
                for (int r = 0; r < 3 * nthr; ++r) std::memcpy(w->exceed_out + r * nq + q0, hout + (4 + r) * ns, row);
            }
        }
    }
    TD_HIP(ctx, hipStreamSynchronize(s));
    return volume_counters_finish(ctx, S, brute_pairs);  // (tdt_volume_counters: this call's sweeps)
}

}  // namespace

IfaceSlab iface_slab(int64_t nx, int64_t ny, int64_t nz, int64_t q0, int64_t nodes) {
    const int64_t sxy = nx * ny, nq = sxy * nz;
    // the halo behind the owned nodes that holds the +x and +y neighbours
    const int64_t hy = ny > 1 ? nx : (nx > 1 ? 1 : 0);
    IfaceSlab sl;
    sl.q0 = q0;
    sl.ns = std::min(nodes, nq - q0);
    const int64_t r1hi = std::min(q0 + sl.ns + hy, nq), r2lo = q0 + sxy, r2hi = std::min(q0 + sl.ns + sxy, nq);
    if (nz == 1 || r2lo >= nq) {  // no +z neighbour
        sl.r1n = sl.ncols = r1hi - q0;
    } else if (r2lo <= r1hi) {  // the ranges meet: one
        sl.r1n = sl.ncols = std::max(r1hi, r2hi) - q0;
        sl.zoff = sxy;
    } else {
        sl.r1n = r1hi - q0;
        sl.r2lo = r2lo;
        sl.r2n = r2hi - r2lo;
        sl.ncols = sl.r1n + sl.r2n;
        sl.zoff = sl.r1n;  // node q0 + sxy is the second range's first column
    }
    return sl;
}

IfacePlan iface_plan(int64_t nmodels, int64_t nx, int64_t ny, int64_t nz, int64_t budget, int64_t forced) {
    const int64_t nm = std::max<int64_t>(nmodels, 1), b = budget > 0 ? budget : kVolDefaultBudget;
    const int64_t nq = nx * ny * nz, hy = ny > 1 ? nx : (nx > 1 ? 1 : 0);
    const int64_t colcap = volume_plan(nm, 0, 0, kVolMaxSlabNodes).nodes;  // the most nodes one sweep takes
    // 2 nodes + hy columns at the most: within the budget's columns and one sweep's
    const int64_t room = std::min(b / 8 / nm, colcap);
    int64_t nodes = forced > 0 ? forced / kVolTile * kVolTile : (room - hy) / 2 / kVolTile * kVolTile;
    nodes = std::min(nodes, (colcap - hy) / 2 / kVolTile * kVolTile);
    nodes = std::max(nodes, kVolTile);
    IfacePlan p;
    p.nodes = nodes;
    p.nslabs = (nq + nodes - 1) / nodes;
    p.maxcols = iface_slab(nx, ny, nz, 0, nodes).ncols;  // (a later slab is clipped no less)
    return p;
}

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_interfaces(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                                       const double *yCell, const double *zCell, const double *zeta,
                                       const td_interfaces *want) {
    const char *who = "td_rasterize_interfaces";
    return ensemble_entry_arrays(
        ctx, who, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta), nullptr, [&] { return iface_check(ctx, want, who); },
        [&](const Ensemble &E) { return iface_core(ctx, who, E, want); });
}

extern "C" int td_history_interfaces(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_interfaces *want) {
    const char *who = "td_history_interfaces";
    return ensemble_entry_histories(
        ctx, who, hs, nh, nullptr, [&] { return iface_check(ctx, want, who); },
        [&](const Ensemble &E) { return iface_core(ctx, who, E, want); });
}

extern "C" int tdt_interfaces_plan(int64_t nmodels, int64_t nx, int64_t ny, int64_t nz, int64_t budget, int64_t forced,
                                   int64_t out[3]) {
    int64_t nxy = 0, nq = 0;
    if (!out || nmodels < 1 || nx < 1 || ny < 1 || nz < 1 || budget < 0 || forced < 0 || !mul_fits(nx, ny, &nxy) ||
        !mul_fits(nxy, nz, &nq) || nq > INT64_MAX / 64)
        return TD_ERR_ARG;
    const IfacePlan p = iface_plan(nmodels, nx, ny, nz, budget, forced);
    out[0] = p.nodes;
    out[1] = p.nslabs;
    out[2] = p.maxcols;
    return TD_OK;
}
