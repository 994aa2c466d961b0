// chain_state.hip -- the device chain's full state from scratch (chain_full_state: nearest search, ray
// sums, then the cells' point counts, the chi^2 prefix sums and tile maxima computed here), and the LDS sizes a chain's launches
// take.  The chain itself, and its one-point query, are in chain_kernels.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "chain_dev.h"
#include "chain_shared.h"
#include "internal.h"

namespace tdstar {

namespace {

// ------------------------------------------------------------ full state ----
// chi^2 prefix sums, sequential (MCsub.jl:170-172), and phi.
__global__ __launch_bounds__(256) void k_chi2_prefix(const double *__restrict__ ptS, const double *__restrict__ tS,
                                                     const double *__restrict__ sig, int n,
                                                     double *__restrict__ prefix, ChainScalars *st) {
    __shared__ double t[2048];
    double C = 0.0;
    for (int base = 0; base < n; base += 2048) {
        const int cnt = min(2048, n - base);
        for (int k = threadIdx.x; k < cnt; k += 256) {
            const double df = ptS[base + k] - tS[base + k];
            const double sg = sig[base + k];
            t[k] = ((df * df) * 1.0) / (sg * sg);
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < cnt; ++k) {
                C = C + t[k];
                prefix[base + k] = C;
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) st->phi = C;
}

__global__ void k_tile_max(const int *__restrict__ tile_start, int ntiles, const double *__restrict__ best_d,
                           double *__restrict__ tile_maxd) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    double mx = -1.0;
    const int sc = tile_start[t];  // start << 5 | count
    for (int q = sc >> 5; q < (sc >> 5) + (sc & 31); ++q) mx = fmax(mx, best_d[q]);
    tile_maxd[t] = mx;
}

// own[slot] = #{q : best_s[q] == slot} (chain_dev.h), over zeroed counts
__global__ __launch_bounds__(256) void k_own_count(const int *__restrict__ best_s, int P, int cap, int *__restrict__ own) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    const int s = best_s[q];
    if (s >= 0 && s < cap) atomicAdd(&own[s], 1);
}

}  // namespace

hipError_t launch_chi2_prefix(const double *ptS, const double *tS, const double *sig, int n, double *prefix,
                              ChainScalars *st, hipStream_t s) {
    hipLaunchKernelGGL(k_chi2_prefix, dim3(1), dim3(256), 0, s, ptS, tS, sig, n, prefix, st);
    return hipGetLastError();
}

hipError_t chain_full_state(DevChain &d, int ncells, NNWork &work, int num_cus, hipStream_t s) {
    Geometry g;
    g.m = 0;
    g.n = d.n;
    g.P = d.P;
    g.px = const_cast<double *>(d.px);
    g.py = const_cast<double *>(d.py);
    g.pz = const_cast<double *>(d.pz);
    g.w = const_cast<double *>(d.w);
    g.ray_off = const_cast<int *>(d.ray_off);
    g.tS = const_cast<double *>(d.tS);
    g.sig = const_cast<double *>(d.sig);
    // slots 0..ncells-1 hold the cells in order, so nearest index == slot
    hipError_t e = launch_nearest(d.px, d.py, d.pz, d.P, 1, 1, d.cx, d.cap, ncells, work, num_cus, d.best_s,
                                  d.best_d, d.zeta0, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(d.own, 0, sizeof(int) * (size_t)d.cap, s);
    if (e != hipSuccess) return e;
    if (d.P > 0) {
        hipLaunchKernelGGL(k_own_count, dim3((d.P + 255) / 256), dim3(256), 0, s, d.best_s, d.P, d.cap, d.own);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    e = launch_ray_sums(g, d.zeta0, d.ptS, s);
    if (e != hipSuccess) return e;
    e = launch_chi2_prefix(d.ptS, d.tS, d.sig, d.n, d.prefix, d.st, s);
    if (e != hipSuccess) return e;
    if (d.ntiles > 0) {
        hipLaunchKernelGGL(k_tile_max, dim3((d.ntiles + 255) / 256), dim3(256), 0, s, d.tile_start, d.ntiles,
                           d.best_d, d.tile_maxd);
        e = hipGetLastError();
    }
    return e;
}

void chain_lds_sizes(const DevChain &d, int64_t out[4]) {
    const LdsPlan a = lds_plan(d.ntiles, d.n, d.cap, true), b = lds_plan(d.ntiles, d.n, d.cap, false);
    out[0] = (int64_t)a.total;      // LDS layout (tiles, rays, order mirrored)
    out[1] = (int64_t)b.total;      // HBM layout
    out[2] = b.super_lds ? 1 : 0;   // HBM layout with super-tiles in LDS
    // the layout a launch of this chain alone, free-running, takes: 1 = LDS
    out[3] = choose_chain_variant(launch_facts(&d, 1)).v.rlds ? 1 : 0;
}

}  // namespace tdstar
