// chain_test_kernels.hip -- testing kernels for pieces of the device chain (tdstar_testing.h hooks; the
// product never launches them): phase F's proposal-time chi^2, the grid query's latency and answers,
// the phase-B tile filters, the wave primitives of wave_ops.h row by row, the full scan on caller-given
// slots, and a chain's nearest-cell query with a killed and a moved cell.
#pragma clang fp contract(off)
// (a unit uses part of what the chain_*.h headers define, each with internal linkage)
#pragma clang diagnostic ignored "-Wunused-function"

#include <hip/hip_runtime.h>

#include "chain_dev.h"
#include "chain_search.h"
#include "chain_shared.h"
#include "chain_tiles.h"
#include "exact_sum.h"
#include "internal.h"
#include "wave_ops.h"

namespace tdstar {

namespace {

// The comparison form of the grid search: it reads the grid's descriptor (DevChain, CellGrid) where the
// product's wave_grid_search (chain_search.h) reads its LDS copy, and proves through grid_block_lb.
// Only the test kernels below run it (modes 1 and 6); test_grid_query_forms_agree holds it against the
// product's.  Lanes 0..53 cover the 3x3x3 buckets around the query, 8 entries per bucket; `skip` = the
// killed slot; slot `moved` is taken at (mx,my,mz) instead of its stored site.
__device__ __forceinline__ Nearest wave_grid_search(const DevChain &d, bool ovf, int lane, double x, double y,
                                                    double z, int skip, int moved, double mx, double my, double mz,
                                                    double mzeta) {
    const CellGrid &G = d.grid;
    const int bi = grid_axis(x, G.x0, G.ix, G.gx), bj = grid_axis(y, G.y0, G.iy, G.gy),
              bk = grid_axis(z, G.z0, G.iz, G.gz);
    const int nb = lane % 27, grp = lane / 27;
    const int ii = bi + nb % 3 - 1, jj = bj + (nb / 3) % 3 - 1, kk = bk + nb / 9 - 1;
    const bool inb = lane < 54 && ii >= 0 && ii < G.gx && jj >= 0 && jj < G.gy && kk >= 0 && kk < G.gz;
    const int b = inb ? (kk * G.gy + jj) * G.gx + ii : 0;
    // global_ loads (vmcnt only): the scalar loads of the grid's fields below wait on lgkmcnt, which a
    // flat_ load would hold until these loads are back
    const int cnt = gload(d.bucket_count + b);
    CellEntry e[4];
    int sl[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const CellEntry *ep = d.buckets + b * kBucketCap + grp * 4 + u;
        e[u].x = gload(&ep->x);
        e[u].y = gload(&ep->y);
        e[u].z = gload(&ep->z);
        e[u].zeta = gload(&ep->zeta);
        sl[u] = gload(d.bslot + b * kBucketCap + grp * 4 + u);
    }
    // every cell outside the 3x3x3 block is at least sqrt(lb) away: computed while the loads fly
    const double lb = grid_block_lb(G, x, y, z, 1);
    double bd = kSentinel, bz = 0.0;
    int bs = -1;
    bool tie = false;
    const bool overfull = inb && cnt > 8;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const bool ok = inb && grp * 4 + u < cnt && sl[u] != skip && sl[u] != moved;
        const double dd = dist2(e[u].x, e[u].y, e[u].z, x, y, z);
        if (ok) {
            if (dd < bd) {
                bd = dd;
                bs = sl[u];
                bz = e[u].zeta;
                tie = false;
            } else if (dd == bd && dd < kSentinel) {
                tie = true;
            }
        }
    }
    if (lane == 63 && moved >= 0) {  // the moved cell, at its proposed site
        const double dd = dist2(mx, my, mz, x, y, z);
        if (dd < bd) {
            bd = dd;
            bs = moved;
            bz = mzeta;
            tie = false;
        } else if (dd == bd && dd < kSentinel) {
            tie = true;
        }
    }
    const unsigned long long key = (unsigned long long)__double_as_longlong(bd);
    const unsigned long long kmin = wave_min_u64(key);
    const unsigned long long who = __ballot(key == kmin);
    const int win = __builtin_ctzll(who);
    Nearest res;
    res.d = __longlong_as_double((long long)kmin);
    const bool found = res.d < kSentinel;
    // distinct slots at the minimum (a slot sits in one lane only), or a tie inside the winner
    const bool tied = found && (__popcll(who) > 1 || __builtin_amdgcn_readlane((int)tie, win) != 0);
    const bool any_over = __ballot(overfull) != 0ull;
    res.s = found ? __builtin_amdgcn_readlane(bs, win) : -1;
    res.z = found ? readlane_f64(bz, win) : 0.0;
    res.proven = !ovf && !tied && !any_over && res.d < lb;
    return res;
}

// The proposal-time chi^2 of phase F on a caller-given ptS (testing): terms as
// phase E writes them, the one-wave exact scan from k0 = 0 and from k0 = n/2
// (C0 = the sequential prefix[k0 - 1] of k_chi2_prefix).
__global__ __launch_bounds__(64) void k_test_chain_chi2(const double *__restrict__ ptS, const double *__restrict__ tS,
                                                        const double *__restrict__ sig, int n,
                                                        const double *__restrict__ prefix, double *term,
                                                        double *cprefix, double *out) {
    const int lane = threadIdx.x;
    for (int r = lane; r < n; r += 64) {
        const double df = ptS[r] - tS[r];
        const double sg = sig[r];
        term[r] = ((df * df) * 1.0) / (sg * sg);  // MCsub.jl:171
    }
    __syncthreads();
    bool stopped = false;
    const double a = wave_seq_sum(term, n, 0.0, cprefix, lane, nullptr, &stopped);
    const int k0 = n / 2;
    stopped = false;
    const double b = k0 < n ? wave_seq_sum(term + k0, n - k0, k0 > 0 ? prefix[k0 - 1] : 0.0, cprefix + k0, lane, nullptr,
                                           &stopped)
                            : a;
    if (lane == 0) {
        out[0] = a;
        out[1] = b;
    }
}

}  // namespace

hipError_t test_chain_chi2(const double *ptS, const double *tS, const double *sig, int n, int path, double *scratch,
                           double *out, hipStream_t s) {
    if (n < 1 || n > 4096) return hipErrorInvalidValue;
    double *prefix = scratch, *term = scratch + n, *cpre = scratch + 2 * n;
    ChainScalars *st = reinterpret_cast<ChainScalars *>(scratch + 3 * n + 8);  // 16-byte aligned slot
    static_assert(sizeof(ChainScalars) <= 1024, "scratch slot");
    hipError_t e = launch_chi2_prefix(ptS, tS, sig, n, prefix, st, s);
    if (e != hipSuccess) return e;
    if (path == 2) return hipMemcpyAsync(out, &st->phi, sizeof(double), hipMemcpyDeviceToDevice, s);
    hipLaunchKernelGGL(k_test_chain_chi2, dim3(1), dim3(64), 0, s, ptS, tS, sig, n, prefix, term, cpre, out);
    return hipGetLastError();
}

// Testing: the latency of a nearest-cell query through the chain's bucket grid, as phases B and D run
// it: one wave answers nq queries back to back, each point offset by 0 * the previous answer (no two
// overlap).  mode 0: wave_nearest; 1: its loads only (the sum of what they bring); 2: its arithmetic only
// (the loads replaced by values made from the lane).  out[0] = cycles, out[1] = unproven queries.
__global__ __launch_bounds__(64) void k_test_query_lat(const DevChain *__restrict__ dptr, const double *__restrict__ pts,
                                                        int nq, int mode, long long *out) {
    __shared__ Shared sh;
    const DevChain &d = *dptr;
    const int lane = threadIdx.x;
    Views v{};
    v.ord = d.order;
    if (lane == 0) {
        sh.grid_ovf = *d.grid_overflow;
        sh.grid_fallbacks32 = 0;
        sh.nslots = d.st->nslots;
        geo_fill(sh.geo, d);
    }
    __syncthreads();
    double acc = 0.0;
    unsigned long long hsh = 0xcbf29ce484222325ull;
    const long long t0 = clock64();
    for (int i = 0; i < nq; ++i) {
        const double k = acc * 0.0;
        const double x = pts[3 * i] + k, y = pts[3 * i + 1] + k, z = pts[3 * i + 2] + k;
        if (mode == 0 || mode == 6) {  // 6: the descriptor-reading search (d.grid), for comparison
            const Nearest r = mode == 0 ? wave_grid_search(sh.geo, sh.grid_ovf != 0, lane, x, y, z, -1, -1, 0.0, 0.0,
                                                           0.0, 0.0)
                                        : wave_grid_search(d, sh.grid_ovf != 0, lane, x, y, z, -1, -1, 0.0, 0.0,
                                                           0.0, 0.0);
            acc = r.z;
            // (a digest of every answer: the two searches must agree)
            hsh = hsh * 0x100000001b3ull ^ (unsigned long long)__double_as_longlong(r.d) ^
                  ((unsigned long long)(unsigned)r.s << 1) ^ (unsigned long long)r.proven;
        } else {
            const CellGrid &G = d.grid;
            const int bi = grid_axis(x, G.x0, G.ix, G.gx), bj = grid_axis(y, G.y0, G.iy, G.gy),
                      bk = grid_axis(z, G.z0, G.iz, G.gz);
            const int nb = lane % 27, grp = lane / 27;
            const int ii = bi + nb % 3 - 1, jj = bj + (nb / 3) % 3 - 1, kk = bk + nb / 9 - 1;
            const bool inb = lane < 54 && ii >= 0 && ii < G.gx && jj >= 0 && jj < G.gy && kk >= 0 && kk < G.gz;
            const int b = inb ? (kk * G.gy + jj) * G.gx + ii : 0;
            double t = 0.0;
            if (mode == 3) {  // the bucket indices alone
                t = (double)(b + grp);
            } else if (mode == 4) {  // the block's face bound alone
                t = grid_block_lb(G, x, y, z, 1);
            } else if (mode == 5) {  // one lexicographic wave minimum alone
                t = (double)wave_min_u64((unsigned long long)(b + lane));
            } else if (mode == 1) {
                const int cnt = gload(d.bucket_count + b);
                double a = 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const CellEntry *ep = d.buckets + b * kBucketCap + grp * 4 + u;
                    a = a + gload(&ep->x) + gload(&ep->y) + gload(&ep->z) + gload(&ep->zeta) +
                        (double)gload(d.bslot + b * kBucketCap + grp * 4 + u);
                }
                t = a + (double)cnt;
                t = wave_sum_f64(t);
            } else {
                double bd = kSentinel;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double dd = dist2((double)b, (double)u, (double)lane, x, y, z);
                    bd = dd < bd ? dd : bd;
                }
                const double lb = grid_block_lb(G, x, y, z, 1);
                const unsigned long long kmin = wave_min_u64((unsigned long long)__double_as_longlong(bd));
                t = __longlong_as_double((long long)kmin) < lb ? 1.0 : 2.0;
            }
            acc = t;
        }
    }
    const long long t1 = clock64();
    if (lane == 0) {
        out[0] = t1 - t0;
        out[1] = sh.grid_fallbacks32;
        out[2] = __double_as_longlong(acc);
        out[3] = (long long)hsh;
    }
}

// Testing: every query's answer (squared distance, the winning cell's value, proven) from the chain's grid
// search, mode 0 (the LDS GridGeo copy with the global first bound) or 6 (the descriptor-reading form):
// the tests compare the proven ones with an exact scan (tdt_chain_query_answers)
__global__ __launch_bounds__(64) void k_test_query_answers(const DevChain *__restrict__ dptr, const double *__restrict__ pts,
                                                           int nq, int mode, double *out_d, double *out_z, int *out_p) {
    __shared__ Shared sh;
    const DevChain &d = *dptr;
    const int lane = threadIdx.x;
    if (lane == 0) {
        sh.grid_ovf = *d.grid_overflow;
        sh.grid_fallbacks32 = 0;
        geo_fill(sh.geo, d);
    }
    __syncthreads();
    for (int i = 0; i < nq; ++i) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const Nearest r = mode == 0 ? wave_grid_search(sh.geo, sh.grid_ovf != 0, lane, x, y, z, -1, -1, 0.0, 0.0, 0.0, 0.0)
                                    : wave_grid_search(d, sh.grid_ovf != 0, lane, x, y, z, -1, -1, 0.0, 0.0, 0.0, 0.0);
        if (lane == 0) {
            out_d[i] = r.d;
            out_z[i] = r.z;
            out_p[i] = r.proven ? 1 : 0;
        }
    }
}

// Testing: the phase-B tile filter on given FP32 boxes (SoA, 3 x nt each), FP64 tile maxima and FP64
// queries: out[q * nt + t] = 1 if the filter lets tile t through for query q (mode 0 tile_may_hit, 1
// tile_may_hit2).  The tests hold it to "never drops a tile holding a point within the maximum".
__global__ void k_test_tile_filter(const float *__restrict__ lo, const float *__restrict__ hi,
                                   const double *__restrict__ maxd, int nt, const double *__restrict__ qs, int nq,
                                   int mode, unsigned char *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nt * nq) return;
    const int t = (int)(i % nt), q = (int)(i / nt);
    const double x = qs[3 * q], y = qs[3 * q + 1], z = qs[3 * q + 2];
    bool h;
    if (mode == 0) {
        h = tile_may_hit(lo, hi, nt, t, tile_query(x, y, z), tile_thr(maxd[t]));
    } else {
        h = tile_may_hit2(tile_box(lo, hi, maxd, nt, t), tile_query2(x, y, z));
    }
    out[i] = h ? 1 : 0;
}

hipError_t test_tile_filter(const float *lo, const float *hi, const double *maxd, int nt, const double *qs, int nq,
                            int mode, unsigned char *out, hipStream_t s) {
    const long long n = (long long)nt * nq;
    hipLaunchKernelGGL(k_test_tile_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lo, hi, maxd, nt, qs,
                       nq, mode, out);
    return hipGetLastError();
}

hipError_t test_query_answers(const DevChain *dev, const double *pts, int nq, int mode, double *out_d, double *out_z,
                              int *out_p, hipStream_t s) {
    hipLaunchKernelGGL(k_test_query_answers, dim3(1), dim3(64), 0, s, dev, pts, nq, mode, out_d, out_z, out_p);
    return hipGetLastError();
}

hipError_t test_query_lat(const DevChain *dev, const double *pts, int nq, int mode, long long *out, hipStream_t s) {
    hipLaunchKernelGGL(k_test_query_lat, dim3(1), dim3(64), 0, s, dev, pts, nq, mode, out);
    return hipGetLastError();
}

namespace {

// Testing: the cross-lane primitives of wave_ops.h, one wave per block: block r applies primitive `op` to
// row r of in[nrows][64] (lane l holds word l) and writes every lane's result to out[nrows][64]
// (tdt_wave_ops).  op 0 wave_min_u64, 1 wave_min_u64_2p, 2 wave_min_u32 on the low words, 3 wave_xor_u64,
// 4 row_max_u64, 5 wave_scan_f64, 6 wave_sum_f64, 7 readlane_f64 of lane arg[r] (the host has checked
// 0 <= arg[r] < 64; one row's lane is wave-uniform).
__global__ __launch_bounds__(64) void k_test_wave_ops(const unsigned long long *__restrict__ in,
                                                       const int *__restrict__ arg, int op,
                                                       unsigned long long *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const unsigned long long v = in[i];
    const double f = __longlong_as_double((long long)v);
    unsigned long long r = 0ull;
    switch (op) {
        case 0: r = wave_min_u64(v); break;
        case 1: r = wave_min_u64_2p(v); break;
        case 2: r = (unsigned long long)wave_min_u32((unsigned)v); break;
        case 3: r = wave_xor_u64(v); break;
        case 4: r = row_max_u64(v); break;
        case 5: r = (unsigned long long)__double_as_longlong(wave_scan_f64(f)); break;
        case 6: r = (unsigned long long)__double_as_longlong(wave_sum_f64(f)); break;
        default: r = (unsigned long long)__double_as_longlong(readlane_f64(f, arg[blockIdx.x])); break;
    }
    out[i] = r;
}

// Testing: wave_full_scan on caller-given slot arrays, one wave answering the queries one after another
// (tdt_nearest_scan).  The host has checked 1 <= cap, 0 <= nslots <= cap and every skip / moved in
// [-1, cap): the scan reads slots min(s, cap - 1) only, and the winner is a slot below nslots.
__global__ __launch_bounds__(64) void k_test_nearest_scan(
    const long long *__restrict__ stamp, const double *__restrict__ cx, const double *__restrict__ cy,
    const double *__restrict__ cz, const double *__restrict__ czeta, int cap, int nslots,
    const double *__restrict__ q, const int *__restrict__ skip, const int *__restrict__ moved,
    const double *__restrict__ msite, int nq, double *out_d, int *out_s, double *out_z) {
    const int lane = threadIdx.x;
    for (int i = 0; i < nq; ++i) {
        const Nearest r = wave_full_scan(stamp, cx, cy, cz, czeta, cap, nslots, lane, q[3 * i], q[3 * i + 1],
                                         q[3 * i + 2], skip[i], moved[i], msite[3 * i], msite[3 * i + 1],
                                         msite[3 * i + 2]);
        if (lane == 0) {
            out_d[i] = r.d;
            out_s[i] = r.s;
            out_z[i] = r.z;
        }
    }
}

// Testing: a chain's nearest-cell query with a killed and a moved cell, as phases B and D and the drop-in
// query ask it (tdt_chain_nearest): per query a killed and a moved cell as 0-based Julia positions (-1:
// none; the host has checked them against ncells), mapped to slots through d.order as k_chain_run maps
// them, the moved cell's site, and czeta[moved] as its value.  mode 0: the product's wave_grid_search on
// the LDS GridGeo, 6: the descriptor form above, 7: wave_nearest (grid, then the full scan).  One wave;
// out_s = the winner's slot (-1: none).
__global__ __launch_bounds__(64) void k_test_chain_nearest(const DevChain *__restrict__ dptr,
                                                           const double *__restrict__ pts,
                                                           const int *__restrict__ kill_pos,
                                                           const int *__restrict__ move_pos,
                                                           const double *__restrict__ msite, int nq, int mode,
                                                           double *out_d, double *out_z, int *out_p, int *out_s) {
    __shared__ Shared sh;
    const DevChain &d = *dptr;
    const int lane = threadIdx.x;
    Views v{};
    v.ord = d.order;
    if (lane == 0) {
        sh.grid_ovf = *d.grid_overflow;
        sh.grid_fallbacks32 = 0;
        sh.nslots = d.st->nslots;
        geo_fill(sh.geo, d);
    }
    __syncthreads();
    for (int i = 0; i < nq; ++i) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const int skip = kill_pos[i] >= 0 ? d.order[kill_pos[i]] : -1;
        const int moved = move_pos[i] >= 0 ? d.order[move_pos[i]] : -1;
        const double mx = msite[3 * i], my = msite[3 * i + 1], mz = msite[3 * i + 2];
        const double mzeta = moved >= 0 ? d.czeta[moved] : 0.0;
        Nearest r;
        if (mode == 0) r = wave_grid_search(sh.geo, sh.grid_ovf != 0, lane, x, y, z, skip, moved, mx, my, mz, mzeta);
        else if (mode == 6) r = wave_grid_search(d, sh.grid_ovf != 0, lane, x, y, z, skip, moved, mx, my, mz, mzeta);
        else r = wave_nearest(d, v, sh, lane, x, y, z, skip, moved, mx, my, mz, mzeta);
        if (lane == 0) {
            out_d[i] = r.d;
            out_z[i] = r.z;
            out_p[i] = r.proven ? 1 : 0;
            out_s[i] = r.s;
        }
    }
}

}  // namespace

hipError_t test_wave_ops(const unsigned long long *in, const int *arg, int nrows, int op, unsigned long long *out,
                         hipStream_t s) {
    hipLaunchKernelGGL(k_test_wave_ops, dim3((unsigned)nrows), dim3(64), 0, s, in, arg, op, out);
    return hipGetLastError();
}

hipError_t test_nearest_scan(const long long *stamp, const double *cx, const double *cy, const double *cz,
                             const double *czeta, int cap, int nslots, const double *q, const int *skip,
                             const int *moved, const double *msite, int nq, double *out_d, int *out_s, double *out_z,
                             hipStream_t s) {
    hipLaunchKernelGGL(k_test_nearest_scan, dim3(1), dim3(64), 0, s, stamp, cx, cy, cz, czeta, cap, nslots, q, skip,
                       moved, msite, nq, out_d, out_s, out_z);
    return hipGetLastError();
}

hipError_t test_chain_nearest(const DevChain *dev, const double *pts, const int *kill_pos, const int *move_pos,
                              const double *msite, int nq, int mode, double *out_d, double *out_z, int *out_p,
                              int *out_s, hipStream_t s) {
    hipLaunchKernelGGL(k_test_chain_nearest, dim3(1), dim3(64), 0, s, dev, pts, kill_pos, move_pos, msite, nq, mode,
                       out_d, out_z, out_p, out_s);
    return hipGetLastError();
}

}  // namespace tdstar
