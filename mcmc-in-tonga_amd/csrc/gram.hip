// gram.hip -- ensemble Gram and distance matrices: gram[a][b] = sum_p X[a][p] X[b][p] and dist2[a][b] =
// sum_p (X[a][p] - X[b][p])^2 over the centred, weighted value matrix X[m][p] = sqrt(w[p]) (V[m][p] - mean[p]) of
// an ensemble on a point list (include/tdstar_gram.h holds the contract; gram.h the host arithmetic).
//
// The search structure is the volume's (volume_build).  The point list is swept slab by slab of volume_plan's
// columns, a multiple of 64, so that no block of the sums' association (64 points, left to right; the block sums
// added in order to an accumulator that starts at +0.0) straddles two slabs.  Per slab:
//   volume_sweep      V_slab[M][ns]
//   k_raster_stats    the slab's mean and sigma (raster.hip's kernel: the numbers are td_rasterize's)
//   k_gram_centre     X_slab in place of V_slab, one lane per element: d = v - mean, then r * d
//   k_gram_pairs      a symmetric FP64 rank-ns update of the M x M matrices in the workspace.  A workgroup of
//                     16 x 16 lanes owns one tile of T x T pairs of the lower triangle (T = 16 RT, a lane keeps
//                     RT x RT pairs: the rows gram_lane_row(ti, .) against the rows gram_lane_row(tj, .)).  It takes
//                     its accumulators from the matrices (the first slab starts them at +0.0: nothing is zeroed
//                     across calls), walks the slab's points in chunks of 16 -- the two tiles' rows of a chunk staged
//                     transposed in LDS, [point][row] with rows of T + 2 doubles, the next chunk's loads in flight
//                     in registers meanwhile -- and per point reads its 2 RT operands as 16-byte pairs (16 lanes of
//                     one ti cover 256 consecutive bytes: no bank is met twice) and forms p = a b, bs = bs + p and
//                     e = a - b, q = e e, bs' = bs' + q, each rounded once.  Every fourth chunk ends a block:
//                     acc = acc + bs, and bs starts again at -0.0 (-0.0 + t is t for every t, the sign of a zero
//                     included: the block's sum runs from its first term).  Rows past M and points past the slab's
//                     end are never read; the rows hold 0.0 and their pairs are not stored, the points are not
//                     walked.  The diagonal's tiles are formed whole.
//   after the last slab k_gram_mirror copies the lower triangle to the upper (32 x 32 through LDS), and the
//   matrices go to the caller.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/tdstar_gram.h"
#include "ctx.h"
#include "ensemble.h"
#include "gram.h"
#include "history.h"
#include "volume.h"

namespace tdstar {

namespace {

constexpr int kGramThreads = kGramLanes * kGramLanes;
constexpr int kGramChunk = 16;  // points staged at a time; kGramBlock / kGramChunk chunks end a block
static_assert(kGramBlock == kVolTile, "a slab is a multiple of the association's block");
static_assert(kGramBlock % kGramChunk == 0 && kGramChunk == kGramLanes, "a thread stages one point of a chunk");
int g_gram_form = 0;  // tdt_set_gram_form: 0 the kept one

// X = X_slab[M][ns] in place of V_slab: r[p] * (V[m][p] - mean[p]), two roundings
__global__ __launch_bounds__(256) void k_gram_centre(double *__restrict__ V, long ns, long total,
                                                     const double *__restrict__ mean, const double *__restrict__ r) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long p = i % ns;
        const double d = V[i] - mean[p];
        V[i] = r[p] * d;
    }
}

// one point of the staged chunk: a, b = the lane's rows of the two tiles at that point
template <int RT, bool kGram, bool kDist>
__device__ __forceinline__ void gram_point(const double *__restrict__ pa, const double *__restrict__ pb, int ti, int tj,
                                           double (&bg)[RT][RT], double (&bd)[RT][RT]) {
    double a[RT], b[RT];
#pragma unroll
    for (int h = 0; h < RT / 2; ++h) {
        const double2 va = *reinterpret_cast<const double2 *>(pa + h * 32 + 2 * ti);
        const double2 vb = *reinterpret_cast<const double2 *>(pb + h * 32 + 2 * tj);
        a[2 * h] = va.x;
        a[2 * h + 1] = va.y;
        b[2 * h] = vb.x;
        b[2 * h + 1] = vb.y;
    }
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < RT; ++j) {
            if (kGram) {
                const double p = a[i] * b[j];
                bg[i][j] = bg[i][j] + p;
            }
            if (kDist) {
                const double e = a[i] - b[j];
                const double q = e * e;
                bd[i][j] = bd[i][j] + q;
            }
        }
}

// X [M][ns]: the slab.  G, D [M][M] (null unless kGram / kDist).  Workgroup = tile blockIdx.x of the lower
// triangle (gram_tile_of).  first: the call's first slab.
template <int RT, bool kGram, bool kDist>
__global__ __launch_bounds__(kGramThreads, RT <= 4 ? 2 : 1) void k_gram_pairs(const double *__restrict__ X, long ns, int M, int first,
                                                             double *__restrict__ G, double *__restrict__ D) {
    constexpr int T = kGramLanes * RT, S = T + 2;
    __shared__ __attribute__((aligned(16))) double sm[2 * kGramChunk * S];
    double *const sa = sm, *const sb = sm + kGramChunk * S;
    int ta, tb;
    gram_tile_of((int)blockIdx.x, &ta, &tb);
    const int tid = (int)threadIdx.x, tj = tid & (kGramLanes - 1), ti = tid >> 4;
    const int ra = ta * T, rb = tb * T;
    double accg[RT][RT], accd[RT][RT], bg[RT][RT], bd[RT][RT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < RT; ++j) {
            const int row = ra + gram_lane_row(ti, i), col = rb + gram_lane_row(tj, j);
            const bool in = !first && row < M && col < M;
            accg[i][j] = kGram && in ? G[(long)row * M + col] : 0.0;
            accd[i][j] = kDist && in ? D[(long)row * M + col] : 0.0;
            bg[i][j] = -0.0;
            bd[i][j] = -0.0;
        }
    // staging: this thread's point of a chunk is tj, its rows of each tile ti + 16 i
    double fa[RT], fb[RT];
    const auto fetch = [&](long k0) {
        const long k = k0 + tj;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const int rowa = ra + ti + kGramLanes * i, rowb = rb + ti + kGramLanes * i;
            fa[i] = k < ns && rowa < M ? X[(long)rowa * ns + k] : 0.0;
            fb[i] = k < ns && rowb < M ? X[(long)rowb * ns + k] : 0.0;
        }
    };
    const long nchunks = (ns + kGramChunk - 1) / kGramChunk;
    fetch(0);
    for (long c = 0; c < nchunks; ++c) {
        __syncthreads();  // (the chunk before has been read)
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            sa[tj * S + ti + kGramLanes * i] = fa[i];
            sb[tj * S + ti + kGramLanes * i] = fb[i];
        }
        __syncthreads();
        if (c + 1 < nchunks) fetch((c + 1) * kGramChunk);
        const int nk = (int)min((long)kGramChunk, ns - c * kGramChunk);
        if (nk == kGramChunk) {
#pragma unroll 4
            for (int k = 0; k < kGramChunk; ++k) gram_point<RT, kGram, kDist>(sa + k * S, sb + k * S, ti, tj, bg, bd);
        } else {
            for (int k = 0; k < nk; ++k) gram_point<RT, kGram, kDist>(sa + k * S, sb + k * S, ti, tj, bg, bd);
        }
        if ((c & (kGramBlock / kGramChunk - 1)) == kGramBlock / kGramChunk - 1 || c + 1 == nchunks) {
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int j = 0; j < RT; ++j) {
                    if (kGram) accg[i][j] = accg[i][j] + bg[i][j];
                    if (kDist) accd[i][j] = accd[i][j] + bd[i][j];
                    bg[i][j] = -0.0;
                    bd[i][j] = -0.0;
                }
        }
    }
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < RT; ++j) {
            const int row = ra + gram_lane_row(ti, i), col = rb + gram_lane_row(tj, j);
            if (row < M && col < M) {
                if (kGram) G[(long)row * M + col] = accg[i][j];
                if (kDist) D[(long)row * M + col] = accd[i][j];
            }
        }
}

// A [M][M]: A[i][j] = A[j][i] for i < j.  Workgroup (x, y), x >= y: the 32 x 32 block of rows 32 x, columns 32 y.
__global__ __launch_bounds__(256) void k_gram_mirror(double *__restrict__ A, int M) {
    __shared__ double t[32][33];
    if (blockIdx.x < blockIdx.y) return;
    const int r0 = (int)blockIdx.x * 32, c0 = (int)blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8)
        if (r0 + r < M && c0 + tx < M) t[r][tx] = A[(long)(r0 + r) * M + c0 + tx];
    __syncthreads();
    for (int c = ty; c < 32; c += 8) {  // the upper element (c0 + c, r0 + tx) from the lower (r0 + tx, c0 + c)
        const int row = c0 + c, col = r0 + tx;
        if (row < col && col < M) A[(long)row * M + col] = t[tx][c];
    }
}

template <int RT>
void gram_launch_pairs(hipStream_t s, unsigned tiles, const double *X, long ns, int M, int first, double *G, double *D) {
    if constexpr (RT <= 4) {
        if (G && D) {
            hipLaunchKernelGGL((k_gram_pairs<RT, true, true>), dim3(tiles), dim3(kGramThreads), 0, s, X, ns, M, first, G, D);
            return;
        }
    }
    // (at 8 x 8 the accumulators of both forms do not fit a lane's registers: a launch each)
    if (G) hipLaunchKernelGGL((k_gram_pairs<RT, true, false>), dim3(tiles), dim3(kGramThreads), 0, s, X, ns, M, first, G, nullptr);
    if (D) hipLaunchKernelGGL((k_gram_pairs<RT, false, true>), dim3(tiles), dim3(kGramThreads), 0, s, X, ns, M, first, nullptr, D);
}

// the checks of both entry points that need no context and no HIP call, in the header's order
int gram_check(td_ctx *ctx, const td_gram *w, const char *who) {
    const std::string n(who);
    if (!w) return set_err(ctx, TD_ERR_ARG, n + ": want is NULL");
    if (const char *what = gram_check_want(w)) return set_err(ctx, TD_ERR_ARG, n + ": " + what);
    return TD_OK;
}

// Both entry points; E and w have been checked (ensemble.h, gram_check).
int gram_core(td_ctx *ctx, const char *who, const Ensemble &E, const td_gram *w) {
    const int64_t M = E.nmodels, np = w->np;
    const bool want_g = w->gram_out != nullptr, want_d = w->dist2_out != nullptr, pairs = want_g || want_d;
    if (pairs && M > kGramMaxModels)
        return set_err(ctx, TD_ERR_ARG, std::string(who) + ": " + std::to_string(M) + " models: a matrix [M][M] exceeds 1 GiB (at most " +
                                            std::to_string(kGramMaxModels) + " models)");
    const double W = gram_weight(w->w, 0, np - 1);
    const VolPlan plan = volume_plan(M, np, kVolDefaultBudget, ctx->vol_slab_nodes);
    const int64_t cap = std::min(plan.nodes, np);
    const GramLayout l = gram_layout(M, cap, want_g, want_d);
    const int form = g_gram_form ? g_gram_form : kGramKeptForm;
    TD_HIP(ctx, hipSetDevice(ctx->device));
    servers_quiesce(nullptr);
    VolSearch S;
    if (int rc = volume_build(ctx, who, E, &S)) return rc;
    hipStream_t s = ctx->stream;
    if (int rc = raster_reserve(ctx, l.words, l.pinned)) return rc;
    double *base = ctx->raster.as<double>(), *dq = base + l.q, *dr = base + l.r, *dv = base + l.v, *dm = base + l.mean,
           *dsd = base + l.sd, *dG = want_g ? base + l.gram : nullptr, *dD = want_d ? base + l.dist2 : nullptr;
    double *hr = ctx->h_raster.as<double>() + 3 * cap;
    TD_HIP(ctx, hipStreamSynchronize(s));  // (the pinned block and the workspace are free)
    const unsigned tiles = (unsigned)gram_tile_count(M, gram_form_tile(form));
    int64_t brute_pairs = 0;
    for (int64_t c0 = 0; c0 < np; c0 += plan.nodes) {
        const int64_t ns = std::min(plan.nodes, np - c0);
        if (int rc = stage_queries(ctx, w->px, w->py, w->pz, c0, ns, dq)) return rc;
        if (pairs) {
            gram_roots(w->w, c0, ns, hr);
            TD_HIP(ctx, hipMemcpyAsync(dr, hr, sizeof(double) * (size_t)ns, hipMemcpyHostToDevice, s));
        }
        if (int rc = volume_sweep(ctx, S, 0, M, dq, ns, dv)) return rc;
        if (!S.grid) brute_pairs += M * ns;
        if (pairs || w->mean_out) {
            TD_HIP(ctx, timed_launch(ctx, "raster_stats", [&] { return launch_raster_stats(dv, (int)M, (int)ns, dm, dsd, s); }));
            if (w->mean_out) {
                TD_HIP(ctx, hipMemcpyAsync(w->mean_out + c0, dm, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
                TD_HIP(ctx, hipMemcpyAsync(w->std_out + c0, dsd, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, s));
            }
        }
        if (pairs) {
            const long total = (long)(M * ns);
            TD_HIP(ctx, timed_launch(ctx, "gram_centre", [&] {
                       hipLaunchKernelGGL(k_gram_centre, dim3((unsigned)std::min<long>((total + 255) / 256, 1 << 16)), dim3(256), 0, s, dv,
                                          (long)ns, total, dm, dr);
                   }));
            TD_HIP(ctx, timed_launch(ctx, "gram_pairs", [&] {  // (a form's launches under the one name)
                       if (form == 2)
                           gram_launch_pairs<8>(s, tiles, dv, (long)ns, (int)M, (int)(c0 == 0), dG, dD);
                       else
                           gram_launch_pairs<4>(s, tiles, dv, (long)ns, (int)M, (int)(c0 == 0), dG, dD);
                   }));
        }
        TD_HIP(ctx, hipStreamSynchronize(s));  // the pinned block is packed again for the next slab
    }
    if (pairs) {
        const unsigned nb = (unsigned)((M + 31) / 32);
        TD_HIP(ctx, timed_launch(ctx, "gram_mirror", [&] {
                   if (dG) hipLaunchKernelGGL(k_gram_mirror, dim3(nb, nb), dim3(256), 0, s, dG, (int)M);
                   if (dD) hipLaunchKernelGGL(k_gram_mirror, dim3(nb, nb), dim3(256), 0, s, dD, (int)M);
               }));
        const size_t bytes = sizeof(double) * (size_t)M * (size_t)M;
        if (dG) TD_HIP(ctx, hipMemcpyAsync(w->gram_out, dG, bytes, hipMemcpyDeviceToHost, s));
        if (dD) TD_HIP(ctx, hipMemcpyAsync(w->dist2_out, dD, bytes, hipMemcpyDeviceToHost, s));
        TD_HIP(ctx, hipStreamSynchronize(s));
    }
    if (w->wsum_out) *w->wsum_out = W;
    return volume_counters_finish(ctx, S, brute_pairs);
}

}  // namespace

}  // namespace tdstar

using namespace tdstar;

extern "C" int td_rasterize_gram(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell, const double *yCell,
                                 const double *zCell, const double *zeta, const td_gram *want) {
    const char *who = "td_rasterize_gram";
    return ensemble_entry_arrays(
        ctx, who, Ensemble(nmodels, cell_off, xCell, yCell, zCell, zeta), nullptr, [&] { return gram_check(ctx, want, who); },
        [&](const Ensemble &E) { return gram_core(ctx, who, E, want); });
}

extern "C" int td_history_gram(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_gram *want) {
    const char *who = "td_history_gram";
    return ensemble_entry_histories(
        ctx, who, hs, nh, nullptr, [&] { return gram_check(ctx, want, who); },
        [&](const Ensemble &E) { return gram_core(ctx, who, E, want); });
}

extern "C" int tdt_gram_plan(int64_t nmodels, int64_t np, int64_t budget, int64_t forced, int64_t out[2]) {
    if (!out || nmodels < 1 || np < 1 || budget < 0 || forced < 0) return TD_ERR_ARG;
    const VolPlan p = volume_plan(nmodels, np, budget, forced);
    out[0] = p.nodes;
    out[1] = p.nslabs;
    return TD_OK;
}

extern "C" int tdt_set_gram_form(int form) {
    if (form < 0 || form > kGramForms) return TD_ERR_ARG;
    g_gram_form = form;
    return TD_OK;
}

extern "C" int tdt_gram_tile(int form) {
    if (form < 0 || form > kGramForms) return -1;
    return gram_form_tile(form ? form : kGramKeptForm);
}

extern "C" int64_t tdt_gram_tiles(int64_t nmodels, int form, int64_t index, int64_t out[2]) {
    if (nmodels < 1 || nmodels > kGramMaxModels || form < 0 || form > kGramForms) return -1;
    const int64_t n = gram_tile_count(nmodels, gram_form_tile(form ? form : kGramKeptForm));
    if (out) {
        if (index < 0 || index >= n) return -1;
        int ta, tb;
        gram_tile_of((int)index, &ta, &tb);
        out[0] = ta;
        out[1] = tb;
    }
    return n;
}
