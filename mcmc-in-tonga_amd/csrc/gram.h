// gram.h -- the host arithmetic of the ensemble Gram and distance matrices (gram.hip; include/tdstar_gram.h): the
// request's checks, the limit of a matrix, the square roots of the weights, the tiles of the lower triangle a
// workgroup owns, and the carving of the call's workspace.  Pure host code on the standard library alone (the tile
// index is the kernel's too), shared by the entry points, the hooks and tools/gram_san.cpp.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/tdstar_gram.h"

#if defined(__HIPCC__)
#define TD_GRAM_HD __host__ __device__
#else
#define TD_GRAM_HD
#endif

namespace tdstar {

constexpr int64_t kGramMaxModels = TD_GRAM_MAX_MODELS;  // 8 M^2 <= 1 GiB
static_assert(8 * kGramMaxModels * kGramMaxModels <= ((int64_t)1 << 30) &&
                  8 * (kGramMaxModels + 1) * (kGramMaxModels + 1) > ((int64_t)1 << 30),
              "the largest M whose matrix fits a GiB");
constexpr int kGramBlock = 64;   // the points of a block of the sums' association (kVolTile: no block straddles a slab)
constexpr int kGramLanes = 16;   // a workgroup is 16 x 16 lanes
constexpr int kGramForms = 2;    // tdt_set_gram_form: 1 .. kGramForms
constexpr int kGramKeptForm = 1; // (the measurements)

// the pairs a lane keeps along each side, and the rows of a workgroup's tile; 0 for a form that does not exist
inline int gram_form_pairs(int form) { return form == 1 ? 4 : form == 2 ? 8 : 0; }
inline int gram_form_tile(int form) { return kGramLanes * gram_form_pairs(form); }

// What is wrong with a request, or null: the header's refusals from `np < 1` to `only one of mean and std`, in its
// order (want is not NULL).
inline const char *gram_check_want(const td_gram *w) {
    if (w->np < 1) return "np must be >= 1";
    if (!w->px || !w->py || !w->pz) return "px, py and pz must be given";
    const double *xyz[3] = {w->px, w->py, w->pz};
    for (int a = 0; a < 3; ++a)
        for (int64_t i = 0; i < w->np; ++i)
            if (!std::isfinite(xyz[a][i])) return "a coordinate is not finite";
    for (int64_t i = 0; w->w && i < w->np; ++i)
        if (!std::isfinite(w->w[i]) || w->w[i] < 0.0) return "every weight must be finite and >= 0";
    if (!w->gram_out && !w->dist2_out && !w->mean_out && !w->std_out && !w->wsum_out) return "no output asked for";
    if (!w->mean_out != !w->std_out) return "mean_out and std_out must be given together";
    return nullptr;
}

// r[i] = sqrt(w[c0 + i]) for a slab's ns points (std::sqrt: IEEE's correctly rounded root); w null: 1.0
inline void gram_roots(const double *w, int64_t c0, int64_t ns, double *r) {
    for (int64_t i = 0; i < ns; ++i) r[i] = w ? std::sqrt(w[c0 + i]) : 1.0;
}

// W: the sum of w[lo .. hi] (null: of ones) in td_rasterize's association -- pairwise halves at (lo + hi) >> 1 down
// to blocks of at most 1024, each left to right (fewer than 16 terms left to right is the same order).  This is
// region_weight of region_sums.h, restated: that header holds kernels of its own for the units that include it.
inline double gram_weight(const double *w, int64_t lo, int64_t hi) {
    if (hi - lo < 1024) {
        double s = w ? w[lo] : 1.0;
        for (int64_t k = lo + 1; k <= hi; ++k) s = s + (w ? w[k] : 1.0);
        return s;
    }
    const int64_t mid = (lo + hi) >> 1;
    const double a = gram_weight(w, lo, mid), b = gram_weight(w, mid + 1, hi);
    return a + b;
}

// The tiles of T rows of the lower triangle of an M x M matrix, the diagonal's included, row tile by row tile:
// index = ta (ta + 1) / 2 + tb, tb <= ta.
inline int64_t gram_tile_count(int64_t M, int T) {
    const int64_t nt = (M + T - 1) / T;
    return nt * (nt + 1) / 2;
}
// (index < 2^31: at most 182 row tiles of 64)
TD_GRAM_HD inline void gram_tile_of(int index, int *ta, int *tb) {
    int a = (int)((sqrt(8.0 * (double)index + 1.0) - 1.0) * 0.5);
    while (a * (a + 1) / 2 > index) --a;  // (the root's rounding, either way)
    while ((a + 1) * (a + 2) / 2 <= index) ++a;
    *ta = a;
    *tb = index - a * (a + 1) / 2;
}
// The row of its tile that lane u (0 .. 15) keeps as its element e (0 .. pairs - 1): the lanes' pairs of rows follow
// each other, so that 16 lanes' 16-byte reads of a staged block cover 256 consecutive bytes of LDS.
TD_GRAM_HD inline int gram_lane_row(int u, int e) { return (e >> 1) * 32 + 2 * u + (e & 1); }

// The call's workspace in 8-byte words, carved by its shape alone (M models, slabs of at most cap points):
// queries [3][cap] | roots [cap] | V_slab = X_slab [M][cap] | mean, std [cap] | gram [M][M] | dist2 [M][M]
struct GramLayout {
    size_t q = 0, r = 0, v = 0, mean = 0, sd = 0, gram = 0, dist2 = 0, words = 0, pinned = 0;
};
inline GramLayout gram_layout(int64_t M, int64_t cap, bool want_gram, bool want_dist2) {
    GramLayout l;
    const size_t c = (size_t)cap, mm = (size_t)M * (size_t)M;
    l.q = 0;
    l.r = l.q + 3 * c;
    l.v = l.r + c;
    l.mean = l.v + (size_t)M * c;
    l.sd = l.mean + c;
    l.gram = l.sd + c;
    l.dist2 = l.gram + (want_gram ? mm : 0);
    l.words = l.dist2 + (want_dist2 ? mm : 0);
    l.pinned = 4 * c;  // queries | roots
    return l;
}

}  // namespace tdstar
