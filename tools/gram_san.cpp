// The host-only part of the ensemble Gram and distance matrices (csrc/gram.h) under the host sanitizers:
// gram_check_want on legal requests and on every malformed one it names, in the header's order, each array exactly
// sized (the sanitizer sees a read past np); gram_roots and gram_weight on slabs and lists of every size around the
// tree's block; the tile bookkeeping (gram_tile_count, gram_tile_of, gram_lane_row) for every model count a matrix
// may have; and gram_layout, the carving of the workspace.  A program of its own:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined --offload-arch=gfx950 \
//         tools/gram_san.cpp -o /tmp/gram_san && /tmp/gram_san
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <set>
#include <utility>
#include <vector>

#include "../mcmc-in-tonga_amd/csrc/gram.h"

static int failures = 0;
static void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

using namespace tdstar;

// an array on the heap, exactly n numbers long
static std::unique_ptr<double[]> exact(int64_t n, double v) {
    std::unique_ptr<double[]> p(new double[(size_t)n]);
    for (int64_t i = 0; i < n; ++i) p[(size_t)i] = v + (double)i;
    return p;
}

static bool refused(const td_gram &w, const char *msg) {
    const char *got = gram_check_want(&w);
    return got && std::strcmp(got, msg) == 0;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    {  // the checks, in the header's order: each request is wrong in this way and in later ways
        for (int64_t np : {(int64_t)1, (int64_t)6, (int64_t)1025}) {
            auto x = exact(np, 0.0), y = exact(np, 1.0), z = exact(np, 2.0), wt = exact(np, 0.0);
            double out[4];
            td_gram w = {x.get(), y.get(), z.get(), wt.get(), np, out, out, out, out, out};
            expect(gram_check_want(&w) == nullptr, "a legal request");
            w.w = nullptr;
            expect(gram_check_want(&w) == nullptr, "no weights");
            w.w = wt.get();
            td_gram b = w;
            b.np = 0;
            b.px = nullptr;
            expect(refused(b, "np must be >= 1"), "np < 1 before the arrays");
            b = w;
            b.py = nullptr;
            x[(size_t)(np - 1)] = nan;
            expect(refused(b, "px, py and pz must be given"), "an array missing before the coordinates are read");
            b = w;
            wt[0] = -1.0;
            expect(refused(b, "a coordinate is not finite"), "the last px NaN, before the weights");
            x[(size_t)(np - 1)] = 0.0;
            z[(size_t)(np - 1)] = -inf;
            expect(refused(b, "a coordinate is not finite"), "the last pz infinite");
            z[(size_t)(np - 1)] = 2.0;
            b.gram_out = b.dist2_out = b.mean_out = b.std_out = b.wsum_out = nullptr;
            expect(refused(b, "every weight must be finite and >= 0"), "a negative weight, before the outputs");
            wt[0] = 0.0;
            wt[(size_t)(np - 1)] = inf;
            expect(refused(b, "every weight must be finite and >= 0"), "the last weight infinite");
            wt[(size_t)(np - 1)] = nan;
            expect(refused(b, "every weight must be finite and >= 0"), "the last weight NaN");
            wt[(size_t)(np - 1)] = -0.0;
            expect(refused(b, "no output asked for"), "no output (and a weight of -0.0 is legal)");
            b.std_out = out;
            expect(refused(b, "mean_out and std_out must be given together"), "std alone");
            b.std_out = nullptr;
            b.mean_out = out;
            b.gram_out = out;
            expect(refused(b, "mean_out and std_out must be given together"), "mean alone");
            b.mean_out = nullptr;
            expect(gram_check_want(&b) == nullptr, "gram alone");
            b.gram_out = nullptr;
            b.wsum_out = out;
            expect(gram_check_want(&b) == nullptr, "the weights' sum alone");
        }
    }
    {  // the roots of a slab and the weights' sum
        for (int64_t np : {(int64_t)1, (int64_t)15, (int64_t)16, (int64_t)64, (int64_t)1023, (int64_t)1024, (int64_t)1025, (int64_t)4099}) {
            auto wt = exact(np, 0.25);
            std::unique_ptr<double[]> r(new double[(size_t)np]);
            gram_roots(wt.get(), 0, np, r.get());
            bool ok = true;
            for (int64_t i = 0; i < np; ++i) ok = ok && r[(size_t)i] == std::sqrt(0.25 + (double)i);
            const int64_t c0 = np / 2, ns = np - c0;
            std::unique_ptr<double[]> tail(new double[(size_t)ns]);
            gram_roots(wt.get(), c0, ns, tail.get());
            for (int64_t i = 0; i < ns; ++i) ok = ok && tail[(size_t)i] == r[(size_t)(c0 + i)];
            gram_roots(nullptr, c0, ns, tail.get());
            for (int64_t i = 0; i < ns; ++i) ok = ok && tail[(size_t)i] == 1.0;
            expect(ok, "the roots of a slab");
            // sums of quarters and integers are exact in any order
            expect(gram_weight(wt.get(), 0, np - 1) == 0.25 * (double)np + 0.5 * (double)np * (double)(np - 1), "the weights' sum");
            expect(gram_weight(nullptr, 0, np - 1) == (double)np, "the sum of no weights");
        }
        // the association: pairwise halves above 1024, each left to right
        const int64_t np = 3000;
        std::unique_ptr<double[]> wt(new double[(size_t)np]);
        for (int64_t i = 0; i < np; ++i) wt[(size_t)i] = 1.0 / (double)(i + 3);
        const auto ltr = [&](int64_t lo, int64_t hi) {
            double s = wt[(size_t)lo];
            for (int64_t k = lo + 1; k <= hi; ++k) s = s + wt[(size_t)k];
            return s;
        };
        const double a = ltr(0, 749) + ltr(750, 1499), b = ltr(1500, 2249) + ltr(2250, 2999);
        expect(gram_weight(wt.get(), 0, np - 1) == a + b, "3000 weights are four blocks of 750");
    }
    {  // the tiles: every model count, both forms
        expect(gram_form_tile(1) == 64 && gram_form_tile(2) == 128 && gram_form_tile(0) == 0 && gram_form_tile(3) == 0, "the forms' tiles");
        expect(gram_form_pairs(kGramKeptForm) > 0, "the kept form exists");
        for (int form = 1; form <= kGramForms; ++form) {
            const int T = gram_form_tile(form), RT = gram_form_pairs(form);
            std::set<int> rows;
            for (int u = 0; u < kGramLanes; ++u)
                for (int e = 0; e < RT; ++e) {
                    const int r = gram_lane_row(u, e);
                    expect(r >= 0 && r < T && (e & 1) == (r & 1), "a lane's row lies in the tile");
                    rows.insert(r);
                }
            expect((int)rows.size() == T, "the lanes' rows cover the tile once");
            bool ok = true;
            for (int64_t M = 1; M <= kGramMaxModels && ok; M += (M < 300 ? 1 : 97)) {
                const int64_t nt = (M + T - 1) / T, n = gram_tile_count(M, T);
                ok = n == nt * (nt + 1) / 2 && n <= INT32_MAX;
            }
            expect(ok, "the count of tiles");
            const int64_t n = gram_tile_count(kGramMaxModels, T);
            int64_t at = 0;
            for (int ta = 0; ok && ta * (int64_t)T < kGramMaxModels; ++ta)
                for (int tb = 0; tb <= ta; ++tb, ++at) {
                    int a = -1, b = -1;
                    gram_tile_of((int)at, &a, &b);
                    ok = ok && a == ta && b == tb;
                }
            expect(ok && at == n, "every index of the largest matrix names its tile");
        }
    }
    {  // the workspace
        for (int64_t M : {(int64_t)1, (int64_t)70, kGramMaxModels})
            for (int64_t cap : {(int64_t)1, (int64_t)64, (int64_t)11520, (int64_t)1 << 18})
                for (int g = 0; g < 2; ++g)
                    for (int d = 0; d < 2; ++d) {
                        const GramLayout l = gram_layout(M, cap, g, d);
                        const size_t c = (size_t)cap, mm = (size_t)M * (size_t)M;
                        bool ok = l.q == 0 && l.r == 3 * c && l.v == 4 * c && l.mean == l.v + (size_t)M * c && l.sd == l.mean + c &&
                                  l.gram == l.sd + c && l.dist2 == l.gram + (g ? mm : 0) && l.words == l.dist2 + (d ? mm : 0) &&
                                  l.pinned == 4 * c;
                        expect(ok, "the parts follow each other without a gap");
                        expect(l.v % 2 == 0 || cap % 2 == 1, "the slab is 16-byte aligned for an even slab");
                    }
        expect(8 * kGramMaxModels * kGramMaxModels <= ((int64_t)1 << 30), "the largest matrix fits a GiB");
    }
    std::printf(failures ? "%d failed\n" : "gram_san: clean\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
