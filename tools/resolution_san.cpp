// The host-only part of the posterior resolution (csrc/resolution.h) under the host sanitizers: res_offsets_check
// on legal lists of 1 and 4096 offsets and on every malformed one it names, res_offsets_on (flat offsets, reach,
// offsets beyond the lattice, the int32 extremes), res_axis_lists (gaps, multiples longer than any list), res_xruns
// (the grouping into x-runs) and res_plan over a grid of (models, nodes, reach, budget, forced) with its refusal, each array exactly sized (the
// sanitizer sees a read past noff triples).  A program of its own:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined --offload-arch=gfx950 \
//         tools/resolution_san.cpp -o /tmp/resolution_san && /tmp/resolution_san
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../mcmc-in-tonga_amd/csrc/resolution.h"

static int failures = 0;
static void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

using namespace tdstar;
using Triples = std::vector<std::array<int32_t, 3>>;

// the list on the heap, exactly 3 noff numbers long
static std::unique_ptr<int32_t[]> exact(const Triples &t) {
    std::unique_ptr<int32_t[]> p(new int32_t[3 * t.size()]);
    for (size_t o = 0; o < t.size(); ++o) std::memcpy(p.get() + 3 * o, t[o].data(), sizeof(int32_t) * 3);
    return p;
}

static bool refused(const Triples &t, const char *msg) {
    const auto p = exact(t);
    const char *got = res_offsets_check(p.get(), (int64_t)t.size());
    return got && std::strcmp(got, msg) == 0;
}

static Triples box(int Lx, int Ly, int Lz) {
    Triples t;
    for (int dk = 0; dk <= Lz; ++dk)
        for (int dj = -Ly; dj <= Ly; ++dj)
            for (int di = -Lx; di <= Lx; ++di)
                if (dk > 0 || (dk == 0 && dj > 0) || (dk == 0 && dj == 0 && di > 0)) t.push_back({di, dj, dk});
    return t;
}

int main() {
    {  // the check
        Triples full;
        for (int i = 0; i < 4096; ++i) full.push_back({i - 2048, 1 + i % 3, i % 5});
        expect(res_offsets_check(exact({{1, 0, 0}}).get(), 1) == nullptr, "one offset");
        expect(res_offsets_check(exact(full).get(), 4096) == nullptr, "4096 offsets");
        expect(res_offsets_check(exact(box(5, 3, 5)).get(), 423) == nullptr && box(5, 3, 5).size() == 423, "the box (5, 3, 5)");
        expect(res_offsets_check(exact({{INT32_MIN, INT32_MIN, 1}, {INT32_MAX, INT32_MAX, INT32_MAX}, {INT32_MIN, 1, 0}}).get(), 3) ==
                   nullptr,
               "the int32 extremes");
        expect(refused({{0, 0, 0}}, "an offset is not forward"), "the null offset");
        expect(refused({{1, 0, 0}, {-1, 0, 0}}, "an offset is not forward"), "(-1, 0, 0)");
        expect(refused({{5, -1, 0}}, "an offset is not forward"), "(5, -1, 0)");
        expect(refused({{5, 5, -1}}, "an offset is not forward"), "(5, 5, -1)");
        expect(refused({{1, 0, 0}, {0, 1, 0}, {1, 0, 0}}, "an offset appears twice"), "a duplicate");
        full[4095] = full[7];
        expect(refused(full, "an offset appears twice"), "a duplicate among 4096");
        expect(refused({{1, 0, 0}, {1, 0, 0}, {0, 0, 0}}, "an offset is not forward"), "not forward is met before twice");
    }
    {  // flat offsets and reach
        const Triples t = {{1, 0, 0}, {-2, 1, 0}, {4, 3, 2}, {5, 0, 0}, {0, 4, 0}, {0, 0, 3}, {-5, 1, 0}, {INT32_MIN, INT32_MAX, INT32_MAX}};
        const auto p = exact(t);
        int64_t reach = -1;
        const std::vector<ResOffset> r = res_offsets_on(p.get(), (int64_t)t.size(), 5, 4, 3, &reach);
        const int64_t want[8] = {1, 3, 4 + 5 * (3 + 4 * 2), 0, 0, 0, 0, 0};
        bool ok = r.size() == t.size() && reach == 59;
        for (size_t o = 0; ok && o < t.size(); ++o) ok = r[o].f == want[o] && r[o].di == t[o][0] && r[o].dj == t[o][1] && r[o].dk == t[o][2];
        expect(ok, "flat offsets on 5 x 4 x 3");
        const std::vector<ResOffset> big = res_offsets_on(p.get(), (int64_t)t.size(), (int64_t)1 << 30, (int64_t)1 << 20, 1 << 7, &reach);
        expect(big[2].f == 4 + ((int64_t)1 << 30) * (3 + ((int64_t)1 << 20) * 2) && reach == big[5].f && big[5].f == (int64_t)3 << 50 && big[7].f == 0,
               "a lattice of 2^57 nodes");
        const std::vector<ResOffset> one = res_offsets_on(p.get(), (int64_t)t.size(), 1, 1, 1, &reach);
        expect(reach == 0 && one[0].f == 0, "a single node: no offset has a pair");
    }
    {  // the axis lists
        const Triples t = {{2, 0, 0}, {0, 0, 1}, {1, 0, 0}, {4, 0, 0}, {0, 2, 0}, {0, 0, 2}, {1, 1, 0}, {INT32_MAX, 0, 0}, {0, 0, 5000}, {0, 0, 3}};
        const auto p = exact(t);
        const auto ax = res_axis_lists(p.get(), (int64_t)t.size());
        expect(ax[0] == std::vector<int32_t>({2, 0}), "x: e, 2 e, then 3 e is missing");
        expect(ax[1].empty(), "y: e is missing");
        expect(ax[2] == std::vector<int32_t>({1, 5, 9}), "z: e, 2 e, 3 e");
        const Triples far = {{0, 4096, 0}, {0, 4097, 0}};
        expect(res_axis_lists(exact(far).get(), 2)[1].empty(), "multiples at the list's limit");
    }
    {  // the x-runs: the box (5, 3, 5) on the shipped lattice, a lattice narrower than the window, runs longer than twelve
        const Triples t = box(5, 3, 5);
        const auto p = exact(t);
        int64_t reach = 0;
        std::vector<int32_t> order;
        std::vector<ResOffset> tab = res_offsets_on(p.get(), (int64_t)t.size(), 58, 34, 34, &reach);
        std::vector<ResRun> runs = res_xruns(tab, &order);
        bool ok = order.size() == 423 && runs.size() == 39 && reach == 5 + 58 * (3 + 34 * 5);
        int64_t covered = 0;
        for (const ResRun &r : runs) {
            ok = ok && r.cnt >= 1 && r.cnt <= kResRunMax && r.first == covered && r.f0 == tab[(size_t)order[(size_t)r.first]].f;
            for (int g = 1; ok && g < r.cnt; ++g) {
                const ResOffset &o = tab[(size_t)order[(size_t)(r.first + g)]], &o0 = tab[(size_t)order[(size_t)r.first]];
                ok = o.dj == o0.dj && o.dk == o0.dk && o.di == o0.di + g && o.f == r.f0 + g;
            }
            covered += r.cnt;
        }
        expect(ok && covered == 423, "39 runs cover the 423 offsets of the box (5, 3, 5)");
        tab = res_offsets_on(p.get(), (int64_t)t.size(), 3, 2, 1, &reach);  // |di| < 3, |dj| < 2, dk < 1: (1, 0, 0), (2, 0, 0), (-2 .. 2, 1, 0)
        runs = res_xruns(tab, &order);
        expect(order.size() == 7 && runs.size() == 2 && runs[0].cnt == 2 && runs[1].cnt == 5 && reach == 5, "a lattice narrower than the window");
        Triples line;
        for (int i = 1; i <= 30; ++i) line.push_back({31 - i, 0, 0});  // (30 .. 1, 0, 0): the list's order does not matter
        tab = res_offsets_on(exact(line).get(), 30, 64, 1, 1, &reach);
        runs = res_xruns(tab, &order);
        expect(runs.size() == 3 && runs[0].cnt == 12 && runs[1].cnt == 12 && runs[2].cnt == 6 && runs[1].f0 == 13 && order[0] == 29,
               "thirty offsets along x are runs of 12, 12 and 6");
        tab = res_offsets_on(exact(line).get(), 30, 1, 1, 1, &reach);
        expect(res_xruns(tab, &order).empty() && order.empty(), "no offset with a pair: no run");
    }
    {  // the plan
        const int64_t ceilings[2] = {(int64_t)1 << 18, 8064};
        int64_t refusals = 0, plans = 0;
        for (int64_t M : {(int64_t)1, (int64_t)40, (int64_t)10000, (int64_t)1 << 25})
            for (int64_t nq : {(int64_t)1, (int64_t)60, (int64_t)540, (int64_t)266265, (int64_t)1 << 56})
                for (int64_t reach : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)372, nq - 1})
                    for (int64_t budget : {(int64_t)0, (int64_t)1 << 20, (int64_t)4 << 30, INT64_MAX})
                        for (int64_t forced : {(int64_t)0, (int64_t)1, (int64_t)100, (int64_t)1 << 40}) {
                            if (reach >= nq) continue;
                            const int64_t ceiling = ceilings[M > 10000];
                            const ResPlan p = res_plan(M, nq, reach, budget, forced, ceiling);
                            if (p.ns == 0) {
                                ++refusals;
                                expect(forced == 0, "a forced block is never refused");
                                continue;
                            }
                            ++plans;
                            const int64_t b = budget > 0 ? budget : kResDefaultBudget;
                            bool ok = p.ns % 64 == 0 && p.ns >= 64 && p.ns <= ceiling && (p.R - 1) * p.ns >= reach &&
                                      (p.R - 2) * p.ns < reach && (p.nblocks - 1) < nq / p.ns + 1 && p.nblocks >= nq / p.ns;
                            if (forced == 0) ok = ok && (__int128)8 * M * p.ns * p.R <= b;
                            expect(ok, "a plan's invariants");
                        }
        expect(refusals > 20 && plans > 500, "the grid holds refusals and plans");
        expect(res_plan(40, 540, 223, 0, 64, 1 << 18).R == 5 && res_plan(40, 540, 223, 0, 0, 1 << 18).ns == 576, "known plans");
        expect(res_plan(10000, 266265, 30000, 0, 0, 1 << 18).ns == 0, "a reach beyond the budget");
    }
    std::printf(failures ? "%d failed\n" : "resolution_san: clean\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
