// The host-only part of csrc/region_sums.h under the host sanitizers: region_list_check on a well-formed list, on
// every malformed reg_off it names and on its other refusals (with and without the extra vector of recovery),
// and region_layout (the part of region_plan that needs no context) on one region of 1 point and on regions of
// 1, 1023, 1024, 1025 and 2049 points.  A program of its own:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined --offload-arch=gfx950 \
//         tools/region_san.cpp -o /tmp/region_san && /tmp/region_san
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../mcmc-in-tonga_amd/csrc/region_sums.h"

static std::string g_err;
int tdstar::set_err(td_ctx *, int code, const std::string &msg) {
    g_err = msg;
    return code;
}
int tdstar::hip_err(td_ctx *, hipError_t, const char *what) {
    g_err = what;
    return TD_ERR_ARG;
}

static int failures = 0;
static void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s (last message: %s)\n", what, g_err.c_str());
        ++failures;
    }
}

using namespace tdstar;

// the list of regions of these sizes over exactly-sized arrays (the sanitizer sees a read past np or nreg + 1)
struct Fixture {
    std::vector<double> p, w, truth;
    std::vector<int64_t> off;
    explicit Fixture(const std::vector<int64_t> &sizes) : off(1, 0) {
        for (int64_t n : sizes) off.push_back(off.back() + n);
        p.assign((size_t)off.back(), 1.5);
        truth.assign((size_t)off.back(), 2.0);
        for (int64_t i = 0; i < off.back(); ++i) w.push_back(0.25 * (double)(i % 7 + 1));
    }
    RegionList list(bool weights) const {
        return {p.data(), p.data(), p.data(), weights ? w.data() : nullptr, (int64_t)p.size(), off.data(), (int64_t)off.size() - 1, 1};
    }
};

static bool refused(const RegionList &l, const RegionVector *extra, const char *msg) {
    return region_list_check(nullptr, "t", l, extra) == TD_ERR_ARG && g_err == msg;
}

// leafp, regleaf, W, most and L as the kernels read them
static void check_layout(const Fixture &f, bool weights, int64_t leaves, const char *what) {
    const RegionList l = f.list(weights);
    RegionPlan p;
    region_layout(l, &p);
    const int64_t R = l.nreg;
    bool ok = p.R == R && p.np == l.np && p.L == leaves && (int64_t)p.leafp.size() == p.L + 1 &&
              (int64_t)p.regleaf.size() == R + 1 && (int64_t)p.W.size() == R && p.leafp.front() == 0 && p.leafp.back() == l.np &&
              p.regleaf.front() == 0 && p.regleaf.back() == p.L;
    int64_t most = 1;
    for (int64_t r = 0; ok && r < R; ++r) {
        const int64_t lo = l.reg_off[r], hi = l.reg_off[r + 1];
        most = std::max(most, hi - lo);
        ok = p.leafp[(size_t)p.regleaf[(size_t)r]] == lo && p.leafp[(size_t)p.regleaf[(size_t)r + 1]] == hi;  // no leaf spans two regions
        double s = 0.0;
        for (int64_t i = lo; i < hi; ++i) s += weights ? l.w[i] : 1.0;  // (quarters: exact in any order)
        ok = ok && p.W[(size_t)r] == s;
    }
    for (int64_t k = 0; ok && k < p.L; ++k) {
        const int64_t n = p.leafp[(size_t)k + 1] - p.leafp[(size_t)k];
        ok = n >= 1 && n <= 1024;
    }
    expect(ok && p.most == most, what);
}

int main() {
    const Fixture one({1}), five({1, 1023, 1024, 1025, 2049});
    const RegionVector truth1{one.truth.data(), "truth"}, truth5{five.truth.data(), "truth"}, no_truth{nullptr, "truth"};
    expect(region_list_check(nullptr, "t", one.list(false), nullptr) == TD_OK, "one region of 1 point");
    expect(region_list_check(nullptr, "t", one.list(true), &truth1) == TD_OK, "one region of 1 point, weights and truth");
    expect(region_list_check(nullptr, "t", five.list(false), nullptr) == TD_OK, "five regions");
    expect(region_list_check(nullptr, "t", five.list(true), &truth5) == TD_OK, "five regions, weights and truth");
    check_layout(one, false, 1, "layout: one region of 1 point");
    check_layout(one, true, 1, "layout: one region of 1 point, weights");
    check_layout(five, false, 8, "layout: 1 + 1 + 1 + 2 + 3 leaves");
    check_layout(five, true, 8, "layout: 1 + 1 + 1 + 2 + 3 leaves, weights");

    {  // every malformed reg_off the check names
        RegionList l = five.list(true);
        std::vector<int64_t> off = five.off;
        l.reg_off = off.data();
        off[0] = 1;
        expect(refused(l, nullptr, "t: reg_off[0] must be 0"), "reg_off[0] = 1");
        off = five.off;
        off[2] = off[1] - 1;
        expect(refused(l, nullptr, "t: reg_off is not monotone"), "descending");
        off = five.off;
        off[3] = off[2];
        expect(refused(l, nullptr, "t: a region without points"), "an empty region");
        off = five.off;
        off[4] = l.np + 1;  // (the next offset is below it, but this one is met first)
        expect(refused(l, nullptr, "t: reg_off[nreg] must be np"), "an offset beyond np");
        off = five.off;
        off[5] = l.np - 1;
        expect(refused(l, nullptr, "t: reg_off[nreg] must be np"), "the last offset below np");
        off = five.off;
        off[5] = l.np + 1;
        expect(refused(l, &truth5, "t: reg_off[nreg] must be np"), "the last offset beyond np");
    }
    {  // the other refusals, in the order they are made
        RegionList l = five.list(true);
        l.np = 0;
        expect(refused(l, nullptr, "t: np and nreg must be >= 1"), "np = 0");
        l = five.list(true);
        l.nreg = 0;
        expect(refused(l, &truth5, "t: np and nreg must be >= 1"), "nreg = 0");
        l = five.list(true);
        l.pz = nullptr;
        expect(refused(l, nullptr, "t: px, py, pz and reg_off must be given"), "pz NULL");
        expect(refused(l, &truth5, "t: px, py, pz, reg_off and truth must be given"), "pz NULL, with truth");
        l = five.list(true);
        l.reg_off = nullptr;
        expect(refused(l, nullptr, "t: px, py, pz and reg_off must be given"), "reg_off NULL");
        l = five.list(true);
        expect(refused(l, &no_truth, "t: px, py, pz, reg_off and truth must be given"), "truth NULL");
        std::vector<double> bad = five.p;
        bad.back() = NAN;
        l.py = bad.data();
        expect(refused(l, &truth5, "t: py is not finite"), "py NaN at the last point");
        l = five.list(true);
        bad = five.w;
        bad.front() = INFINITY;
        l.w = bad.data();
        expect(refused(l, &truth5, "t: w is not finite"), "w infinite");
        l = five.list(false);
        const RegionVector bad_truth{bad.data(), "truth"};
        expect(refused(l, &bad_truth, "t: truth is not finite"), "truth infinite, no weights");
        l.normalize = 2;
        expect(refused(l, nullptr, "t: normalize must be 0 or 1"), "normalize = 2");
        expect(refused(l, &bad_truth, "t: truth is not finite"), "truth before normalize");
    }
    std::printf(failures ? "%d failed\n" : "region_san: clean\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
