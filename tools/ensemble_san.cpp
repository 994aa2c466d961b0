// The host-only part of csrc/ensemble.h under the host sanitizers: ensemble_check_arrays on the refusal
// table's offset arrays and the fold of ensemble_from_histories (HistoryRule::SameDevice: no context, no HIP
// call) over hand-made host mirrors, an ensemble of 0-cell models among them.  A program of its own:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined --offload-arch=gfx950 \
//         tools/ensemble_san.cpp -o /tmp/ensemble_san && /tmp/ensemble_san
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../mcmc-in-tonga_amd/csrc/ensemble.h"

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

int main() {
    using namespace tdstar;
    const std::vector<double> c(8, 0.0);
    const double *a = c.data();
    const std::vector<int64_t> good{0, 1, 2, 3, 4, 5, 6, 7, 8}, first1{1, 1, 2, 3, 4, 5, 6, 7, 8},
        desc{0, 8, 5, 6, 7, 8, 8, 8, 8}, neg{0, 1, 2, 3, 4, 5, 6, 7, -1}, none(9, 0), two{0, 8, 5};
    expect(ensemble_check_arrays(nullptr, "t", 8, good.data(), a, a, a, a) == TD_OK, "valid offsets");
    expect(ensemble_check_arrays(nullptr, "t", 8, none.data(), nullptr, nullptr, nullptr, nullptr) == TD_OK, "0-cell models");
    expect(ensemble_check_arrays(nullptr, "t", 0, good.data(), a, a, a, a) != TD_OK && g_err == "t: need nmodels >= 1 and cell_off", "nmodels = 0");
    expect(ensemble_check_arrays(nullptr, "t", 8, nullptr, a, a, a, a) != TD_OK && g_err == "t: need nmodels >= 1 and cell_off", "cell_off NULL");
    expect(ensemble_check_arrays(nullptr, "t", 8, first1.data(), a, a, a, a) != TD_OK && g_err == "t: bad cell offsets or arrays", "cell_off[0] = 1");
    expect(ensemble_check_arrays(nullptr, "t", 8, neg.data(), a, a, a, a) != TD_OK && g_err == "t: bad cell offsets or arrays", "negative total");
    expect(ensemble_check_arrays(nullptr, "t", 8, good.data(), nullptr, a, a, a) != TD_OK && g_err == "t: bad cell offsets or arrays", "arrays NULL");
    expect(ensemble_check_arrays(nullptr, "t", 8, desc.data(), a, a, a, a) != TD_OK && g_err == "t: offsets not monotone", "descending");
    expect(ensemble_check_arrays(nullptr, "t", 2, two.data(), a, a, a, a) != TD_OK && g_err == "t: offsets not monotone", "[0, 8, 5]");

    // histories by their host mirrors: 3 samples of 5, 8, 12 cells; none; 2 samples of 0 cells
    td_history h1, h2, h3;
    h1.samples = 3;
    h1.off = {0, 5, 13, 25};
    h2.samples = 0;
    h2.off = {0};
    h3.samples = 2;
    h3.off = {0, 0, 0};
    {
        td_history *hs[] = {&h1, &h2, &h3};
        Ensemble E;
        expect(ensemble_from_histories(nullptr, "t", hs, 3, HistoryRule::SameDevice, &E) == TD_OK, "the fold");
        const std::vector<int64_t> want{0, 5, 13, 25, 25, 25};
        expect(E.nmodels == 5 && E.own_off == want && E.total() == 25, "the prefix");
        expect(E.segs && E.segs->size() == 2 && (*E.segs)[0] == &h1 && (*E.segs)[1] == &h3, "the segments skip the empty history");
        expect(E.nchains == 2 && E.chain_len[0] == 3 && E.chain_len[1] == 2, "the chains");
        expect(ensemble_check_arrays(nullptr, "t", E.nmodels, E.cell_off, nullptr, nullptr, nullptr, nullptr) != TD_OK, "a fold has no host arrays");
    }
    {
        td_history *hs[] = {&h3};
        Ensemble E;
        expect(ensemble_from_histories(nullptr, "t", hs, 1, HistoryRule::SameDevice, &E) == TD_OK && E.nmodels == 2 && E.total() == 0, "only 0-cell models");
        expect(ensemble_check_arrays(nullptr, "t", E.nmodels, E.cell_off, nullptr, nullptr, nullptr, nullptr) == TD_OK, "0-cell models need no arrays");
    }
    {
        td_history *hs[] = {&h2, nullptr};
        Ensemble E, F, G, H;
        expect(ensemble_from_histories(nullptr, "t", hs, 1, HistoryRule::SameDevice, &E) != TD_OK && g_err == "t: the histories hold no sample", "only empty histories");
        expect(ensemble_from_histories(nullptr, "t", hs, 2, HistoryRule::SameDevice, &F) != TD_OK && g_err == "t: a history is NULL", "a NULL history");
        expect(ensemble_from_histories(nullptr, "t", nullptr, 3, HistoryRule::SameDevice, &G) != TD_OK && g_err == "t: the histories hold no sample", "hs NULL");
        expect(ensemble_from_histories(nullptr, "t", hs, 2, HistoryRule::SameContext, &H) != TD_OK && g_err == "t: ctx is NULL", "same context, no context");
    }
    std::printf(failures ? "%d failed\n" : "ensemble_san: clean\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
