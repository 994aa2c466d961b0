// history.h -- td_history: thinned chain samples recorded in device memory
// (include/tdstar.h "Sample history").  The buffers are what a recorded launch's
// RecDesc points to (chain_dev.h); the host keeps the number of samples and a
// mirror of their cell offsets, refreshed after every call that appends.
#pragma once
#include <cstdint>
#include <vector>

#include "chain_dev.h"
#include "ctx.h"

struct td_history {
    td_ctx *ctx = nullptr;
    int64_t max_samples = 0, max_cells = 0;  // capacity: samples, cells of all samples together
    int64_t n = 0;                           // rays (a ptS row)
    void *block = nullptr;                   // one device allocation behind every buffer
    tdstar::RecDesc d{};                     // the buffers (base / first / every are a launch's, unused here)
    int64_t samples = 0;                     // samples held
    std::vector<int64_t> off;                // host mirror of off[0 .. samples]
};

namespace tdstar {

// Samples a run of `iterations` takes at first, first + every, ... (1-based).
inline int64_t history_new_samples(int64_t iterations, int64_t first, int64_t every) {
    return first <= iterations ? (iterations - first) / every + 1 : 0;
}
// TD_ERR_ARG (message set) unless h has room for `added` more samples of at most `cells_each` cells.
int history_check_room(const td_history *h, int64_t added, int64_t cells_each, const char *who);
// After a launch appended `added` samples: their offsets into the host mirror (one small copy).
int history_adopt(td_history *h, int64_t added);
// A recorded ladder's call (chain.cpp td_rounds_temper_recorded / td_rounds_exchange_recorded): its
// `added` samples lie in slots of `cells_each` cells from the history's first free cell on, their headers
// at samples, samples + 1, ...  Packs them in place (history_pack.hip; the context's stream, timer name
// "history_pack"), forms their offsets on the device and adopts them.  The launch that wrote the slots
// has ended.
int history_pack_adopt(td_history *h, int64_t added, int64_t cells_each);
// The pack kernel: `count` slots of S cells from cell slot0 of each of the four component arrays, ncells
// [count] the cells each holds, off[0] = slot0 in place -> off[1 .. count].  kPackChunk: the cells one
// round of its block moves (the tests cross it).
constexpr int kPackChunk = 1024;
hipError_t launch_history_pack(double *cells, long long stride, long long slot0, long long S, const int *ncells,
                               long long count, long long *off, hipStream_t s);
// One sample from host arrays (the HOST and DROPIN engines' loop): copies into the same buffers.
int history_append_host(td_history *h, const double *x, const double *y, const double *z, const double *zeta,
                        int64_t ncells, double phi, int64_t iter, int action, int accept, const double *ptS);

}  // namespace tdstar
