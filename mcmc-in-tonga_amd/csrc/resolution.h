// resolution.h -- the host arithmetic of the posterior resolution (resolution.hip; include/tdstar_resolution.h):
// the offsets' check, their flat offsets and reach on a lattice, the axis lists the runs walk, and the plan of the
// ring of blocks.  Pure host code on the standard library alone, shared by the entry points, the hook
// tdt_resolution_plan and tools/resolution_san.cpp.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <vector>

namespace tdstar {

constexpr int64_t kResMaxOffsets = 4096;
constexpr int64_t kResDefaultBudget = (int64_t)2 << 30;  // bytes of the resident blocks' value matrices (a choice: DESIGN 4.6m)
constexpr int64_t kResTile = 64;                         // a block is a multiple of this many nodes

// What is wrong with off[noff][3] (noff in 1 .. kResMaxOffsets), or null: every offset forward, none twice.
inline const char *res_offsets_check(const int32_t *off, int64_t noff) {
    std::vector<std::array<int32_t, 3>> seen((size_t)noff);
    for (int64_t o = 0; o < noff; ++o) {
        const int32_t di = off[3 * o], dj = off[3 * o + 1], dk = off[3 * o + 2];
        if (!(dk > 0 || (dk == 0 && dj > 0) || (dk == 0 && dj == 0 && di > 0))) return "an offset is not forward";
        seen[(size_t)o] = {dk, dj, di};
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return "an offset appears twice";
    return nullptr;
}

// One offset on a lattice: f > 0, the flat offset, where |di| < nx, |dj| < ny and dk < nz; else f = 0 -- no pair of
// it lies on the lattice.
struct ResOffset {
    int32_t di, dj, dk, pad;
    int64_t f;
};
// (nx, ny, nz <= 2^30 and nx ny nz < 2^63: the sum fits)
inline std::vector<ResOffset> res_offsets_on(const int32_t *off, int64_t noff, int64_t nx, int64_t ny, int64_t nz, int64_t *reach) {
    std::vector<ResOffset> t((size_t)noff);
    *reach = 0;
    for (int64_t o = 0; o < noff; ++o) {
        const int64_t di = off[3 * o], dj = off[3 * o + 1], dk = off[3 * o + 2];
        const bool in = di > -nx && di < nx && dj > -ny && dj < ny && dk < nz;
        t[(size_t)o] = {(int32_t)di, (int32_t)dj, (int32_t)dk, 0, in ? di + nx * (dj + ny * dk) : 0};
        *reach = std::max(*reach, t[(size_t)o].f);
    }
    return t;
}

// The runs' lists: ax[a] = the indices in the list of e_a, 2 e_a, ... up to the first multiple that is missing.
inline std::array<std::vector<int32_t>, 3> res_axis_lists(const int32_t *off, int64_t noff) {
    std::array<std::vector<int32_t>, 3> ax;
    for (int a = 0; a < 3; ++a) {
        std::vector<int32_t> at;  // at[l - 1] = the index of l e_a, -1: not in the list
        for (int64_t o = 0; o < noff; ++o) {
            const int32_t *d = off + 3 * o;
            if (d[(a + 1) % 3] != 0 || d[(a + 2) % 3] != 0 || d[a] > kResMaxOffsets) continue;  // (longer than any list: never reached)
            if ((size_t)d[a] > at.size()) at.resize((size_t)d[a], -1);
            at[(size_t)d[a] - 1] = (int32_t)o;
        }
        for (int32_t i : at) {
            if (i < 0) break;
            ax[(size_t)a].push_back(i);
        }
    }
    return ax;
}

// The x-runs: the offsets with pairs on the lattice in the order (dk, dj, di) -- `order`, indices into the list -- cut
// into runs of at most kResRunMax offsets that share (dj, dk) and whose di follow each other by one: the partners of a
// run's offsets are one contiguous segment of columns.  first = the run's first position in `order`, f0 = the flat
// offset of that offset.
constexpr int kResRunMax = 12;
struct ResRun {
    int32_t first, cnt;
    int64_t f0;
};
inline std::vector<ResRun> res_xruns(const std::vector<ResOffset> &tab, std::vector<int32_t> *order) {
    order->clear();
    for (size_t o = 0; o < tab.size(); ++o)
        if (tab[o].f > 0) order->push_back((int32_t)o);
    std::sort(order->begin(), order->end(), [&](int32_t a, int32_t b) {
        const ResOffset &x = tab[(size_t)a], &y = tab[(size_t)b];
        return std::array<int32_t, 3>{x.dk, x.dj, x.di} < std::array<int32_t, 3>{y.dk, y.dj, y.di};
    });
    std::vector<ResRun> runs;
    for (size_t p = 0; p < order->size(); ++p) {
        const ResOffset &o = tab[(size_t)(*order)[p]];
        if (!runs.empty() && runs.back().cnt < kResRunMax) {
            const ResOffset &last = tab[(size_t)(*order)[p - 1]];
            if (last.dk == o.dk && last.dj == o.dj && (int64_t)last.di + 1 == o.di) {
                ++runs.back().cnt;
                continue;
            }
        }
        runs.push_back({(int32_t)p, 1, o.f});
    }
    return runs;
}

// The ring: blocks of ns consecutive flat nodes, R = ceil(reach / ns) + 1 of them resident, nblocks covering
// [0, nq).  ns = the largest multiple of 64, at most `ceiling` (one sweep's nodes: volume_plan) and nq rounded up
// to 64, with 8 nmodels ns R <= budget; `forced` (> 0) rounded down to a multiple of 64, at least 64, at most the
// ceiling, whatever the budget.  ns == 0: no block of 64 nodes fits.  (0 <= reach < nq <= 2^56, ceiling >= 64.)
struct ResPlan {
    int64_t ns = 0, R = 0, nblocks = 0;
};
inline ResPlan res_plan(int64_t nmodels, int64_t nq, int64_t reach, int64_t budget, int64_t forced, int64_t ceiling) {
    const int64_t nm = std::max<int64_t>(nmodels, 1), b = budget > 0 ? budget : kResDefaultBudget;
    const int64_t top = std::min(ceiling, (nq + kResTile - 1) / kResTile * kResTile);
    auto ring = [&](int64_t ns) { return (reach + ns - 1) / ns + 1; };
    ResPlan p;
    if (forced > 0) {
        p.ns = std::min(std::max(forced / kResTile * kResTile, kResTile), ceiling);
    } else {
        const int64_t room = b / 8 / nm;  // columns of all resident blocks
        for (int64_t ns = top; ns >= kResTile && p.ns == 0; ns -= kResTile)
            if (ring(ns) <= room / ns) p.ns = ns;  // (ns R <= room, without the product)
        if (p.ns == 0) return p;
    }
    p.R = ring(p.ns);
    p.nblocks = (nq + p.ns - 1) / p.ns;
    return p;
}

}  // namespace tdstar
