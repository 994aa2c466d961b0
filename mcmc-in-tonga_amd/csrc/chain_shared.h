// chain_shared.h -- the chain kernels' shared state and LDS layout: the constants, the records kept in
// LDS, the bucket grid's LDS copy (GridGeo), the workgroup's Shared block, the LDS carve-up both host and
// device compute (lds_plan), the Views of the arrays a launch works on, the fused block copy (CopySeg)
// and a nearest-cell query's result.  Everything here has internal linkage: each unit that includes it
// (chain_kernels.hip, chain_state.hip, chain_test_kernels.hip) gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "chain_dev.h"
#include "exact_sum.h"
#include "internal.h"

namespace tdstar {

namespace {

using tdchain::Proposal;

constexpr int kWaves = kChainThreads / 64;
static_assert(kTilePts == 16, "a tile is one 16-lane DPP row (row_max_u64)");
constexpr int kOrphanLds = 96;  // orphan records kept in LDS (more: read back from HBM)
constexpr int kPre = 64 / kTilePts;  // LDS layout: hit tiles per wave whose points phase B preloads
static_assert(kPre == 4, "the preload slots are four registers");
constexpr int kCtmLds = 256;    // tiles in LDS, rays in HBM: hit tiles' candidate maxima kept in LDS
constexpr int kListLds = 1024;  // rays in HBM: hit tiles / changed rays / hit super-tiles kept in LDS
// LDS layout, phase D: from this many orphans on, one search for all of them (the bucket region
// around them staged once in LDS, a thread per orphan) instead of one wave's grid search each
constexpr int kBatchOrphans = 64;
constexpr int kBatchCand = 192;     // cell entries staged (phase E's idle ray scratch: 28 B each)
constexpr int kBatchBuckets = 512;  // buckets in the region at most
// Phase C leaves lanes idle (16 per hit tile, ~8 tiles): wave 7 lane 0 forms the decision's
// phi_n-free parts; wave 6 lane 0 (LDS layout) begins the next proposal's guess -- its global loads
// fly across the phase barriers until phase F finishes it there
// The LDS layout could sum chi^2 with the event walk too; its tails are ~60 terms and the
// one-wave binade scan with the early-rejection bound is faster there (measured: the walk
// costs ~1.2k more cycles per proposal at 381 rays x 5000 cells)
constexpr bool kSmallWalk = false;

// A changed point's candidate (what mark() stores in the overlay), kept in LDS for the first kChgLds of
// a proposal: phase G commits them from here with stores only -- no dependent round trips to the
// changed list and the overlay in HBM
// (o: the point's owner before the proposal -- what phase G needs to keep DevChain::own without a load)
struct ChgRec {
    int q, s;
    double d, z;
    int o;
};
constexpr int kChgLds = 64;

// A point whose nearest cell is removed or moved: re-searched in phase D.
struct OrphanRec {
    double x, y, z;
    int q, ray;
};

__device__ __forceinline__ double dist2(double cx, double cy, double cz, double x, double y, double z) {
    // (mx-x)^2 + (my-y)^2 + (mz-z)^2, MCsub.jl:254 -- same ops as k_nn_partial
    const double dx = cx - x, dy = cy - y, dz = cz - z;
    double d = dx * dx;
    d = d + dy * dy;
    d = d + dz * dz;
    return d;
}

// (distance, Julia position) lexicographic order; a cell must also beat the
// 1e9 sentinel strictly (MCsub.jl:250,255).
template <class R>
__device__ __forceinline__ bool better(double d, R r, double bd, R br) {
    return d < bd || (d == bd && d < kSentinel && r < br);
}

// A proposal with what it needs from the model (tid 0 builds it).
struct PState {
    Proposal p;
    double kx, ky, kz, zeta_killed;  // site and value of the selected cell (not birth)
    int slot_k, new_slot, eval;
    // the selected cell owned no ray point (DevChain::own) when the proposal was made AND nothing can have
    // changed ownership since: set only on a guess of phase F, cleared at its adoption unless the iteration
    // it was made in left every owner alone (k_chain_run, the iteration's end).  Down, it says nothing (the
    // guess read a count above 0, or was cleared; a proposal wave 0 makes at an iteration's end, and a
    // launch's first, never asked): a free-running change or death then reads the count at the loop top.  A
    // change or death whose cell owns no point changes no ray: it takes the short road (no tile pass, no
    // phases C-E)
    int barren;
};

// The bucket grid's geometry and arrays, copied into LDS when a launch starts: a query reads them in
// one round of LDS loads rather than one scalar load (and wait) per descriptor field, and bounds the
// block without branches (wave_grid_search)
struct GridGeo {
    double x0, y0, z0, ix, iy, iz, hx, hy, hz, ex, ey, ez;
    double lo[3], hi[3];
    // a bound every query may use first: each face of a query's 3x3x3 block is at least h - e (the
    // cells' allowance) - e (the query's own bucket rounding, within the same allowance) away on its
    // axis, so every cell outside the block is at least lb0 away (+inf when no axis can have a face)
    double lb0;
    const int *count;
    const CellEntry *buckets;
    const int *bslot;
    int gx, gy, gz, sealed;
};
__device__ __forceinline__ void geo_fill(GridGeo &g, const DevChain &d) {
    const CellGrid &G = d.grid;
    g.x0 = G.x0; g.y0 = G.y0; g.z0 = G.z0;
    g.ix = G.ix; g.iy = G.iy; g.iz = G.iz;
    g.hx = G.hx; g.hy = G.hy; g.hz = G.hz;
    g.ex = G.ex; g.ey = G.ey; g.ez = G.ez;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = G.lo[a];
        g.hi[a] = G.hi[a];
    }
    g.count = d.bucket_count;
    g.buckets = d.buckets;
    g.bslot = d.bslot;
    g.gx = G.gx; g.gy = G.gy; g.gz = G.gz;
    g.sealed = G.sealed;
    const double h3[3] = {G.hx, G.hy, G.hz}, e3[3] = {G.ex, G.ey, G.ez};
    const int g3[3] = {G.gx, G.gy, G.gz};
    double lb0 = __builtin_huge_val();
    for (int a = 0; a < 3; ++a) {
        if (g3[a] < 3) continue;  // the block spans the axis: no face on it
        const double gap = (h3[a] - 2.0 * e3[a]) * (1.0 - 0x1p-30);
        const double f = gap > 0.0 ? gap * gap : 0.0;
        lb0 = f < lb0 ? f : lb0;
    }
    g.lb0 = grid_lb_close(lb0);
}

struct Shared {
    GridGeo geo;       // the bucket grid (geo_fill at a launch's start)
    PState ps[2];      // this iteration's proposal (ps[cur]) and the next one guessed in phase F
    int cur, spec_ok;
    int defer;  // phase F: accepted on bounds (LDS layout): the new chi^2 partial sums are not formed
    double phi_n;
    // decisions on bounds (phase F; wave 0): prefix[] exact below ex_upto, phi_r an
    // estimate in [phi_lo, phi_hi] (held here, not in registers: the kernel is at its VGPR limit)
    int ex_upto;
    double phi_lo, phi_hi, b_lo, b_hi;
    // The proposal's counters (atomic adds in phases B-E; wave 0 clears them at the iteration's end for the
    // next one).  No wave reads them after phase F's barrier: phase G reads the snapshot gs instead.
    int n_tiles, n_changed, n_orphans, n_rays, k0;
    // What phase G needs of the proposal, taken by tid 0 in phase F before its barrier (the counters are
    // final by then: n_tiles after B, the others after D) and read after it; written again only in the next
    // iteration's phase F, after the iteration-end barrier -- so nothing writes it while a wave may read it,
    // and the counters above can be cleared at the iteration's end whatever the waves' skew.  accept: the
    // decision (phase F), or a server's next command (phase G, wave 0, then a block barrier).
    struct GSnap {
        int nc, nr, nt, k0, accept;
    } gs;
    int ob_lo[3], ob_hi[3], ob_ncand, ob_nfb;  // phase D's orphan-batch search (LDS layout)
    int n_super[2];  // rays in HBM: super-tiles hit, by iteration parity (the next iteration refreshes their maxima)
    int pts_seen, ray_pts;
    int e_done;  // LDS layout: waves done with their phase-E rays (waves 1..; wave 0 waits for them)
    int b_done;  // LDS layout: waves done with their phase-B tile pass (phase B without its barrier)    // bucket-grid update of an accepted proposal (applied by the last wave in phase G)
    int g_op, g_slot;           // bit 1: remove at old site, bit 2: insert at new site, bit 4: new value in place
    // what the update needs from the grid, read during phase F (G only writes)
    int gp_bo, gp_co, gp_pos, gp_bn, gp_cn;
    CellEntry gp_last;
    int gp_last_slot;
    double g_nzeta;
    double g_ox, g_oy, g_oz, g_nx, g_ny, g_nz;
    // chain scalars, resident for the whole launch
    long long iter, evaluations, bytes;
    long long proposed[5], accepted[5];
    double phi;
    int ncells, nslots, nfree;
    long long next_stamp;  // the next birth's stamp (tid 0)
    double lnN[3];     // logN[ncells - 1 .. ncells + 1]
    double lnN_far[2];  // logN[ncells - 2], logN[ncells + 2]: read during phase F for a birth/death commit
    double q_zeta;         // result of the birth/death Interpolation query
    int grid_fallbacks32;  // grid searches that needed the full scan
    int grid_ovf;          // LDS copy of *d.grid_overflow
    // scripted / server steps: the current step, a server command's steps
    ScriptStep step_cur;
    ScriptStep srv_step[kMaxScript];
    int srv_n, srv_k, srv_quit;
    // resident tempering rounds: the temperature of the current round (for reject_bound) and its last seq
    double rT, rinv2t;
    long long rseq;
    int rK, rskip;
    long long srv_seq, srv_busy_c, srv_busy_w;
    long long mbox[40];  // server mode: the last command read from the mailbox
    OrphanRec orph[kOrphanLds];
    ChgRec chg[kChgLds];
    tdchain::AlphaParts ap;  // the decision's phi-free part (phase C, last wave), for phase F
    DeltaSegs dseg;  // rays in HBM: phase F's new chi^2 partial sums as segments over the old ones
    long long prof[kProfSlots], t_last, t_iter;  // diagnostic phase stamps
    // rays in HBM: the committed terms' sum kept in any order, |tsum - (the exact real sum)| <=
    // terr; a proposal adds dsum = its terms' changes (any order), dabs = their magnitudes (phase E)
    double tsum, terr, dsum, dabs, b_T, b_E;
    double wpart[kChainThreads / 64];  // each wave's part of a block-wide any-order sum of the terms
    // a death, rays in LDS, free-running: phase G's deleteat! shift (shift_range) by waves 1.. -- each
    // wave's last source read in phase F (shift_edge), the waves done counted in shift_done, which wave 0
    // waits for before it reads the order for the next proposal
    int shift_done;
    int shift_edge[kChainThreads / 64];
    int dbg_site[kChainThreads / 64];  // the skew build's trail: each wave's last skew site (SKEW)
    // LDS layout, free-running: a short-road death's killed-site query is answered (q_zeta): raised by the
    // query wave, waited for by wave 0 before it decides, cleared with e_done and b_done.  (Last, in what was
    // padding: every other offset, and the block's size in 16-byte units, stay what they were.)
    int q_done;
};

// LDS carve-up (host and device agree on it through this function).
struct LdsPlan {
    size_t scratch, draws, smask, cmask, slo, shi, smax, shit, hrec, rhitl, tlo, thi, tmaxd, tstart, thit, ctm, tray, rayoff, ptS, prefix, cptS, cprefix, term, cterm,
        tS, sig, rflag, rhit, ord, total;
    bool super_lds;  // rays in HBM: super-tile boxes, maxima and hit lists in LDS
    bool lists_lds;  // rays in HBM: the first kListLds hit tiles (as records) and changed rays in LDS
};

constexpr size_t kLdsBudget = 160 * 1024;
constexpr size_t kDrawsBudget = (size_t)256 << 20;  // precomputed draws of one launch, at most (chain_run)

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// small: the tiles in LDS (and, rays_lds, the per-ray arrays and the order too -- else those stay in
// HBM, and the first kCtmLds hit tiles' candidate maxima are in LDS: the 4-wave two-chains-per-CU
// kernel's "tiles" layout)
__host__ __device__ inline LdsPlan lds_plan(int ntiles, int n, int cap, bool small, int waves = kWaves,
                                            bool rays_lds = true) {
    LdsPlan L{};
    size_t o = align16(sizeof(Shared));
    L.scratch = o; o += align16(sizeof(double) * waves * (small ? 96 : 192));  // (HBM layout: two rays a wave)
    L.draws = o; o += align16(sizeof(tdchain::Draws) * 64);                     // 64 iterations ahead
    if (!small || kSmallWalk) {  // the chi^2 walk's event words (exact_sum.h): static ones, kept; changed rays
        L.smask = o; o += align16(sizeof(unsigned long long) * delta_words(n));
        L.cmask = o; o += align16(sizeof(unsigned long long) * delta_words(n));
    }
    if (small) {
        L.tlo = o; o += align16(sizeof(float) * 3 * ntiles);
        L.thi = o; o += align16(sizeof(float) * 3 * ntiles);
        L.tmaxd = o; o += align16(sizeof(double) * ntiles);
        L.tstart = o; o += align16(sizeof(int) * (ntiles + 1));
        L.thit = o; o += align16(sizeof(int) * (ntiles + 1));
        L.ctm = o; o += align16(sizeof(double) * (rays_lds ? ntiles + 1 : kCtmLds));
        L.tray = o; o += align16(sizeof(int) * ntiles);
        if (rays_lds) {
            L.rayoff = o; o += align16(sizeof(int) * (n + 1));
            L.ptS = o; o += align16(sizeof(double) * n);
            L.prefix = o; o += align16(sizeof(double) * n);
            L.cptS = o; o += align16(sizeof(double) * n);
            L.cprefix = o; o += align16(sizeof(double) * n);
            L.term = o; o += align16(sizeof(double) * n);
            L.cterm = o; o += align16(sizeof(double) * n);
            L.tS = o; o += align16(sizeof(double) * n);
            L.sig = o; o += align16(sizeof(double) * n);
            L.rflag = o; o += align16(sizeof(int) * n);
            L.rhit = o; o += align16(sizeof(int) * n);
            L.ord = o; o += align16(sizeof(int) * cap);
        }
    } else {
        // the first hit tiles as {tile, start << 5 | count, ray} records, the first changed rays
        size_t q = o;
        L.hrec = q; q += align16(sizeof(int4) * kListLds);
        L.rhitl = q; q += align16(sizeof(int) * kListLds);
        L.lists_lds = q <= kLdsBudget;
        if (L.lists_lds) o = q;
        // super-tiles (16 tiles each): boxes, maxima (FP32, rounded up), two hit lists
        const int ns = (ntiles + kTilePts - 1) / kTilePts;
        q = o;
        L.slo = q; q += align16(sizeof(float) * 3 * ns);
        L.shi = q; q += align16(sizeof(float) * 3 * ns);
        L.smax = q; q += align16(sizeof(float) * ns);
        L.shit = q; q += align16(sizeof(int) * 2 * kListLds);
        L.super_lds = q <= kLdsBudget;
        if (L.super_lds) o = q;
    }
    L.total = o;
    return L;
}

// What the choice of k_chain_run instance (chain_variant.h) needs of a launch's chains: one LDS size
// for the whole grid, the largest plan of any chain, and what their lds_modes ask for.  The caller adds
// how the launch is driven (scripted, rx, rb) and num_cus.
inline ChainLaunchFacts launch_facts(const DevChain *host, int nchains) {
    ChainLaunchFacts f{};
    f.packed = f.tiles_ok = f.all_auto = true;
    for (int b = 0; b < nchains; ++b) {
        const DevChain &d = host[b];
        f.small = std::max(f.small, lds_plan(d.ntiles, d.n, d.cap, true).total);
        f.big = std::max(f.big, lds_plan(d.ntiles, d.n, d.cap, false).total);
        f.half = std::max(f.half, lds_plan(d.ntiles, d.n, d.cap, false, kWaves / 2).total);
        f.hyb = std::max(f.hyb, lds_plan(d.ntiles, d.n, d.cap, true, kWaves / 2, false).total);
        f.force_hbm = f.force_hbm || d.lds_mode >= 1;
        f.packed = f.packed && d.lds_mode >= 2;
        f.tiles_ok = f.tiles_ok && d.lds_mode == 2;
        f.all_auto = f.all_auto && d.lds_mode == 0;
        f.rec = f.rec || d.rec.every > 0;
    }
    f.nchains = nchains;
    f.budget = kLdsBudget;
    return f;
}

// Views of the arrays a launch works on: LDS copies in SMALL mode, else HBM.
struct Views {
    const float *tlo, *thi;
    double *tmaxd, *ptS, *prefix, *cptS, *cprefix, *term, *cterm;
    const double *tS, *sig;
    const int *tstart, *ray_off, *tray;
    int *thit, *rflag, *rhit, *ord;
    // rays in HBM: the first kListLds changed rays in LDS (rhit), the rest in rhit_g;
    // the first kListLds hit tiles also as LDS records
    int *rhit_g;
    int rhit_cap;
    int4 *hrec;
    int hrec_cap;
    // hit tile i's maximum if the proposal is accepted: the first ctm_cap in LDS (ctm), the rest in ctm_g
    double *ctm, *ctm_g;
    int ctm_cap;
    __device__ __forceinline__ double ctm_at(int i) const { return i < ctm_cap ? ctm[i] : ctm_g[i]; }
    __device__ __forceinline__ void ctm_put(int i, double x) const {
        if (i < ctm_cap) ctm[i] = x;
        else ctm_g[i] = x;
    }
    __device__ __forceinline__ int ray_at(int i) const { return i < rhit_cap ? rhit[i] : rhit_g[i]; }
    __device__ __forceinline__ void ray_put(int i, int r) const {
        if (i < rhit_cap) rhit[i] = r;
        else rhit_g[i] = r;
    }
    // hit tile i: {tile, start << 5 | count, ray}
    __device__ __forceinline__ int4 tile_rec(int i) const {
        if (i < hrec_cap) return hrec[i];
        const int t = thit[i] & 0x7fffffff;  // LDS layout: the high bit marks a tile preloaded in phase B
        return int4{t, tstart[t], tray[t], 0};
    }
};

// Result of one nearest-cell query, the same in every lane of the wave.
struct Nearest {
    double d, z;  // squared distance (1e9 sentinel if none) and the cell's value (0.0 if none)
    int s;        // slot (-1 if none)
    bool proven;
};

// One array of a fused block copy: U elements per thread per round, loaded
// into registers by load(), written by store().  Several Segs loaded before
// any is stored keep all their loads in flight at once: the launch preamble
// is a handful of memory round trips whatever the number of arrays.  S = the
// block's thread count (the caller's loop steps by U * S).
template <class T, int U, int S = kChainThreads>
struct CopySeg {
    T *dst;
    const T *src;
    int n;
    T v[U];
    __device__ __forceinline__ void load(int b) {
        if (n <= 0) return;
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = src[min(b + u * S, n - 1)];
    }
    __device__ __forceinline__ void store(int b) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (b + u * S < n) dst[b + u * S] = v[u];
    }
};

}  // namespace

}  // namespace tdstar
