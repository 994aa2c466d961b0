// chain_kernels.hip -- the device-resident rj-MCMC chain (TD_ENGINE_DEVICE).
//
// One persistent workgroup per chain -- 512 threads, or 256 where two chains share a CU -- runs `iters`
// iterations of
// TD_inversion_function.jl:70-274 without returning to the host: draw the
// proposal (chain_logic.h, shared with the host engine), evaluate it
// incrementally against the cached per-point nearest cells (chain_dev.h),
// recompute t* only for the rays whose points changed (Julia sum order,
// ray_sum.h) and chi^2 only from the first changed ray on (the cached prefix
// sums ARE the reference's sequential partial sums), then accept or reject.
// Every phi it produces is bit-identical to a full evaluate of the proposed
// model (tests/test_gpu_chain.py checks it against the host engine).
//
// Why one workgroup: a proposal touches ~P/N points and a few rays, i.e.
// microseconds of latency-bound work; a grid-wide barrier costs 4-10 us on
// MI355X (MI355X_MICROARCH.md, barrier-xcd) and a kernel boundary ~1.5 us.
// One CU keeps the loop free of both.  What bounds an iteration is then the
// chain of dependent memory round trips and barriers, so:
//   * tile boxes (FP32, outward-rounded), tile maxima, every per-ray array and
//     the position->slot map live in LDS when they fit (SMALL: the 381-ray
//     configs) and are written back to HBM when the launch ends;
//   * the RNG draws of 64 iterations are computed ahead, one lane each;
//   * nearest-cell queries go through the bucket grid, one wave per query,
//     one round of loads, and overlap the tile pass;
//   * candidate flags are cleared, and the bucket grid updated, at the start of
//     the NEXT iteration, off the critical path;
//   * the sequential chi^2 tail runs on one lane from LDS, 8 terms per trip.
//
// This unit: the proposal helpers, the rare exact sums, the recorded sample, k_chain_run with its 12
// instances, the one-point query (k_chain_query), the pre-drawn draws (k_draws) and the host launchers
// chain_run and chain_query.  What the kernel is built
// from sits in headers by concern: chain_shared.h (the Shared block, the LDS plan, Views),
// chain_search.h (nearest cell through the bucket grid), chain_tiles.h (the tile filters),
// chain_resident.h (the mailbox server and the tempering-round protocols), chain_diag.h (STAMP, SKEW,
// SPIN_WAIT, BPROBE); chain_variant.h chooses the instance.  The full-state kernels are in
// chain_state.hip, the testing kernels in chain_test_kernels.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstddef>
#include <cstdlib>

#include "chain_dev.h"
#include "chain_diag.h"
#include "chain_resident.h"
#include "chain_search.h"
#include "chain_shared.h"
#include "chain_tiles.h"
#include "chain_variant.h"
#include "exact_sum.h"
#include "internal.h"
#include "ray_sum.h"
#include "wave_ops.h"

namespace tdstar {

namespace {

struct OverlayZeta {
    const unsigned char *flag;
    const double *cand, *cur;
    __device__ __forceinline__ double operator()(int k) const {
        const double a = cand[k], b = cur[k];  // both loads issued at once, then select
        return flag[k] ? a : b;
    }
};

// TD_inversion_function.jl:72-80,127-128,184-188,221-232: the proposal of one
// iteration from its draws and the model.  slot_at(pos) = slot at Julia
// position pos.
// In two halves: the draws' proposal and the loads of what it needs from the
// model (the selected cell, or the slot a birth takes), then the rest -- so the
// loads of a guessed next proposal can fly while other work runs.
struct ProposalLoads {
    Proposal q;
    int s, new_slot;
    int own;  // DevChain::own of the selected cell; -1: not asked (no guess), or a birth
    double x, y, z, ze;
};
template <bool OWN = false, class SlotAt>
__device__ __forceinline__ ProposalLoads proposal_begin(const tdchain::Params &P, const tdchain::Draws &dr,
                                                        int ncells, int nfree, int nslots, const int *free_slots,
                                                        const double *cx, const double *cy, const double *cz,
                                                        const double *czeta, SlotAt slot_at,
                                                        const int *own = nullptr) {
    ProposalLoads l;
    l.q = tdchain::propose(P, dr, ncells);
    l.s = -1;
    l.new_slot = -1;
    l.own = -1;
    l.x = l.y = l.z = l.ze = 0.0;
    if (l.q.active && l.q.action != tdchain::kBirth) {  // (global loads: no LDS wait or barrier waits for them)
        l.s = slot_at((int)l.q.index);
        l.x = gload(cx + l.s);
        l.y = gload(cy + l.s);
        l.z = gload(cz + l.s);
        l.ze = gload(czeta + l.s);
        // The cell's point count, in the same round trip.  Other waves of the workgroup keep it with atomics
        // performed in L2 (phase G), so the read is an agent-scope atomic load: a plain load could be served
        // from a line this CU's L1 has held since before them.
        if constexpr (OWN)
            l.own = __hip_atomic_load((const __attribute__((address_space(1))) int *)(own + l.s), __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
    }
    if (l.q.active && l.q.action == tdchain::kBirth) l.new_slot = nfree > 0 ? gload(free_slots + nfree - 1) : nslots;
    return l;
}
__device__ __forceinline__ void proposal_end(PState &o, const tdchain::Params &P, const tdchain::Draws &dr,
                                             ProposalLoads l) {
    Proposal q = l.q;
    o.slot_k = -1;
    o.new_slot = l.new_slot;
    o.barren = l.own == 0 ? 1 : 0;  // (trusted only once the guess is adopted: k_chain_run, the iteration's end)
    if (q.active && q.action != tdchain::kBirth) {
        o.slot_k = l.s;
        o.kx = l.x;
        o.ky = l.y;
        o.kz = l.z;
        o.zeta_killed = l.ze;
        tdchain::complete_proposal(P, dr, q, l.x, l.y, l.z, l.ze);
    }
    o.p = q;
    // forward evaluation needed (birth validity is only known after its query)
    o.eval = q.active && (q.valid || q.action == tdchain::kBirth) && P.debug_prior != 1;
}
template <bool OWN = false, class SlotAt>
__device__ __forceinline__ void make_proposal(PState &o, const tdchain::Params &P, const tdchain::Draws &dr,
                                              int ncells, int nfree, int nslots, const int *free_slots,
                                              const double *cx, const double *cy, const double *cz,
                                              const double *czeta, SlotAt slot_at, const int *own = nullptr) {
    proposal_end(o, P, dr, proposal_begin<OWN>(P, dr, ncells, nfree, nslots, free_slots, cx, cy, cz, czeta, slot_at, own));
}

// A scripted step (td_evaluate's incremental path) as the proposal: always
// active and valid, no draws; birth's zeta is given (birth_zeta is not called).
template <class SlotAt>
__device__ __forceinline__ void script_proposal(PState &o, const ScriptStep &st, int nfree, int nslots,
                                               const int *free_slots, SlotAt slot_at) {
    Proposal q{};
    q.action = st.action;
    q.active = 1;
    q.valid = 1;
    q.index = st.index;
    q.x = st.x;
    q.y = st.y;
    q.z = st.z;
    q.zeta = st.zeta;
    o.slot_k = -1;
    o.new_slot = -1;
    o.barren = 0;
    if (q.action != tdchain::kBirth) {
        const int s = slot_at(st.index);
        o.slot_k = s;
        o.kx = st.old[0];  // the cell's values came with the step (a round trip to the cell arrays saved)
        o.ky = st.old[1];
        o.kz = st.old[2];
        o.zeta_killed = st.old[3];
        if (q.action == tdchain::kChange) {  // the site stays; only zeta is new
            q.x = o.kx;
            q.y = o.ky;
            q.z = o.kz;
        } else if (q.action == tdchain::kMove) {
            q.zeta = o.zeta_killed;
        }
    } else {
        o.new_slot = nfree > 0 ? free_slots[nfree - 1] : nslots;
    }
    o.p = q;
    o.eval = 1;
}

// deleteat! at Julia position `index` (rays in LDS, free-running): positions index+1 .. ncells-1 move down
// one, wave w (1 .. nw) taking the source positions [a, b).  Each wave reads its sources and writes
// them one lower in passes of 64 (a pass reads before it writes); the one source another wave writes
// over -- position b-1, the next wave's first target -- was read in phase F (Shared::shift_edge).
__device__ __forceinline__ void shift_range(int index, int ncells, int w, int nw, int &a, int &b) {
    const int first = index + 1, C = (ncells - first + nw - 1) / nw;
    a = first + (w - 1) * C;
    b = min(a + C, ncells);
}

// The decisions on bounds (phase F): 2u, u = 2^-53 the unit roundoff -- every rounding bound below is
// taken twice over
constexpr double kSumSlack = 2.3e-16;

// LDS layout, one wave (the rare paths of the decisions on bounds, phase F):
// prefix[ex_upto..n) exact again -- the committed terms added in k order
// (MCsub.jl:170-172, exact_sum.h) -- and the committed phi returned; then, if
// k0 < n, the proposal's partial sums from k0 into cprefix, its phi_n in
// *phi_n.  `overlay`: a proposal's terms are in place (its rays flagged, their
// committed terms in cterm), staged through cprefix.  Out of line: it is
// rare, and the kernel is at its register limit.
// (The arrays by value: a Views passed by reference would be spilled to scratch in the caller; phi_n
// comes back in the result for the same reason -- an out-pointer would keep the caller's phi_n in scratch.)
struct ExactPhis {
    double phi, phi_n;
};
__device__ __attribute__((noinline)) ExactPhis exact_sums(const double *term, double *prefix, double *cprefix,
                                                          const double *cterm, const int *rflag, Shared &sh, int n,
                                                          int lane, bool overlay, int k0, double phi, double phi_n) {
    const int ex_upto = sh.ex_upto;
    if (ex_upto < n) {
        const double C0 = ex_upto > 0 ? prefix[ex_upto - 1] : 0.0;
        const double *t = term + ex_upto;
        if (overlay) {
            for (int k = ex_upto + lane; k < n; k += 64) cprefix[k] = rflag[k] ? cterm[k] : term[k];
            wave_sync_lds();
            t = cprefix + ex_upto;
        }
        bool stopped = false;
        phi = wave_seq_sum(t, n - ex_upto, C0, prefix + ex_upto, lane, nullptr, &stopped);
        wave_sync_lds();
        if (lane == 0) {
            sh.ex_upto = n;
            sh.phi_lo = sh.phi_hi = phi;
        }
        wave_sync_lds();
    }
    if (k0 < n) {
        bool stopped = false;
        phi_n = wave_seq_sum(term + k0, n - k0, k0 > 0 ? prefix[k0 - 1] : 0.0, cprefix + k0, lane, nullptr, &stopped);
    }
    return ExactPhis{phi, phi_n};
}

// One sample of a recorded launch (RecDesc, chain_dev.h), by the whole block right after the
// iteration-end barrier: the model of the iteration just finished is complete there -- the cells by
// slot in HBM (tid 0, phase G), ptS committed (all threads, phase G), the Julia order shifted or
// appended (phase G; the LDS layout's shifting waves are past the barrier too), and sh.phi exact (wave
// 0 made it so before the barrier).  The cells are gathered through the order into the history's packed
// arrays by the whole block, U = 4 cells (16 loads) in flight per thread: 5000 cells are three rounds
// of 512 threads, where one wave alone would need twenty.  (The unroll hardly matters: the copy takes
// 15.6-17k cycles at 5000 cells with U = 1, 2 or 4, and 21k with 8 -- 40000 8-byte accesses through
// one CU's memory pipeline, not a latency chain)  Then ptS; tid 0 writes the header and the
// next sample's offset.  The caller's barrier follows before phase G of a later iteration can change
// what is read here.  Out of line, the arrays by value (as exact_sums): the
// kernel is at its register limit.
__device__ __attribute__((noinline)) void record_sample(const DevChain &d, const int *ord, const double *ptS,
                                                        const Shared &sh, long long it, long long iter0, int action,
                                                        int accept, int tid, int nth) {
    const RecDesc &rc = d.rec;
    const int nc = sh.ncells, n = d.n;
    const long long k = rc.base + (it + 1 - rc.first) / rc.every, iter = iter0 + it;  // (one division per sample)
    // (written by tid 0 at the previous sample, before a block barrier: a plain vector load)
    const long long o = __hip_atomic_load(rc.off + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    double *ox = rc.cells + o, *oy = ox + rc.stride, *oz = oy + rc.stride, *oze = oz + rc.stride;
    const double *cx = d.cx, *cy = d.cy, *cz = d.cz, *cze = d.czeta;
    constexpr int U = 4;
    for (int j0 = tid; j0 < nc; j0 += U * nth) {
        int s[U];
        double x[U], y[U], z[U], ze[U];
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] = ord[min(j0 + u * nth, nc - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            x[u] = gload(cx + s[u]);
            y[u] = gload(cy + s[u]);
            z[u] = gload(cz + s[u]);
            ze[u] = gload(cze + s[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * nth;
            if (j < nc) {
                gstore(ox + j, x[u]);
                gstore(oy + j, y[u]);
                gstore(oz + j, z[u]);
                gstore(oze + j, ze[u]);
            }
        }
    }
    if (rc.ptS) {
        double *op = rc.ptS + k * n;
        for (int r = tid; r < n; r += nth) gstore(op + r, ptS[r]);
    }
    if (tid == 0) {
        rc.iter[k] = iter;
        rc.phi[k] = sh.phi;
        rc.ncells[k] = nc;
        rc.action[k] = action;
        rc.accept[k] = accept;
        rc.off[k + 1] = o + nc;
    }
}

// One sample of a recorded ladder (RecDesc, chain_dev.h; the ROUNDS && REC instances), by the whole block
// after the barrier that ends a round's last iteration: record_sample's copy into slot i of the call --
// cells + i * slot, a place that is a function of the round alone, since the previous sample was another
// workgroup's, whose stores this one has no way to see -- and the header at base + i.  No offset is read
// or written (history_pack.hip).  A function of its own: record_sample and its callers stay as they are.
__device__ __attribute__((noinline)) void record_round_sample(const DevChain &d, const int *ord, const double *ptS,
                                                              const Shared &sh, long long i, long long iter,
                                                              int action, int accept, int tid, int nth) {
    const RecDesc &rc = d.rec;
    const int nc = sh.ncells, n = d.n;
    const long long k = rc.base + i;
    double *ox = rc.cells + i * rec_slot(rc), *oy = ox + rc.stride, *oz = oy + rc.stride, *oze = oz + rc.stride;
    const double *cx = d.cx, *cy = d.cy, *cz = d.cz, *cze = d.czeta;
    constexpr int U = 4;
    for (int j0 = tid; j0 < nc; j0 += U * nth) {
        int s[U];
        double x[U], y[U], z[U], ze[U];
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] = ord[min(j0 + u * nth, nc - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            x[u] = gload(cx + s[u]);
            y[u] = gload(cy + s[u]);
            z[u] = gload(cz + s[u]);
            ze[u] = gload(cze + s[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * nth;
            if (j < nc) {
                gstore(ox + j, x[u]);
                gstore(oy + j, y[u]);
                gstore(oz + j, z[u]);
                gstore(oze + j, ze[u]);
            }
        }
    }
    if (rc.ptS) {
        double *op = rc.ptS + k * n;
        for (int r = tid; r < n; r += nth) gstore(op + r, ptS[r]);
    }
    if (tid == 0) {
        rc.iter[k] = iter;
        rc.phi[k] = sh.phi;
        rc.ncells[k] = nc;
        rc.action[k] = action;
        rc.accept[k] = accept;
    }
}

// ---------------------------------------------------------------- k_chain_run ----
// The body below is one function on purpose, and is changed only with a comparison of the generated
// assembly of all 14 instances and a same-machine A/B: every instance sits at 256 VGPRs with 976-1280 B
// per lane of scratch, and its register allocation moves with any restructuring -- wrapping only the
// mirror preamble in an always-inlined lambda changed the allocation of every LDS-layout instance
// (scratch +16 B/lane in two, spill counts up in three and down in two).  So no phase is extracted and
// no local renamed; code that can live outside it does (the headers above).
// SCRIPT: host-given proposals (td_evaluate's incremental path: scripted
// steps, the resident server); a free-running chain's instance has none of
// that code on its path.
// SMALL: the tiles mirrored in LDS (else in HBM, with super-tiles); RLDS: the per-ray arrays and the
// Julia order mirrored too (the 381-ray configs, 8 waves); NTH: 512 threads, or 256 (two chains per CU)
// REC: a recorded launch (RecDesc): the instances without it carry none of its code.  With ROUNDS: a
// ladder's recording (either round protocol: sa.rb or sa.rx), the sample of a round taken by the workgroup
// that ran it at ladder level 0 (record_round_sample); without: a free-running chain's (record_sample)
template <bool SMALL, bool SCRIPT, int NTH, bool RLDS = SMALL, bool ROUNDS = false, bool REC = false>
__global__ __launch_bounds__(NTH, 2) void k_chain_run(const DevChain *__restrict__ dptr, long long iters,
                                                             ScriptArgs sa) {
    constexpr bool WALK = !SMALL || kSmallWalk;  // chi^2 by the event walk
    constexpr bool kNoBarB = RLDS && !SCRIPT;     // phase B may end without a block barrier (below)
    constexpr int kWv = NTH / 64;  // waves: 8 (one chain per CU), or 4 (rays in HBM: two chains per CU)
    static_assert(!RLDS || SMALL, "rays in LDS only with the tiles in LDS");
    static_assert(!REC || !SCRIPT, "recording: drawn proposals (free-running chains, tempering rounds)");
    static_assert(NTH == kChainThreads || (!RLDS && !SCRIPT && NTH == kChainThreads / 2),
                  "512 threads, or 256 with the rays in HBM");
    if (sa.pin >= 0) {  // one chain, launched as 8 workgroups: only the one on XCD `pin` runs it
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        if ((int)(xcc & 15u) != sa.pin) return;
    }
    const DevChain &d = dptr[sa.pin >= 0 ? 0 : blockIdx.x];  // fields read from memory as needed
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Shared &sh = *reinterpret_cast<Shared *>(lds);
    const LdsPlan L = lds_plan(d.ntiles, d.n, d.cap, SMALL, kWv, RLDS);
    double(*ray_scratch)[96] = reinterpret_cast<double(*)[96]>(lds + L.scratch);
    tdchain::Draws *draws = reinterpret_cast<tdchain::Draws *>(lds + L.draws);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const tdchain::Params &P = d.params;
    const int n = d.n, NT = d.ntiles;
    const bool prof_on = d.profile != 0;
    const long long t_start = prof_on ? clock64() : 0;  // diagnostic: launch preamble / epilogue (prof[76..79])
    Mailbox *const mb = SCRIPT ? sa.mb : nullptr;  // server mode: resident, steps from the mailbox (iters ignored)
    RoundBox *const rbx = SCRIPT ? nullptr : sa.rb;  // resident tempering rounds (iters ignored)
    // exchange rounds, swaps decided here (ROUNDS instances only: the others carry none of their registers)
    const RoundX *const rxp = (SCRIPT || !ROUNDS) ? nullptr : sa.rx;
    const bool xch = rxp != nullptr;
    const int bchain = sa.pin >= 0 ? 0 : (int)blockIdx.x;
    const int nscript = SCRIPT ? (mb ? 1 : sa.n) : 0;  // > 0: host-given proposals (td_evaluate), iters == nscript

    // ---- views: LDS copies of the tile / ray / order arrays when they fit ----
    Views v;
    v.tlo = d.tile_lo; v.thi = d.tile_hi; v.tmaxd = d.tile_maxd; v.tstart = d.tile_start; v.thit = d.tiles_hit;
    v.ray_off = d.ray_off; v.ptS = d.ptS; v.prefix = d.prefix; v.cptS = d.cand_ptS; v.cprefix = d.cand_prefix;
    v.tS = d.tS; v.sig = d.sig; v.rflag = d.ray_flag; v.rhit = d.rays_hit; v.ord = d.order; v.tray = d.tile_ray;
    v.rhit_g = d.rays_hit;
    v.rhit_cap = 0;
    v.hrec = nullptr;
    v.hrec_cap = 0;
    if (!SMALL && L.lists_lds) {
        v.rhit = reinterpret_cast<int *>(lds + L.rhitl);
        v.rhit_cap = kListLds;
        v.hrec = reinterpret_cast<int4 *>(lds + L.hrec);
        v.hrec_cap = kListLds;
    }
    v.term = d.term;
    v.cterm = d.cand_term;
    v.ctm = v.ctm_g = d.tile_cmax;
    v.ctm_cap = 0;
    if constexpr (SMALL && !RLDS) {  // the tiles only (the rays, the order, the candidate maxima in HBM)
        float *a = reinterpret_cast<float *>(lds + L.tlo), *b = reinterpret_cast<float *>(lds + L.thi);
        double *m = reinterpret_cast<double *>(lds + L.tmaxd);
        int *ts = reinterpret_cast<int *>(lds + L.tstart), *tr = reinterpret_cast<int *>(lds + L.tray);
        {
            constexpr int U = 4;
            CopySeg<float, U, NTH> c0{a, d.tile_lo, 3 * NT}, c1{b, d.tile_hi, 3 * NT};
            CopySeg<double, U, NTH> c2{m, d.tile_maxd, NT};
            CopySeg<int, U, NTH> c7{ts, d.tile_start, NT + 1}, c8{tr, d.tile_ray, NT};
            for (int b0 = tid; b0 < 3 * NT; b0 += U * NTH) {
                c0.load(b0); c1.load(b0); c2.load(b0); c7.load(b0); c8.load(b0);
                c0.store(b0); c1.store(b0); c2.store(b0); c7.store(b0); c8.store(b0);
            }
        }
        v.tlo = a; v.thi = b; v.tmaxd = m; v.tstart = ts; v.tray = tr;
        v.thit = reinterpret_cast<int *>(lds + L.thit);
        v.ctm = reinterpret_cast<double *>(lds + L.ctm);
        v.ctm_cap = kCtmLds;
        __syncthreads();
    }
    if constexpr (RLDS) {
        float *a = reinterpret_cast<float *>(lds + L.tlo), *b = reinterpret_cast<float *>(lds + L.thi);
        double *m = reinterpret_cast<double *>(lds + L.tmaxd);
        int *ts = reinterpret_cast<int *>(lds + L.tstart), *ro = reinterpret_cast<int *>(lds + L.rayoff);
        double *p = reinterpret_cast<double *>(lds + L.ptS), *pf = reinterpret_cast<double *>(lds + L.prefix);
        double *t = reinterpret_cast<double *>(lds + L.tS), *sg = reinterpret_cast<double *>(lds + L.sig);
        int *rf = reinterpret_cast<int *>(lds + L.rflag), *od = reinterpret_cast<int *>(lds + L.ord);
        int *tr = reinterpret_cast<int *>(lds + L.tray);
        v.tray = tr;
        {  // every mirror in one fused copy (positions >= ncells of the order are written before read)
            constexpr int U = 4;
            CopySeg<float, U, NTH> c0{a, d.tile_lo, 3 * NT}, c1{b, d.tile_hi, 3 * NT};
            CopySeg<double, U, NTH> c2{m, d.tile_maxd, NT}, c3{p, d.ptS, n}, c4{pf, d.prefix, n}, c5{t, d.tS, n},
                c6{sg, d.sig, n};
            CopySeg<int, U, NTH> c7{ts, d.tile_start, NT + 1}, c8{tr, d.tile_ray, NT}, c9{ro, d.ray_off, n + 1},
                c10{od, d.order, d.st->ncells};
            const int most = max(max(3 * NT, NT + 1), max(n + 1, c10.n));
            for (int b0 = tid; b0 < most; b0 += U * NTH) {
                c0.load(b0); c1.load(b0); c2.load(b0); c3.load(b0); c4.load(b0); c5.load(b0);
                c6.load(b0); c7.load(b0); c8.load(b0); c9.load(b0); c10.load(b0);
                c0.store(b0); c1.store(b0); c2.store(b0); c3.store(b0); c4.store(b0); c5.store(b0);
                c6.store(b0); c7.store(b0); c8.store(b0); c9.store(b0); c10.store(b0);
            }
        }
        for (int i = tid; i < n; i += NTH) rf[i] = 0;
        v.tlo = a; v.thi = b; v.tmaxd = m; v.tstart = ts; v.ray_off = ro; v.ptS = p; v.prefix = pf; v.tS = t;
        v.sig = sg; v.rflag = rf; v.ord = od;
        v.cptS = reinterpret_cast<double *>(lds + L.cptS);
        v.cprefix = reinterpret_cast<double *>(lds + L.cprefix);
        v.term = reinterpret_cast<double *>(lds + L.term);
        v.cterm = reinterpret_cast<double *>(lds + L.cterm);
        v.thit = reinterpret_cast<int *>(lds + L.thit);
        v.ctm = reinterpret_cast<double *>(lds + L.ctm);
        v.ctm_cap = NT + 1;
        v.rhit = reinterpret_cast<int *>(lds + L.rhit);
        v.rhit_cap = n;
        __syncthreads();  // ptS, tS, sig mirrored
    }
    const long long t_mirror = prof_on ? clock64() : 0;
    // chi^2 term of every ray in the current state (MCsub.jl:171), cached: a
    // proposal recomputes only the terms of the rays it changes
    {
        double part = 0.0;  // (rays in HBM: their sum in any order, the running total of phase F)
        for (int r = tid; r < n; r += NTH) {
            const double df = v.ptS[r] - v.tS[r];
            const double sg = v.sig[r];
            const double t = ((df * df) * 1.0) / (sg * sg);
            v.term[r] = t;
            part = part + t;
        }
        if constexpr (!RLDS) {
            part = wave_sum_f64(part);
            if (lane == 0) sh.wpart[wv] = part;
        }
    }
    if (tid == 0) {
        const ChainScalars &s0 = *d.st;
        sh.iter = s0.iter;
        sh.evaluations = 0;
        sh.bytes = 0;
        sh.cur = 0;
        sh.defer = 0;
        if (!RLDS) sh.dsum = sh.dabs = 0.0;
        sh.grid_fallbacks32 = 0;
        sh.e_done = sh.b_done = 0;
        if constexpr (kNoBarB) sh.q_done = 0;
        geo_fill(sh.geo, d);
        for (int a = 0; a < 5; ++a) sh.proposed[a] = sh.accepted[a] = 0;
        sh.phi = s0.phi;
        sh.ncells = s0.ncells;
        for (int k = 0; k < 3; ++k) sh.lnN[k] = d.logN[max(s0.ncells - 1 + k, 0)];
        sh.nslots = s0.nslots;
        sh.nfree = s0.nfree;
        sh.next_stamp = s0.next_stamp;
        sh.g_op = 0;
        sh.grid_ovf = *d.grid_overflow;
        sh.rT = P.temperature;
        sh.rinv2t = P.inv_2t;
        sh.srv_quit = 0;
        sh.rK = 0;
        for (int k = 0; k < kProfSlots; ++k) sh.prof[k] = 0;
        sh.t_last = clock64();
        sh.dseg.nseg = 0;
    }
    __syncthreads();
    const long long t_init = prof_on ? clock64() : 0;
    unsigned long long *smask = reinterpret_cast<unsigned long long *>(lds + L.smask);
    unsigned long long *cmask = reinterpret_cast<unsigned long long *>(lds + L.cmask);
    const int NS = d.nsuper;
    float *slo = reinterpret_cast<float *>(lds + L.slo), *shi = reinterpret_cast<float *>(lds + L.shi);
    float *smax = reinterpret_cast<float *>(lds + L.smax);  // >= the max of its tiles' maxima
    int *shit = reinterpret_cast<int *>(lds + L.shit);
    const bool super_on = !SMALL && L.super_lds;
    if constexpr (WALK) {  // the chi^2 walk's static event words of the current state
        if constexpr (SMALL) __syncthreads();  // the terms above
        delta_marks(v.term, v.prefix, nullptr, n, smask, wv, delta_words(n), kWv, lane);
        for (int w = tid; w < delta_words(n); w += NTH) cmask[w] = 0ull;
    }
    if constexpr (!SMALL) {
        if (super_on) {  // super-tile boxes, and maxima = the max of their tiles' maxima
            for (int i = tid; i < 3 * NS; i += NTH) {
                slo[i] = d.super_lo[i];
                shi[i] = d.super_hi[i];
            }
            for (int S = tid; S < NS; S += NTH) {
                double m = 0.0;
                for (int t = S * kTilePts; t < min(NT, (S + 1) * kTilePts); ++t) m = fmax(m, d.tile_maxd[t]);
                smax[S] = f32_up(m);
            }
            if (tid == 0) sh.n_super[0] = sh.n_super[1] = 0;
        }
        __syncthreads();
    }

    // the draws (and their normal quantiles) of 64 iterations, one lane each:
    // a function of (seed, chain, iteration) only; and the first proposal
    if (wv == 0) {
        if (sa.pre) {  // precomputed (k_draws): one round of loads
            if (lane < iters) draws[lane] = sa.pre[(long long)bchain * sa.pre_stride + lane];
        } else if (!nscript) {
            draws[lane] = tdchain::draw_iteration(d.seed, d.chain, (uint64_t)(sh.iter + lane));
        }
        wave_sync_lds();
        if (mb) {  // the first command (no proposal pending yet)
            if (lane == 0) {
                sh.srv_seq = mb_load(&mb->done);
                sh.srv_quit = 0;
                sh.srv_busy_c = 0;
            }
            wave_sync_lds();
            server_wait(mb, d, v, sh, lane);
        }
        if (rbx) {  // the first round (the last one done is in the slot)
            if (lane == 0) sh.rseq = mb_load(&rbx->slot[bchain].done);
            wave_sync_lds();
            round_wait(rbx, bchain, sh, lane, false, sh.phi);  // (the stored phi is exact)
        }
        if (lane == 0 && iters > 0 && !((mb || rbx) && sh.srv_quit)) {
            if (nscript) {
                sh.step_cur = mb ? sh.srv_step[sh.srv_k++] : sa.step[0];
                script_proposal(sh.ps[0], sh.step_cur, sh.nfree, sh.nslots, d.free_slots,
                                [&](int pos) { return v.ord[pos]; });
            }
            else
                make_proposal(sh.ps[0], P, draws[0], sh.ncells, sh.nfree, sh.nslots, d.free_slots, d.cx, d.cy, d.cz,
                              d.czeta, [&](int pos) { return v.ord[pos]; });
            if (sh.ps[0].p.active) sh.proposed[sh.ps[0].p.action] += 1;
            sh.n_tiles = sh.n_changed = sh.n_orphans = sh.n_rays = 0;
            sh.pts_seen = sh.ray_pts = 0;
            sh.k0 = n;
            sh.gs.accept = 0;
        }
        if (lane == 0) sh.spec_ok = 0;
    }
    __syncthreads();

    // wave 0 lane 0 decides, commits and proposes: the scalars only it changes
    // live in its registers (LDS copies are written, never read back on its path)
    const long long iter0 = sh.iter;
    if (prof_on && tid == 0) {
        const long long t_now = clock64();
        sh.prof[76] += t_now - t_start;  // preamble: mirrors, terms, draws, 1st proposal
#ifdef TD_B_PROBE
        if (false) {
#else
        if (SMALL) {  // its parts (slots of the rays-in-HBM walk diagnostics, unused in this layout)
#endif
            sh.prof[72] += t_mirror - t_start;
            sh.prof[73] += t_init - t_mirror;
            sh.prof[74] += t_now - t_init;
        }
    }
    double phi_r = sh.phi;
    // wave 0: the temperature of the round (tid 0 decides with it) and the round's last iteration
    double inv2t_r = sh.rinv2t;
    long long round_end = rbx ? sh.rK : xch ? (long long)rxp->K : LLONG_MAX;
    int cur_r = 0;
    bool pend_r = false;    // rays in HBM: an accepted proposal's chi^2 partial sums not yet written
    bool pend_sup = false;  // rays in HBM: its super-tiles' maxima not yet refreshed
    int last_action = 0, last_accept = 0;  // tid 0: Model.action / accept of the last iteration
    long long it_done = 0;                 // iterations run (server mode: until QUIT)
    // recording (RecDesc): the launch's next sampled iteration, 1-based (block-uniform; never, when off)
    long long rec_next = LLONG_MAX;
    if constexpr (REC && !ROUNDS)
        if (d.rec.every > 0 && !rbx) rec_next = d.rec.first;
    // a ladder's recording: wave 0 latches a round's sample index in sh.mbox[0] (-1: none) and the round's
    // last iteration, 1-based, in sh.mbox[1] (server words, idle in these instances) before the round's
    // barrier; the block reads them after it
    if constexpr (REC && ROUNDS)
        if (tid == 0) sh.mbox[0] = sh.mbox[1] = -1;
    // LDS layout, decisions on bounds (phase F): a proposal accepted on bounds of phi_n leaves its
    // chi^2 partial sums unformed -- prefix[] stays exact below ex_upto only (wave 0), and tid 0
    // keeps phi_r as an estimate inside [phi_lo, phi_hi].  They are made exact again by the next
    // decision the bounds cannot take, at a tempering round's end and at the launch's end.
    if (tid == 0) {
        sh.ex_upto = n;
        sh.phi_lo = sh.phi_hi = phi_r;
        if constexpr (!RLDS) {
            double T = 0.0;
            for (int w = 0; w < kWv; ++w) T = T + sh.wpart[w];
            sh.tsum = T;
            sh.terr = kSumSlack * (double)(n + 1) * fabs(T);  // (any order: within (n - 1) ulps of the exact sum)
        }
    }
    __syncthreads();
    for (long long it = 0; it < iters && !((mb || rbx || xch) && sh.srv_quit); ++it) {
        if (prof_on && tid == 0) sh.t_iter = clock64();
        // rays in HBM: the previous accepted proposal's super-tile maxima (their first round of
        // loads issued here, so it overlaps the partial sums' commit below)
        int sup_n = 0, sup_S = 0, sup_par = 0;
        bool sup_all = false;
        unsigned long long sup_mk = 0ull;
        if constexpr (!SMALL) {
            if (pend_sup) {
                sup_par = (int)((it - 1) & 1);
                const int nsh = sh.n_super[sup_par];
                sup_all = nsh > kListLds;  // the list overflowed: every super-tile
                sup_n = sup_all ? NS : nsh;
                if ((tid >> 4) < sup_n) {
                    sup_S = sup_all ? (tid >> 4) : shit[sup_par * kListLds + (tid >> 4)];
                    const int t = sup_S * kTilePts + (tid & 15);
                    sup_mk = t < NT ? (unsigned long long)__double_as_longlong(d.tile_maxd[t]) : 0ull;
                }
            }
        }
        if constexpr (WALK) {
            // the previous accepted proposal's partial sums (read again only in phase F,
            // after at least one barrier): off its critical path, before this one's tiles
            if (pend_r) delta_commit<SMALL ? 1 : 16>(v.prefix, v.cprefix, n, sh.dseg, tid, NTH);
            pend_r = false;
        }
        if constexpr (!SMALL) {
            if (pend_sup) {  // its hit super-tiles: max of their tiles' new maxima (a tile row each)
                if ((tid >> 4) < sup_n) {  // whole rows: the DPP row max
                    const unsigned long long mk = row_max_u64(sup_mk);
                    if ((tid & 15) == 15) smax[sup_S] = f32_up(__longlong_as_double((long long)mk));
                }
                for (int i = (tid >> 4) + NTH / kTilePts; i < sup_n; i += NTH / kTilePts) {
                    const int S = sup_all ? i : shit[sup_par * kListLds + i], t = S * kTilePts + (tid & 15);
                    unsigned long long mk = t < NT ? (unsigned long long)__double_as_longlong(d.tile_maxd[t]) : 0ull;
                    mk = row_max_u64(mk);
                    if ((tid & 15) == 15) smax[S] = f32_up(__longlong_as_double((long long)mk));
                }
                __syncthreads();
                SKEW(1);
                pend_sup = false;
            }
        }
        bool acc_r = false;
        const PState &cur = sh.ps[sh.cur];
        const Proposal p = cur.p;
        const int action = p.action;
        const int ncells = sh.ncells;
        const int slot_k = cur.slot_k;
        const bool eval = cur.eval != 0;
        const double kx = cur.kx, ky = cur.ky, kz = cur.kz;
        const int new_slot = cur.new_slot;
        const double zeta_killed = cur.zeta_killed;
        double czeta = 0.0, zetanew_death = 0.0;
        STAMP(0);
        // LDS layout: the points of the first kPre hit tiles a wave finds are loaded in
        // phase B (their global round trip overlaps the B barrier and the birth/death
        // query) and judged in phase C
        bool pre_on = false;
        bool nobar = false;  // phase B without its block barrier (block-uniform; below)
        int pre_q = 0, pre_ray = 0, pre_s = 0;
        double pre_bd = 0.0, pre_x = 0.0, pre_y = 0.0, pre_z = 0.0;
        // The short road (block-uniform; free-running instances): a change or death whose cell owns no ray
        // point changes no point and no ray -- no tile pass, no b_done hand-off, no
        // phases C-E; every counter stays 0 and k0 == n, so phase F decides on phi_n = phi_r as it does for any
        // proposal that turned out empty, and phase G's loops are empty.  A death keeps its killed-site query
        // and (rays in HBM, 4 waves) phase B's barrier, after which the decision reads the answer; a change
        // goes straight to phase F, whose barrier is then the one between the loop top's reads and wave 0's
        // end-of-iteration writes -- and so does the LDS layout's death (qroad, below).
        // Whether the cell owns a point: PState::barren when the guess that read the count was adopted
        // untouched; else (a launch's first proposal, every 64th, one wave 0 made at the last iteration's end)
        // every wave reads DevChain::own here for itself -- one wave-uniform address, an agent-scope load
        // served by L2 as phase F's, no LDS word and no barrier.  The answer is the same in every wave: own's
        // only writers are phase G's commit atomics, each waited for by its wave before the iteration-end
        // barrier this wave has just passed, and the next ones come after this iteration's phase F barrier;
        // at a launch's start the count is the launch-boundary invariant (tdt_chain_own_check).
        bool sroad = false;
        int own_top = -1;  // the count read here (>= 0), or not asked
        if constexpr (!SCRIPT) {
            // (the action first, what the registers hold: a birth or a move waits for nothing here; debug_prior,
            // a load, last and beside the count's)
            if ((action == tdchain::kChange || action == tdchain::kDeath) && p.active && p.valid) {
                const bool up = cur.barren != 0;
                if (!up)
                    own_top = __builtin_amdgcn_readfirstlane(
                        __hip_atomic_load((const __attribute__((address_space(1))) int *)(d.own + slot_k),
                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                sroad = (up || own_top == 0) && P.debug_prior != 1;
            }
        }
        // LDS layout: the short road's death takes no barrier before phase F either.  Only wave 0's decision
        // reads the killed-site query's answer: the query wave publishes it (q_zeta, then q_done) and wave 0
        // waits for the flag just before it decides, while phase F's side work -- tid 64's guess, the grid
        // prefetch (on wave kWv - 3: the last wave is asking), the shift edges -- starts at the loop top.
        // Phase F's barrier is then the one between the loop top's reads and wave 0's end-of-iteration writes,
        // as for the short road's change.
        const bool qroad = kNoBarB && sroad && action == tdchain::kDeath;
        if (p.active) {
            // ============ phase B: tile pass || birth/death Interpolation ============
            // (a scripted step brings its own values: no Interpolation query -- but for a server's death
            // step the reference next asks Interpolation of the proposed model at the killed site
            // (TD_inversion_function.jl:146): the idle query wave answers it here, posted with the report)
            const bool kill_q = SCRIPT && mb && action == tdchain::kDeath && sh.step_cur.decision == kDecideLater;
            const bool query = (!nscript && (action == tdchain::kBirth || action == tdchain::kDeath)) || kill_q;
            // LDS layout, free-running, no birth: phase B ends without a block barrier.  Phase C needs of
            // the tile pass only each wave's own first hit tiles (their points are in its registers) until
            // it walks the whole hit list: each wave counts itself done after its tile pass (a death's
            // query wave before its query, whose answer only the decision reads) and a wave waits for all
            // of them after its own points.  (A birth's marks need the query's answer: the barrier stays.)
            nobar = kNoBarB && action != tdchain::kBirth && p.valid && P.debug_prior != 1 && !sroad;
            if (eval && !sroad) {
                // tiles whose box can hold a point the proposal changes (the last
                // wave answers the Interpolation query meanwhile)
                const bool q0 = action != tdchain::kBirth;  // old site of the selected cell
                const bool q1 = action == tdchain::kBirth || action == tdchain::kMove;  // new site
                const TileQuery tq0 = tile_query(kx, ky, kz), tq1 = tile_query(p.x, p.y, p.z);
                const int nthr = query ? NTH - 64 : NTH;
                // tiles in flight per thread: LDS latency is short; HBM needs more
                constexpr int TU = SMALL ? 3 : 8;
                if (super_on) {
                    // rays in HBM: the super-tiles (LDS) first, then the tiles of those hit
                    const int par = (int)(it & 1);
                    int *hl = shit + par * kListLds;
                    if (tid < nthr)
                        for (int S0 = tid; S0 < NS; S0 += 4 * nthr) {
                            bool hit[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const int S = min(S0 + u * nthr, NS - 1);
                                const float thr = smax[S] * (1.0f + 0x1p-20f);
                                const bool h0 = tile_may_hit(slo, shi, NS, S, tq0, thr);
                                const bool h1 = tile_may_hit(slo, shi, NS, S, tq1, thr);
                                hit[u] = S0 + u * nthr < NS && ((q0 && h0) || (q1 && h1));
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                if (hit[u]) {
                                    const int k = atomicAdd(&sh.n_super[par], 1);
                                    if (k < kListLds) hl[k] = S0 + u * nthr;
                                }
                        }
                    __syncthreads();  // (the query wave too: it starts its query after this)
                    SKEW(2);
                    const int nsh = sh.n_super[par];
                    const bool all = nsh > kListLds;  // the list overflowed: every tile
                    const int nitems = all ? NS * kTilePts : nsh * kTilePts;
                    if (tid < nthr)
                        for (int i0 = tid; i0 < nitems; i0 += 4 * nthr) {
                            bool hit[4];
                            int4 rec[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const int i = min(i0 + u * nthr, nitems - 1);
                                const int tu = (all ? (i >> 4) : hl[i >> 4]) * kTilePts + (i & 15);
                                const int t = min(tu, NT - 1);
                                const float thr = tile_thr(v.tmaxd[t]);
                                const bool h0 = tile_may_hit(v.tlo, v.thi, NT, t, tq0, thr);
                                const bool h1 = tile_may_hit(v.tlo, v.thi, NT, t, tq1, thr);
                                rec[u] = int4{t, v.tstart[t], v.tray[t], 0};  // loaded with the box
                                hit[u] = i0 + u * nthr < nitems && tu < NT && ((q0 && h0) || (q1 && h1));
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                if (hit[u]) {
                                    const int k = atomicAdd(&sh.n_tiles, 1);
                                    v.thit[k] = rec[u].x;
                                    if (k < v.hrec_cap) v.hrec[k] = rec[u];
                                }
                        }
                } else if (SMALL) {
                    const TileQuery2 tr0 = tile_query2(kx, ky, kz), tr1 = tile_query2(p.x, p.y, p.z);
                    if (tid < nthr) {  // wave-uniform
                        int npre = 0;  // preload slots this wave has taken (wave-uniform)
                        int pt[kPre] = {0, 0, 0, 0};  // their tiles (wave-uniform: from the ballots, no LDS)
                        for (int b0 = wv * 64; b0 < NT; b0 += TU * nthr) {  // the same trip count in every lane
                            const int t0 = b0 + lane;
                            bool hit[TU];
                            if constexpr (TD_TILE2) {
                                // every box loaded first (one round of LDS loads), then only the sites the action
                                // has, on scalar branches (the action made wave-uniform for the compiler)
                                TileBox bx[TU];
#pragma unroll
                                for (int u = 0; u < TU; ++u)
                                    bx[u] = tile_box(v.tlo, v.thi, v.tmaxd, NT, min(t0 + u * nthr, NT - 1));
                                const int au = __builtin_amdgcn_readfirstlane(action);
                                const bool s0 = au != tdchain::kBirth, s1 = au == tdchain::kBirth || au == tdchain::kMove;
#pragma unroll
                                for (int u = 0; u < TU; ++u) hit[u] = false;
                                if (s0) {
#pragma unroll
                                    for (int u = 0; u < TU; ++u) hit[u] = tile_may_hit2(bx[u], tr0);
                                }
                                if (s1) {
#pragma unroll
                                    for (int u = 0; u < TU; ++u) hit[u] = hit[u] || tile_may_hit2(bx[u], tr1);
                                }
#pragma unroll
                                for (int u = 0; u < TU; ++u) hit[u] = hit[u] && t0 + u * nthr < NT;
                            } else {
#pragma unroll
                                for (int u = 0; u < TU; ++u) {
                                    const int t = min(t0 + u * nthr, NT - 1);  // clamped: loads stay unconditional
                                    const float thr = tile_thr(v.tmaxd[t]);
                                    const bool h0 = tile_may_hit(v.tlo, v.thi, NT, t, tq0, thr);
                                    const bool h1 = tile_may_hit(v.tlo, v.thi, NT, t, tq1, thr);
                                    hit[u] = t0 + u * nthr < NT && ((q0 && h0) || (q1 && h1));
                                }
                            }
#pragma unroll
                            for (int u = 0; u < TU; ++u) {
                                const unsigned long long m = __ballot(hit[u]);
                                if (m == 0ull) continue;
                                const int first = __builtin_ctzll(m), cnt = __popcll(m);
                                const int rank = __popcll(m & ((1ull << lane) - 1ull));
                                int base = 0;
                                if (lane == first) base = atomicAdd(&sh.n_tiles, cnt);  // one atomic per wave
                                base = __builtin_amdgcn_readlane(base, first);
                                if (hit[u]) {
                                    const int t = t0 + u * nthr, slot = npre + rank;
                                    v.thit[base + rank] = slot < kPre ? (t | INT_MIN) : t;
                                }
                                for (unsigned long long mm = m; mm && npre < kPre; mm &= mm - 1ull) {
                                    const int t = b0 + __builtin_ctzll(mm) + u * nthr;
#pragma unroll
                                    for (int k = 0; k < kPre; ++k) pt[k] = k == npre ? t : pt[k];
                                    ++npre;
                                }
                            }
                        }
                        BPROBE(0);  // (tile pass done)
                        if (npre > 0) {
                            if (lane < kTilePts * npre) {
                                const int g = lane / kTilePts;
                                const int t = g == 0 ? pt[0] : g == 1 ? pt[1] : g == 2 ? pt[2] : pt[3];
                                const int sc = v.tstart[t];
                                if (lane % kTilePts < (sc & 31)) {
                                    const int q = (sc >> 5) + lane % kTilePts;
                                    pre_on = true;
                                    pre_q = q;
                                    pre_ray = v.tray[t];
                                    pre_s = d.best_s[q];  // independent loads: one round trip
                                    pre_bd = d.best_d[q];
                                    pre_x = d.px[q];
                                    pre_y = d.py[q];
                                    pre_z = d.pz[q];
                                }
                            }
                        }
                    }
                } else if (tid < nthr)
                    for (int t0 = tid; t0 < NT; t0 += TU * nthr) {
                        bool hit[TU];
#pragma unroll
                        for (int u = 0; u < TU; ++u) {
                            const int t = min(t0 + u * nthr, NT - 1);  // clamped: loads stay unconditional
                            const float thr = tile_thr(v.tmaxd[t]);
                            const bool h0 = tile_may_hit(v.tlo, v.thi, NT, t, tq0, thr);
                            const bool h1 = tile_may_hit(v.tlo, v.thi, NT, t, tq1, thr);
                            hit[u] = t0 + u * nthr < NT && ((q0 && h0) || (q1 && h1));
                        }
#pragma unroll
                        for (int u = 0; u < TU; ++u)
                            if (hit[u]) {
                                const int k = atomicAdd(&sh.n_tiles, 1), t = t0 + u * nthr;
                                v.thit[k] = t;
                                if (!SMALL && k < v.hrec_cap) v.hrec[k] = int4{t, v.tstart[t], v.tray[t], 0};
                            }
                    }
            }
            BPROBE(1);  // (preload issued)
            if (nobar && !(query && wv == kWv - 1)) {  // (every wave but the query wave: its tile pass is done)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (lane == 0) atomicAdd(&sh.b_done, 1);
                SKEW(3);
            }
            if (RLDS && action == tdchain::kDeath && nscript) {  // deleteat! shift, staged before we know if it is accepted
                const int sthr = query ? NTH - 64 : NTH;  // not the query wave: it starts at once
                // (the order in HBM: no staging -- an accepted death shifts it in phase G)
                if constexpr (RLDS) {
                    if (tid < sthr)
                        for (int j = (int)p.index + 1 + tid; j < ncells; j += sthr) d.order_tmp[j] = v.ord[j];
                }
            }
            if (query && wv == kWv - 1) {  // TD_inversion_function.jl:81 (birth), :146 (death)
                const bool birth = action == tdchain::kBirth;
                if (nobar && lane == 0) atomicAdd(&sh.b_done, 1);  // (a death: nothing in phase C waits for this query)
                const Nearest r = wave_nearest(d, v, sh, lane, birth ? p.x : kx, birth ? p.y : ky, birth ? p.z : kz,
                                               birth ? -1 : slot_k, -1, 0.0, 0.0, 0.0, 0.0);
                if (lane == 0) sh.q_zeta = r.z;
                if (qroad) {  // (no barrier follows: the answer released before the flag wave 0 acquires)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    if (lane == 0) atomicAdd(&sh.q_done, 1);
                    SKEW(22);
                }
            }
        }
        // Phase B's barrier (tile list complete, query answered) -- taken by an inactive proposal too (a birth
        // at max_cells, a death at min_cells: the reference skips the iteration, nobar stays false).  That one
        // has no phase B-G, and without this barrier nothing would separate the other waves' reads at the
        // loop top (sh.cur, the proposal, sh.srv_quit) from wave 0's writes at this iteration's end (the next
        // proposal goes into ps[cur] when no guess is adopted): a wave still at the loop top would read the
        // NEXT proposal.  So every iteration has a block barrier between the loop top and wave 0's
        // end-of-iteration writes (this one, or C's and F's).  Found by the wave-skew build
        // (tools/skew_probe.py, the 8-cell model at max_cells 12).
        // (the short road's change, and its death in the LDS layout: phase F's barrier)
        if (!nobar && !(sroad && action == tdchain::kChange) && !qroad) {
            __syncthreads();
            SKEW(4);
            if (p.active && action == tdchain::kBirth) czeta = sh.q_zeta;
            if (p.active && action == tdchain::kDeath) zetanew_death = sh.q_zeta;
        }
        BPROBE(2);  // (counted / barrier passed)
        Proposal pp = p;
        if (p.active && action == tdchain::kBirth && !nscript) tdchain::birth_zeta(P, pp, czeta);  // every lane, same value
        STAMP(1);
        // the next iteration's proposal can be guessed during phase F if its draws are here
        const bool can_spec = !nscript && it + 1 < iters && ((it + 1) & 63) != 0;
        if (pp.active && pp.valid) {
            const bool fwd = P.debug_prior != 1;
            int no = 0;
            if (fwd && !sroad) {
                // ================= phase C: affected points =================
                if (!nscript && tid == NTH - 64)  // the decision's phi-free part, off phase F's path
                    sh.ap = tdchain::alpha_parts(P, pp, czeta, zeta_killed,
                                                 nobar && action == tdchain::kDeath ? sh.q_zeta : zetanew_death,
                                                 sh.lnN);  // (nobar: this lane asked the death's query itself)

                const int nt = sh.n_tiles;
                // the selected cell's value, known since the proposal was made: czeta[slot_k] = zeta_killed
                const double zeta_k = slot_k >= 0 ? zeta_killed : 0.0;
                int seen = 0;
                // one candidate point: captured (birth, move), re-valued (change) or orphaned
                // (death, move: its nearest cell is the selected one)
                auto point = [&](int q, int ray, int s, double bd, double qx, double qy, double qz) {
                    if (action == tdchain::kBirth) {  // appended cell: strict capture
                        const double dd = dist2(pp.x, pp.y, pp.z, qx, qy, qz);
                        if (dd < bd) mark(d, v, sh, q, ray, new_slot, dd, pp.zeta, s);
                    } else if (action == tdchain::kChange) {
                        if (s == slot_k) mark(d, v, sh, q, ray, s, bd, pp.zeta, s);
                    } else if (s == slot_k) {  // death / move: its points are re-searched
                        const int o = atomicAdd(&sh.n_orphans, 1);
                        d.orphans[o] = q;
                        if (o < kOrphanLds) sh.orph[o] = OrphanRec{qx, qy, qz, q, ray};
                    } else if (action == tdchain::kMove) {
                        const double dd = dist2(pp.x, pp.y, pp.z, qx, qy, qz);
                        // (an exact tie: Julia positions, through the stamps -- loaded only then)
                        if (dd < bd || (dd == bd && s >= 0 && d.stamp[slot_k] < d.stamp[s]))
                            mark(d, v, sh, q, ray, slot_k, dd, zeta_k, s);
                    }
                };
                if constexpr (SMALL) {
                    if (pre_on) {  // loaded in phase B
                        ++seen;
                        point(pre_q, pre_ray, pre_s, pre_bd, pre_x, pre_y, pre_z);
                    }
                    if (nobar)  // the whole hit list from here on: every wave's tile pass done
                        SPIN_WAIT(__hip_atomic_load(&sh.b_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < kWv, 1);
                    const int nt = sh.n_tiles;
                    for (int item = tid; item < nt * kTilePts; item += NTH) {
                        const int t = v.thit[item / kTilePts];
                        if (t < 0) continue;  // preloaded
                        const int sc = v.tstart[t];  // start << 5 | count
                        if (item % kTilePts >= (sc & 31)) continue;
                        const int q = (sc >> 5) + item % kTilePts;
                        ++seen;
                        // independent loads: one round trip
                        const int s = d.best_s[q];
                        const double bd = d.best_d[q];
                        const double qx = d.px[q], qy = d.py[q], qz = d.pz[q];
                        point(q, v.tray[t], s, bd, qx, qy, qz);
                    }
                } else {
                    constexpr int CU = 4;  // items in flight per thread (rays in HBM: latency)
                    for (int item0 = tid; item0 < nt * kTilePts; item0 += CU * NTH) {
                        int qq[CU], rr[CU], ss[CU];
                        double bb[CU], xx[CU], yy[CU], zz[CU];
#pragma unroll
                        for (int u = 0; u < CU; ++u) {  // every load of the CU items: one round trip
                            const int item = item0 + u * NTH;
                            const int4 rec = v.tile_rec(min(item, nt * kTilePts - 1) / kTilePts);
                            const int sc = rec.y;  // start << 5 | count
                            const bool in = item < nt * kTilePts && item % kTilePts < (sc & 31);
                            const int q = in ? (sc >> 5) + item % kTilePts : 0;
                            qq[u] = in ? q : -1;
                            rr[u] = rec.z;
                            ss[u] = d.best_s[q];
                            bb[u] = d.best_d[q];
                            xx[u] = d.px[q];
                            yy[u] = d.py[q];
                            zz[u] = d.pz[q];
                        }
#pragma unroll
                        for (int u = 0; u < CU; ++u)
                            if (qq[u] >= 0) {
                                ++seen;
                                point(qq[u], rr[u], ss[u], bb[u], xx[u], yy[u], zz[u]);
                            }
                    }
                }
                if (seen) atomicAdd(&sh.pts_seen, seen);
                __syncthreads();
                SKEW(5);
                if (nobar && action == tdchain::kDeath) zetanew_death = sh.q_zeta;  // (the query wave is past it)
                STAMP(2);
                // ========= phase D: re-search orphaned points, one wave each =========
                no = sh.n_orphans;
                const bool death = action == tdchain::kDeath;
                const int skip_s = death ? slot_k : -1, moved_s = death ? -1 : slot_k;
                // the orphans the per-wave search takes: all of them in order, or the batch's unproven ones
                int nlist = no;
                const int *olist = nullptr;
                if constexpr (RLDS) {
                    if (no >= kBatchOrphans && 2 * n >= no && sh.grid_ovf == 0) {  // (block-uniform)
                        // The nearest cell of every orphan, at once: the buckets of the orphans' bucket
                        // box grown by one on each side, their entries staged in LDS (phase E's ray
                        // scratch is idle), then a thread per orphan over all of them, with the moved cell
                        // at its new site.  Proven as the per-wave search proves: a distance strictly
                        // below the region's faces (the region holds every orphan's 3x3x3 block), no tie
                        // at the minimum; else the orphan goes to the per-wave search (its full scan).
                        const CellGrid &G = d.grid;
                        double *ex = reinterpret_cast<double *>(ray_scratch);
                        double *ey = ex + kBatchCand, *ez = ey + kBatchCand;
                        int *es = reinterpret_cast<int *>(ez + kBatchCand);
                        int *fb = reinterpret_cast<int *>(v.cptS);  // (candidate t* of phase E: idle)
                        auto orphan_xyz = [&](int o, double &qx, double &qy, double &qz) {
                            if (o < kOrphanLds) {
                                qx = sh.orph[o].x;
                                qy = sh.orph[o].y;
                                qz = sh.orph[o].z;
                            } else {
                                const int q = d.orphans[o];
                                qx = d.px[q];
                                qy = d.py[q];
                                qz = d.pz[q];
                            }
                        };
                        if (tid == 0) {
                            for (int a3 = 0; a3 < 3; ++a3) {
                                sh.ob_lo[a3] = INT_MAX;
                                sh.ob_hi[a3] = -1;
                            }
                            sh.ob_ncand = sh.ob_nfb = 0;
                        }
                        __syncthreads();
                        SKEW(6);
                        for (int o = tid; o < no; o += NTH) {
                            double qx, qy, qz;
                            orphan_xyz(o, qx, qy, qz);
                            const int bi = grid_axis(qx, G.x0, G.ix, G.gx), bj = grid_axis(qy, G.y0, G.iy, G.gy),
                                      bk = grid_axis(qz, G.z0, G.iz, G.gz);
                            atomicMin(&sh.ob_lo[0], bi);
                            atomicMax(&sh.ob_hi[0], bi);
                            atomicMin(&sh.ob_lo[1], bj);
                            atomicMax(&sh.ob_hi[1], bj);
                            atomicMin(&sh.ob_lo[2], bk);
                            atomicMax(&sh.ob_hi[2], bk);
                        }
                        __syncthreads();
                        SKEW(7);
                        const int i0 = max(sh.ob_lo[0] - 1, 0), i1 = min(sh.ob_hi[0] + 1, G.gx - 1);
                        const int j0 = max(sh.ob_lo[1] - 1, 0), j1 = min(sh.ob_hi[1] + 1, G.gy - 1);
                        const int k0b = max(sh.ob_lo[2] - 1, 0), k1b = min(sh.ob_hi[2] + 1, G.gz - 1);
                        const int nbx = i1 - i0 + 1, nby = j1 - j0 + 1, nbz = k1b - k0b + 1;
                        if (nbx * nby * nbz <= kBatchBuckets) {
                            for (int b = tid; b < nbx * nby * nbz; b += NTH) {
                                const int bucket = ((k0b + b / (nbx * nby)) * G.gy + (j0 + (b / nbx) % nby)) * G.gx +
                                                   (i0 + b % nbx);
                                const int cnt = d.bucket_count[bucket];
                                const int base = cnt > 0 ? atomicAdd(&sh.ob_ncand, cnt) : 0;
                                for (int e = 0; e < cnt && base + e < kBatchCand; ++e) {
                                    const CellEntry &be = d.buckets[bucket * kBucketCap + e];
                                    ex[base + e] = be.x;
                                    ey[base + e] = be.y;
                                    ez[base + e] = be.z;
                                    es[base + e] = d.bslot[bucket * kBucketCap + e];
                                }
                            }
                            __syncthreads();
                            SKEW(8);
                            const int nc = sh.ob_ncand;
                            if (nc <= kBatchCand) {
                                // four lanes per orphan (a quad), each over a quarter of the entries,
                                // then the quad's lexicographic minimum (the loop is wave-uniform)
                                for (int o0 = 0; o0 < no; o0 += NTH / 4) {
                                    const int o = o0 + tid / 4, part = tid & 3;
                                    const bool act = o < no;
                                    double qx = 0.0, qy = 0.0, qz = 0.0;
                                    if (act) orphan_xyz(o, qx, qy, qz);
                                    double bd = kSentinel;
                                    int bs = -1;
                                    bool tie = false;
                                    auto take = [&](double dd, int sl) {
                                        if (dd < bd) {
                                            bd = dd;
                                            bs = sl;
                                            tie = false;
                                        } else if (dd == bd && dd < kSentinel) {
                                            tie = true;
                                        }
                                    };
                                    for (int c = part; c < nc; c += 4) {
                                        const int sl = es[c];
                                        const double dd = dist2(ex[c], ey[c], ez[c], qx, qy, qz);
                                        if (sl != skip_s && sl != moved_s) take(dd, sl);
                                    }
                                    if (moved_s >= 0 && part == 0)  // the moved cell, at its proposed site
                                        take(dist2(pp.x, pp.y, pp.z, qx, qy, qz), moved_s);
#pragma unroll
                                    for (int m = 1; m <= 2; m <<= 1) {  // quad reduction (distinct slots per lane)
                                        const double od = __shfl_xor(bd, m, 4);
                                        const int os = __shfl_xor(bs, m, 4);
                                        const bool ot = __shfl_xor((int)tie, m, 4) != 0;
                                        if (od < bd) {
                                            bd = od;
                                            bs = os;
                                            tie = ot;
                                        } else if (od == bd && od < kSentinel) {
                                            tie = true;
                                        }
                                    }
                                    if (!act || part != 0) continue;
                                    // every cell outside the region lies beyond one of its inner faces
                                    double lb = __builtin_huge_val();
                                    // (and, the grid sealed, its distance to the cells' box: internal.h grid_block_lb)
                                    double o2[3];
                                    grid_out2(G, qx, qy, qz, o2);
                                    auto face = [&lb](double w, double w0, double h, double e, int g, int lo, int hi,
                                                      double other) {
                                        if (lo > 0) {
                                            const double gap = (w - (w0 + (double)lo * h)) - e;
                                            const double f = (gap > 0.0 ? gap * gap : 0.0) + other;
                                            lb = f < lb ? f : lb;
                                        }
                                        if (hi < g - 1) {
                                            const double gap = ((w0 + (double)(hi + 1) * h) - w) - e;
                                            const double f = (gap > 0.0 ? gap * gap : 0.0) + other;
                                            lb = f < lb ? f : lb;
                                        }
                                    };
                                    face(qx, G.x0, G.hx, G.ex, G.gx, i0, i1, o2[1] + o2[2]);
                                    face(qy, G.y0, G.hy, G.ey, G.gy, j0, j1, o2[0] + o2[2]);
                                    face(qz, G.z0, G.hz, G.ez, G.gz, k0b, k1b, o2[0] + o2[1]);
                                    lb = grid_lb_close(lb);
                                    if (bs >= 0 && bd < kSentinel && !tie && bd < lb) {
                                        const int q = o < kOrphanLds ? sh.orph[o].q : d.orphans[o];
                                        const int ray = o < kOrphanLds ? sh.orph[o].ray : d.pt_ray[q];
                                        mark(d, v, sh, q, ray, bs, bd, d.czeta[bs], slot_k);
                                    } else {
                                        fb[atomicAdd(&sh.ob_nfb, 1)] = o;
                                    }
                                }
                                __syncthreads();
                                SKEW(9);
                                nlist = sh.ob_nfb;
                                olist = fb;
                            }
                        }
                    }
                }
                for (int k = wv; k < nlist; k += kWv) {  // one wave per orphan, no block barrier
                    const int o = olist ? olist[k] : k;
                    double qx, qy, qz;
                    int q, ray;
                    if (o < kOrphanLds) {
                        qx = sh.orph[o].x;
                        qy = sh.orph[o].y;
                        qz = sh.orph[o].z;
                        q = sh.orph[o].q;
                        ray = sh.orph[o].ray;
                    } else {
                        q = d.orphans[o];
                        qx = d.px[q];
                        qy = d.py[q];
                        qz = d.pz[q];
                        ray = d.pt_ray[q];
                    }
                    const Nearest r =
                        wave_nearest(d, v, sh, lane, qx, qy, qz, skip_s, moved_s, pp.x, pp.y, pp.z, zeta_killed);
                    if (lane == 0) mark(d, v, sh, q, ray, r.s, r.d, r.z, slot_k);  // (an orphan: its owner was the selected cell)
                }
                if (nlist > 0) __syncthreads();
                SKEW(10);
                STAMP(3);
                // ================= phase E: t* of the rays that changed =================
                const int nr = sh.n_rays;
                const OverlayZeta oz{d.cand_flag, d.cand_z, d.zeta0};
                // the t* of a changed ray and its chi^2 term (MCsub.jl:147-171), kept beside the old
                auto ray_done = [&](int r, double val, double tsr, double sgr, double old_term, int npr) {
                    v.cptS[r] = val;
                    const double df = val - tsr;
                    const double sg = sgr;
                    v.cterm[r] = old_term;                       // kept to undo a rejection
                    const double nterm = ((df * df) * 1.0) / (sg * sg);  // MCsub.jl:171
                    v.term[r] = nterm;
                    if constexpr (!RLDS) {  // (the running total: any order; rays in LDS re-add them all)
                        atomicAdd(&sh.dsum, nterm - old_term);
                        atomicAdd(&sh.dabs, fabs(nterm) + fabs(old_term));
                    }
                    if constexpr (RLDS)  // (the accounting below may run before phase E is over)
                        atomicAdd((unsigned long long *)&sh.bytes, (unsigned long long)npr * 17ull);
                    else
                        atomicAdd(&sh.ray_pts, npr);
                    if constexpr (WALK)  // an event of the walk (scripted steps: the decisions on bounds need none)
                        if (nscript) atomicOr(&cmask[r >> 6], 1ull << (r & 63));
                };
                if constexpr (!SMALL) {
                    // the large geometries (~15 changed rays a proposal, every load from HBM): two rays per
                    // wave at a time, one per half (ray_sum.h half_ray_sum), their loads in one round trip.
                    // Lane l holds the offsets, tS, sigma and old term of the wave's ray of turn l / 2,
                    // half l % 2 (one round of loads before the first sum; past 32 turns: per ray)
                    const int half = lane >> 5, hl = lane & 31;
                    const int mine = 2 * wv + (lane & 1) + 2 * kWv * (lane >> 1);
                    int ra = 0, s0a = 0, e0a = 0;
                    double tsa = 0.0, sga = 0.0, ota = 0.0;
                    if (mine < nr) {
                        ra = v.ray_at(mine);
                        s0a = v.ray_off[ra];
                        e0a = v.ray_off[ra + 1];
                        tsa = v.tS[ra];
                        sga = v.sig[ra];
                        ota = v.term[ra];
                    }
                    double *hs = reinterpret_cast<double *>(lds + L.scratch) + wv * 192 + half * 96;
                    for (int base = 2 * wv, j = 0; base < nr; base += 2 * kWv, ++j) {
                        const int rr = base + half;
                        const bool have = rr < nr;
                        int r = 0, s0 = 0, npr = 0;
                        double tsr = 0.0, sgr = 0.0, old_term = 0.0;
                        if (j < 32) {  // (wave-uniform)
                            const int src = 2 * j + half;
                            r = __shfl(ra, src);
                            s0 = __shfl(s0a, src);
                            npr = __shfl(e0a, src) - s0;
                            tsr = __shfl(tsa, src);
                            sgr = __shfl(sga, src);
                            old_term = __shfl(ota, src);
                        } else if (have) {
                            r = v.ray_at(rr);
                            s0 = v.ray_off[r];
                            npr = v.ray_off[r + 1] - s0;
                            tsr = v.tS[r];
                            sgr = v.sig[r];
                            old_term = v.term[r];
                        }
                        const double val = half_ray_sum(hl, d.w, oz, s0, have ? npr : 0, hs);
                        if (have && hl == 0) ray_done(r, val, tsr, sgr, old_term, npr);
                    }
                } else {
                    // rays in HBM: a wave's rays' offsets, tS, sigma and old terms, one per lane,
                    // in one round of loads before its first sum (the 64 first; more: per ray)
                    int ra = 0, s0a = 0, e0a = 0;
                    double tsa = 0.0, sga = 0.0, ota = 0.0;
                    if (!RLDS && wv + kWv * lane < nr && lane < 64) {
                        ra = v.ray_at(wv + kWv * lane);
                        s0a = v.ray_off[ra];
                        e0a = v.ray_off[ra + 1];
                        tsa = v.tS[ra];
                        sga = v.sig[ra];
                        ota = v.term[ra];
                    }
                    for (int rr = wv, j = 0; rr < nr; rr += kWv, ++j) {
                        int r, s0, npr;
                        double tsr, sgr, old_term;
                        if (!RLDS && j < 64) {
                            r = __builtin_amdgcn_readlane(ra, j);
                            s0 = __builtin_amdgcn_readlane(s0a, j);
                            npr = __builtin_amdgcn_readlane(e0a, j) - s0;
                            tsr = readlane_f64(tsa, j);
                            sgr = readlane_f64(sga, j);
                            old_term = readlane_f64(ota, j);
                        } else {
                            r = v.ray_at(rr);
                            s0 = v.ray_off[r];
                            npr = v.ray_off[r + 1] - s0;
                            tsr = v.tS[r];  // with the offsets
                            sgr = v.sig[r];
                            old_term = v.term[r];
                        }
                        const double val = wave_ray_sum(lane, d.w, oz, s0, npr, ray_scratch[wv]);
                        if (lane == 0) ray_done(r, val, tsr, sgr, old_term, npr);
                    }
                    if constexpr (RLDS) {
                        // no block barrier after phase E: only wave 0's decision reads the new terms, so a
                        // wave that summed rays counts itself done (its LDS writes first) and wave 0 waits
                        // for those (~1.2 rays a proposal: mostly none); the other waves go straight on to
                        // phase F's side work
                        if (wv != 0 && wv < nr) {
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                            if (lane == 0) atomicAdd(&sh.e_done, 1);
                        } else if (wv == 0 && nr > 1) {
                            const int want = min(nr, kWv) - 1;
                            SPIN_WAIT(__hip_atomic_load(&sh.e_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < want,
                                      1000);
                        }
                        SKEW(11);
                    }
                }
                if constexpr (!RLDS) __syncthreads();
                SKEW(12);
                STAMP(4);
            }
            // a server's step decided later: its answer goes out now, before phase F -- the changed rays'
            // new t*, from which the host forms phi_n itself (the sequential sum from the first changed
            // ray on its own partial sums, incremental.cpp), and a death's killed-site Interpolation
            // (phase B); this step's exact sums below then overlap the host's work
            const bool early = SCRIPT && mb && sh.step_cur.decision == kDecideLater;
            // the step's decision, read here, before phase F's barrier: wave 0 writes the next step into
            // step_cur at the iteration's end, which a wave still in phase G must not see
            const int sdec = nscript ? sh.step_cur.decision : 1;
            if (early && wv == 0) {
                server_report(sa.out, v, sh, n, lane, __builtin_nan(""));
                // the answer's system-scope stores acknowledged before done: no system-scope
                // fence, which would write back this XCD's L2 at every call
                __builtin_amdgcn_s_waitcnt(0);
                wave_sync_lds();
                if (lane == 0) {
                    mb_store(&mb->done, sh.srv_seq);
                    if (action == tdchain::kDeath) {  // left in the mailbox under this command's seq
                        mb_store(reinterpret_cast<long long *>(&mb->pq_val), __double_as_longlong(sh.q_zeta));
                        __builtin_amdgcn_s_waitcnt(0);
                        mb_store(&mb->pq_seq, sh.srv_seq);
                    }
                }
            }
            // ==== phase F: chi^2 + decision (wave 0) || next proposal, tile maxima (rays in HBM) ====
            const long long tF = prof_on ? clock64() : 0;  // diagnostic: per-wave time in F
            constexpr bool spec_in_F = true;
            double phi_n = 1.0;  // debug_prior: MCsub.jl:134-136
            int bdec = 0;        // wave 0, LDS layout: 1 rejected / 2 accepted on bounds, 0 on the exact phi_n
            // The proposal's terms summed in any order (decisions on bounds, below): the committed
            // running total plus phase E's changes, Tp, within Ep of the exact real sum (every
            // rounding bounded twice over: the total's own bound, the changes and their magnitudes
            // added in any order, the one add).  When Ep passes 1e-10 of Tp (or is not finite) the
            // sum is formed afresh from all the terms (block-uniform: every lane reads the same LDS).
            // Rays in LDS: the ~400 terms are re-added every time (one wave, one DPP reduction: as
            // cheap as keeping the total).
            const double Tp = RLDS ? 0.0 : sh.tsum + sh.dsum;
            const double Ep = RLDS ? 0.0 : sh.terr + kSumSlack * ((double)(sh.n_rays + 2) * sh.dabs + fabs(Tp));
            const bool anchor = RLDS || !(Ep <= 1e-10 * Tp);
            if constexpr (WALK) {
                // rays in HBM: the whole block adds the proposal's terms afresh in any order --
                // n / 512 global loads per thread, four in flight
                if (!nscript && fwd && sh.k0 < n && anchor) {  // (block-uniform)
                    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
                    int k = tid;
                    for (; k + 3 * NTH < n; k += 4 * NTH) {
                        p0 = p0 + gload(v.term + k);
                        p1 = p1 + gload(v.term + k + NTH);
                        p2 = p2 + gload(v.term + k + 2 * NTH);
                        p3 = p3 + gload(v.term + k + 3 * NTH);
                    }
                    for (; k < n; k += NTH) p0 = p0 + gload(v.term + k);
                    const double wsum = wave_sum_f64((p0 + p1) + (p2 + p3));
                    if (lane == 0) sh.wpart[wv] = wsum;
                    __syncthreads();
                    SKEW(13);
                }
            }
            if (RLDS && !nscript && action == tdchain::kDeath && lane == 0) {  // what phase G's shift overwrites
                if (wv != 0) {
                    int a, b;
                    shift_range((int)p.index, ncells, wv, kWv - 1, a, b);
                    if (b > a) sh.shift_edge[wv] = v.ord[b - 1];
                } else {
                    sh.shift_done = 0;
                }
            }
            if (wv == 0) {
                const int k0 = sh.k0;
                if (fwd) {
                    // the terms added in k order (MCsub.jl:170-172), bit for bit, by this
                    // wave (exact_sum.h); phase E put the changed rays' new terms in place
                    // (the old ones wait in cterm, their sums in prefix).
                    // Rays in LDS: the decision first, on bounds.  The terms are >= 0, so
                    // their sequential sum is within n ulps of any other association: the
                    // sum of ALL the proposal's terms in any order (one DPP reduction,
                    // whatever k0) brackets phi_n within 1e-9; phi_r is exact or likewise
                    // bracketed; the decision is monotone (up in phi, down in phi_n), so
                    // when it is the same at both corners of the brackets it is the one the
                    // exact values give.  A rejection then needs no exact sum; an acceptance
                    // leaves its partial sums unformed (prefix exact below ex_upto, phi_r an
                    // estimate in [phi_lo, phi_hi]) until a decision the brackets cannot
                    // take (phi_n within ~1e-9 of the threshold), a tempering round's end or
                    // the launch's end: then the committed terms from ex_upto and the
                    // proposal's from k0 are added in order, the binade-run scans.
                    // Rays in HBM: the same, the sum of all terms formed by the whole block
                    // (above); a scripted step (exact every time) walks the events instead --
                    // the new sums follow the old ones at a checked constant offset between
                    // events (exact_sum.h delta_walk).
                    if (!WALK || !nscript) {
                        // nothing changed (k0 == n): phi_n IS phi_r, estimate or not (MCsub.jl:169-172
                        // adds the same terms), and phi - phi_n = 0 in the decision either way
                        bool exact = nscript != 0;
                        if (k0 >= n) phi_n = phi_r;
                        if (!exact && k0 < n) {
                            double Sa = Tp, Ea = Ep;
                            if (anchor) {
                                Sa = 0.0;
                                if constexpr (WALK) {
                                    for (int w = 0; w < kWv; ++w) Sa = Sa + sh.wpart[w];
                                } else {
                                    double part = 0.0;
                                    for (int k = lane; k < n; k += 64) part = part + v.term[k];
                                    Sa = wave_sum_f64(part);
                                }
                                Ea = kSumSlack * (double)(n + 1) * fabs(Sa);
                            }
                            if (!RLDS && lane == 0) {  // the running total if the proposal is committed
                                sh.b_T = Sa;
                                sh.b_E = Ea;
                            }
                            // the sequential phi_n lies within (n - 1) ulps of the exact sum, far inside 1e-9
                            const double b_lo = (Sa - Ea) * (1.0 - 1e-9), b_hi = (Sa + Ea) * (1.0 + 1e-9);
                            // most decisions at once from the phi-free part (chain_logic.h decide_sure),
                            // else the two corners side by side: lane 0 (phi_lo, b_hi), lane 1 (phi_hi, b_lo)
                            const int sure = tdchain::decide_sure(sh.ap, pp.log_u, (sh.phi_lo - b_hi) * inv2t_r,
                                                                  (sh.phi_hi - b_lo) * inv2t_r);
                            if (sure != 0) {
                                bdec = sure > 0 ? 2 : 1;
                            } else {
                                const bool lo = lane == 0;
                                const int a = lane < 2 ? (int)tdchain::accept_t(P, inv2t_r, pp, lo ? sh.phi_lo : sh.phi_hi,
                                                                               lo ? b_hi : b_lo, czeta, zeta_killed,
                                                                               zetanew_death, sh.lnN)
                                                       : 0;
                                const int a_min = __builtin_amdgcn_readlane(a, 0), a_max = __builtin_amdgcn_readlane(a, 1);
                                bdec = a_min != a_max ? 0 : a_min ? 2 : 1;
                            }
                            // a tempering round's last iteration publishes phi: decided exactly (and
                            // every sum made exact) whatever the bounds say (testing: every k-th too)
                            if ((rbx || xch) && it + 1 == round_end) bdec = 0;
                            if constexpr (REC)
                                if (it + 1 == rec_next) bdec = 0;  // a recorded sample carries the exact phi: likewise
                            if (d.exact_every > 0 && (it % d.exact_every) == d.exact_every - 1) bdec = 0;
                            exact = bdec == 0;
                            phi_n = Sa;  // (an estimate on a decided proposal)
                            if (bdec == 2 && lane == 0) {  // the accepted terms' sums: unformed
                                sh.ex_upto = min(sh.ex_upto, k0);
                                sh.b_lo = b_lo;
                                sh.b_hi = b_hi;
                            }
                        }
                        if (exact && k0 < n) {  // the committed partial sums and phi_r, then the proposal's
                            const ExactPhis ex = exact_sums(v.term, v.prefix, v.cprefix, v.cterm, v.rflag, sh, n, lane,
                                                            true, k0, phi_r, phi_n);
                            phi_r = ex.phi;
                            phi_n = ex.phi_n;
                            if (prof_on && lane == 0) sh.prof[65] += 1;  // (diagnostic: exact decisions)
                        }
                        if (prof_on && lane == 0 && k0 < n) sh.prof[64] += n - k0;
                    } else {
                        double C = k0 > 0 ? v.prefix[k0 - 1] : 0.0;  // MCsub.jl:169 C = 0
                        if (k0 < n) {  // O(events), not O(tail): exact_sum.h delta_walk
                            C = delta_walk(v.term, v.prefix, v.rflag, k0, n, C, smask, cmask, v.cprefix, sh.dseg, lane,
                                           prof_on ? &sh.prof[72] : nullptr);
                            if (prof_on && lane == 0) sh.prof[64] += n - k0;
                        }
                        phi_n = k0 < n ? C : sh.phi;
                    }
                }
                if (prof_on && lane == 0) sh.prof[66] += clock64() - tF;  // diagnostic: scan done
                if (qroad) {  // the query wave's answer (no barrier since the loop top)
                    SPIN_WAIT(__hip_atomic_load(&sh.q_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < 1,
                              1000000000);
                    zetanew_death = sh.q_zeta;
                }
            }
            if (tid == 0) {
                // Metropolis-Hastings decision (on bounds: the one accept() gives on the exact values);
                // a scripted step's decision is given (kDecideLater: by the server's next command;
                // the grid update below is then staged and applied only if it is a commit)
                const bool acc = nscript ? sh.step_cur.decision == 1
                                 : bdec != 0 ? bdec == 2
                                             : tdchain::accept_t(P, inv2t_r, pp, phi_r, phi_n, czeta, zeta_killed,
                                                                 zetanew_death, sh.lnN);
                acc_r = acc;
                sh.gs = Shared::GSnap{sh.n_changed, sh.n_rays, sh.n_tiles, sh.k0, acc ? 1 : 0};
                sh.defer = bdec == 2 ? 1 : 0;
                sh.phi_n = phi_n;
                if (prof_on) sh.prof[67] += clock64() - tF;  // diagnostic: decision taken
                if (acc || (mb && sh.step_cur.decision == kDecideLater)) {
                    sh.g_op = action == tdchain::kBirth ? 2 : action == tdchain::kDeath ? 1
                              : action == tdchain::kMove ? 3 : 4;
                    sh.g_slot = action == tdchain::kBirth ? new_slot : slot_k;
                    sh.g_ox = kx;
                    sh.g_oy = ky;
                    sh.g_oz = kz;
                    sh.g_nx = pp.x;
                    sh.g_ny = pp.y;
                    sh.g_nz = pp.z;
                    sh.g_nzeta = pp.zeta;
                    if (acc) atomicAdd((unsigned long long *)&sh.accepted[action], 1ull);
                }
                if (prof_on && bdec == 1) atomicAdd((unsigned long long *)&sh.prof[14], 1ull);  // rejected on bounds
            } else if (spec_in_F && tid == 64) {  // the next proposal as if this one were rejected
                if (can_spec) {
                    // (with the cell's point count: every commit atomic of earlier iterations is performed --
                    // phase G's waves wait for theirs before the iteration-end barrier)
                    make_proposal<true>(sh.ps[sh.cur ^ 1], P, draws[(it + 1) & 63], ncells, sh.nfree, sh.nslots,
                                        d.free_slots, d.cx, d.cy, d.cz, d.czeta, [&](int pos) { return v.ord[pos]; }, d.own);
                    sh.spec_ok = 1;
                }
            } else if (wv == kWv - 1 || (kWv >= 6 && wv == kWv - 2) || (qroad && wv == kWv - 3)) {
                // wave kWv - 1: the grid data an accepted update will need (the LDS layout's short-road death:
                // wave kWv - 3, which has no tile to refresh -- the last wave comes here from its query with
                // nothing left to do); wave kWv - 2 (with 8 waves; with 4 the last wave after its prefetch):
                // accounting and the model-size factors
                if (wv == (qroad ? kWv - 3 : kWv - 1))
                    grid_prefetch(d, sh, lane, action, action == tdchain::kBirth ? new_slot : slot_k, kx, ky,
                                  kz, pp.x, pp.y, pp.z);
                if (wv == (kWv >= 6 ? kWv - 2 : kWv - 1)) {
                    if (prof_on && lane == 0) {  // diagnostic: work sizes
                        if (sroad) sh.prof[action == tdchain::kDeath ? 35 : 45] += 1;  // the short road, by action
                        // counts read at the loop top, by action ([7] deaths, [75] changes) and by answer: "owns
                        // none" in the low 32 bits, "owns points" in the high
                        if (own_top >= 0 && fwd)
                            sh.prof[action == tdchain::kDeath ? 7 : 75] += own_top == 0 ? 1ll : 1ll << 32;
                        // a change or death that turned out to own no point and took the full path all the same
                        // (none, once every unknown count is read at the loop top): the high 32 bits of [35] / [45]
                        if (!SCRIPT && fwd && !sroad &&
                            ((action == tdchain::kChange && sh.n_changed == 0) || (action == tdchain::kDeath && no == 0)))
                            sh.prof[action == tdchain::kDeath ? 35 : 45] += 1ll << 32;
                        sh.prof[68] += sh.n_tiles;
                        sh.prof[69] += sh.pts_seen;
                        sh.prof[70] += sh.n_changed;
                        sh.prof[71] += sh.n_rays;
                    }
                    if (lane == 0 && fwd) {  // accounting, off wave 0's path
                        atomicAdd((unsigned long long *)&sh.evaluations, 1ull);
                        // bytes this proposal's algorithm must read: tile boxes + maxima (32 B),
                        // candidate points (coords + cached slot/distance, 36 B), grid queries
                        // (27 buckets x 8 entries x 32 B), rays (w, zeta, flag: 17 B per point),
                        // chi^2 tail (ptS, tS, sig, flag: 28 B per ray).  A change or death whose cell owns no
                        // point needs no tile box and no point: counted so on either road -- the full path,
                        // which finds it out (nothing marked, no orphan), reads them for nothing -- so the
                        // count does not depend on which proposals a launch's first or an untrusted guess is
                        // (tests/test_gpu_tempering_history.py holds the stats of split calls to one call's)
                        // (scripted steps always take the full path: counted as before)
                        const bool owns_none = !SCRIPT && ((action == tdchain::kChange && sh.n_changed == 0) ||
                                                          (action == tdchain::kDeath && no == 0));
                        atomicAdd((unsigned long long *)&sh.bytes,
                                  (unsigned long long)((owns_none  ? 0ll
                                                        : super_on ? (long long)NS * 32 +
                                                                         (long long)sh.n_super[it & 1] * kTilePts * 32 +
                                                                         (long long)sh.pts_seen * 36
                                                                   : (long long)NT * 32 + (long long)sh.pts_seen * 36) +
                                                       (long long)(no + (action <= 2 ? 1 : 0)) * 27 * 8 * 32 +
                                                       (RLDS ? 0ll : (long long)sh.ray_pts * 17) + (long long)(n - sh.k0) * 28));
                    }
                    if (lane == 0 && (action == tdchain::kBirth || action == tdchain::kDeath)) {
                        sh.lnN_far[0] = d.logN[max(ncells - 2, 0)];
                        sh.lnN_far[1] = d.logN[ncells + 2];
                    }
                }
            } else if (wv >= 2 && wv <= (kWv >= 6 ? kWv - 3 : 2) && fwd && action != tdchain::kChange) {
                // (waves 2..5 of 8, wave 2 of 4) the hit tiles' maxima if the proposal is accepted (a tile =
                // a DPP row): four items per thread in flight (rays in HBM: ~140 hit tiles, each load a
                // round trip)
                const int nt = sh.n_tiles;
                constexpr int MU = 4, MS = (kWv >= 6 ? kWv - 4 : 1) * 64;
                if constexpr (RLDS) {  // (~8 hit tiles over 4 waves: one item per thread)
                    for (int i = tid - 128; i < nt * kTilePts; i += MS) {
                        const int sc = v.tile_rec(i / kTilePts).y;  // start << 5 | count
                        const int q = (sc >> 5) + (i % kTilePts);
                        unsigned long long mk = 0ull;  // distances are >= 0: max as bit patterns
                        if (i % kTilePts < (sc & 31)) {
                            const double cd = d.cand_d[q], bd = d.best_d[q];
                            mk = (unsigned long long)__double_as_longlong(d.cand_flag[q] ? cd : bd);
                        }
                        mk = row_max_u64(mk);
                        if ((i % kTilePts) == kTilePts - 1) v.ctm_put(i / kTilePts, __longlong_as_double((long long)mk));
                    }
                } else
                for (int i0 = tid - 128; i0 < nt * kTilePts; i0 += MU * MS) {
                    int q[MU];
                    bool in[MU];
#pragma unroll
                    for (int u = 0; u < MU; ++u) {
                        const int i = min(i0 + u * MS, nt * kTilePts - 1);
                        const int sc = v.tile_rec(i / kTilePts).y;  // start << 5 | count
                        in[u] = i0 + u * MS < nt * kTilePts && (i % kTilePts) < (sc & 31);
                        q[u] = in[u] ? (sc >> 5) + (i % kTilePts) : 0;
                    }
                    double cd[MU], bd[MU];
                    unsigned char cf[MU];
#pragma unroll
                    for (int u = 0; u < MU; ++u) {
                        cd[u] = d.cand_d[q[u]];
                        bd[u] = d.best_d[q[u]];
                        cf[u] = d.cand_flag[q[u]];
                    }
#pragma unroll
                    for (int u = 0; u < MU; ++u) {
                        const int i = i0 + u * MS;
                        if (i >= nt * kTilePts) break;  // (whole rows: the same in the 16 lanes of a tile)
                        unsigned long long mk = 0ull;  // distances are >= 0: max as bit patterns
                        if (in[u]) mk = (unsigned long long)__double_as_longlong(cf[u] ? cd[u] : bd[u]);
                        mk = row_max_u64(mk);
                        if ((i % kTilePts) == kTilePts - 1) v.ctm_put(i / kTilePts, __longlong_as_double((long long)mk));
                    }
                }
            }
            if (prof_on && lane == 0)
                atomicAdd((unsigned long long *)&sh.prof[56 + wv], (unsigned long long)(clock64() - tF));
            __syncthreads();
            STAMP(5);
            SKEW(14);
            // ================= phase G: commit (or undo) =================
            const int nc = sh.gs.nc, nr = sh.gs.nr;
            if (nscript && sdec != 1 && !early && wv == 0) server_report(sa.out, v, sh, n, lane, sh.phi_n);
            if (mb && sdec == kDecideLater) {  // answered before phase F; its fate comes with the next command
                if (wv == 0) server_wait(mb, d, v, sh, lane);
                __syncthreads();
                SKEW(15);
                if (tid == 0) acc_r = sh.gs.accept != 0;
            }
            // the changed points' global records (two dependent L2 round trips) and the
            // deleteat! shift go to waves 1.., so wave 0 goes straight to its scalars and
            // the next proposal (kW threads, index w = tid - 64)
            constexpr int kW = NTH - 64;
            const int w = tid - 64;
            if (sh.gs.accept) {
                const int nt = sh.gs.nt, k0 = sh.gs.k0;
                if (wv != 0) {
                    // DevChain::own follows every point whose owner changes: two no-return atomics in L2 (an
                    // accepted change moves no owner -- block-uniform).  The old owner came with the record
                    // (LDS), or is loaded beside the overlay (HBM: the same round trip, before the store).
                    const bool owners = action != tdchain::kChange;
                    for (int c = w; c < nc; c += kW) {
                        int so, sn;
                        if (c < kChgLds) {  // (LDS: stores only)
                            const ChgRec r = sh.chg[c];
                            d.best_s[r.q] = r.s;
                            d.best_d[r.q] = r.d;
                            d.zeta0[r.q] = r.z;
                            d.cand_flag[r.q] = 0;
                            so = r.o;
                            sn = r.s;
                        } else {
                            const int q = d.changed[c];
                            so = d.best_s[q];
                            sn = d.cand_s[q];
                            d.best_s[q] = sn;
                            d.best_d[q] = d.cand_d[q];
                            d.zeta0[q] = d.cand_z[q];
                            d.cand_flag[q] = 0;
                        }
                        if (owners && so != sn) {
                            if (so >= 0) atomicAdd(&d.own[so], -1);
                            if (sn >= 0) atomicAdd(&d.own[sn], 1);
                        }
                    }
                    // The next iteration's guess reads own in phase F (tid 64), and its flag is trusted when
                    // that iteration changes no owner: these atomics must be performed by then.  Counted in
                    // vmcnt like stores, they are waited for here, before this wave reaches the
                    // iteration-end barrier -- the s_barrier alone orders nothing in the vector memory pipe.
                    if (owners && w < nc) __builtin_amdgcn_s_waitcnt(0);
                }
                if (fwd && action != tdchain::kChange) {
                    for (int i = tid; i < nt; i += NTH) v.tmaxd[v.tile_rec(i).x] = v.ctm_at(i);
                    pend_sup = super_on;  // their super-tiles' maxima: at the top of the next iteration
                }
                for (int rr = tid; rr < nr; rr += NTH) {
                    const int r = v.ray_at(rr);
                    v.ptS[r] = v.cptS[r];
                    v.rflag[r] = 0;
                }
                if (!WALK || !nscript) {
                    if (!sh.defer)  // (accepted on bounds: its partial sums are left unformed)
                        for (int r = k0 + tid; r < n; r += NTH) v.prefix[r] = v.cprefix[r];
                } else if (fwd && k0 < n) {
                    pend_r = true;  // written at the top of the next iteration
                    if (wv == 1) delta_remark(v.term, v.prefix, v.cprefix, n, sh.dseg, smask, lane);
                }
                if (RLDS && action == tdchain::kDeath && wv != 0 && !nscript) {  // deleteat!, in LDS (shift_range)
                    int a, b;
                    shift_range((int)pp.index, ncells, wv, kWv - 1, a, b);
                    if (b > a) {
                        const int edge = sh.shift_edge[wv];
                        for (int j0 = a; j0 < b; j0 += 64) {
                            const int j = j0 + lane;
                            if (j < b) {
                                const int sl = j == b - 1 ? edge : v.ord[j];
                                v.ord[j - 1] = sl;
                            }
                        }
                    }
                    // this wave's shifted stores, released before its count (wave 0 acquires it below)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    if (lane == 0) atomicAdd(&sh.shift_done, 1);
                    SKEW(16);
                }
                if (RLDS && action == tdchain::kDeath && wv != 0 && nscript) {  // deleteat!: from the staged copy
                    constexpr int U = 4;                                 // U loads in flight per thread
                    for (int j0 = (int)pp.index + 1 + w; j0 < ncells; j0 += U * kW) {
                        int sl[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) sl[u] = d.order_tmp[min(j0 + u * kW, ncells - 1)];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int j = j0 + u * kW;
                            if (j < ncells) v.ord[j - 1] = sl[u];
                        }
                    }
                }
                if (tid == NTH - 64 && sh.g_op) grid_apply(d, sh);
                if (tid == 0) {
                    const int sk = slot_k;
                    if (action == tdchain::kBirth) {  // append!
                        const int s = new_slot;
                        d.cx[s] = pp.x;
                        d.cy[s] = pp.y;
                        d.cz[s] = pp.z;
                        d.czeta[s] = pp.zeta;
                        v.ord[ncells] = s;
                        const long long st_new = sh.next_stamp;  // appended: after every live cell in Julia order
                        d.stamp[s] = st_new;
                        sh.next_stamp = st_new + 1;
                        if (sh.nfree > 0)
                            sh.nfree -= 1;
                        else
                            sh.nslots += 1;
                        sh.ncells = ncells + 1;
                        const double a = sh.lnN[1], b = sh.lnN[2], c = sh.lnN_far[1];
                        sh.lnN[0] = a;
                        sh.lnN[1] = b;
                        sh.lnN[2] = c;
                    } else if (action == tdchain::kDeath) {
                        d.free_slots[sh.nfree] = sk;
                        sh.nfree += 1;
                        d.stamp[sk] = -1;  // a free slot
                        sh.ncells = ncells - 1;
                        const double a = sh.lnN_far[0], b = sh.lnN[0], c = sh.lnN[1];
                        sh.lnN[0] = a;
                        sh.lnN[1] = b;
                        sh.lnN[2] = c;
                    } else if (action == tdchain::kChange) {
                        d.czeta[sk] = pp.zeta;
                    } else {
                        d.cx[sk] = pp.x;
                        d.cy[sk] = pp.y;
                        d.cz[sk] = pp.z;
                    }
                    if (!RLDS && !nscript && fwd && k0 < n) {  // the running total follows the committed terms
                        sh.tsum = sh.b_T;
                        sh.terr = sh.b_E;
                    }
                    if (bdec == 2) {  // an estimate inside the bracket of phase F
                        phi_r = sh.phi_n;
                        sh.phi_lo = sh.b_lo;
                        sh.phi_hi = sh.b_hi;
                    } else if (!(!nscript && fwd && k0 >= n)) {  // (nothing changed: phi_r stays)
                        phi_r = sh.phi_n;
                        sh.phi_lo = sh.phi_hi = phi_r;
                        sh.phi = phi_r;
                    }
                }
                if constexpr (!RLDS) {
                    // the order in HBM, an accepted death (block-uniform): deleteat! in place, the whole
                    // block -- a round's loads, a barrier, its shifted stores (the next round reads
                    // only positions past the ones this one writes); a barrier before wave 0 reads
                    // the shifted order for the next proposal
                    if (action == tdchain::kDeath) {
                        constexpr int U = 8;
                        for (int b0 = (int)pp.index + 1; b0 < ncells; b0 += U * NTH) {
                            int sl[U];
#pragma unroll
                            for (int u = 0; u < U; ++u) sl[u] = gload(v.ord + min(b0 + tid + u * NTH, ncells - 1));
                            __syncthreads();
                            SKEW(18);
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const int j = b0 + tid + u * NTH;
                                if (j < ncells) v.ord[j - 1] = sl[u];
                            }
                        }
                        __syncthreads();
                        SKEW(21);
                    }
                }
            } else {  // rejected: flags down, the changed rays get their old chi^2 terms back
                if (wv != 0)
                    for (int c = w; c < nc; c += kW) d.cand_flag[c < kChgLds ? sh.chg[c].q : d.changed[c]] = 0;
                for (int rr = tid; rr < nr; rr += NTH) {
                    const int r = v.ray_at(rr);
                    v.term[r] = v.cterm[r];
                    v.rflag[r] = 0;
                }
            }
        }
        last_action = action;
        last_accept = acc_r ? 1 : 0;
        STAMP(12);
        // ===== end of iteration: the next proposal (wave 0; draws refilled every 64) =====
        if (wv == 0) {
            if (prof_on && lane == 0) sh.prof[7 + action] += clock64() - sh.t_iter;  // per-action totals
            if constexpr (REC && !ROUNDS) {
                if (it + 1 == rec_next) {  // a sample's phi is exact (phase F made the sums so, unless nothing was evaluated)
                    phi_r = exact_sums(v.term, v.prefix, v.cprefix, v.cterm, v.rflag, sh, n, lane, false, n, phi_r, 0.0).phi;
                    if (lane == 0) sh.phi = phi_r;  // read by record_sample after the iteration-end barrier
                }
            }
            if ((rbx || xch) && it + 1 == round_end) {  // a tempering round is done: publish phi, take the next temperature
                {  // (a phase F of this iteration made every sum exact already)
                    phi_r = exact_sums(v.term, v.prefix, v.cprefix, v.cterm, v.rflag, sh, n, lane, false, n, phi_r, 0.0).phi;
                    if (lane == 0) sh.phi = phi_r;
                }
                if constexpr (REC && ROUNDS) {
                    // Does this workgroup record the round?  Latched here, before round_wait /
                    // round_exchange publish phi and take the next round's level: host-decided rounds
                    // carry the answer in the slot (still the posted round's words: the host rewrites
                    // them only once it has seen `done`); exchange rounds have the levels of the round
                    // in x.lev (each lane reads the word it wrote itself) and the round's number
                    long long ri = -1;
                    if (rbx) {
                        if (lane == 0) ri = mb_load(&rbx->slot[bchain].rec_i);
                    } else if (d.rec.every > 0) {
                        const RoundX &x = *rxp;
                        const int lv = lane < x.R ? x.lev[bchain * x.R + lane] : -1;
                        const int mine = __shfl(lv, (x.rank * x.local + bchain) & 63);
                        const long long jr = (it + 1) / x.K;  // the call's round, 1-based
                        if (mine == 0 && jr >= d.rec.first && (jr - d.rec.first) % d.rec.every == 0)
                            ri = (jr - d.rec.first) / d.rec.every;
                    }
                    if (lane == 0) {
                        sh.mbox[0] = d.rec.every > 0 ? ri : -1;
                        sh.mbox[1] = it + 1;
                    }
                }
                if (rbx) {
                    round_wait(rbx, bchain, sh, lane, true, phi_r);  // (lane 0 = tid 0 holds phi)
                    round_end = it + 1 + sh.rK;
                } else {
                    const long long Kx = rxp->K;
                    round_exchange(*rxp, bchain, (it + 1) / Kx - 1, sh, lane, phi_r);
                    round_end = it + 1 + Kx;
                }
                inv2t_r = sh.rinv2t;
            }
            if (it + 1 < iters && !((mb || rbx || xch) && sh.srv_quit)) {
                if (((it + 1) & 63) == 0 && !nscript) {
                    wave_sync_lds();
                    if (sa.pre) {
                        if (it + 1 + lane < iters) draws[lane] = sa.pre[(long long)bchain * sa.pre_stride + it + 1 + lane];
                    } else {
                        draws[lane] = tdchain::draw_iteration(d.seed, d.chain, (uint64_t)(iter0 + it + 1 + lane));
                    }
                    wave_sync_lds();
                }
                if (lane == 0) {
                    const bool acc = acc_r;
                    // the guess holds unless an accepted proposal changed what it read
                    const PState &g = sh.ps[cur_r ^ 1];
                    const bool keep = sh.spec_ok && can_spec &&
                                      (!acc || ((action == tdchain::kChange || action == tdchain::kMove) &&
                                                g.slot_k != slot_k));
                    if (keep) {
                        cur_r ^= 1;  // adopt the guess: no copy
                        sh.cur = cur_r;
                        // Its barren flag holds what own[] said in phase F, before this iteration's commit: it
                        // stays only if the commit moved no owner -- a rejection, an accepted change, or an
                        // accepted proposal that changed no point (a kept guess follows nothing else but a
                        // move).  Else the count is not known: the proposal reads it at the loop top.
                        // (The flag is not read here: cleared whether up or not, off the common path.)
                        if (prof_on && g.barren) sh.prof[55] += 1;  // diagnostic: guesses adopted with the flag up
                        if (acc && action != tdchain::kChange && sh.gs.nc != 0) {
                            if (prof_on && g.barren) sh.prof[25] += 1;  // diagnostic: ... and cleared here
                            sh.ps[cur_r].barren = 0;
                        }
                    } else {
                        // a just-killed position (LDS layout; in the HBM order phase G has shifted it already):
                        // scripted steps read the staged pre-shift order; a free-running chain the order once
                        // the shifting waves are done
                        const bool killed = RLDS && acc && action == tdchain::kDeath;
                        if (killed && !nscript)
                            SPIN_WAIT(__hip_atomic_load(&sh.shift_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <
                                          kWv - 1,
                                      1000000);
                        auto slot_at = [&](int pos) {
                            return (killed && nscript && pos >= (int)pp.index) ? d.order_tmp[pos + 1] : v.ord[pos];
                        };
                        if (nscript) {
                            sh.step_cur = mb ? sh.srv_step[sh.srv_k++] : sa.step[it + 1];
                            script_proposal(sh.ps[cur_r], sh.step_cur, sh.nfree, sh.nslots, d.free_slots, slot_at);
                        }
                        else
                            make_proposal(sh.ps[cur_r], P, draws[(it + 1) & 63], sh.ncells, sh.nfree, sh.nslots,
                                          d.free_slots, d.cx, d.cy, d.cz, d.czeta, slot_at);
                    }
                    const tdchain::Proposal &np = sh.ps[cur_r].p;
                    if (np.active) atomicAdd((unsigned long long *)&sh.proposed[np.action], 1ull);
                    sh.spec_ok = 0;
                    // the next proposal's counters: no wave reads them after phase F's barrier (phase G reads
                    // the snapshot sh.gs), so they are clear before the iteration-end barrier whatever the skew
                    sh.n_tiles = sh.n_changed = sh.n_orphans = sh.n_rays = 0;
                    if (!RLDS) sh.dsum = sh.dabs = 0.0;
                    sh.n_super[(it + 1) & 1] = 0;  // the other parity's list is refreshed first
                    sh.pts_seen = sh.ray_pts = 0;
                    sh.e_done = sh.b_done = 0;
                    if constexpr (kNoBarB) sh.q_done = 0;
                    sh.k0 = n;
                }
            }
        }
        STAMP(13);
        it_done = it + 1;
        __syncthreads();
        STAMP(6);
        SKEW(17);
        if constexpr (REC && ROUNDS) {
            // a round this workgroup ran at level 0 (wave 0's latch, above this barrier; block-uniform):
            // its model into the round's slot.  The next latch is at least one iteration's barriers away.
            if (sh.mbox[1] == it + 1 && sh.mbox[0] >= 0) {
                record_round_sample(d, v.ord, v.ptS, sh, sh.mbox[0], iter0 + it, last_action, last_accept, tid, NTH);
                __syncthreads();  // the copy is done before a later phase G changes the cells, the order or ptS
                SKEW(20);
            }
        }
        if constexpr (REC && !ROUNDS) {
            if (it + 1 == rec_next) {  // this iteration's model into the history (block-uniform)
                record_sample(d, v.ord, v.ptS, sh, it, iter0, last_action, last_accept, tid, NTH);
                rec_next += d.rec.every;
                __syncthreads();  // the copy is done before a later phase G changes the cells, the order or ptS
                SKEW(19);  // (the profile mode charges the copy to the next iteration's first stamp, phase 0)
            }
        }
    }

    const long long t_loop_end = prof_on ? clock64() : 0;
    {  // decisions on bounds: the partial sums and phi exact again (the launch leaves them)
        if (wv == 0) {
            phi_r = exact_sums(v.term, v.prefix, v.cprefix, v.cterm, v.rflag, sh, n, lane, false, n, phi_r, 0.0).phi;
            if (lane == 0) sh.phi = phi_r;
        }
        __syncthreads();
    }
    if constexpr (WALK) {
        if (pend_r) delta_commit<SMALL ? 1 : 16>(v.prefix, v.cprefix, n, sh.dseg, tid, NTH);
        if constexpr (SMALL) __syncthreads();  // the LDS sums are written back below
    }
    // ---- leave the LDS copies behind (flags and grid are already clean) ----
    if constexpr (SMALL) {
        for (int i = tid; i < NT; i += NTH) d.tile_maxd[i] = v.tmaxd[i];
        if constexpr (RLDS) {
            for (int i = tid; i < n; i += NTH) {
                d.ptS[i] = v.ptS[i];
                d.prefix[i] = v.prefix[i];
            }
            for (int i = tid; i < sh.ncells; i += NTH) d.order[i] = v.ord[i];
        }
    }
    if (tid == 0) {
        ChainScalars &s = *d.st;
        s.iter = iter0 + it_done;
        s.evaluations += sh.evaluations;
        s.bytes += sh.bytes;
        for (int a = 0; a < 5; ++a) {
            s.proposed[a] += sh.proposed[a];
            s.accepted[a] += sh.accepted[a];
        }
        s.phi = sh.phi;
        s.ncells = sh.ncells;
        s.nslots = sh.nslots;
        s.nfree = sh.nfree;
        s.next_stamp = sh.next_stamp;
        if (iters > 0) {
            s.last_action = last_action;
            s.last_accept = last_accept;
        }
        if (prof_on) {
            sh.prof[77] += clock64() - t_loop_end;  // epilogue (write-backs, scalars) up to here
            sh.prof[78] += 1;                        // launches
        }
        for (int k = 0; k < kProfSlots; ++k) s.prof[k] += sh.prof[k];
        s.prof[15] += sh.grid_fallbacks32;  // diagnostic: unproven grid searches
        if (d.st_host) *d.st_host = s;  // the host's pinned mirror: no copy back per chain
        if (mb) {
            __threadfence_system();
            mb_store(&mb->exited, 1);
        }
        if (rbx) {
            __threadfence_system();
            mb_store(&rbx->slot[bchain].exited, 1);
        }
    }
}

// ------------------------------------------------- one-point queries ----
// (In this unit because k_chain_run's generated code depends on it: the device code of a unit is
// optimised as one module, and without this second caller of wave_nearest in it the grid search inlined
// into every k_chain_run instance, and server_wait, come out with other instructions.)
// Interpolation at one point (MCsub.jl:306-327 with 1-element X/Y/Z, as the
// reference's birth and death queries call it, TD_inversion_function.jl:81,
// 146) against a chain's committed model, or that model plus one edit
// (td_evaluate's pending proposal, incremental.cpp): one wave, the chain's
// bucket grid (full scan when unproven), the same lexicographic (distance,
// Julia position) answer as v_nearest.  out[0] = the value.
__global__ __launch_bounds__(64) void k_chain_query(const DevChain *__restrict__ dptr, double x, double y, double z,
                                                   ScriptStep e, int has_edit, double *out) {
    const DevChain &d = *dptr;
    __shared__ Shared sh;
    const int lane = threadIdx.x;
    if (lane == 0) {
        sh.grid_ovf = *d.grid_overflow;
        sh.nslots = d.st->nslots;
        sh.grid_fallbacks32 = 0;
        geo_fill(sh.geo, d);
    }
    __syncthreads();
    Views v{};
    v.ord = d.order;
    int skip = -1, moved = -1, slot_k = -1;
    if (has_edit && e.action != tdchain::kBirth) slot_k = d.order[e.index];
    if (has_edit && e.action == tdchain::kDeath) skip = slot_k;  // the reduced model (:132-135)
    if (has_edit && e.action == tdchain::kMove) moved = slot_k;  // the cell at its new site
    Nearest r = wave_nearest(d, v, sh, lane, x, y, z, skip, moved, e.x, e.y, e.z, moved >= 0 ? d.czeta[moved] : 0.0);
    double val = r.z;
    if (has_edit && e.action == tdchain::kChange && r.s == slot_k) val = e.zeta;
    if (has_edit && e.action == tdchain::kBirth) {  // the appended cell: last position, wins only strictly
        const double dd = dist2(e.x, e.y, e.z, x, y, z);
        if (dd < r.d && dd < kSentinel) val = e.zeta;
    }
    if (lane == 0) out[0] = val;
}

}  // namespace

// Every iteration's draws of a launch (a function of seed, chain, iteration: tdchain::draw_iteration),
// one thread each, ahead of k_chain_run: its per-64-iteration refill -- one wave computing 64 draws'
// quantiles and logarithm on the chain's critical path -- becomes one round of loads.
__global__ __launch_bounds__(256) void k_draws(const DevChain *__restrict__ dptr, long long iters,
                                               tdchain::Draws *__restrict__ out) {
    const DevChain &d = dptr[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= iters) return;
    out[(long long)blockIdx.y * iters + i] = tdchain::draw_iteration(d.seed, d.chain, (uint64_t)(d.st->iter + i));
}

hipError_t chain_query(const DevChain *dev, double x, double y, double z, const ScriptStep *edit, double *out,
                       hipStream_t s) {
    ScriptStep e{};
    if (edit) e = *edit;
    hipLaunchKernelGGL(k_chain_query, dim3(1), dim3(64), 0, s, dev, x, y, z, e, edit ? 1 : 0, out);
    return hipGetLastError();
}

// The k_chain_run instances: what choose_chain_variant (chain_variant.h) can name, and nothing else.
static_assert(kVariantThreads == kChainThreads, "chain_variant.h's thread count");
using ChainKernel = void (*)(const DevChain *, long long, ScriptArgs);
#define TD_CHAIN_INSTANCE(SMALL, SCRIPT, NTH, RLDS, ROUNDS, REC) \
    {{SMALL, SCRIPT, NTH, RLDS, ROUNDS, REC}, k_chain_run<SMALL, SCRIPT, NTH, RLDS, ROUNDS, REC>}
static const struct {
    ChainVariant v;
    ChainKernel k;
} kChainInstances[] = {
    // (the table's order is the instances' order of instantiation, so their order in the device module:
    // treat a reordering like a change of k_chain_run's body, above)
    // one 8-wave chain per CU, tiles, rays and order in LDS: free-running, scripted; the same, all in HBM
    TD_CHAIN_INSTANCE(true, false, kChainThreads, true, false, false),
    TD_CHAIN_INSTANCE(true, true, kChainThreads, true, false, false),
    TD_CHAIN_INSTANCE(false, false, kChainThreads, false, false, false),
    TD_CHAIN_INSTANCE(false, true, kChainThreads, false, false, false),
    // two 4-wave chains per CU, free-running: all in HBM; the tiles in LDS
    TD_CHAIN_INSTANCE(false, false, kChainThreads / 2, false, false, false),
    TD_CHAIN_INSTANCE(true, false, kChainThreads / 2, false, false, false),
    // exchange rounds (8 waves): LDS layout; all in HBM
    TD_CHAIN_INSTANCE(true, false, kChainThreads, true, true, false),
    TD_CHAIN_INSTANCE(false, false, kChainThreads, false, true, false),
    // the four free-running ones, recording
    TD_CHAIN_INSTANCE(true, false, kChainThreads, true, false, true),
    TD_CHAIN_INSTANCE(false, false, kChainThreads, false, false, true),
    TD_CHAIN_INSTANCE(false, false, kChainThreads / 2, false, false, true),
    TD_CHAIN_INSTANCE(true, false, kChainThreads / 2, false, false, true),
    // a ladder's recording (host-decided rounds and exchange rounds alike): LDS layout; all in HBM
    TD_CHAIN_INSTANCE(true, false, kChainThreads, true, true, true),
    TD_CHAIN_INSTANCE(false, false, kChainThreads, false, true, true),
};
#undef TD_CHAIN_INSTANCE

int chain_variant_index(const ChainVariant &v) {
    int i = 0;
    for (const auto &e : kChainInstances) {
        if (e.v == v) return i;
        ++i;
    }
    return -1;
}

// Launches of each table entry by this process (host only; testing: a case that means to run one
// instance can tell that it did, tdt_chain_launch_counts)
static std::atomic<int64_t> g_launches[sizeof(kChainInstances) / sizeof(kChainInstances[0])];

int chain_launch_counts(int64_t *out, int cap) {
    const int n = (int)(sizeof(kChainInstances) / sizeof(kChainInstances[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = g_launches[i].load(std::memory_order_relaxed);
    return n;
}

// ... and of k_draws (host only; testing: a launch that means to draw inside the kernel can tell that no
// draws were precomputed for it, tdt_chain_draws_launches)
static std::atomic<int64_t> g_draws_launches;

int64_t chain_draws_launches() { return g_draws_launches.load(std::memory_order_relaxed); }

hipError_t chain_run(const DevChain *host, const DevChain *dev, int nchains, int64_t iters, hipStream_t s,
                     const ScriptArgs *script, DrawsBuf db, int num_cus) {
    ScriptArgs sa{};
    if (script) sa = *script;
    sa.pin = -1;
    sa.pre = nullptr;
    sa.pre_stride = 0;
    static const bool pre_env = [] {  // diagnostic: TD_PRE_DRAWS=0 keeps the in-kernel draws
        const char *e = std::getenv("TD_PRE_DRAWS");
        return !(e && e[0] == '0');
    }();
    const bool resident = sa.n > 0 || sa.mb != nullptr || sa.rb != nullptr;
    const size_t pre_bytes = sizeof(tdchain::Draws) * (size_t)nchains * (size_t)std::max<int64_t>(iters, 0);
    if (pre_env && db.p && !resident && iters > 0 && pre_bytes <= kDrawsBudget) {
        if (pre_bytes > *db.bytes) {
            if (*db.p) {
                hipError_t e = hipStreamSynchronize(s);
                if (e != hipSuccess) return e;
                (void)hipFree(*db.p);
                *db.p = nullptr;
                *db.bytes = 0;
            }
            hipError_t e = hipMalloc(db.p, pre_bytes);
            if (e != hipSuccess) return e;
            *db.bytes = pre_bytes;
        }
        g_draws_launches.fetch_add(1, std::memory_order_relaxed);
        hipLaunchKernelGGL(k_draws, dim3((unsigned)((iters + 255) / 256), (unsigned)nchains), dim3(256), 0, s, dev,
                           (long long)iters, static_cast<tdchain::Draws *>(*db.p));
        sa.pre = static_cast<const tdchain::Draws *>(*db.p);
        sa.pre_stride = iters;
    }
    static const int pin_env = [] {
        const char *e = std::getenv("TD_XCC_PIN");
        return e ? std::atoi(e) : -1;
    }();
    int grid = nchains;
    if (nchains == 1 && pin_env >= 0) {
        sa.pin = pin_env;
        grid = 8;
    }
    ChainLaunchFacts f = launch_facts(host, nchains);
    f.scripted = sa.n > 0 || sa.mb != nullptr;
    f.rx = sa.rx != nullptr;
    f.rb = sa.rb != nullptr;
    f.rounds_rec = f.rec && (f.rx || f.rb);  // set by td_rounds_temper_recorded / td_rounds_exchange_recorded alone
    f.num_cus = num_cus;
    const ChainChoice c = choose_chain_variant(f);
    static bool attr_set = false;  // dynamic LDS above 64 KB needs the attribute (once per kernel)
    if (!attr_set) {
        for (const auto &e : kChainInstances) {
            hipError_t err = hipFuncSetAttribute((const void *)e.k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)kLdsBudget);
            if (err != hipSuccess) return err;
        }
        attr_set = true;
    }
    const int at = chain_variant_index(c.v);
    if (at < 0) return hipErrorInvalidValue;  // no such instance: never another kernel in its place
    g_launches[at].fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(kChainInstances[at].k, dim3(grid), dim3(c.v.nth), c.lds, s, dev, (long long)iters, sa);
    return hipGetLastError();
}

}  // namespace tdstar
